"""Batches past a level's hand-over buffer (-m gpu).  tz_model_prepare gives P[l] min(max_batch, kPBytes / per_item) slots
(Pcap[l]), and both split forms of a gate convolution ask per batch whether it fits: 'E-part ahead' under TZ-PA2 (tz_prednet.hip
epart_levels: n <= Pcap[l]) and the k_convlat_pair split under TZ-PA1 (slot0 + n <= Pcap[l]).  A command-line job prepares
min(windows, 64) slots, so from 128x128 on its full batches run one set of levels split and its trailing small batch another.

The job: the default model (3, 48, 96, 192) at 128x128, 56 slots, 60 windows of three frames -- four predictor calls, batches of
56 and 4 at depth 1 and at depth 2.  Level 1 holds 53 windows, level 2 all 56: a forced step of 56 splits level 2 ALONE, with the
side launch going out behind A_1, and a step of 4 splits both.  Every comparison is of bit patterns: against the fused step, a
context whose every batch fits, tz_set_conv_impl(0) and the C oracle at the windows either side of every boundary.  The GPU side
of a case runs in one child process under a time limit (tests/sched_jobs.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import sched_jobs as S
import test_gpu_wino2q as W

pytestmark = pytest.mark.gpu

K_P_BYTES = 160 << 20                      # tz_prednet.hip kPBytes
HP = WP = 128
MAXB, NWIN = 56, 60
WINDOWS = (0, 52, 53, 55, 56, 59)          # the first, the two either side of Pcap[1], the last of the full batch, the trailing batch's ends
KINDS = ("zero", "bias")                   # every gate launch in the three-tile form / in the four-tile form


def pcap(level, max_batch):
    """tz_model_prepare: [item][pixel][4 R] float32 accumulators, as many items as fit kPBytes."""
    cfg, _ = S.model("zero")
    per_item = (HP >> level) * (WP >> level) * 4 * cfg.R_stack_sizes[level] * 4
    return min(max_batch, K_P_BYTES // per_item)


def test_the_job_straddles_the_buffer_of_level_1():
    """If kPBytes is ever changed, this says that the cases below no longer cover the boundary."""
    assert (pcap(1, MAXB), pcap(2, MAXB)) == (53, 56)
    assert pcap(1, MAXB) < MAXB <= pcap(2, MAXB)
    assert NWIN - MAXB <= pcap(1, MAXB)                     # the trailing batch fits both levels
    assert WINDOWS[1] == pcap(1, MAXB) - 1 and WINDOWS[2] == pcap(1, MAXB)
    assert pcap(1, 4) == pcap(2, 4) == 4                    # (the LEVELS case and the context whose every batch fits)


def _job(kind, contract=2, max_batch=MAXB, nwin=NWIN, **more):
    return S.job(kind, HP, WP, max_batch, nwin, contract=contract, **more)


@pytest.fixture(scope="module", params=KINDS)
def pa2(request, tmp_path_factory):
    """The job under TZ-PA2, fused and with the split forced: (kind, results, logs), shared by the cases over it."""
    kind = request.param
    res, logs = S.child(tmp_path_factory.mktemp("pa2_" + kind), {
        "fused": _job(kind, prof=True, env={"TEZIP_EPART": 0}),
        "forced": _job(kind, prof=True, env={"TEZIP_EPART": 1, "TEZIP_WINO2Q_LOG": 1})})
    for r in res.values():
        for a in r.values():
            a.setflags(write=False)
    return kind, res, logs


def test_forced_split_past_the_buffer_of_level_1(pa2):
    """A.1: level 2 splits and level 1 does not (epart_top == 2, epart[1] == false) in the steps of 56, both in the steps of 4."""
    kind, res, logs = pa2
    assert res["forced"]["contract"] == res["fused"]["contract"] == 2
    n_fused, n_forced = int(res["fused"]["n_wino_pa2"]), int(res["forced"]["n_wino_pa2"])
    print("k_wino launches of the four calls: fused %d, forced %d" % (n_fused, n_forced))
    S.same_bits(res["forced"], res["fused"], "forced against fused")
    assert n_fused == 4 * 5                                 # A_1, A_2, gates 3, 2, 1
    assert n_forced == 2 * 6 + 2 * 7                        # 56 windows: + the side launch of level 2; 4 windows: + both
    rows = W._log(logs["forced"])
    for row in sorted(rows.items()):
        print(row)
    if kind == "zero":                                      # what tests/test_gpu_wino2q.py expects for this model
        assert {k: (r["same"], r["up"], r["tiles"], r["form"]) for k, r in rows.items()} == {
            (1, "gates"): (12, 24, "three", "two-quad"), (1, "A"): (12, 0, "three", "two-quad"), (2, "gates"): (24, 48, "three", "two-quad"),
            (2, "A"): (24, 0, "four", "one-quad"), (3, "gates"): (48, 0, "three", "two-quad")}, rows
    else:
        assert [k for k, r in rows.items() if r["tiles"] == "three"] == [(1, "A")], rows
        assert (rows[(1, "A")]["same"], rows[(1, "A")]["form"]) == (24, "two-quad"), rows


def test_the_oracle_either_side_of_every_boundary(pa2):
    """A.4: twelve oracle steps under contract 2."""
    kind, res, _ = pa2
    for name in ("fused", "forced"):
        S.oracle_bits(res[name], _job(kind), WINDOWS, name)


def test_split_by_measurement_for_two_batch_sizes_of_one_model(tmp_path):
    """A.2: epart_choice[56] and epart_choice[4] measured in one rollout, whichever way they fall; a second rollout runs on the
    cached decisions."""
    res, logs = S.child(tmp_path, {"fused": _job("zero", env={"TEZIP_EPART": 0}),
                                   "measured": _job("zero", again=True, env={"TEZIP_EPART_LOG": 1})})
    lines = [ln for ln in logs["measured"].splitlines() if "E-part ahead" in ln]
    print("\n".join(lines))
    S.same_bits(res["measured"], res["fused"], "measured against fused")
    np.testing.assert_array_equal(res["measured"]["key2"], res["measured"]["key"])
    np.testing.assert_array_equal(S.D.bits(res["measured"]["roll2"]), S.D.bits(res["measured"]["roll"]))
    S.oracle_bits(res["measured"], _job("zero"), WINDOWS, "measured")


@pytest.mark.parametrize("levels,per_call", [(2, 6), (4, 6), (6, 7)])
def test_the_levels_switch_makes_the_same_mix_by_hand(levels, per_call, tmp_path):
    """A.3: TEZIP_EPART_LEVELS (bit l: level l may split; read once per process) at 4 slots, 12 windows: six calls of 4."""
    res, _ = S.child(tmp_path, {"fused": _job("zero", max_batch=4, nwin=12, prof=True, env={"TEZIP_EPART": 0}),
                                "mixed": _job("zero", max_batch=4, nwin=12, prof=True, env={"TEZIP_EPART": 1})}, TEZIP_EPART_LEVELS=levels)
    n_fused, n_mixed = int(res["fused"]["n_wino_pa2"]), int(res["mixed"]["n_wino_pa2"])
    print("k_wino launches of the six calls: fused %d, TEZIP_EPART_LEVELS=%d %d" % (n_fused, levels, n_mixed))
    S.same_bits(res["mixed"], res["fused"], "TEZIP_EPART_LEVELS=%d against fused" % levels)
    assert n_fused == 6 * 5
    assert n_mixed == 6 * per_call


@pytest.mark.parametrize("kind", KINDS)
def test_pa1_at_the_same_shape(kind, tmp_path):
    """A.5: the contract by size is TZ-PA1 at 128x128.  56 slots against 4 slots (15 calls, every one inside its buffer), against
    tz_set_conv_impl(0), against k_convlat wherever eligible and against the oracle under contract 1.
    lat_plan takes k_convlat only where a launch has at most 768 k_conv16 workgroups, and the pair only where its two halves have at
    most 1024 workgroups together: at this frame size neither a step of 56 nor one of 4 meets both (a level-1 half alone is
    3 x 16 x 16 x n workgroups, a level-2 pair (3 + 6) x 8 x 8 x n), so k_convlat_pair never runs and `slot0 + n <= Pcap[l]` decides
    nothing here.  Asserted on the counters: what the 768 rule alone fixes, under `always` (no cost model) -- of A_1, A_2 and the gates
    of levels 3, 2, 1 (column blocks x tiles x n = 2 x 16 n, 3 x 4 n, 12 x 1 n, 6 x 4 n, 3 x 16 n) a step of 56 runs A_2 and the
    gates of level 3 on k_convlat and the other three on k_conv16, a step of 4 all five on k_convlat."""
    variants = {"big": _job(kind, 0, prof=True), "small": _job(kind, 0, max_batch=4, prof=True), "ref": _job(kind, 0, impl=0, prof=True),
                "always": _job(kind, 0, lat="always", prof=True)}
    res, _ = S.child(tmp_path, variants)
    for name, r in res.items():
        assert r["contract"] == 1
        print(name, {k[2:]: int(v) for k, v in r.items() if k.startswith("n_")})
    assert (int(res["always"]["n_convlat_small_grid"]), int(res["always"]["n_conv16_lds_dma"])) == (2 * 2 + 2 * 5, 2 * 3)
    assert int(res["big"]["n_convlat_small_grid"]) <= int(res["always"]["n_convlat_small_grid"])     # (the cost model only takes away)
    assert int(res["ref"]["n_convlat_small_grid"]) == int(res["ref"]["n_conv16_lds_dma"]) == 0
    for name in ("small", "ref", "always"):   # (the last call of every variant starts at window 56: the same taps)
        S.same_bits(res["big"], res[name], "56 slots against " + name)
    S.oracle_bits(res["big"], _job(kind, 1), WINDOWS, "TZ-PA1")


@pytest.mark.parametrize("enc,dec", [(1, 0), (0, 1)])
def test_a_lossless_job_through_the_command_line(enc, dec, tmp_path):
    """A.6: 60 windows of 128x128 images, `-c` with the split forced / forbidden and `-u` the other way round (its context holds 64
    slots: one batch of 60).  A lossless round trip survives only if encoder and decoder form the same predictions."""
    from PIL import Image
    from tezip_amd import weights
    cfg, wts = S.model("zero")
    mdir, ddir, cdir, udir = (str(tmp_path / d) for d in ("model", "data", "comp", "out"))
    weights.save_model(mdir, cfg, wts, HP, WP)
    u8 = S.frames(HP, WP, NWIN)
    os.makedirs(ddir)
    names = ["frame_%03d.png" % t for t in range(len(u8))]
    for n, f in zip(names, u8):
        Image.fromarray(f, mode="RGB").save(os.path.join(ddir, n), compress_level=1)
    env = {k: v for k, v in os.environ.items() if k not in S.ENV}
    for flag, a, b, mode in (("-c", ddir, cdir, enc), ("-u", cdir, udir, dec)):
        cmd = ["timeout", "-k", "10", "200", sys.executable, "-m", "tezip_amd.tezip", flag, mdir, a, b, "--pa", "2"]
        if flag == "-c":
            cmd += ["-w", "3", "-p", "0", "-m", "abs", "-b", "0"]
        r = subprocess.run(cmd, env=dict(env, TEZIP_EPART=str(mode)), cwd=S.ROOT, capture_output=True, text=True, timeout=230)
        assert r.returncode == 0, (flag, r.returncode, r.stdout[-1500:] + r.stderr[-1500:])
    for n, f in zip(names, u8):
        assert np.array_equal(np.array(Image.open(os.path.join(udir, n))), f), n
