"""Dead leading blocks of the error maps (-m gpu): the same-resolution source of every k_wino launch is E_l = [relu(Ahat0_l -
A_l), relu(A_l - Ahat0_l)].  Where the per-model constant Ahat0_l is +-0 over the whole plane for the first 16 d channels,
those channels of E_l are +0 in every frame, and k_wino leaves their 4 d stages out (tz_prednet.hip measure_dead /
launch_wino): every Winograd chain starts from the literal +0 and fmaf(+0, U, +0) = +0 for finite U, so not a bit may change
(tests/test_deadsrc_oracle.py states the lemma on the C oracle).  tz_model_prepare MEASURES the property; nothing is assumed.

Every case runs a few predictor steps under TZ-PA2 (set_contract(2)) through the C ABI and compares predictions and every
level's E / R taps as BIT PATTERNS with (a) the same job in a fresh child with TEZIP_DEADSRC=0, (b) tz_set_conv_impl(0) (k_wino_ref,
which never skips) and (c) the C oracle under contract 2.  What was measured is read from the TEZIP_DEADSRC_LOG=1 lines of a
fresh child and compared with the rule restated on the numpy oracle's Ahat0_l.

tz_model_load refuses stack sizes that are not multiples of 16, so no accepted model has a 16-channel block that straddles the
two halves of E_l; the guard 16 (b + 1) <= stack_l of measure_dead cannot be reached through the API.  The closest shape is
run instead: 80 channels (five blocks: an odd number, not a multiple of the 32-channel pairs the default shape has)."""
import functools
import json
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import pytest  # noqa: E402

from tezip_amd.prednet import PredNetConfig  # noqa: E402

pytestmark = pytest.mark.gpu

DEFAULT = ((3, 48, 96, 192), None)
M9 = ((3, 80, 128), None)               # tests/model_space.py M9: five blocks in the positive half of E_1
TINY = ((3, 16), (3, 16))               # one k_wino convolution: the gates of level 1, one block per half
TINY_SEED = 97980                       # bias_scale 0.1: block 0 of Ahat0_1 is zero at the centre pixel, not on the border (asserted below)
ENV = ("TEZIP_DEADSRC", "TEZIP_DEADSRC_LOG", "TEZIP_UNIFORM", "TEZIP_UNIFORM_LOG", "TEZIP_EPART")
LOG_LINE = re.compile(r"\[tezip\] dead source, level (\d+) (gates|A): (\d+) of (\d+) leading positive-half blocks dead, (\d+) skipped: "
                      r"(\d+) of (\d+) same-resolution stages")


def _spec(kind, hp, wp, batch, shape=DEFAULT, seed=123):
    """A job: `batch` windows and one frame more than fits a batch, so that the last call is a batch of one (whose taps the
    library holds)."""
    return (kind, shape, hp, wp, batch, 3 if batch == 1 else batch + 1, int(seed))


def _ahat_bias(cfg, w, l):
    return w[2 * (cfg.nb_layers - 1) + 2 * l + 1]


def _model(spec):
    kind, (stack, rstack), hp, wp, _, n, seed = spec
    cfg = PredNetConfig(stack_sizes=stack, R_stack_sizes=rstack)
    L = cfg.nb_layers
    if kind in ("zero", "nonfinite"):
        w = cfg.init_weights(seed=seed)                             # Keras' default initialisation: zero biases
    else:
        w = cfg.init_weights(seed=seed, bias_scale=0.1)
    if kind in ("neg0", "neg1"):                                    # Ahat biases: -1 on one block, small positive elsewhere
        rng = np.random.default_rng(seed + 1)
        lo = 0 if kind == "neg0" else 16
        for l in range(1, L):
            b = _ahat_bias(cfg, w, l)
            b[:] = rng.uniform(0.01, 0.05, b.shape).astype(np.float32)
            b[lo:lo + 16] = -1.0
    if kind == "nonfinite":                                         # gate i of level 2, input channel 5 of E_2's positive half
        names = [nm for nm, _ in cfg.weight_shapes()]
        w[names.index("i2/kernel")][1, 1, cfg.R_stack_sizes[2] + 5, 7] = np.inf
    frames = np.random.default_rng(hp * 31 + wp).integers(0, 256, (n, hp, wp, 3)).astype(np.float32) / np.float32(255)
    return cfg, w, frames


def _names(cfg):
    return ["pred"] + ["e%d" % l for l in range(cfg.nb_layers)] + ["r%d" % l for l in range(cfg.nb_layers)]


def run_job(spec, impl=1):
    """The job on the GPU, in this process: predictions of all frames, the taps of the last one, k_wino launches."""
    from tezip_amd import _lib
    cfg, w, frames = _model(spec)
    c = _lib.Context(0)
    try:
        c.set_contract(2)
        c.set_conv_impl(impl)
        c.load_model(cfg, w)
        c.prepare(spec[2], spec[3], max_batch=spec[4])
        c.prof_enable(True)
        c.prof_reset()
        out = {"pred": c.predict_next(frames)}
        out["n_wino"] = np.array(c.prof_get()["wino_pa2"][1])
        c.prof_enable(False)
        for l in range(cfg.nb_layers):
            out["e%d" % l] = c.predict_tap(0, l)
            out["r%d" % l] = c.predict_tap(1, l)
    finally:
        c.close()
    return out


def _child(spec, tmp_path, tag, **env):
    """The same job in a fresh process with `env` set: (results, stderr)."""
    out = str(tmp_path / (tag + ".npz"))
    e = dict(os.environ)
    for k in ENV:
        e.pop(k, None)
    e.update({k: str(v) for k, v in env.items()})
    r = subprocess.run([sys.executable, os.path.abspath(__file__), json.dumps(spec), out], env=e, cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    with np.load(out) as z:
        return {k: z[k] for k in z.files}, r.stderr


@functools.lru_cache(maxsize=None)
def _oracle(spec):
    """Computed once per (model, size, frames); shared by the cases over the same job and never written to."""
    from oracle import coracle
    cfg, w, frames = _model(spec)
    net = coracle.CPredNet(w, cfg.stack_sizes, cfg.R_stack_sizes, spec[2], spec[3]).set_contract(2)
    pred = np.empty_like(frames)
    for i in range(len(frames) - 1):
        pred[i] = net.next(frames[i])
    pred[-1], dbg = net.next(frames[-1], debug=True)
    ref = {"pred": pred}
    for l in range(cfg.nb_layers):
        ref["e%d" % l], ref["r%d" % l] = dbg["e"][l], dbg["r"][l]
    for v in ref.values():
        v.setflags(write=False)
    return ref


def _same_bits(got, want, what, cfg):
    for k in _names(cfg):
        a, b = np.ascontiguousarray(got[k], np.float32).view(np.uint32), np.ascontiguousarray(want[k], np.float32).view(np.uint32)
        np.testing.assert_array_equal(a, b, err_msg="%s: %s" % (what, k))


def _log(stderr):
    rows = {(int(m[1]), m[2]): dict(dead=int(m[3]), half=int(m[4]), skipped=int(m[5]), stages=int(m[6]), of=int(m[7]))
            for m in (LOG_LINE.search(ln) for ln in stderr.splitlines()) if m}
    assert rows, stderr[-1500:]
    return rows


# ------------------------------------------------------------------------------------- the rule, restated on the numpy oracle
@functools.lru_cache(maxsize=None)
def _ahat0_pre(spec):
    """Pre-activations of Ahat_l at t = 0 (zero state, zero errors: only the upsampled r of the level above is non-zero),
    oracle/prednet_np.py step's top-down pass."""
    from oracle import prednet_np as P
    cfg, w, _ = _model(spec)
    L, hp, wp = cfg.nb_layers, spec[2], spec[3]
    sw = P.split_weights(w, L)
    r_up, z = None, [None] * L
    for l in reversed(range(L)):
        x = np.zeros((hp >> l, wp >> l, cfg.R_stack_sizes[l] + 2 * cfg.stack_sizes[l]), np.float32)
        if r_up is not None:
            x = np.concatenate([x, r_up], axis=-1)
        i, o = P.hard_sigmoid(P.conv_same(x, *sw["i"][l])), P.hard_sigmoid(P.conv_same(x, *sw["o"][l]))
        g = np.tanh(P.conv_same(x, *sw["c"][l])).astype(np.float32)
        r = o * np.tanh(i * g).astype(np.float32)                   # (c_{-1} = 0: the forget gate has nothing to keep)
        z[l] = P.conv_same(r, *sw["ahat"][l])
        r_up = P.upsample(r)
    return z


def _expected_dead(spec):
    """dead[l] by the rule of measure_dead over the whole plane; every block the rule looks at must be decided by a margin the
    numpy oracle's rounding (~1e-5) cannot cross."""
    cfg = _model(spec)[0]
    z, dead = _ahat0_pre(spec), {}
    for l in range(1, cfg.nb_layers):
        st, d = cfg.stack_sizes[l], 0
        while 16 * (d + 1) <= st and d + 1 < 2 * st // 16:
            top = float(z[l][:, :, 16 * d:16 * d + 16].max())
            assert abs(top) > 1e-4 or top == 0.0, (l, d, top)
            if top > 0:
                break
            d += 1
        dead[l] = d
    return dead


def _check_log(spec, rows, want=None):
    """Every k_wino convolution of the model has its line; found == the rule on the numpy oracle (== `want` where given);
    skipped == found (finite weights) and the stage counts follow."""
    cfg = _model(spec)[0]
    L, st = cfg.nb_layers, cfg.stack_sizes
    exp = _expected_dead(spec)
    for l in range(1, L):
        for conv in ("gates",) + (("A",) if l < L - 1 else ()):
            row = rows[(l, conv)]
            print("level %d %s: %r" % (l, conv, row))
            assert row["half"] == st[l] // 16 and row["of"] == 2 * st[l] // 4, (l, conv, row)
            assert row["dead"] == exp[l], (l, conv, row, exp)
            if want is not None:
                assert row["dead"] == want(l), (l, conv, row)
            assert row["skipped"] == row["dead"] and row["stages"] == 4 * row["dead"], (l, conv, row)
            assert 16 * row["skipped"] <= st[l] and row["stages"] + 4 <= row["of"], (l, conv, row)


def _check(spec, tmp_path, want=None, ref_impl=True, oracle=True):
    cfg = _model(spec)[0]
    on, err = _child(spec, tmp_path, "on", TEZIP_DEADSRC_LOG=1)
    rows = _log(err)
    off, err_off = _child(spec, tmp_path, "off", TEZIP_DEADSRC=0)
    assert "dead source" not in err_off                              # nothing is printed unless asked
    _same_bits(on, off, "against TEZIP_DEADSRC=0", cfg)
    assert on["n_wino"] == off["n_wino"]                             # no launch added or removed
    if ref_impl:
        _same_bits(on, run_job(spec, impl=0), "against tz_set_conv_impl(0)", cfg)
    if oracle:
        _same_bits(on, _oracle(spec[:4] + (1,) + spec[5:]), "against the C oracle", cfg)   # (the oracle has no batches)
    if want is not False:
        _check_log(spec, rows, want)
    return on, rows


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("hp,wp,batch", [(64, 64, 1), (64, 64, 3), (72, 88, 1), (72, 88, 3)])
def test_zero_bias_model_skips_the_whole_positive_half(hp, wp, batch, tmp_path):
    """Keras' default initialisation (the bench's model): Ahat0_l = 0 at every level -- 12 of 24 / 24 of 48 / 48 of 96 stages
    of the gates, 12 of 24 / 24 of 48 of A_1 / A_2.  72 x 88: cut tiles at levels 2 and 3."""
    spec = _spec("zero", hp, wp, batch)
    st = DEFAULT[0]
    on, rows = _check(spec, tmp_path, want=lambda l: st[l] // 16)
    assert {k: (r["stages"], r["of"]) for k, r in rows.items()} == {
        (1, "gates"): (12, 24), (1, "A"): (12, 24), (2, "gates"): (24, 48), (2, "A"): (24, 48), (3, "gates"): (48, 96)}
    for l in range(1, 4):                                            # the dead channels are still WRITTEN: other kernels read them
        assert (on["e%d" % l][:, :, :st[l]].view(np.uint32) == 0).all() and (on["e%d" % l][:, :, st[l]:] > 0).any()


def test_one_dead_block(tmp_path):
    """Ahat biases of -1 on channels 0..15 of levels 1..3, small positive ones elsewhere: exactly one block."""
    _check(_spec("neg0", 72, 88, 3), tmp_path, want=lambda l: 1)


def test_a_dead_block_behind_a_live_one_is_not_skipped(tmp_path):
    """-1 on channels 16..31 only: block 1 is dead, block 0 is not -- nothing is a prefix, nothing is skipped."""
    _check(_spec("neg1", 64, 64, 1), tmp_path, want=lambda l: 0)


@pytest.mark.parametrize("hp,wp,batch,seed", [(64, 64, 3, 123), (72, 88, 1, 31)])
def test_biased_models_skip_what_the_rule_says(hp, wp, batch, seed, tmp_path):
    """bias_scale = 0.1: the expected counts come from the numpy oracle's Ahat0_l alone (as a rule: none)."""
    _check(_spec("bias", hp, wp, batch, seed=seed), tmp_path)


def test_a_block_that_is_zero_at_the_centre_but_not_on_the_border(tmp_path):
    """bias_scale = 0.1, the seed chosen on the CPU: every channel of block 0 of Ahat0_1 is zero at the centre pixel -- a
    measurement that looked at one pixel would call the block dead -- and some channel is non-zero on the border, where the
    zero padding takes taps away.  Asserted on the oracle's arrays, so the case cannot pass vacuously; the log must say 0."""
    spec = _spec("bias", 64, 64, 1, shape=TINY, seed=TINY_SEED)
    z = _ahat0_pre(spec)[1]
    assert z[16, 16, :16].max() < -1e-3, z[16, 16, :16].max()
    border = np.concatenate([z[0, :, :16], z[-1, :, :16], z[:, 0, :16], z[:, -1, :16]])
    assert border.max() > 1e-3, border.max()
    assert (z[2:-2, 2:-2, :16].max() < -1e-3)                       # ... and ONLY there: the whole interior is zero
    on, rows = _check(spec, tmp_path, want=lambda l: 0)
    assert set(rows) == {(1, "gates")} and rows[(1, "gates")]["dead"] == 0


def test_five_blocks_in_the_positive_half(tmp_path):
    """(3, 80, 128) at 72 x 88, zero biases: E_1 has 10 blocks, the first 5 are the positive half and all of it is skipped --
    20 of 40 stages, an odd number of rounds of the ring -- and no block beyond the half is."""
    spec = _spec("zero", 72, 88, 1, shape=M9, seed=13)
    _, rows = _check(spec, tmp_path, want=lambda l: M9[0][l] // 16)
    assert (rows[(1, "gates")]["stages"], rows[(1, "A")]["stages"], rows[(2, "gates")]["stages"]) == (20, 20, 32)


def test_a_non_finite_weight_in_a_dead_stage_forbids_the_skip(tmp_path):
    """One +inf in gate i of level 2, on a channel of E_2's dead positive half: 0 x inf is a NaN the chain must keep, so that
    convolution skips nothing (the others still do) and the bits are those of TEZIP_DEADSRC=0.  (What the hardware makes of a
    NaN -- its payload, the clamp of the hard sigmoid behind it -- is its business: no comparison with the CPU oracle or the
    plain kernel here.)  The weight does reach the result: channel 7 of R_2 is not what the model without it gives."""
    spec = _spec("nonfinite", 64, 64, 1)
    on, rows = _check(spec, tmp_path, want=False, ref_impl=False, oracle=False)
    assert rows[(2, "gates")] == dict(dead=6, half=6, skipped=0, stages=0, of=48), rows
    for key in ((1, "gates"), (1, "A"), (2, "A"), (3, "gates")):
        assert rows[key]["skipped"] == rows[key]["dead"] == rows[key]["half"], (key, rows[key])
    clean = run_job(_spec("zero", 64, 64, 1))
    assert not np.array_equal(on["r2"][:, :, 7].view(np.uint32), clean["r2"][:, :, 7].view(np.uint32))
    assert np.array_equal(on["r3"].view(np.uint32), clean["r3"].view(np.uint32))          # (level 3 comes before it)


def test_forced_split_on_the_zero_bias_model(monkeypatch):
    """'E-part ahead' forced (TEZIP_EPART=1): the side launches <4, EPI_RAW, false> of levels 1 and 2 walk the live half of
    E_l only, the NOSAME launches index the full stage image as before.  Bit-identical to the fused step and to the oracle;
    5 k_wino launches per predictor call fused, 7 split (tests/test_gpu_epart.py), two calls."""
    spec = _spec("zero", 72, 88, 3)
    cfg = _model(spec)[0]
    got = {}
    for mode in (0, 1):
        monkeypatch.setenv("TEZIP_EPART", str(mode))
        got[mode] = run_job(spec)
        assert got[mode]["n_wino"] == (14 if mode else 10), (mode, got[mode]["n_wino"])
    _same_bits(got[1], got[0], "split against fused", cfg)
    _same_bits(got[1], _oracle(spec[:4] + (1,) + spec[5:]), "split against the C oracle", cfg)


def test_cli_round_trip_256(tmp_path):
    """-c then -u of a 256 x 256 job with the zero-bias model, contract by default (TZ-PA2 at this size: every k_wino launch of
    encoder and decoder skips), lossless: the output is the input."""
    from PIL import Image
    from tezip_amd import compress, decompress, synth, weights
    cfg = PredNetConfig()
    mdir = str(tmp_path / "model")
    weights.save_model(mdir, cfg, cfg.init_weights(seed=123), 256, 256)
    frames = synth.translating_scene(5, 256, 256, seed=29)
    ddir = tmp_path / "data"
    ddir.mkdir()
    for t in range(frames.shape[0]):
        Image.fromarray(frames[t], mode="RGB").save(ddir / ("frame_%03d.png" % t))
    cdir, udir = str(tmp_path / "comp"), str(tmp_path / "out")
    compress.run(mdir, str(ddir), cdir, 0, 3, None, "abs", [0.0], True, False, True)
    decompress.run(mdir, cdir, udir, True, False)
    got = np.stack([np.array(Image.open(os.path.join(udir, "frame_%03d.png" % t))) for t in range(5)])
    np.testing.assert_array_equal(got, frames)


if __name__ == "__main__":   # the child process of _child: the job named on the command line, results into an .npz
    spec_ = json.loads(sys.argv[1])
    spec_ = (spec_[0], tuple(tuple(s) if s is not None else None for s in spec_[1])) + tuple(spec_[2:])
    np.savez(sys.argv[2], **run_job(spec_))
