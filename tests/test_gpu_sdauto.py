"""`-c --sdelta auto` on a MI355X (definition TZ-SDA1, tezip_amd/sdauto.py): the plane layouts of k_size_count and k_size_bits
against their slow statement, tz_sdelta_probe against tz_encode + tz_<coder>_counts + tz_<coder>_encode under every layout field
for field, and the command line end to end against the three explicit jobs.  Integers throughout."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import devmem
from conftest import ROOT

pytestmark = pytest.mark.gpu

SMALL_STACKS = (3, 16, 32)
CODERS = ("huff", "huffr", "huffd")


def _model(seed=1):
    """Random weights whose integer predictions span a range and differ between the channels (tests/test_gpu_ratetarget.py)."""
    from tezip_amd.prednet import PredNetConfig
    cfg = PredNetConfig(stack_sizes=SMALL_STACKS)
    wts = cfg.init_weights(seed=seed, bias_scale=0.2)
    names = [n for n, _ in cfg.weight_shapes()]
    wts[names.index("ahat0/kernel")] = wts[names.index("ahat0/kernel")] * np.float32(6.0)
    wts[names.index("ahat0/bias")] = np.array([0.35, 0.5, 0.65], np.float32)
    return cfg, wts


@pytest.fixture(scope="module")
def ctx():
    from tezip_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------------------------------- 1. the kernels alone
# H == 1; W == 1; several frames inside one run of 256; rows that are no 16-byte groups; whole 16-byte rows (the row above as
# 16-byte loads); a frame of 16 470 elements: a chunk boundary (16 384 symbols) falls inside a row
SEAM_SHAPES = ((1, 1, 1), (3, 1, 7), (3, 5, 1), (2, 3, 5), (5, 21, 30), (3, 16, 32), (2, 61, 90))


def _stack(shape, kind, seed):
    """int16 (nt, H, W, 3) in [-255, 255].  "random": every plane symbol differs from its neighbours; "sparse": long equal
    stretches across run and chunk starts, and matches at both distances."""
    rng = np.random.default_rng(seed)
    q = rng.integers(-255, 256, tuple(shape) + (3,))
    if kind == "sparse":
        q = np.where(rng.random(q.shape) < 0.03, q, 0)
    return q.astype(np.int16)


def _lens(rng, dist, holes):
    from tezip_amd import ratetarget as rt
    lens = rng.integers(1, 13, rt.BINS + 8).astype(np.uint8)
    if holes:
        lens[rng.random(lens.size) < 0.3] = 0
    if not dist:
        lens[rt.BINS:] = 0
    return lens


@pytest.mark.parametrize("channels", [3, 1])
@pytest.mark.parametrize("shape", SEAM_SHAPES, ids=["x".join(str(v) for v in s) for s in SEAM_SHAPES])
def test_plane_seams_equal_their_slow_statement(ctx, shape, channels):
    from tezip_amd import ratetarget as rt
    from tezip_amd import sdauto
    rng = np.random.default_rng(sum(shape) + channels)
    saw_bad = False
    for kind in ("random", "sparse"):
        q = _stack(shape, kind, seed=shape[1] * 7 + len(kind))
        # device stacks 2 bytes off the 16-byte grid (an odd element offset) and on it
        views = [devmem.view(q, off) for off in (2, 0)]
        for offset in (True, False):
            want, want_bad = sdauto.count_of_plane(q, channels, offset)
            assert not want_bad and int(want[0].sum()) == q.size // 3 * channels
            if kind == "sparse" and q.size > 3000:
                assert want[1, rt.BINS:].any() and want[2, rt.BINS:].any(), "stretches at both distances"
            for where, buf in [("host", q)] + [("device", v) for v, _ in views]:
                got, bad = ctx.size_count_plane_buf(buf, shape, channels, offset)
                np.testing.assert_array_equal(got, want, err_msg="%s %s offset=%s %s" % (shape, kind, offset, where))
                assert not bad
            for dist in (0, 1, 3):
                for holes in (False, True):
                    lens = _lens(rng, dist, holes)
                    want_b = sdauto.bits_of_plane(q, lens, dist, channels, offset)
                    saw_bad |= want_b[2]
                    for where, buf in (("host", q), ("device", views[0][0])):
                        assert ctx.size_bits_plane_buf(buf, shape, lens, dist, channels, offset) == want_b, (shape, kind, offset, dist, holes, where)
        assert all(intact() for _, intact in views)
    assert saw_bad or q.size < 100      # a hole in the code meets a symbol present


def test_plane_seam_argument_errors(ctx):
    import ctypes as C
    from tezip_amd import _lib
    q = np.zeros(2 * 3 * 4 * 3, np.int16)
    counts = np.zeros((3, _lib.SIZE_BINS + 8), np.uint64)
    bad = C.c_int(0)
    f = ctx.lib.tz_size_count_plane_buf
    for nt, h, w, ch in ((2, 3, 4, 2), (2, 0, 4, 3), (2, 3, 0, 3), (-1, 3, 4, 3), (0, 3, 4, 3), (2, 3, 4, 0)):
        assert f(ctx.h, q.ctypes.data, nt, h, w, ch, 1, counts.ctypes.data, C.byref(bad)) == -1, (nt, h, w, ch)
    assert f(ctx.h, None, 2, 3, 4, 3, 1, counts.ctypes.data, C.byref(bad)) == -1
    with pytest.raises(_lib.TezipError):
        ctx.size_bits_plane_buf(q, (2, 3, 4), np.ones(_lib.SIZE_BINS + 8, np.uint8), 2)      # no such match distance
    with pytest.raises(ValueError):
        ctx.size_count_plane_buf(q, (2, 3, 5))
    assert ctx.size_count_plane_buf(q, (2, 3, 4), 3, True)[0][0, _lib.SIZE_BIAS + 1600] == q.size     # (a refused call leaves it usable)
    assert ctx.size_count_plane_buf(q, (2, 3, 4), 1, False)[0][0, _lib.SIZE_BIAS] == q.size // 3


# ------------------------------------------------------------------------------------------ 2. a probe is the real job
def _scene():
    from tezip_amd import synth
    return synth.translating_scene(5, 61, 90)     # 82 350 elements: 322 runs, 6 chunks, the last one ragged


def _blobs():
    from tezip_amd import synth
    return synth.moving_blobs(8, 64, 64)          # gray: three equal channels


def _rollout(ctx, frames, p, window):
    from tezip_amd import _lib
    cfg, wts = _model()
    ctx.load_model(cfg, wts)
    ctx.prepare(_lib.pad8(frames.shape[1]), _lib.pad8(frames.shape[2]), max_batch=4)
    key, _ = ctx.rollout(frames, p, window, None)
    return key


def _real(ctx, coder, bound, entropy):
    """what the job's chain reports in the layout in force: tz_encode (resident), tz_<coder>_counts, the host's choice,
    tz_<coder>_encode -- and the stream's words"""
    from tezip_amd import huff, huffd, huffr
    _, table, _ = ctx.encode("abs", [bound], entropy, payload="resident")
    counts, base = getattr(ctx, coder + "_counts")()
    if coder == "huffd":
        dist, lengths, costs = huffd.choose(counts)
        nbytes = ctx.huffd_encode(lengths, base, dist)
        A = counts.shape[1] - 8
    elif coder == "huffr":
        lengths = huffr.code_lengths(counts)
        dist, A = 3, counts.size - 8
        costs = (0, 0, huffd.cost_bits(counts, lengths))
        nbytes = ctx.huffr_encode(lengths, base)
    else:
        lengths = huff.code_lengths(counts)
        dist, A = 0, counts.size
        costs = (int((counts.astype(object) * lengths.astype(object)).sum()), 0, 0)
        nbytes = ctx.huff_encode(lengths, base)
    return {"A": A, "base": base, "dist": dist, "costs": tuple(int(c) for c in costs), "bytes": nbytes,
            "table_len": len(table) if entropy else -1}


def _fields(rec):
    return {"A": int(rec["A"]), "base": int(rec["base"]), "dist": int(rec["dist"]), "costs": tuple(int(c) for c in rec["cost_bits"]),
            "bytes": int(rec["bytes"]), "table_len": int(rec["table_len"])}


def _set_layout(ctx, mode):
    ctx.set_delta_plane(0)
    ctx.set_delta_stride(1 if mode == "channel" else 0)
    ctx.set_delta_plane(1 if mode == "plane" else 0)


PROBE_KS = (0, 4, 13)
PROBE_JOBS = {"colour": (_scene, 3), "gray_three_channels": (_blobs, 3), "gray_one_channel": (_blobs, 1)}


@pytest.mark.parametrize("quant", ["greedy", "lattice"])
@pytest.mark.parametrize("job", sorted(PROBE_JOBS))
def test_probe_equals_the_real_chain_under_every_layout(ctx, job, quant):
    from tezip_amd import huff, sdauto
    make, channels = PROBE_JOBS[job]
    frames = make()
    try:
        ctx.set_payload_channels(channels)
        ctx.set_quantiser(quant)
        _rollout(ctx, frames, 0, 2)
        n = frames.size // 3 * channels
        chosen = set()
        for k in PROBE_KS:
            for coder in CODERS:
                for entropy in ((True, False) if k == 4 else (True,)):
                    want = {}
                    for mode in sdauto.CANDIDATES:
                        if mode == "channel" and channels == 1:
                            continue
                        _set_layout(ctx, mode)
                        want[mode] = _real(ctx, coder, k / 2, entropy)
                        if mode != "plane":     # (tz_size_probe refuses the plane setting)
                            assert _fields(ctx.size_probe("abs", [k / 2], entropy, coder)) == want[mode]
                    # whatever spatial delta the context is set to, the probe neither reads nor changes it
                    for setting in sdauto.CANDIDATES:
                        if setting == "channel" and channels == 1:
                            continue
                        _set_layout(ctx, setting)
                        recs = ctx.sdelta_probe("abs", [k / 2], entropy, coder)
                        assert (ctx.get_delta_stride(), ctx.get_delta_plane()) == (int(setting == "channel"), int(setting == "plane"))
                        for mode, rec in zip(sdauto.CANDIDATES, recs):
                            if mode not in want:
                                assert int(rec["n"]) == 0 and not np.frombuffer(rec.tobytes(), np.uint8).any()
                                continue
                            assert _fields(rec) == want[mode], "%s k=%d %s entropy=%s: %s under %s" % (job, k, coder, entropy, mode, setting)
                            assert int(rec["n"]) == n and int(rec["bytes"]) == huff.body_bytes(n, int(rec["stream_words"]))
                    chosen.add(sdauto.choose(recs, coder)[0])
        print(job, quant, "chosen:", sorted(chosen))
    finally:
        _set_layout(ctx, "flat")
        ctx.set_payload_channels(3)
        ctx.set_quantiser("greedy")


def test_probe_honours_frame_bounds_and_leaves_a_resident_payload(ctx):
    import hashlib
    from tezip_amd import sdauto
    frames = _scene()
    try:
        _rollout(ctx, frames, 0, 2)
        bounds = [0.0, 3.0, 0.5, 6.0, 2.0]
        ctx.set_frame_bounds(bounds)
        want = {}
        for mode in sdauto.CANDIDATES:
            _set_layout(ctx, mode)
            want[mode] = _real(ctx, "huffd", 0.0, True)
        # (the plane payload and its stream are resident now)
        digest = lambda: hashlib.sha256(np.ascontiguousarray(ctx.payload_get(0, frames.size)).tobytes()).hexdigest()   # noqa: E731
        before, stream = digest(), ctx.huff_get(0, want["plane"]["bytes"]).copy()
        recs = ctx.sdelta_probe("abs", [0.0], True, "huffd")
        assert [_fields(r) for r in recs] == [want[m] for m in sdauto.CANDIDATES]
        assert digest() == before
        np.testing.assert_array_equal(ctx.huff_get(0, want["plane"]["bytes"]), stream)
        ctx.set_frame_bounds(None)
        assert [_fields(r) for r in ctx.sdelta_probe("abs", [0.0], True, "huffd")] != [want[m] for m in sdauto.CANDIDATES]
    finally:
        ctx.set_frame_bounds(None)
        _set_layout(ctx, "flat")


def test_probe_state_and_argument_errors():
    """call for call what tz_size_probe answers (tests/test_gpu_ratetarget.py)"""
    from tezip_amd import _lib
    c = _lib.Context(0)
    try:
        out, one = np.zeros(3, _lib.SIZE_DTYPE), np.zeros(1, _lib.SIZE_DTYPE)
        calls = []

        def both(mode, b0, b1, entropy, coder, null=False):
            a = c.lib.tz_sdelta_probe(c.h, mode, b0, b1, entropy, coder, None if null else out.ctypes.data)
            b = c.lib.tz_size_probe(c.h, mode, b0, b1, entropy, coder, None if null else one.ctypes.data)
            assert a == b, (mode, b0, b1, entropy, coder, null, a, b)
            calls.append(a)
            return a

        assert both(0, 2.0, 0.0, 1, 2) == -4   # no rollout
        _rollout(c, _blobs(), 0, 2)
        assert both(0, 2.0, 0.0, 1, 2) == 0
        assert both(0, 2.0, 0.0, 1, 2, null=True) == -1
        assert both(0, 2.0, 0.0, 1, 3) == -1    # no such coder
        assert both(0, 2.0, 0.0, 3, 2) == -1    # byte planes
        assert both(4, 2.0, 0.0, 1, 2) == -1
        assert both(0, float("nan"), 0.0, 1, 2) == -1
        assert both(1, -0.5, 0.0, 1, 2) == -1
        assert both(0, 2.0, 0.0, 1, 2) == 0     # a refused call leaves it usable
        c.set_payload_channels(1)
        assert both(0, 2.0, 0.0, 1, 2) == 0     # a gray stack
        assert int(out[1]["n"]) == 0 and int(out[0]["n"]) == int(out[2]["n"]) == 8 * 64 * 64
        _rollout(c, _scene(), 0, 2)
        assert both(0, 2.0, 0.0, 1, 2) == -1    # colour: refused as tz_encode refuses it
        with pytest.raises(_lib.TezipError, match="has colour"):
            c.sdelta_probe("abs", [2.0], True, "huffd")
        c.set_payload_channels(3)
        assert both(0, 2.0, 0.0, 1, 2) == 0
        c.set_delta_plane(1)                    # the one difference: the probe of all layouts does not read the setting
        assert c.lib.tz_sdelta_probe(c.h, 0, 2.0, 0.0, 1, 2, out.ctypes.data) == 0
        assert c.lib.tz_size_probe(c.h, 0, 2.0, 0.0, 1, 2, one.ctypes.data) == -6
    finally:
        c.close()


# ---------------------------------------------------------------------------------------------------------- 3. CLI
def _main(argv, capsys):
    """tezip.py's main in this process -> (exit status, stdout)"""
    from tezip_amd import tezip
    capsys.readouterr()
    code = 0
    try:
        tezip.main(tezip.build_parser().parse_args(argv))
    except SystemExit as e:
        code = e.code or 0
    return code, capsys.readouterr().out


@pytest.fixture(scope="module")
def jobs(tmp_path_factory):
    """{name: (model directory, image directory, names)} on disk once for the CLI tests"""
    from PIL import Image
    from tezip_amd import _lib, synth, weights
    root = tmp_path_factory.mktemp("sdauto_cli")
    cfg, wts = _model()
    out = {}
    for name, frames in (("scene", synth.translating_scene(8, 64, 80)), ("blobs", synth.moving_blobs(8, 64, 64))):
        mdir, ddir = str(root / (name + "_model")), root / (name + "_data")
        weights.save_model(mdir, cfg, wts, _lib.pad8(frames.shape[1]), _lib.pad8(frames.shape[2]))
        ddir.mkdir()
        names = ["f_%03d.png" % t for t in range(len(frames))]
        for t, n in enumerate(names):
            Image.fromarray(frames[t]).save(ddir / n)
        out[name] = (mdir, str(ddir), names)
    return out


def _read(directory, name):
    with open(os.path.join(directory, name), "rb") as f:
        return f.read()


JOB = ["-p", "0", "-w", "2"]
LINE = re.compile(r"^sdelta: auto -> (flat|channel|plane) \(bytes: flat (\d+|-), channel (\d+|-), plane (\d+|-)\)$", re.M)
CLI_CASES = {   # job, flags, poison
    "scene_lossless_huffd": ("scene", ["-m", "abs", "-b", "0", "--coder", "huffd"], False),
    "scene_abs6_huffr_report": ("scene", ["-m", "abs", "-b", "6", "--coder", "huffr", "--report", "--digests", "--key-coder", "huff"], True),
    "blobs_abs6_huffd": ("blobs", ["-m", "abs", "-b", "6", "--coder", "huffd"], False),
    "blobs_gray_lossless_huff": ("blobs", ["-m", "abs", "-b", "0", "--coder", "huff", "--gray", "--key-coder", "huffg"], False),
    "scene_psnr40_lattice_huffd": ("scene", ["--target-psnr", "40", "--coder", "huffd", "--quant", "lattice"], False),
}


@pytest.mark.parametrize("case", sorted(CLI_CASES))
def test_cli_auto_is_the_explicit_job_of_the_smallest_file(tmp_path, capsys, monkeypatch, jobs, case):
    job, flags, poison = CLI_CASES[case]
    mdir, ddir, names = jobs[job]
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    dirs, size = {}, {}
    for mode in ("flat", "channel", "plane", "auto"):
        dirs[mode] = str(tmp_path / mode)
        code, out = _main(["-c", mdir, ddir, dirs[mode]] + JOB + flags + ["--sdelta", mode], capsys)
        assert code == 0, out
        assert (len(LINE.findall(out)) == 1) == (mode == "auto"), out
        size[mode] = os.path.getsize(os.path.join(dirs[mode], "entropy.dat"))
    chosen, *printed = LINE.search(out).groups()
    gray = "--gray" in flags
    print(case, "->", chosen, size)
    # the printed sizes are the three files' sizes; on a one-channel payload channel is no candidate (its job is the flat job)
    assert printed == [str(size["flat"]), "-" if gray else str(size["channel"]), str(size["plane"])]
    if gray:
        assert _read(dirs["channel"], "entropy.dat") == _read(dirs["flat"], "entropy.dat")
    # the smallest, a tie to the earlier; every file is the chosen explicit job's
    order = [m for m in ("flat", "channel", "plane") if not (gray and m == "channel")]
    assert chosen == min(order, key=lambda m: (size[m], order.index(m)))
    assert size["auto"] == size[chosen] <= min(size[m] for m in order)
    assert sorted(os.listdir(dirs["auto"])) == sorted(os.listdir(dirs[chosen])) and "entropy.dat" in os.listdir(dirs["auto"])
    for n in os.listdir(dirs[chosen]):
        assert _read(dirs["auto"], n) == _read(dirs[chosen], n), n
    # the chosen mode's own line follows the choice
    follow = {"flat": None, "channel": "sdelta: channel (stride 3)", "plane": "sdelta: plane (TZ-SD2)"}[chosen]
    lines = out.splitlines()
    at = next(i for i, ln in enumerate(lines) if LINE.match(ln))
    assert (lines[at + 1] == follow) if follow else not any(ln.startswith("sdelta:") for ln in lines[at + 1:])
    # -u needs nothing new: the images are the flat job's
    u_auto, u_flat = str(tmp_path / "u_auto"), str(tmp_path / "u_flat")
    for src, dst in ((dirs["auto"], u_auto), (dirs["flat"], u_flat)):
        code, text = _main(["-u", mdir, src, dst], capsys)
        assert code == 0, text
    assert sorted(os.listdir(u_auto)) == names
    for n in names:
        assert _read(u_auto, n) == _read(u_flat, n), n
    if poison:   # TEZIP_POISON is read once per process: a fresh child writes the same files from poisoned scratch
        pdir = str(tmp_path / "poison")
        r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m", "tezip_amd.tezip", "-c", mdir, ddir, pdir] + JOB + flags
                           + ["--sdelta", "auto"], cwd=ROOT, capture_output=True, text=True, env=dict(os.environ, TEZIP_POISON="170"),
                           timeout=330)
        assert r.returncode == 0, r.stdout + r.stderr
        assert LINE.search(r.stdout).group(0) == LINE.search(out).group(0)
        for n in os.listdir(dirs["auto"]):
            assert _read(pdir, n) == _read(dirs["auto"], n), n
