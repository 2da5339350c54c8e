"""`-c --target-ratio` on a MI355X (definition TZ-TRATIO-1, tezip_amd/ratetarget.py): k_size_count and k_size_bits against their
slow statements, tz_size_probe against tz_encode + tz_<coder>_counts + tz_<coder>_encode field for field, and the command line end
to end.  Integers throughout."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

SMALL_STACKS = (3, 16, 32)
LAYOUTS = {"flat": (3, 1), "gray": (1, 1), "channel": (3, 3)}
CODERS = ("huff", "huffr", "huffd")


def _model(seed=1):
    """Random weights whose integer predictions span a range and differ between the channels (tests/test_gpu_target.py)."""
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


def _scene():
    from tezip_amd import synth
    return synth.translating_scene(5, 61, 90)     # 82 350 elements: 322 runs, 6 chunks, the last one ragged


def _blobs():
    from tezip_amd import synth
    return synth.moving_blobs(8, 64, 64)          # gray: three equal channels


# ------------------------------------------------------------------------------------------- 1. the kernels alone
def _stack(n, layout, kind, seed):
    """An int16 stack that yields n symbols in the layout.  kind "random": deltas in [-255, 255]; "runs": symbols with long
    equal stretches (also across run starts and chunk starts), built by undoing the spatial delta; "far": one symbol outside
    the bins."""
    channels, stride = LAYOUTS[layout]
    rng = np.random.default_rng(seed)
    nq = n * (3 if channels == 1 else 1)
    if kind == "runs":
        m = n // 50 + 2
        sym = np.repeat(rng.integers(-4, 5, m), rng.integers(1, 700, m))          # sd values; y = 1600 - sd
        sym = np.r_[sym, np.zeros(n, np.int64)][:n].astype(np.int64)
        x = np.zeros(n, np.int64)
        for c in range(min(stride, n)):
            x[c::stride] = -np.cumsum(sym[c::stride])
            x[c::stride] += 2 * sym[c]                                              # (x[c] = sd[c] at the stream start)
        x = ((x + 32768) % 65536 - 32768).astype(np.int16)
        if channels == 1:
            q = rng.integers(-255, 256, nq).astype(np.int16)
            q[0::3] = x
            return q
        return x
    q = rng.integers(-255, 256, nq).astype(np.int16)
    if kind == "far":
        q[(nq // 2) // 3 * 3] = 9000
    return q


def _lens(rng, dist, holes=False):
    from tezip_amd import ratetarget as rt
    lens = rng.integers(1, 13, rt.BINS + 8).astype(np.uint8)
    if holes:
        lens[rng.random(lens.size) < 0.3] = 0
    if not dist:
        lens[rt.BINS:] = 0
    return lens


SEAM_LENGTHS = (1, 7, 255, 256, 257, 16383, 16385)


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("n", SEAM_LENGTHS)
def test_seams_equal_their_slow_statements(ctx, layout, n):
    import torch
    from tezip_amd import ratetarget as rt
    channels, stride = LAYOUTS[layout]
    rng = np.random.default_rng(n)
    for kind in ("random", "runs", "far"):
        q = _stack(n, layout, kind, seed=n * 7 + len(kind))
        for offset in (True, False):
            want, want_bad = rt.count_of(q, channels, stride, offset)
            assert want_bad == (kind == "far")
            if kind == "runs" and n > 600:
                assert want[1, rt.BINS + 7] > 0 and want[2, rt.BINS + 7] > 0, "stretches that only a run start cuts"
            got, bad = ctx.size_count_buf(q, channels, stride, offset)
            np.testing.assert_array_equal(got, want, err_msg="%s %s offset=%s" % (layout, kind, offset))
            assert bad == want_bad
            # a device stack off the 16-byte grid (2 and 6 bytes in) and on it
            for off in (1, 3, 8):
                t = torch.zeros(q.size + 16, dtype=torch.int16, device="cuda")
                t[off: off + q.size] = torch.from_numpy(q).cuda()
                torch.cuda.synchronize()
                got, bad = ctx.size_count_buf(t[off: off + q.size], channels, stride, offset)
                np.testing.assert_array_equal(got, want, err_msg="%s %s offset=%s device +%d" % (layout, kind, offset, off))
                assert bad == want_bad
            for dist in (0, 1, 3):
                for holes in (False, True):
                    lens = _lens(rng, dist, holes)
                    want_b = rt.bits_of(q, lens, dist, channels, stride, offset)
                    assert ctx.size_bits_buf(q, lens, dist, channels, stride, offset) == want_b, (layout, kind, offset, dist, holes)
                    t = torch.zeros(q.size + 16, dtype=torch.int16, device="cuda")
                    t[1: 1 + q.size] = torch.from_numpy(q).cuda()
                    torch.cuda.synchronize()
                    assert ctx.size_bits_buf(t[1: 1 + q.size], lens, dist, channels, stride, offset) == want_b
                    if kind == "far" and not holes:
                        assert want_b[2]       # the symbol outside the bins has no code


def test_seam_argument_errors(ctx):
    from tezip_amd import _lib
    q = np.zeros(12, np.int16)
    counts = np.zeros((3, _lib.SIZE_BINS + 8), np.uint64)
    import ctypes as C
    bad = C.c_int(0)
    for channels, stride in ((1, 3), (2, 1), (3, 2), (3, 0)):
        assert ctx.lib.tz_size_count_buf(ctx.h, q.ctypes.data, 12, channels, stride, 1, counts.ctypes.data, C.byref(bad)) == -1
    assert ctx.lib.tz_size_count_buf(ctx.h, q.ctypes.data, 11, 1, 1, 1, counts.ctypes.data, C.byref(bad)) == -1     # no whole pixels
    assert ctx.lib.tz_size_count_buf(ctx.h, q.ctypes.data, 0, 3, 1, 1, counts.ctypes.data, C.byref(bad)) == -1
    assert ctx.lib.tz_size_count_buf(ctx.h, None, 12, 3, 1, 1, counts.ctypes.data, C.byref(bad)) == -1
    with pytest.raises(_lib.TezipError):
        ctx.size_bits_buf(q, np.ones(_lib.SIZE_BINS + 8, np.uint8), 2)      # no such match distance
    assert ctx.size_count_buf(q, 3, 1, True)[0][0, _lib.SIZE_BIAS + 1600] == 12     # (a refused call leaves it usable)


# ------------------------------------------------------------------------------------------ 2. a probe is the real job
def _rollout(ctx, frames, p, window):
    from tezip_amd import _lib
    cfg, wts = _model()
    ctx.load_model(cfg, wts)
    ctx.prepare(_lib.pad8(frames.shape[1]), _lib.pad8(frames.shape[2]), max_batch=4)
    key, _ = ctx.rollout(frames, p, window, None)
    return key


def _real(ctx, coder, bound, entropy):
    """what the job's chain reports: tz_encode (resident), tz_<coder>_counts, the host's choice, tz_<coder>_encode"""
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
            "table_len": len(table) if entropy else -1}, table


def _digest(ctx, n):
    return hashlib.sha256(np.ascontiguousarray(ctx.payload_get(0, n)).tobytes()).hexdigest()


PROBE_KS = (0, 1, 4, 13, 127, 510)
# job -> (layout, frames).  flat_aligned: frames of the padded size with whole 16-byte groups, where tz_encode quantises in its fused
# pass and the probe in the general one
PROBE_JOBS = {"flat": ("flat", _scene), "flat_aligned": ("flat", _blobs), "gray": ("gray", _blobs), "channel": ("channel", _scene)}


@pytest.mark.parametrize("job", sorted(PROBE_JOBS))
def test_probe_equals_encode_counts_and_encode(ctx, job):
    from tezip_amd import huff
    from tezip_amd import ratetarget as rt
    layout, make = PROBE_JOBS[job]
    channels, stride = LAYOUTS[layout]
    frames = make()
    try:
        ctx.set_payload_channels(channels)
        ctx.set_delta_stride(1 if stride == 3 else 0)
        _rollout(ctx, frames, 0, 2)
        n = frames.size // 3 * channels
        dists = set()
        for k in PROBE_KS:
            for coder in CODERS:
                for entropy in ((True, False) if k in (0, 13) else (True,)):
                    want, table = _real(ctx, coder, k / 2, entropy)
                    before, stream = _digest(ctx, n), ctx.huff_get(0, want["bytes"]).copy()
                    rec = ctx.size_probe("abs", [k / 2], entropy, coder)
                    got = {"A": int(rec["A"]), "base": int(rec["base"]), "dist": int(rec["dist"]),
                           "costs": tuple(int(c) for c in rec["cost_bits"]), "bytes": int(rec["bytes"]), "table_len": int(rec["table_len"])}
                    assert got == want, "%s k=%d %s entropy=%s" % (layout, k, coder, entropy)
                    assert int(rec["n"]) == n and int(rec["bytes"]) == huff.body_bytes(n, int(rec["stream_words"]))
                    # every other candidate and coder leaves what is resident as it found it
                    for other in CODERS:
                        ctx.size_probe("abs", [(k + 7) / 2], entropy, other)
                    assert _digest(ctx, n) == before
                    np.testing.assert_array_equal(ctx.huff_get(0, want["bytes"]), stream)
                    # (still resident: the encoder's state is untouched)
                    assert len(ctx.encode_quality("resident", table if entropy else None)) == len(frames)
                    dists.add((coder, got["dist"]))
                    trailer = rt.trailer_len(got["table_len"])
                    assert rt.file_bytes(rec, coder) == 48 + (trailer * 2 + 3) // 4 * 4 + (got["A"] + (0 if coder == "huff" else 8) + 3) // 4 * 4 + got["bytes"]
        print(layout, sorted(dists))
    finally:
        ctx.set_payload_channels(3)
        ctx.set_delta_stride(0)


def test_probe_state_and_argument_errors():
    from tezip_amd import _lib
    c = _lib.Context(0)
    try:
        out = np.zeros(1, _lib.SIZE_DTYPE)
        assert c.lib.tz_size_probe(c.h, 0, 2.0, 0.0, 1, 2, out.ctypes.data) == -4   # no rollout
        _rollout(c, _blobs(), 0, 2)
        assert c.lib.tz_size_probe(c.h, 0, 2.0, 0.0, 1, 2, out.ctypes.data) == 0
        assert c.lib.tz_size_probe(c.h, 0, 2.0, 0.0, 1, 2, None) == -1
        assert c.lib.tz_size_probe(c.h, 0, 2.0, 0.0, 1, 3, out.ctypes.data) == -1    # no such coder
        assert c.lib.tz_size_probe(c.h, 0, 2.0, 0.0, 3, 2, out.ctypes.data) == -1    # byte planes
        assert c.lib.tz_size_probe(c.h, 4, 2.0, 0.0, 1, 2, out.ctypes.data) == -1
        assert c.lib.tz_size_probe(c.h, 0, float("nan"), 0.0, 1, 2, out.ctypes.data) == -1
        assert c.lib.tz_size_probe(c.h, 1, -0.5, 0.0, 1, 2, out.ctypes.data) == -1
        assert c.lib.tz_size_probe(c.h, 0, 2.0, 0.0, 1, 2, out.ctypes.data) == 0     # a refused call leaves it usable
        c.set_payload_channels(1)
        assert c.lib.tz_size_probe(c.h, 0, 2.0, 0.0, 1, 2, out.ctypes.data) == 0     # a gray stack
        _rollout(c, _scene(), 0, 2)
        assert c.lib.tz_size_probe(c.h, 0, 2.0, 0.0, 1, 2, out.ctypes.data) == -1    # colour: refused as tz_encode refuses it
        with pytest.raises(_lib.TezipError, match="has colour"):
            c.encode("abs", [2.0], True, payload="resident")
        c.set_payload_channels(3)
        assert c.lib.tz_size_probe(c.h, 0, 2.0, 0.0, 1, 2, out.ctypes.data) == 0
    finally:
        c.close()


# ---------------------------------------------------------------------------------------------------------- 3. CLI
def _cli(args, timeout=300, env=None):
    return subprocess.run(["timeout", "-k", "10", str(timeout), sys.executable, "-m", "tezip_amd.tezip"] + args, cwd=ROOT,
                          capture_output=True, text=True, timeout=timeout + 30, env=dict(os.environ, **(env or {})))


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
    """{name: (model directory, image directory, names, frames)} on disk once for the CLI tests"""
    from PIL import Image
    from tezip_amd import _lib, weights
    root = tmp_path_factory.mktemp("ratio_cli")
    cfg, wts = _model()
    out = {}
    for name, frames in (("scene", _scene()), ("blobs", _blobs())):
        mdir, ddir = str(root / (name + "_model")), root / (name + "_data")
        weights.save_model(mdir, cfg, wts, _lib.pad8(frames.shape[1]), _lib.pad8(frames.shape[2]))
        ddir.mkdir()
        names = ["f_%03d.png" % t for t in range(len(frames))]
        for t, n in enumerate(names):
            Image.fromarray(frames[t]).save(ddir / n)
        out[name] = (mdir, str(ddir), names, frames)
    return out


JOB = ["-p", "0", "-w", "2"]
FILES = ("filename.txt", "key_frame.dat", "entropy.dat")


def _total(directory):
    return sum(os.path.getsize(os.path.join(directory, n)) for n in FILES)


def _images(directory, names):
    from PIL import Image
    return np.stack([np.asarray(Image.open(os.path.join(directory, n)).convert("RGB")) for n in names])


CLI_CASES = {   # job, flags
    "scene_huffd": ("scene", ["--coder", "huffd"]),
    "scene_huff_channel_keyhuff": ("scene", ["--coder", "huff", "--sdelta", "channel", "--key-coder", "huff"]),
    "blobs_huffr_gray_keyhuffg": ("blobs", ["--coder", "huffr", "--gray", "--key-coder", "huffg"]),
}


@pytest.mark.parametrize("case", sorted(CLI_CASES))
def test_cli_target_ratio_is_the_abs_job_it_finds(tmp_path, capsys, jobs, case):
    from tezip_amd import ratetarget as rt
    job, flags = CLI_CASES[case]
    mdir, ddir, names, frames = jobs[job]
    flags = flags + ["--report", "--digests"]
    # a target between what the lossless job and the loosest job take
    sizes = {}
    for b in ("0", "255"):
        code, out = _main(["-c", mdir, ddir, str(tmp_path / ("plain" + b))] + JOB + ["-m", "abs", "-b", b] + flags, capsys)
        assert code == 0, out
        sizes[b] = _total(str(tmp_path / ("plain" + b)))
    assert sizes["255"] < sizes["0"]
    R = frames.size / ((sizes["0"] + sizes["255"]) / 2.0)
    found, plain = str(tmp_path / "comp_t"), str(tmp_path / "comp")
    code, out = _main(["-c", mdir, ddir, found] + JOB + ["--target-ratio", repr(R)] + flags, capsys)
    assert code == 0, out
    doc = json.load(open(os.path.join(found, "bound_search.json")))
    assert [ln for ln in out.splitlines() if ln.startswith("target: ")] == [rt.stdout_line(doc)] and "abs" in out.splitlines()
    budget = rt.budget(frames.size, R)
    fixed = sum(os.path.getsize(os.path.join(found, n)) for n in FILES[:2])
    k = doc["result"]["k"]
    print(case, "R = %.4f" % R, "k =", k, [(t["k"], t["entropy_bytes"], t["pass"]) for t in doc["trace"]])
    assert (doc["definition"], doc["target_ratio"], doc["raw_bytes"], doc["budget_bytes"], doc["fixed_bytes"]) == \
        ("TZ-TRATIO-1", R, frames.size, budget, fixed)
    assert 1 <= k <= 509 and doc["result"]["bound"] == k / 2 and doc["probes"] == len(doc["trace"]) <= 11
    assert all(t["pass"] == (fixed + t["entropy_bytes"] <= budget) and t["bound"] == t["k"] / 2 for t in doc["trace"])
    by_k = {t["k"]: t for t in doc["trace"]}
    assert by_k[k]["pass"] and not by_k[k - 1]["pass"]                                   # the guarantee
    passing = [t for t in doc["trace"] if t["pass"]]
    assert passing[-1]["k"] == k and os.path.getsize(os.path.join(found, "entropy.dat")) == passing[-1]["entropy_bytes"] == doc["result"]["entropy_bytes"]
    assert by_k[0]["entropy_bytes"] == os.path.getsize(str(tmp_path / "plain0" / "entropy.dat"))
    assert by_k[510]["entropy_bytes"] == os.path.getsize(str(tmp_path / "plain255" / "entropy.dat"))
    code, out = _main(["-c", mdir, ddir, plain] + JOB + ["-m", "abs", "-b", repr(k / 2)] + flags, capsys)
    assert code == 0, out
    assert sorted(os.listdir(plain)) == ["entropy.dat", "filename.txt", "frame_digests.json", "key_frame.dat", "quality.json", "tezip_amd.json"]
    assert sorted(os.listdir(found)) == sorted(os.listdir(plain) + ["bound_search.json"])
    for n in os.listdir(plain):
        assert open(os.path.join(found, n), "rb").read() == open(os.path.join(plain, n), "rb").read(), n
    quality = json.load(open(os.path.join(found, "quality.json")))
    assert quality["ratio"] >= R and _total(found) <= budget
    udir = str(tmp_path / "dec_t")
    code, out = _main(["-u", mdir, found, udir, "--verify", "require"], capsys)
    assert code == 0 and "verified: %d frames" % len(names) in out, out
    assert sorted(os.listdir(udir)) == names
    assert int(np.abs(_images(udir, names).astype(np.int64) - frames).max()) == quality["max_abs_err"]


def test_cli_ratio_one_is_lossless_in_one_probe(tmp_path, capsys, jobs):
    mdir, ddir, names, frames = jobs["blobs"]    # mostly black: the lossless job is smaller than the frames
    found, udir = str(tmp_path / "comp"), str(tmp_path / "dec")
    code, out = _main(["-c", mdir, ddir, found] + JOB + ["--target-ratio", "1", "--coder", "huffd"], capsys)
    assert code == 0, out
    doc = json.load(open(os.path.join(found, "bound_search.json")))
    assert doc["result"]["k"] == 0 and doc["probes"] == 1 and doc["trace"][0]["pass"] and _total(found) <= frames.size
    assert "target: ratio >= 1 -> abs bound 0 (1 probes, " in out
    assert os.path.getsize(os.path.join(found, "entropy.dat")) == doc["result"]["entropy_bytes"]
    code, out = _main(["-u", mdir, found, udir], capsys)
    assert code == 0, out
    np.testing.assert_array_equal(_images(udir, names), frames)


def test_cli_unreachable_target_and_poison(tmp_path, jobs):
    """through the command line proper: the exit status of a target that cannot be met, and the same search whatever the
    scratch held"""
    mdir, ddir, names, frames = jobs["scene"]
    gone = str(tmp_path / "comp_x")
    r = _cli(["-c", mdir, ddir, gone] + JOB + ["--target-ratio", "100000", "--coder", "huffd"])
    assert r.returncode == 4, r.stdout + r.stderr
    doc = json.load(open(os.path.join(gone, "bound_search.json")))
    assert doc["result"] is None and doc["probes"] == 2 and [t["k"] for t in doc["trace"]] == [0, 510] and doc["budget_bytes"] == frames.size // 100000
    total = doc["fixed_bytes"] + doc["trace"][1]["entropy_bytes"]
    assert "ERROR: --target-ratio 100000 cannot be met: at abs 255 the files take %d bytes (ratio " % total in r.stdout
    assert sorted(os.listdir(gone)) == ["bound_search.json", "filename.txt", "key_frame.dat"]
    docs = []
    for name, env in (("a", {}), ("b", {"TEZIP_POISON": "0xA5"})):
        out = str(tmp_path / ("comp_" + name))
        r = _cli(["-c", mdir, ddir, out] + JOB + ["--target-ratio", "3", "--coder", "huffd", "--sdelta", "channel"], env=env)
        assert r.returncode in (0, 4), r.stdout + r.stderr
        docs.append(open(os.path.join(out, "bound_search.json"), "rb").read())
    assert docs[0] == docs[1] and len(json.loads(docs[0])["trace"]) >= 2
