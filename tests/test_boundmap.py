"""One abs bound per pixel on the CPU (tezip_amd/boundmap.py, `-c -m abs --bound-map FILE`; definition TZ-BM1): the slow
statement against the oracle's pwrel walk with the map in place of the originals, the properties of the definition, the
loader, the command line's refusals and the check tool."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as O
from tezip_amd import boundmap as bm
from tezip_amd import lattice

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 21, 30


def _stacks(h=H, w=W):
    """int16 deltas: slow triangle ramps, the same with jitter, and the full range (the stacks of the GPU seam tests)"""
    n = h * w
    i = np.arange(n)
    rng = np.random.default_rng(h * 1000 + w)
    frames = []
    for f, (period, step) in enumerate(((10, 1), (7, 1), (23, 2), (3, 1))):
        tri = np.abs(((i // period) * step % 400) - 200) - 100
        jit = rng.integers(-4, 5, n)
        wide = rng.integers(-255, 256, n)
        frames.append(np.stack([tri, np.clip(2 * tri + jit, -255, 255), wide if f % 2 else -tri], axis=-1).reshape(h, w, 3))
    return np.stack(frames).astype(np.int16)


def maps(h=H, w=W, seed=5):
    rng = np.random.default_rng(seed)
    roi = np.full((h, w), 6, np.uint8)
    roi[5:18, 3:23] = 0
    wide = np.full((h, w), 255, np.uint8)
    wide[:, w // 3] = 0
    return {"uniform2": np.full((h, w), 2, np.uint8), "roi": roi, "random": rng.integers(0, 9, (h, w)).astype(np.uint8), "wide": wide}


# ------------------------------------------------------------------------------------- 1. the quantiser against the oracle
@pytest.mark.parametrize("name", sorted(maps()))
def test_greedy_is_the_oracles_pwrel_walk_over_the_map(name):
    from oracle import coracle
    M, diff = maps()[name], _stacks()
    got = bm.quantise(diff, M, quant="greedy")
    T3 = np.ascontiguousarray(np.repeat(M[..., None], 3, axis=-1))
    for f in range(len(diff)):
        np.testing.assert_array_equal(got[f], coracle.error_bound_frame(T3, diff[f], "pwrel", [1.0]), err_msg="frame %d" % f)
        for c in range(3):
            np.testing.assert_array_equal(got[f, :, :, c], O.error_bound(M, diff[f, :, :, c], "pwrel", (1.0,)), err_msg="slab %d %d" % (f, c))
    assert (got != diff).any()


def test_skipped_frames_are_left_alone():
    M, diff = maps()["random"], _stacks()
    for quant in bm.QUANTS:
        got = bm.quantise(diff, M, skip=[0, 1, 0, 1], quant=quant)
        np.testing.assert_array_equal(got[[1, 3]], diff[[1, 3]])
        np.testing.assert_array_equal(got[[0, 2]], bm.quantise(diff, M, quant=quant)[[0, 2]])


# ------------------------------------------------------------------------------------------ 2. properties of the definition
@pytest.mark.parametrize("k", [1, 2, 7, 63, 255])
def test_a_uniform_map_is_abs_k(k):
    diff = _stacks()
    M = np.full((H, W), k, np.uint8)
    got = bm.quantise(diff, M, quant="greedy")
    for f in range(len(diff)):
        for c in range(3):
            np.testing.assert_array_equal(got[f, :, :, c], O.error_bound(M, diff[f, :, :, c], "abs", (float(k),)))
    np.testing.assert_array_equal(bm.quantise(diff, M, quant="lattice"), lattice.quantise_stack(np.zeros(diff.shape, np.uint8), diff, "abs", [float(k)]))


def test_a_zero_map_is_the_identity():
    diff = _stacks()
    for quant in bm.QUANTS:
        np.testing.assert_array_equal(bm.quantise(diff, np.zeros((H, W), np.uint8), quant=quant), diff)


@pytest.mark.parametrize("quant", bm.QUANTS)
def test_every_sample_is_within_its_pixels_tolerance(quant):
    diff = _stacks()
    cases = [np.random.default_rng(s).integers(0, 9, (H, W)).astype(np.uint8) for s in range(4)] + [maps()["wide"], maps()["roi"]]
    for M in cases:
        q = bm.quantise(diff, M, quant=quant).astype(np.int64)
        err = np.abs(q - diff)
        assert (err <= M[None, :, :, None]).all()
        np.testing.assert_array_equal(q[:, M == 0], diff[:, M == 0])          # M = 0: exact
        assert err.max() > 0


def test_check_counts_samples_and_excess():
    rng = np.random.default_rng(3)
    orig = rng.integers(0, 256, (3, H, W, 3)).astype(np.uint8)
    M = maps()["random"]
    dec = np.clip(orig.astype(np.int64) + rng.integers(-1, 2, orig.shape) * M[None, :, :, None], 0, 255).astype(np.uint8)
    assert all(r == {"violations": 0, "max_excess": 0} for r in bm.check(orig, dec, M))
    bad = dec.copy()
    y, x = np.argwhere(M == 0)[0]
    bad[1, y, x, 2] = orig[1, y, x, 2] ^ 4                                      # an exact pixel off by 4
    rec = bm.check(orig, bad, M)
    assert rec[1] == {"violations": 1, "max_excess": 4} and rec[0]["violations"] == 0 and rec[2]["violations"] == 0


# --------------------------------------------------------------------------------------------------------- 3. the loader
def _png(path, arr):
    from PIL import Image
    Image.fromarray(arr).save(path)
    return str(path)


def test_loader_accepts_npy_gray_png_and_equal_channels(tmp_path):
    M = maps()["roi"]
    np.save(tmp_path / "m.npy", M)
    for path in (str(tmp_path / "m.npy"), _png(tmp_path / "g.png", M), _png(tmp_path / "rgb.png", np.repeat(M[..., None], 3, axis=-1))):
        got = bm.load(path, H, W)
        assert got.dtype == np.uint8 and got.flags["C_CONTIGUOUS"]
        np.testing.assert_array_equal(got, M)
    assert bm.stdout_line(M) == "bound map: 21x30, abs 0..6, %.1f %% of pixels exact" % (100.0 * 13 * 20 / (H * W))
    assert bm.stats(M) == {"max": 6, "exact_pixels": 260}


def test_loader_refusals_name_file_and_rule(tmp_path):
    M = maps()["roi"]
    colour = np.repeat(M[..., None], 3, axis=-1)
    colour[2, 2, 1] += 1
    np.save(tmp_path / "f.npy", M.astype(np.float32))
    np.save(tmp_path / "d3.npy", colour)
    np.save(tmp_path / "ok.npy", M)
    cases = [(_png(tmp_path / "c.png", colour), None, "colour"), (str(tmp_path / "f.npy"), None, "uint8"), (str(tmp_path / "d3.npy"), None, "2-D"),
             (str(tmp_path / "ok.npy"), (H, W + 1), "own size"), (str(tmp_path / "none.png"), None, "cannot be read")]
    for path, size, word in cases:
        with pytest.raises(ValueError) as e:
            bm.load(path, *(size or (None, None)))
        assert path in str(e.value) and word in str(e.value), str(e.value)


# --------------------------------------------------------------------------------------------------------- 4. refusals
JOB = ["-c", "m", "d", "o", "-p", "0", "-w", "4"]
GOOD, BAD = "@good@", "@bad@"


@pytest.mark.parametrize("argv,env,word", [
    (["-u", "m", "c", "d", "--bound-map", GOOD], {}, "-c"),
    (["-l", "m", "d", "--bound-map", GOOD], {}, "-c"),
    (["-c", "m", "d", "o", "-p", "0", "-m", "abs", "--sweep", "4", "8", "--bound-map", GOOD], {}, "--sweep"),
    (JOB + ["-m", "abs", "--bound-map", GOOD], {"WORLD_SIZE": "2"}, "sharded"),
    (JOB + ["-m", "abs", "-b", "2", "--bound-map", GOOD], {}, "-b"),
    (JOB + ["-m", "abs", "--bound-map", GOOD, "--frame-bounds", "x.json"], {}, "--frame-bounds"),
    (JOB + ["--bound-map", GOOD, "--target-psnr", "40"], {}, "--target-psnr"),
    (JOB + ["--bound-map", GOOD, "--target-ratio", "4", "--coder", "huffd"], {}, "--target-ratio"),
    (JOB + ["--bound-map", GOOD, "--target-psnr", "40", "--per-frame"], {}, "--per-frame"),
    (JOB + ["-m", "rel", "--bound-map", GOOD], {}, "-m abs"),
    (JOB + ["-m", "pwrel", "--bound-map", GOOD], {}, "-m abs"),
    (JOB + ["--bound-map", GOOD], {}, "-m abs"),
    (JOB + ["-m", "abs", "--bound-map", BAD], {}, "colour"),
    (JOB + ["-m", "abs", "--bound-map", "@missing@"], {}, "cannot be read"),
])
def test_cli_refusals(monkeypatch, capsys, tmp_path, argv, env, word):
    from tezip_amd import tezip
    M = maps()["roi"]
    np.save(tmp_path / "good.npy", M)
    colour = np.repeat(M[..., None], 3, axis=-1)
    colour[0, 0, 0] = 9
    names = {GOOD: str(tmp_path / "good.npy"), BAD: _png(tmp_path / "bad.png", colour), "@missing@": str(tmp_path / "missing.npy")}
    argv = [names.get(a, a) for a in argv]
    arg = tezip.build_parser().parse_args(argv)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setattr(tezip, "probe_gpu", lambda force: pytest.fail("refused before a GPU is touched"))
    with pytest.raises(SystemExit) as e:
        tezip.main(arg)
    out = capsys.readouterr().out
    assert e.value.code == 2 and out.startswith("ERROR:") and word in out and len(out.strip().splitlines()) == 1, out
    if names[BAD] in argv or names["@missing@"] in argv:
        assert argv[-1] in out          # the message names the file


def test_the_flag_reaches_run_with_every_other_flag(monkeypatch, capsys, tmp_path):
    from tezip_amd import compress, tezip
    np.save(tmp_path / "good.npy", maps()["roi"])
    good = str(tmp_path / "good.npy")
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    seen = {}
    monkeypatch.setattr(compress, "run", lambda *a, **kw: seen.update(kw, args=a))
    monkeypatch.setattr(tezip, "probe_gpu", lambda force: True)
    tezip.main(tezip.build_parser().parse_args(JOB + ["-m", "abs", "--bound-map", good, "--quant", "lattice", "--coder", "huffd", "--key-coder", "huffg",
                                                      "--gray", "--sdelta", "auto", "--report", "--ssim", "--digests", "-n"]))
    assert seen["BOUND_MAP"] == good and seen["QUANT"] == "lattice" and seen["CODER"] == "huffd" and seen["SDELTA"] == "auto"
    assert seen["args"][6:8] == ("abs", []) and seen["REPORT"] and seen["SSIM"] and seen["DIGESTS"] and seen["GRAY"]
    assert "abs" in capsys.readouterr().out.splitlines()          # printed where the reference prints the mode
    seen.clear()
    tezip.main(tezip.build_parser().parse_args(JOB + ["-m", "abs", "-b", "2"]))      # the job without the flag is the call it was
    assert "BOUND_MAP" not in seen


def test_a_direct_caller_of_run_is_refused(monkeypatch, capsys, tmp_path):
    from tezip_amd import compress
    M = maps()["roi"]
    monkeypatch.setattr(compress, "make_context", lambda *a, **k: pytest.fail("refused before a GPU is touched"))
    run = lambda mode, bound, **kw: compress.run("m", str(tmp_path), str(tmp_path / "o"), 0, 4, None, mode, bound, True, False, True, **kw)  # noqa: E731
    cases = [
        (("abs", [2.0]), dict(BOUND_MAP=M), "-b"),
        (("rel", []), dict(BOUND_MAP=M), "-m abs"),
        (("abs", []), dict(BOUND_MAP=M, TARGET_PSNR=40.0), "--target-psnr"),
        (("abs", []), dict(BOUND_MAP=M, FRAME_BOUNDS=[0, 1]), "--frame-bounds"),
        (("abs", []), dict(BOUND_MAP=M.astype(np.int32)), "uint8"),
        (("abs", []), dict(BOUND_MAP=str(tmp_path / "none.npy")), "cannot be read"),
    ]
    for (mode, bound), kw, word in cases:
        with pytest.raises(SystemExit) as e:
            run(mode, bound, **kw)
        out = capsys.readouterr().out
        assert e.value.code == 2 and out.startswith("ERROR:") and word in out and len(out.strip().splitlines()) == 1, (kw, out)
    monkeypatch.setattr(compress.tzdist, "active", lambda: (0, 2))
    with pytest.raises(SystemExit) as e:
        run("abs", [], BOUND_MAP=M)
    assert e.value.code == 2 and "sharded" in capsys.readouterr().out


def test_a_map_of_the_wrong_size_is_refused_once_the_directory_is_listed(monkeypatch, capsys, tmp_path):
    from PIL import Image
    from tezip_amd import compress
    ddir = tmp_path / "data"
    ddir.mkdir()
    for t in range(3):
        Image.fromarray(np.full((8, 8, 3), 40 * t, np.uint8)).save(ddir / ("f_%d.png" % t))
    monkeypatch.setattr(compress, "open_model", lambda d: pytest.fail("refused before the model is read"))
    monkeypatch.setattr(compress, "make_context", lambda *a, **k: pytest.fail("refused before a GPU is touched"))
    np.save(tmp_path / "m.npy", maps()["roi"])
    for spec in (str(tmp_path / "m.npy"), maps()["roi"]):
        with pytest.raises(SystemExit) as e:
            compress.run("m", str(ddir), str(tmp_path / "o"), 0, 4, None, "abs", [], True, False, True, BOUND_MAP=spec)
        out = capsys.readouterr().out
        assert e.value.code == 2 and out.startswith("ERROR:") and "21 x 30 for images of 8 x 8" in out and len(out.strip().splitlines()) == 1
    assert not os.path.exists(tmp_path / "o")


# ------------------------------------------------------------------------------------------------------ 5. the check tool
def test_check_tool_exit_status(tmp_path):
    from PIL import Image
    rng = np.random.default_rng(11)
    M = maps()["roi"]
    src, ok, broken = tmp_path / "src", tmp_path / "ok", tmp_path / "broken"
    for d in (src, ok, broken):
        d.mkdir()
    np.save(tmp_path / "m.npy", M)
    for t in range(3):
        o = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
        r = np.clip(o.astype(np.int64) + rng.integers(-1, 2, o.shape) * M[:, :, None], 0, 255).astype(np.uint8)
        Image.fromarray(o).save(src / ("f_%d.png" % t))
        Image.fromarray(r).save(ok / ("f_%d.png" % t))
        if t == 1:
            r = r.copy()
            r[6, 4, 0] = o[6, 4, 0] ^ 1                     # inside the zero rectangle
            r[0, 0, 1] = o[0, 0, 1] + 7 if o[0, 0, 1] < 200 else o[0, 0, 1] - 7
        Image.fromarray(r).save(broken / ("f_%d.png" % t))
    run = lambda d: subprocess.run([sys.executable, "-m", "tezip_amd.boundmap", str(tmp_path / "m.npy"), str(src), str(d)], cwd=ROOT,  # noqa: E731
                                   capture_output=True, text=True, timeout=120)
    good = run(ok)
    assert good.returncode == 0 and good.stdout.strip() == bm.HELD_LINE, good.stdout + good.stderr
    bad = run(broken)
    assert bad.returncode == 3 and bad.stdout.strip().splitlines() == [bm.broken_line(1, "f_1.png", 2)], bad.stdout + bad.stderr
