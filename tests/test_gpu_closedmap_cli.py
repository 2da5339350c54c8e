"""`-c --loop closed --quant lattice -m abs --loop-map FILE` and `-u` end to end on a MI355X (definition TZ-CLM1,
tezip_amd/closedmap.py): 8 PNG files of 24 x 40 through the command line's own entry (tezip.main on parsed arguments, in this
process: a job is a second or two), against the slow statement, the map's own check of the restored directory and the jobs the
flag must equal."""
import json
import os

import numpy as np
import pytest

import closedloop_jobs as J
import closedmap_jobs as M

pytestmark = pytest.mark.gpu

NT, H, W = 8, 24, 40
P, WIN = 1, 3
JOB = ["-p", str(P), "-w", str(WIN), "--loop", "closed", "--quant", "lattice", "-m", "abs"]
STREAM = ("entropy.dat", "key_frame.dat", "filename.txt")


@pytest.fixture(scope="module")
def job(tmp_path_factory):
    """model directory, per scene an image directory, the names, and the maps as files, on disk once"""
    from PIL import Image
    from tezip_amd import weights
    root = tmp_path_factory.mktemp("closedmap_cli")
    cfg, wts = J.model()
    mdir = str(root / "model")
    weights.save_model(mdir, cfg, wts, H, W)
    names = ["f_%03d.png" % t for t in range(NT)]
    dirs = {}
    for scene in ("translating", "flicker"):
        d = root / scene
        d.mkdir()
        for t, n in enumerate(names):
            Image.fromarray(np.ascontiguousarray(M.frames(scene, NT, H, W)[t])).save(d / n)
        dirs[scene] = str(d)
    maps = {"map": str(root / "map.npy"), "six": str(root / "six.png"), "zero": str(root / "zero.npy")}
    np.save(maps["map"], M.the_map(H, W))
    Image.fromarray(M.uniform(H, W, 6)).save(maps["six"])                  # (a single-channel image is a map too)
    np.save(maps["zero"], M.uniform(H, W, 0))
    return mdir, dirs, names, maps


def _tezip(argv, capsys):
    """-> (exit status, stdout) of one run of the command line"""
    from tezip_amd import tezip
    status = 0
    try:
        tezip.main(tezip.build_parser().parse_args(argv))
    except SystemExit as e:
        status = 0 if e.code is None else e.code
    return status, capsys.readouterr().out


def _images(directory, names):
    from PIL import Image
    return np.stack([np.asarray(Image.open(os.path.join(directory, n)).convert("RGB")) for n in names])


def _stream(d, extra=()):
    return {n: open(os.path.join(d, n), "rb").read() for n in STREAM + tuple(extra)}


def _sidecar(d):
    return json.load(open(os.path.join(d, "tezip_amd.json")))


def test_a_map_job_round_trips_and_holds_its_map(tmp_path, job, capsys):
    from tezip_amd import boundmap
    mdir, dirs, names, maps = job
    comp, dec = str(tmp_path / "comp"), str(tmp_path / "dec")
    m = M.the_map(H, W)
    status, out = _tezip(["-c", mdir, dirs["translating"], comp] + JOB + ["--loop-map", maps["map"], "--report", "--digests"], capsys)
    assert status == 0, out
    want = M.statement("translating", NT, H, W, P, WIN, "map", False, 0)
    lines = out.splitlines()
    assert lines.index("abs") < lines.index("loop: closed (TZ-CL1)") < lines.index(
        "loop map: 24x40, abs 0..255, %.1f %% of pixels exact (TZ-CLM1)" % (100.0 * (m == 0).sum() / m.size)), out
    assert "quant: lattice (TZ-QL1)" in lines and boundmap.HELD_LINE in lines
    assert sorted(os.listdir(comp)) == ["entropy.dat", "filename.txt", "frame_digests.json", "key_frame.dat", "quality.json", "tezip_amd.json"]
    side = _sidecar(comp)
    assert side["loop"] == "closed" and side["quant"] == "lattice" and side["bound_map"] == boundmap.stats(m) and "pred" not in side
    quality = json.load(open(os.path.join(comp, "quality.json")))
    assert quality["bound_map"] == {"file": maps["map"], "max": 255, "violations": 0, "max_excess": 0}
    assert [f["violations"] for f in quality["per_frame"]] == [0] * NT
    frames = M.frames("translating", NT, H, W)
    assert [f["sse"] for f in quality["per_frame"]] == [int(v) for v in ((want["dec"].astype(np.int64) - frames) ** 2).reshape(NT, -1).sum(1)]
    status, out = _tezip(["-u", mdir, comp, dec, "--verify", "require"], capsys)           # no flag for the map
    assert status == 0 and "verified: %d frames" % NT in out, out
    got = _images(dec, names)
    np.testing.assert_array_equal(got, want["dec"])
    np.testing.assert_array_equal(got[:, m == 0], frames[:, m == 0])                      # exact pixels are the source's
    assert boundmap.main([maps["map"], dirs["translating"], dec]) == 0
    assert boundmap.HELD_LINE in capsys.readouterr().out


@pytest.mark.parametrize("select", [False, True])
def test_a_uniform_map_is_the_closed_job(tmp_path, job, capsys, select):
    """Every file equals what `--loop closed -m abs -b 6 --quant lattice` writes; tezip_amd.json has the informational key more."""
    mdir, dirs, names, maps = job
    scene = "flicker" if select else "translating"
    extra = ["--pred", "select"] if select else []
    a, c = str(tmp_path / "map"), str(tmp_path / "closed")
    status, out = _tezip(["-c", mdir, dirs[scene], a] + JOB + ["--loop-map", maps["six"]] + extra, capsys)
    assert status == 0, out
    assert "loop map: 24x40, abs 6..6, 0.0 % of pixels exact (TZ-CLM1)" in out.splitlines(), out
    status, out = _tezip(["-c", mdir, dirs[scene], c] + JOB + ["-b", "6"] + extra, capsys)
    assert status == 0, out
    files = ("pred_modes.dat",) if select else ()
    assert _stream(a, files) == _stream(c, files) and sorted(os.listdir(a)) == sorted(os.listdir(c))
    side = _sidecar(a)
    assert side.pop("bound_map") == {"max": 6, "exact_pixels": 0} and side == _sidecar(c)


def test_a_zero_map_is_the_lossless_job(tmp_path, job, capsys):
    mdir, dirs, names, maps = job
    a, c, dec = str(tmp_path / "map"), str(tmp_path / "closed"), str(tmp_path / "dec")
    status, out = _tezip(["-c", mdir, dirs["translating"], a] + JOB + ["--loop-map", maps["zero"]], capsys)
    assert status == 0, out
    status, out = _tezip(["-c", mdir, dirs["translating"], c] + JOB + ["-b", "0"], capsys)
    assert status == 0, out
    assert _stream(a) == _stream(c)
    status, out = _tezip(["-u", mdir, a, dec], capsys)
    assert status == 0, out
    np.testing.assert_array_equal(_images(dec, names), M.frames("translating", NT, H, W))


def test_selection_under_the_map_with_gpu_coders_and_auto_layout(tmp_path, job, capsys, monkeypatch):
    from tezip_amd import boundmap, predselect
    mdir, dirs, names, maps = job
    comp, dec, dec2 = str(tmp_path / "comp"), str(tmp_path / "dec"), str(tmp_path / "dec2")
    status, out = _tezip(["-c", mdir, dirs["flicker"], comp] + JOB + ["--loop-map", maps["map"], "--pred", "select", "--coder", "huffd",
                                                                     "--sdelta", "auto", "--key-coder", "huff", "--report", "--ssim"], capsys)
    assert status == 0, out
    want = M.statement("flicker", NT, H, W, P, WIN, "map", True, 0)
    k, n = M.check_mixed(want)
    lines = out.splitlines()
    assert any(ln.startswith("sdelta: auto") for ln in lines) and boundmap.HELD_LINE in lines, out
    loop_map = [i for i, ln in enumerate(lines) if ln.startswith("loop map: ")]
    assert len(loop_map) == 1 and lines[loop_map[0] + 1] == predselect.stdout_line(want["modes"][~want["key"]]), out
    assert "%d of %d tiles" % (k, n) in lines[loop_map[0] + 1]
    assert _sidecar(comp)["pred"] == "select"
    np.testing.assert_array_equal(predselect.read(comp, NT, H, W), want["modes"])          # pred_modes.dat round-trips
    status, out = _tezip(["-u", mdir, comp, dec], capsys)
    assert status == 0, out
    np.testing.assert_array_equal(_images(dec, names), want["dec"])
    assert boundmap.main([maps["map"], dirs["flicker"], dec]) == 0
    capsys.readouterr()
    monkeypatch.setenv("TEZIP_NO_STREAMING", "1")
    status, out = _tezip(["-u", mdir, comp, dec2], capsys)
    assert status == 0, out
    np.testing.assert_array_equal(_images(dec2, names), want["dec"])


def test_a_map_of_the_wrong_size(tmp_path, job, capsys):
    mdir, dirs, names, maps = job
    wrong = str(tmp_path / "wrong.npy")
    np.save(wrong, np.zeros((H, W + 1), np.uint8))
    comp = str(tmp_path / "comp")
    status, out = _tezip(["-c", mdir, dirs["translating"], comp] + JOB + ["--loop-map", wrong], capsys)
    assert status == 2 and "ERROR: bound map %s is %d x %d for images of %d x %d" % (wrong, H, W + 1, H, W) in out, out
    assert not os.path.exists(os.path.join(comp, "entropy.dat"))
