"""`-c --loop closed --quant lattice --loop-psnr DB`, `--loop-bounds FILE` and `-u` end to end on a MI355X (definition TZ-CLF1,
tezip_amd/closedframes.py): 8 frames of 61 x 90 through the command line's own entry (tezip.main on parsed arguments, in this
process: a job is a second or two), against the slow statement, the search's own file and the jobs the flags must equal."""
import json
import os

import numpy as np
import pytest

import closedframes_jobs as F
import closedloop_jobs as J

pytestmark = pytest.mark.gpu

NT, H, W = 8, 61, 90
P, WIN = 1, 3
JOB = ["-p", str(P), "-w", str(WIN), "--loop", "closed", "--quant", "lattice"]
STREAM = ("entropy.dat", "key_frame.dat", "filename.txt", "tezip_amd.json")


@pytest.fixture(scope="module")
def job(tmp_path_factory):
    """model directory, image directory, names and frames, on disk once"""
    from PIL import Image
    from tezip_amd import weights
    root = tmp_path_factory.mktemp("closedframes_cli")
    frames = np.ascontiguousarray(F.frames(NT, H, W))
    cfg, wts = J.model()
    mdir = str(root / "model")
    weights.save_model(mdir, cfg, wts, 64, 96)
    ddir = root / "data"
    ddir.mkdir()
    names = ["f_%03d.png" % t for t in range(NT)]
    for t, n in enumerate(names):
        Image.fromarray(frames[t]).save(ddir / n)
    return mdir, str(ddir), names, frames


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


def _stream(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in STREAM}


def test_a_psnr_floor_found_inside_the_loop_and_its_replay(tmp_path, job, capsys):
    mdir, ddir, names, frames = job
    comp, dec, again = str(tmp_path / "comp"), str(tmp_path / "dec"), str(tmp_path / "again")
    status, out = _tezip(["-c", mdir, ddir, comp] + JOB + ["--loop-psnr", "36", "--report", "--digests"], capsys)
    assert status == 0, out
    want = F.searched(NT, H, W, P, WIN, 36.0, 0)
    ks = F.check_spread(want)
    lines = out.splitlines()
    assert lines.index("abs") < lines.index("loop: closed (TZ-CL1)") and "quant: lattice (TZ-QL1)" in lines
    assert ("loop target: PSNR >= 36 dB in every frame -> abs bounds %g..%g (TZ-CLF1, %d of %d frames searched)"
            % (min(ks) / 2.0, max(ks) / 2.0, len(ks), NT)) in lines, out
    assert sorted(os.listdir(comp)) == ["bound_search.json", "entropy.dat", "filename.txt", "frame_digests.json", "key_frame.dat",
                                        "quality.json", "tezip_amd.json"]
    side = json.load(open(os.path.join(comp, "tezip_amd.json")))
    assert side["loop"] == "closed" and side["quant"] == "lattice"
    search = json.load(open(os.path.join(comp, "bound_search.json")))
    limit = F.limit_of(36.0, H, W)
    assert search["definition"] == "TZ-CLF1" and search["sse_limit"] == limit and search["frame_samples"] == H * W * 3
    assert search["target_psnr_db"] == 36.0
    assert search["frame_bounds"] == list(want["bounds"])
    assert [fr["k"] for fr in search["frames"]] == want["k"] and [fr["sse"] for fr in search["frames"]] == want["sse"]
    assert [fr["name"] for fr in search["frames"]] == names and [fr["fixed"] for fr in search["frames"]] == [bool(k) for k in want["key"]]
    assert [r["sse"] for r in search["trace"]] == [[None if v == 2 ** 64 - 1 else v for v in row] for row in want["trace"]]
    quality = json.load(open(os.path.join(comp, "quality.json")))
    assert quality["frame_bounds"] == search["frame_bounds"]
    sse = [f["sse"] for f in quality["per_frame"]]
    for t in range(NT):
        assert sse[t] <= limit and sse[t] == search["frames"][t]["sse"], t      # (0 at the frames stored exactly)
    assert sse == [int(v) for v in ((want["dec"].astype(np.int64) - frames) ** 2).reshape(NT, -1).sum(1)]
    status, out = _tezip(["-u", mdir, comp, dec, "--verify", "require"], capsys)
    assert status == 0 and "verified: %d frames" % NT in out, out
    np.testing.assert_array_equal(_images(dec, names), want["dec"])
    # the search's file replays: the same stream, byte for byte
    status, out = _tezip(["-c", mdir, ddir, again] + JOB + ["-m", "abs", "--loop-bounds", os.path.join(comp, "bound_search.json")], capsys)
    assert status == 0, out
    assert "loop bounds: %d frames, abs 0..%g" % (NT, max(ks) / 2.0) in out.splitlines(), out
    assert not os.path.exists(os.path.join(again, "bound_search.json"))
    assert _stream(again) == _stream(comp)


def test_uniform_bounds_and_zeros_are_the_closed_jobs(tmp_path, job, capsys):
    mdir, ddir, names, frames = job
    for b in (6, 0):
        bounds = tmp_path / ("bounds_%d.json" % b)
        bounds.write_text(json.dumps([b] * NT))
        a, c = str(tmp_path / ("given_%d" % b)), str(tmp_path / ("closed_%d" % b))
        status, out = _tezip(["-c", mdir, ddir, a] + JOB + ["-m", "abs", "--loop-bounds", str(bounds)], capsys)
        assert status == 0, out
        assert "loop bounds: %d frames, abs 0..%d" % (NT, b) in out.splitlines(), out
        status, out = _tezip(["-c", mdir, ddir, c] + JOB + ["-m", "abs", "-b", str(b)], capsys)
        assert status == 0, out
        assert _stream(a) == _stream(c) and sorted(os.listdir(a)) == sorted(STREAM)
    dec = str(tmp_path / "dec")
    status, out = _tezip(["-u", mdir, str(tmp_path / "given_0"), dec], capsys)
    assert status == 0, out
    np.testing.assert_array_equal(_images(dec, names), frames)


def test_given_bounds_with_gpu_coders_auto_layout_and_the_whole_array_decoder(tmp_path, job, capsys, monkeypatch):
    mdir, ddir, names, frames = job
    comp, dec, dec2 = str(tmp_path / "comp"), str(tmp_path / "dec"), str(tmp_path / "dec2")
    bounds = tmp_path / "bounds.json"
    bounds.write_text(json.dumps({"frame_bounds": F.given(NT)}))
    status, out = _tezip(["-c", mdir, ddir, comp] + JOB + ["-m", "abs", "--loop-bounds", str(bounds), "--coder", "huffd", "--sdelta", "auto",
                                                           "--key-coder", "huff", "--report", "--ssim"], capsys)
    assert status == 0, out
    want = F.with_bounds(NT, H, W, P, WIN, tuple(F.given(NT)), 0)
    assert any(ln.startswith("sdelta: auto") for ln in out.splitlines()), out
    quality = json.load(open(os.path.join(comp, "quality.json")))
    assert quality["frame_bounds"] == list(want["bounds"])
    status, out = _tezip(["-u", mdir, comp, dec], capsys)
    assert status == 0, out
    np.testing.assert_array_equal(_images(dec, names), want["dec"])
    monkeypatch.setenv("TEZIP_NO_STREAMING", "1")
    status, out = _tezip(["-u", mdir, comp, dec2], capsys)
    assert status == 0, out
    np.testing.assert_array_equal(_images(dec2, names), want["dec"])


def test_a_list_of_the_wrong_length(tmp_path, job, capsys):
    mdir, ddir, names, frames = job
    bounds = tmp_path / "short.json"
    bounds.write_text(json.dumps([1.0] * (NT - 1)))
    comp = str(tmp_path / "comp")
    status, out = _tezip(["-c", mdir, ddir, comp] + JOB + ["-m", "abs", "--loop-bounds", str(bounds)], capsys)
    assert status == 2 and "ERROR: --loop-bounds %s: %d bounds for %d images" % (bounds, NT - 1, NT) in out, out
    assert not os.path.exists(os.path.join(comp, "entropy.dat"))
