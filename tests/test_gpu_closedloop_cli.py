"""`-c --loop closed` and `-u` end to end on a MI355X (definition TZ-CL1, tezip_amd/closedloop.py): 7 frames of 61 x 90 through
the command line's own entry (tezip.main on parsed arguments, in this process: a job is a second or two), against the slow
statement and the source images."""
import json
import os

import numpy as np
import pytest

import closedloop_jobs as J

pytestmark = pytest.mark.gpu

NT, H, W = 7, 61, 90
JOB = ["-p", "0", "-w", "3"]


@pytest.fixture(scope="module")
def job(tmp_path_factory):
    """model directory, image directory, names and frames, on disk once"""
    from PIL import Image
    from tezip_amd import weights
    root = tmp_path_factory.mktemp("closedloop_cli")
    frames = np.ascontiguousarray(J.frames(NT, H, W))
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


def _trailer_mark(path):
    from tezip_amd import decompress, zstd
    return decompress.parse_stream(zstd.decompress(open(path, "rb").read()))[2][0]


def _files(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d))}


def test_lossless_round_trip_default_format(tmp_path, job, capsys):
    mdir, ddir, names, frames = job
    comp, dec = str(tmp_path / "comp"), str(tmp_path / "dec")
    status, out = _tezip(["-c", mdir, ddir, comp] + JOB + ["-m", "abs", "-b", "0", "--loop", "closed", "-v"], capsys)
    assert status == 0, out
    assert out.splitlines().count("loop: closed (TZ-CL1)") == 1 and "MSE:" not in out and "predict:" in out
    assert sorted(os.listdir(comp)) == ["entropy.dat", "filename.txt", "key_frame.dat", "tezip_amd.json"]
    assert json.load(open(os.path.join(comp, "tezip_amd.json")))["loop"] == "closed"
    assert _trailer_mark(os.path.join(comp, "entropy.dat")) == 17
    status, out = _tezip(["-u", mdir, comp, dec], capsys)
    assert status == 0, out
    assert sorted(os.listdir(dec)) == names
    np.testing.assert_array_equal(_images(dec, names), frames)                 # byte for byte
    # the stream is the statement's: the same payload, table and trailer
    from tezip_amd import closedloop, decompress, zstd
    want = J.statement(NT, H, W, 0, 3, "abs", (0.0,), "greedy", 0)
    payload, table, shape, warm_up = decompress.parse_stream(zstd.decompress(open(os.path.join(comp, "entropy.dat"), "rb").read()))
    want_payload, want_table = closedloop.payload_of(want["q"], "flat")
    assert shape == (17, NT, H, W, 3) and warm_up == 0
    np.testing.assert_array_equal(payload, want_payload)
    np.testing.assert_array_equal(table, want_table)


def test_lattice_bound_report_and_the_whole_array_decoder(tmp_path, job, capsys, monkeypatch):
    mdir, ddir, names, frames = job
    comp, dec, dec2 = str(tmp_path / "comp"), str(tmp_path / "dec"), str(tmp_path / "dec2")
    status, out = _tezip(["-c", mdir, ddir, comp] + JOB + ["-m", "abs", "-b", "2", "--quant", "lattice", "--loop", "closed", "--report",
                                                           "--ssim"], capsys)
    assert status == 0, out
    lines = out.splitlines()
    assert "loop: closed (TZ-CL1)" in lines and "quant: lattice (TZ-QL1)" in lines and "max_abs_err: 2" in lines
    doc = json.load(open(os.path.join(comp, "tezip_amd.json")))
    assert doc["loop"] == "closed" and doc["quant"] == "lattice"
    assert _trailer_mark(os.path.join(comp, "entropy.dat")) == 17
    want = J.statement(NT, H, W, 0, 3, "abs", (2.0,), "lattice", 0)
    quality = json.load(open(os.path.join(comp, "quality.json")))
    assert quality["max_abs_err"] == 2
    assert [f["sse"] for f in quality["per_frame"]] == [int(v) for v in ((want["dec"].astype(np.int64) - frames) ** 2).reshape(NT, -1).sum(1)]
    status, out = _tezip(["-u", mdir, comp, dec], capsys)
    assert status == 0, out
    got = _images(dec, names)
    assert np.abs(got.astype(int) - frames.astype(int)).max() == 2
    np.testing.assert_array_equal(got, want["dec"])
    monkeypatch.setenv("TEZIP_NO_STREAMING", "1")
    status, out = _tezip(["-u", mdir, comp, dec2], capsys)
    assert status == 0, out
    np.testing.assert_array_equal(_images(dec2, names), want["dec"])


def test_gpu_coders_auto_layout_digests_and_verify(tmp_path, job, capsys, monkeypatch):
    mdir, ddir, names, frames = job
    comp, dec, dec2 = str(tmp_path / "comp"), str(tmp_path / "dec"), str(tmp_path / "dec2")
    status, out = _tezip(["-c", mdir, ddir, comp] + JOB + ["-m", "abs", "-b", "6", "--quant", "lattice", "--loop", "closed", "--coder", "huffd",
                                                           "--sdelta", "auto", "--key-coder", "huff", "--digests"], capsys)
    assert status == 0, out
    assert "loop: closed (TZ-CL1)" in out.splitlines() and any(ln.startswith("sdelta: auto") for ln in out.splitlines()), out
    assert sorted(os.listdir(comp)) == ["entropy.dat", "filename.txt", "frame_digests.json", "key_frame.dat", "tezip_amd.json"]
    from tezip_amd import huffd
    mark = huffd.parse(np.fromfile(os.path.join(comp, "entropy.dat"), np.uint8)).shape[0]
    assert mark in (17, 20, 24)
    want = J.statement(NT, H, W, 0, 3, "abs", (6.0,), "lattice", 0)
    status, out = _tezip(["-u", mdir, comp, dec, "--verify", "require"], capsys)
    assert status == 0 and "verified: %d frames" % NT in out, out
    np.testing.assert_array_equal(_images(dec, names), want["dec"])
    monkeypatch.setenv("TEZIP_NO_STREAMING", "1")
    status, out = _tezip(["-u", mdir, comp, dec2, "--verify", "require"], capsys)
    assert status == 0 and "verified: %d frames" % NT in out, out
    np.testing.assert_array_equal(_images(dec2, names), want["dec"])


def test_without_the_rank_table(tmp_path, job, capsys):
    """-n: the payload holds the spatial delta itself and the trailer no table"""
    from tezip_amd import closedloop, decompress, zstd
    mdir, ddir, names, frames = job
    comp, dec = str(tmp_path / "comp"), str(tmp_path / "dec")
    status, out = _tezip(["-c", mdir, ddir, comp] + JOB + ["-m", "abs", "-b", "6", "--quant", "lattice", "--loop", "closed", "-n",
                                                           "--sdelta", "channel"], capsys)
    assert status == 0, out
    want = J.statement(NT, H, W, 0, 3, "abs", (6.0,), "lattice", 0)
    payload, table, shape, warm_up = decompress.parse_stream(zstd.decompress(open(os.path.join(comp, "entropy.dat"), "rb").read()))
    assert table is None and shape == (20, NT, H, W, 3)
    np.testing.assert_array_equal(payload, closedloop.payload_of(want["q"], "channel", entropy=False)[0])
    status, out = _tezip(["-u", mdir, comp, dec], capsys)
    assert status == 0, out
    np.testing.assert_array_equal(_images(dec, names), want["dec"])


def test_byte_planes(tmp_path, job, capsys):
    """--shuffle needs a multiple of 8 elements: 8 frames.  Marks 21 (channel stride) and 25 (plane); -u takes the whole-array path."""
    from PIL import Image
    mdir = job[0]
    frames = np.ascontiguousarray(J.frames(8, H, W))
    ddir = tmp_path / "data"
    ddir.mkdir()
    names = ["g_%03d.png" % t for t in range(8)]
    for t, n in enumerate(names):
        Image.fromarray(frames[t]).save(ddir / n)
    want = J.statement(8, H, W, 1, 3, "abs", (6.0,), "lattice", 0)
    for sd, mark in (("channel", 21), ("plane", 25)):
        comp, dec = str(tmp_path / ("comp_" + sd)), str(tmp_path / ("dec_" + sd))
        status, out = _tezip(["-c", mdir, str(ddir), comp, "-p", "1", "-w", "3", "-m", "abs", "-b", "6", "--quant", "lattice", "--loop", "closed",
                              "--shuffle", "--sdelta", sd], capsys)
        assert status == 0, out
        assert _trailer_mark(os.path.join(comp, "entropy.dat")) == mark
        status, out = _tezip(["-u", mdir, comp, dec], capsys)
        assert status == 0, out
        np.testing.assert_array_equal(_images(dec, names), want["dec"])


def test_decoder_refusals(tmp_path, job, capsys, monkeypatch):
    mdir, ddir, names, frames = job
    comp = str(tmp_path / "comp")
    status, out = _tezip(["-c", mdir, ddir, comp] + JOB + ["-m", "abs", "-b", "0", "--loop", "closed", "--sdelta", "plane"], capsys)
    assert status == 0, out
    assert _trailer_mark(os.path.join(comp, "entropy.dat")) == 24
    for env in ({}, {"TEZIP_NO_STREAMING": "1"}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        dec = str(tmp_path / ("dec" + "".join(env)))
        status, out = _tezip(["-u", mdir, comp, dec, "--frames", "1:3"], capsys)
        assert status == 2 and "ERROR:" in out and "--frames" in out, out
        assert not os.path.exists(dec) or os.listdir(dec) == []
    monkeypatch.delenv("TEZIP_NO_STREAMING")
    # a sidecar that contradicts the trailer is an error, whichever says what
    side = os.path.join(comp, "tezip_amd.json")
    doc = json.load(open(side))
    del doc["loop"]
    json.dump(doc, open(side, "w"))
    with pytest.raises(ValueError, match="prediction loop as open, entropy.dat's trailer as closed"):
        _tezip(["-u", mdir, comp, str(tmp_path / "dec_x")], capsys)
    os.remove(side)                                                            # no sidecar: the trailer alone decides
    dec = str(tmp_path / "dec_y")
    status, out = _tezip(["-u", mdir, comp, dec], capsys)
    assert status == 0, out
    np.testing.assert_array_equal(_images(dec, names), frames)


def test_loop_open_writes_the_files_of_no_flag(tmp_path, job, capsys):
    mdir, ddir, names, frames = job
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    args = JOB + ["-m", "abs", "-b", "2", "--quant", "lattice"]
    status, out_a = _tezip(["-c", mdir, ddir, a] + args, capsys)
    assert status == 0, out_a
    status, out_b = _tezip(["-c", mdir, ddir, b] + args + ["--loop", "open"], capsys)
    assert status == 0, out_b
    assert _files(a) == _files(b) and out_a == out_b
    assert "loop" not in json.load(open(os.path.join(a, "tezip_amd.json"))) and "loop:" not in out_a
    assert _trailer_mark(os.path.join(a, "entropy.dat")) == 1
