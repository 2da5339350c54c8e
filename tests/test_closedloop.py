"""Closed-loop prediction TZ-CL1 (tezip_amd/closedloop.py) without a GPU: the slow numpy statement held to first principles
with the C oracle's PredNet (model (3, 16, 32) at 24 x 40 and at 61 x 90, which pads to 64 x 96), and the six marks of the
format in every parser.  tests/test_gpu_closedloop.py holds the library to this statement bit for bit."""
import numpy as np
import pytest

import closedloop_jobs as J

ONE_JOB = (7, 0, 3)      # (nt, warm_up, window) of the lossy checks: three-frame windows, two steps inside each


def _xhat(pred, h, w):
    return (np.asarray(pred, np.float32)[:, :h, :w] * np.float32(255.0)).astype(np.int64)


@pytest.mark.parametrize("nt,p,w", J.TRIPLES)
def test_key_mask_is_the_open_loop_jobs(nt, p, w):
    from oracle import oracle as O
    from tezip_amd import closedloop
    h, wd = J.SIZES[0]
    want = O.rollout(J.frames(nt, h, wd), p, w, None, J.predictor(h, wd))
    np.testing.assert_array_equal(closedloop.key_mask(nt, p, w), want["key"])
    np.testing.assert_array_equal(J.statement(nt, h, wd, p, w, "abs", (0.0,), "greedy")["key"], want["key"])
    # slot 0 of every open-loop group is where the stored delta is zeroed
    starts = np.zeros(nt, bool)
    starts[[s for s, _ in want["groups"]]] = True
    np.testing.assert_array_equal(closedloop.group_first(nt, p, w), starts)


def test_the_trigger_on_the_last_frame_is_among_the_triples():
    assert any((nt - 1 - p) % w == 0 for nt, p, w in J.TRIPLES[4:])
    for nt, p, w in J.TRIPLES[4:]:
        from tezip_amd import closedloop
        assert closedloop.key_mask(nt, p, w)[nt - 1]


@pytest.mark.parametrize("h,wd", J.SIZES)
@pytest.mark.parametrize("nt,p,w", J.TRIPLES)
def test_lossless_every_prediction_is_one_step_and_the_round_trip_is_exact(nt, p, w, h, wd):
    from oracle import coracle
    from tezip_amd import closedloop
    frames, net = J.frames(nt, h, wd), J.predictor(h, wd)
    got = J.statement(nt, h, wd, p, w, "abs", (0.0,), "greedy")
    hp, wp = got["pred"].shape[1:3]
    for t in range(nt):
        if got["key"][t]:
            np.testing.assert_array_equal(got["pred"][t], net.c0(hp, wp))
        else:   # next(u8_to_f32(orig[t-1])), with the oracle's own statement of the u8 feed
            np.testing.assert_array_equal(got["pred"][t], net.next(coracle.u8_to_f32_frame(frames[t - 1], hp, wp)))
            np.testing.assert_array_equal(closedloop.u8_to_f32(frames[t - 1], hp, wp), coracle.u8_to_f32_frame(frames[t - 1], hp, wp))
    np.testing.assert_array_equal(got["dec"], frames)
    # the decoder's statement from key frames + payload alone, in every layout
    kf = np.zeros_like(frames)
    kf[got["key"]] = frames[got["key"]]
    for layout in J.LAYOUTS:
        payload, table = closedloop.payload_of(got["q"], layout)
        dec = closedloop.decode(kf, p, payload, table, layout, J.predictor(h, wd))
        np.testing.assert_array_equal(dec["dec"], frames, err_msg=layout)
        np.testing.assert_array_equal(dec["pred"], got["pred"], err_msg=layout)


@pytest.mark.parametrize("h,wd", J.SIZES)
@pytest.mark.parametrize("b", [2.0, 6.0])
def test_lossy_bound_decoder_and_the_open_loop_formulas(b, h, wd):
    from oracle import oracle as O
    from tezip_amd import closedloop, lattice
    nt, p, w = ONE_JOB
    frames = J.frames(nt, h, wd)
    got = J.statement(nt, h, wd, p, w, "abs", (b,), "lattice")
    E = min(255, int(np.floor(b)))
    err = np.abs(got["dec"].astype(np.int64) - frames.astype(np.int64))
    assert err.max() <= E                                       # at every sample
    assert err[~got["key"]].max() > 0                           # and the bound bites: this is not the lossless job
    np.testing.assert_array_equal(got["dec"][got["key"]], frames[got["key"]])
    # every non-key prediction came from the DECODED frame in front, and dec is oracle.reconstruct_int of it
    net = J.predictor(h, wd)
    hp, wp = got["pred"].shape[1:3]
    for t in np.nonzero(~got["key"])[0]:
        np.testing.assert_array_equal(got["pred"][t], net.next(closedloop.u8_to_f32(got["dec"][t - 1], hp, wp)))
    nk = ~got["key"]
    np.testing.assert_array_equal(got["dec"][nk], O.reconstruct_int(_xhat(got["pred"][nk], h, wd), got["q"][nk]))
    # q is TZ-QL1 of the deltas of the final predictions ...
    d = _xhat(got["pred"], h, wd) - frames.astype(np.int64)
    np.testing.assert_array_equal(got["q"][nk], lattice.quantise_e(d[nk], b))
    # ... which is what the open-loop back half computes on them: O.delta_group per group + the stack quantiser with its skips
    key = got["key"]
    gfirst = closedloop.group_first(nt, p, w)
    starts = list(np.nonzero(gfirst)[0]) + [nt]
    dm = np.concatenate([O.delta_group(got["pred"][a:z], frames[a:z]) for a, z in zip(starts[:-1], starts[1:])]).astype(np.int16)
    skip = gfirst.copy()
    skip[:p] = True
    want_q = lattice.quantise_stack(frames, dm, "abs", [b], skip)
    np.testing.assert_array_equal(got["q"], want_q)
    np.testing.assert_array_equal(closedloop.open_loop_q(got["pred"], frames, p, w, "abs", [b], "lattice"), want_q)
    # the decoder's statement reproduces dec from key frames + payload alone
    kf = np.zeros_like(frames)
    kf[key] = frames[key]
    for layout in J.LAYOUTS:
        payload, table = closedloop.payload_of(got["q"], layout)
        dec = closedloop.decode(kf, p, payload, table, layout, J.predictor(h, wd))
        np.testing.assert_array_equal(dec["key"], key)
        np.testing.assert_array_equal(dec["dec"], got["dec"], err_msg=layout)
        np.testing.assert_array_equal(dec["pred"], got["pred"], err_msg=layout)


def test_the_closed_loop_differs_from_the_open_one_and_feeds_the_decoded_frame():
    """What tests/test_gpu_closedloop.py asserts of the library holds for the statement it is compared with."""
    h, wd = J.SIZES[0]
    nt, p, w = ONE_JOB
    a = J.statement(nt, h, wd, p, w, "abs", (0.0,), "greedy")
    b = J.statement(nt, h, wd, p, w, "abs", (6.0,), "lattice")
    o = J.open_loop(nt, h, wd, p, w)
    nk = ~a["key"]
    assert (a["pred"][nk] != o["pred"][nk]).any()
    assert (a["pred"][nk] != b["pred"][nk]).any()
    first = [t for t in range(nt) if nk[t] and a["key"][t - 1]]     # a window's first prediction starts from the key frame in all three
    np.testing.assert_array_equal(a["pred"][first], o["pred"][first])
    np.testing.assert_array_equal(a["pred"][first], b["pred"][first])


def test_warm_up_frames_decode_to_the_original():
    from tezip_amd import closedloop
    h, wd = J.SIZES[0]
    frames = J.frames(8, h, wd)
    got = closedloop.encode(frames, 3, 2, "abs", [6.0], "lattice", J.predictor(h, wd))
    np.testing.assert_array_equal(got["key"], [1, 1, 1, 1, 0, 1, 0, 1])
    np.testing.assert_array_equal(got["dec"][got["key"]], frames[got["key"]])
    assert got["q"][1].any() and got["q"][2].any() and not got["q"][0].any() and not got["q"][3].any()
    np.testing.assert_array_equal(got["q"], closedloop.open_loop_q(got["pred"], frames, 3, 2, "abs", [6.0], "lattice"))


# ----------------------------------------------------------------------------------------------------------- the marks
def test_marks():
    from tezip_amd import closedloop, sdelta
    assert closedloop.MARKS == (17, 18, 20, 21, 24, 25)
    for m in closedloop.MARKS:
        assert closedloop.is_closed(m) and closedloop.open_mark(m) == m - 16
    for m in (1, 2, 4, 5, 8, 9):
        assert not closedloop.is_closed(m) and closedloop.open_mark(m) == m
    for m in (3, 6, 7, 16, 19, 22, 23, 26, 33):
        assert not closedloop.is_closed(m)
    assert [sdelta.mode_of(closedloop.open_mark(m)) for m in closedloop.MARKS] == ["flat", "flat", "channel", "channel", "plane", "plane"]
    assert [sdelta.is_shuffled(closedloop.open_mark(m)) for m in closedloop.MARKS] == [False, True] * 3


def test_check_stream_accepts_the_six_marks_and_refuses_the_rest():
    from tezip_amd import decompress
    nt, H, W = 3, 4, 6
    n = nt * H * W * 3
    for one in (17, 18, 20, 21, 24, 25):
        decompress.check_stream((one, nt, H, W, 3), 0, n, n)
        with pytest.raises(ValueError, match="closed-loop"):       # a closed-loop payload has three channels
            decompress.check_stream((one, nt, H, W, 1), 0, n // 3, n)
        with pytest.raises(ValueError, match="payload holds"):
            decompress.check_stream((one, nt, H, W, 3), 0, n - 1, n)
    for one in (3, 6, 7, 16, 19, 22, 23, 26, 32, 33):
        with pytest.raises(ValueError, match="unsupported stack shape"):
            decompress.check_stream((one, nt, H, W, 3), 0, n, n)


@pytest.mark.parametrize("coder", ["huff", "huffr", "huffd"])
def test_huffman_parsers_accept_the_marks_of_their_layouts(coder):
    """A Huffman-coded file never holds byte planes (--coder refuses --shuffle): 17, 20 and 24 parse as 1, 4 and 8 do, and
    18, 21 and 25 are refused as 2, 5 and 9 are."""
    import importlib
    from tezip_amd import closedloop
    fmt = importlib.import_module("tezip_amd." + coder)
    nt, H, W = 3, 4, 6
    rng = np.random.default_rng(3)
    q = rng.integers(-9, 10, (nt, H, W, 3)).astype(np.int16)
    for one, layout in ((17, "flat"), (20, "channel"), (24, "plane")):
        payload, table = closedloop.payload_of(q, layout)
        data = fmt.encode_file(payload, table, (one, nt, H, W, 3), 0)
        p = fmt.parse(data, nt * H * W * 3)
        assert p.shape == (one, nt, H, W, 3) and p.warm_up == 0
        got, _ = fmt.decode_file(data, nt * H * W * 3)
        np.testing.assert_array_equal(closedloop.q_of(got, p.table, q.shape, layout), q)
        with pytest.raises(ValueError, match="unsupported stack shape"):      # a closed-loop payload has three channels
            fmt.parse(fmt.encode_file(payload[: nt * H * W], table, (one, nt, H, W, 1), 0))
    payload, table = closedloop.payload_of(q, "flat")
    for one in (18, 21, 25, 2, 5, 9, 3, 16, 19, 33):
        with pytest.raises(ValueError, match="unsupported stack shape"):
            fmt.parse(fmt.encode_file(payload, table, (one, nt, H, W, 3), 0))


def test_sidecar_records_the_loop(tmp_path):
    from tezip_amd import decompress, sidecar
    cfg, wts = J.model()
    d = tmp_path / "a"
    d.mkdir()
    doc = sidecar.write(str(d), 1, wts, 24, 40, (7, 24, 40, 0), loop="closed")
    assert doc["loop"] == "closed" and sidecar.loop_of(sidecar.read(str(d))) == "closed"
    assert decompress.check_loop(str(d), 17) is True
    with pytest.raises(ValueError, match="prediction loop as closed, entropy.dat's trailer as open"):
        decompress.check_loop(str(d), 1)
    e = tmp_path / "b"
    e.mkdir()
    doc = sidecar.write(str(e), 1, wts, 24, 40, (7, 24, 40, 0))
    assert "loop" not in doc and sidecar.loop_of(sidecar.read(str(e))) == "open"
    assert decompress.check_loop(str(e), 8) is False
    with pytest.raises(ValueError, match="prediction loop as open, entropy.dat's trailer as closed"):
        decompress.check_loop(str(e), 24)
    assert decompress.check_loop(str(tmp_path), 20) is True and sidecar.loop_of(None) is None      # no sidecar: the trailer alone
    with pytest.raises(sidecar.SidecarMismatch):
        sidecar.loop_of({"loop": "open"})


# ------------------------------------------------------------------------------------------------- the flag's refusals
def test_check_flags():
    from tezip_amd import closedloop
    ok = dict(loop="closed", mode="abs", bound=[0.0], quant=None)
    assert closedloop.check_flags(**ok) is None
    assert closedloop.check_flags("open", "rel", [0.1], None, threshold=0.1, gray=True) is None      # open is the job without the flag
    assert closedloop.check_flags("closed", "abs", [2.0], "lattice") is None
    assert closedloop.check_flags("closed", "abs", [0.4], None) is None                               # the greedy identity
    assert closedloop.check_flags("closed", "abs", [0.9], "lattice") is None                          # the lattice identity
    assert closedloop.check_flags("closed", "abs", [0.9], None) == closedloop.NEEDS_LATTICE
    assert closedloop.check_flags("closed", "abs", [2.0], None) == closedloop.NEEDS_LATTICE
    assert "--quant lattice" in closedloop.NEEDS_LATTICE
    assert closedloop.check_flags("closed", "abs", [2.0], "greedy") == closedloop.NEEDS_LATTICE
    for mode, bound in (("rel", [0.1]), ("absrel", [2.0, 0.1]), ("pwrel", [0.1]), ("rel", [0.0])):
        assert closedloop.check_flags("closed", mode, bound, "lattice") == closedloop.NEEDS_ABS
    for kw, flag in ((dict(threshold=0.01), "-t"), (dict(sweep=True), "--sweep"), (dict(gray=True), "--gray"),
                     (dict(target_psnr=40.0), "--target-psnr"), (dict(target_ratio=4.0), "--target-ratio"),
                     (dict(per_frame=True), "--per-frame"), (dict(frame_bounds="f.json"), "--frame-bounds"),
                     (dict(bound_map="m.npy"), "--bound-map")):
        msg = closedloop.check_flags(**dict(ok, **kw))
        assert msg and msg.startswith("--loop closed cannot be combined with %s " % flag), (flag, msg)
    assert "sharded" in closedloop.check_flags(**dict(ok, sharded=True))
    assert "--loop takes one of" in closedloop.check_flags("half", "abs", [0.0], None)


def _cli(argv):
    from tezip_amd import tezip
    return tezip.build_parser().parse_args(argv)


@pytest.mark.parametrize("argv,needle", [
    (["-u", "m", "d", "o", "--loop", "closed"], "valid with -c"),
    (["-u", "m", "d", "o", "--loop", "open"], "valid with -c"),
    (["-l", "m", "d", "--loop", "closed"], "valid with -c"),
    (["-c", "m", "d", "o", "-p", "0", "-t", "0.01", "-m", "abs", "-b", "0", "--loop", "closed"], "-t"),
    (["-c", "m", "d", "o", "-p", "0", "--sweep", "-m", "abs", "-b", "0", "--loop", "closed"], "--sweep"),
    (["-c", "m", "d", "o", "-p", "0", "-w", "3", "-m", "abs", "-b", "0", "--gray", "--loop", "closed"], "--gray"),
    (["-c", "m", "d", "o", "-p", "0", "-w", "3", "--target-psnr", "40", "--loop", "closed"], "--target-psnr"),
    (["-c", "m", "d", "o", "-p", "0", "-w", "3", "--target-ratio", "4", "--coder", "huffd", "--loop", "closed"], "--target-ratio"),
    (["-c", "m", "d", "o", "-p", "0", "-w", "3", "--target-psnr", "40", "--per-frame", "--loop", "closed"], "--target-psnr"),
    (["-c", "m", "d", "o", "-p", "0", "-w", "3", "-m", "abs", "--frame-bounds", "f.json", "--loop", "closed"], "--frame-bounds"),
    (["-c", "m", "d", "o", "-p", "0", "-w", "3", "-m", "abs", "--bound-map", "m.npy", "--loop", "closed"], "--bound-map"),
    (["-c", "m", "d", "o", "-p", "0", "-w", "3", "-m", "rel", "-b", "0.1", "--loop", "closed"], "-m abs"),
    (["-c", "m", "d", "o", "-p", "0", "-w", "3", "-m", "abs", "-b", "2", "--loop", "closed"], "--quant lattice"),
])
def test_cli_refuses_before_a_gpu_is_touched(argv, needle, capsys, tmp_path, monkeypatch):
    from tezip_amd import tezip
    monkeypatch.setattr(tezip, "probe_gpu", lambda force: pytest.fail("a GPU was probed"))
    out = tmp_path / "o"
    argv = [str(out) if a == "o" else a for a in argv]
    with pytest.raises(SystemExit) as e:
        tezip.main(_cli(argv))
    assert e.value.code == 2
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    assert len(lines) == 1 and lines[0].startswith("ERROR:") and needle in lines[0], lines
    assert not out.exists()


def test_cli_refuses_a_sharded_closed_job(capsys, monkeypatch):
    from tezip_amd import tezip
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setattr(tezip, "probe_gpu", lambda force: pytest.fail("a GPU was probed"))
    with pytest.raises(SystemExit) as e:
        tezip.main(_cli(["-c", "m", "d", "o", "-p", "0", "-w", "3", "-m", "abs", "-b", "0", "--loop", "closed"]))
    assert e.value.code == 2
    out = capsys.readouterr().out
    assert out.startswith("ERROR:") and "sharded" in out


def test_cli_passes_the_loop_to_compress_run_and_open_is_the_job_without_the_flag(monkeypatch):
    from tezip_amd import compress, tezip
    calls = []
    monkeypatch.setattr(tezip, "probe_gpu", lambda force: True)
    monkeypatch.setattr(compress, "run", lambda *a, **kw: calls.append((a, kw)))
    base = ["-c", "m", "d", "o", "-p", "0", "-w", "3", "-m", "abs", "-b", "2"]
    tezip.main(_cli(base))
    tezip.main(_cli(base + ["--loop", "open"]))
    assert calls[0] == calls[1] and "LOOP" not in calls[0][1]
    tezip.main(_cli(base + ["--loop", "closed", "--quant", "lattice", "--sdelta", "auto", "--coder", "huffd", "--key-coder", "huff",
                            "--report", "--ssim", "--digests"]))
    a, kw = calls[2]
    assert a[:8] == ("m", "d", "o", 0, 3, None, "abs", [2.0])
    assert kw == dict(SHUFFLE=False, REPORT=True, CODER="huffd", KEY_CODER="huff", DIGESTS=True, SDELTA="auto", SSIM=True, QUANT="lattice",
                      LOOP="closed")
