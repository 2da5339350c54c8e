"""Per-tile selection TZ-PS1 (tezip_amd/predselect.py) without a GPU: the rule from first principles with hand-made predictors, the
slow statement's round trip and its L1 property on the jobs of tests/closedloop_jobs.py, the float32 value that expresses a chosen
tile in the prediction stack, pred_modes.dat, the marks, and the flag's refusals.  tests/test_gpu_predselect.py holds the library to
this statement bit for bit."""
import struct

import numpy as np
import pytest

import closedloop_jobs as J
import predselect_jobs as PJ


class _Hand:
    """A predictor made by hand: c0 is zero, next(frame) is what `rule` makes of the fed frame."""

    def __init__(self, rule):
        self.rule = rule
        self.fed = []

    def c0(self, hp, wp):
        return np.zeros((hp, wp, 3), np.float32)

    def next(self, frame):
        self.fed.append(np.array(frame))
        return np.asarray(self.rule(frame), np.float32)


def _scene(nt, h, w, seed=11):
    """frames with content in every tile and motion between frames"""
    rng = np.random.default_rng(seed)
    base = rng.integers(40, 216, (h + nt, w + nt, 3), dtype=np.uint8)
    return np.stack([base[t: t + h, t: t + w] for t in range(nt)])


def _tiles_naive(a):
    """tile sums by two loops: what predselect.tile_sums must give"""
    from tezip_amd import predselect
    h, w = a.shape[:2]
    th, tw = predselect.tiles_of(h, w)
    return np.array([[int(a[16 * i: 16 * i + 16, 16 * j: 16 * j + 16].sum()) for j in range(tw)] for i in range(th)])


# ------------------------------------------------------------------------------------------------ the rule, by hand
@pytest.mark.parametrize("h,w", [(24, 40), (16, 16), (33, 17)])
def test_a_predictor_of_zeros_loses_every_tile(h, w):
    from tezip_amd import predselect
    frames = _scene(6, h, w)
    got = predselect.encode(frames, 0, 3, "abs", [0.0], "greedy", _Hand(lambda f: np.zeros_like(f)))
    assert got["modes"].shape == (6,) + predselect.tiles_of(h, w)
    assert got["modes"][~got["key"]].all() and not got["modes"][got["key"]].any()
    np.testing.assert_array_equal(got["dec"], frames)
    nk = np.nonzero(~got["key"])[0]
    np.testing.assert_array_equal(got["q"][nk], frames[nk - 1].astype(np.int64) - frames[nk])      # a temporal delta


def test_a_predictor_that_knows_the_next_frame_keeps_every_tile():
    from tezip_amd import predselect
    h, w = 24, 40
    frames = _scene(6, h, w)
    state = {"t": 0}
    order = [t for t in range(6) if not predselect.closedloop.key_mask(6, 0, 3)[t]]

    def exact(_):
        t = order[state["t"]]
        state["t"] += 1
        return predselect.pv(frames[t])                                   # truncates back to the frame itself

    got = predselect.encode(frames, 0, 3, "abs", [0.0], "greedy", _Hand(exact))
    assert not got["modes"].any() and not got["q"][~got["key"]].any()


def test_a_tie_goes_to_the_network():
    from tezip_amd import predselect
    h, w = 16, 32
    frames = np.full((3, h, w, 3), 100, np.uint8)
    frames[1] = 110                                                       # the frame in front misses by -10 everywhere ...
    net = _Hand(lambda f: np.full_like(f, predselect.pv(np.uint8(120))))  # ... and the network by +10
    got = predselect.encode(frames, 0, 4, "abs", [0.0], "greedy", net)
    assert (got["q"][1] == 10).all() and not got["modes"][1].any()
    frames2 = frames.copy()
    frames2[1, 0, 0, 0] = 109                                             # one sample: the frame in front now wins the left tile by 1
    got = predselect.encode(frames2, 0, 4, "abs", [0.0], "greedy", net)
    assert got["modes"][1].tolist() == [[1, 0]]


def test_the_network_is_fed_the_decoded_frame_whatever_the_modes():
    from tezip_amd import closedloop, predselect
    h, w = 24, 40
    frames = _scene(5, h, w)
    net = _Hand(lambda f: np.zeros_like(f))
    got = predselect.encode(frames, 0, 4, "abs", [6.0], "lattice", net)
    nk = np.nonzero(~got["key"])[0]
    assert len(net.fed) == len(nk)
    for fed, t in zip(net.fed, nk):
        np.testing.assert_array_equal(fed, closedloop.u8_to_f32(got["dec"][t - 1], 24, 40))
    err = np.abs(got["dec"].astype(int) - frames.astype(int))
    assert err.max() <= 6 and err[nk].max() > 0


def test_tile_sums_and_edge_tiles():
    from tezip_amd import predselect
    rng = np.random.default_rng(5)
    for h, w in [(24, 40), (61, 90), (16, 16), (1, 1), (17, 33)]:
        a = rng.integers(0, 300, (h, w, 3))
        np.testing.assert_array_equal(predselect.tile_sums(a), _tiles_naive(a))
        assert predselect.tiles_of(h, w) == (-(-h // 16), -(-w // 16))


# ------------------------------------------------------------------------------------------------- the float trick
def test_pv_round_trips_all_256_values_in_float32():
    from tezip_amd import predselect
    v = np.arange(256, dtype=np.uint8)
    p = predselect.pv(v)
    assert p.dtype == np.float32 and p.max() == np.float32(1.0) and p.min() > 0
    x = (p * np.float32(255.0)).astype(np.int64)                          # trunc(f32(pv * 255)), as x_hat
    np.testing.assert_array_equal(x, v)
    # the unguarded formula exceeds 1.0 at 255 alone: hence the special case
    raw = (v.astype(np.float32) + np.float32(0.5)) / np.float32(255.0)
    assert (raw > np.float32(1.0)).tolist() == [False] * 255 + [True]
    np.testing.assert_array_equal(raw[:255], p[:255])
    # one value at a time, as a kernel computes it
    for i in range(256):
        one = np.float32(1.0) if i == 255 else (np.float32(i) + np.float32(0.5)) / np.float32(255.0)
        assert int(np.float32(one * np.float32(255.0))) == i and one == p[i]


# ------------------------------------------------------------------------- the statement on the closed-loop jobs
@pytest.mark.parametrize("scene", PJ.SCENES)
@pytest.mark.parametrize("h,wd", J.SIZES)
@pytest.mark.parametrize("nt,p,w", J.TRIPLES)
def test_round_trip_bound_l1_property_and_patched_stack(nt, p, w, h, wd, scene):
    from tezip_amd import closedloop, predselect
    frames = PJ.frames(scene, nt, h, wd)
    for mode, bound, quant in J.BOUNDS:
        what = "%s %g %s" % (mode, bound[0], quant)
        got = PJ.statement(scene, nt, h, wd, p, w, mode, bound, quant)
        key = got["key"]
        np.testing.assert_array_equal(key, closedloop.key_mask(nt, p, w))
        assert not got["modes"][key].any() and got["modes"].max() <= 1
        E = min(255, int(np.floor(bound[0])))
        err = np.abs(got["dec"].astype(np.int64) - frames.astype(np.int64))
        assert err.max() <= E, what
        if E == 0:
            np.testing.assert_array_equal(got["dec"], frames)
            # the L1 property: per tile, sum |q| is at most TZ-CL1's, and equal where the network was kept
            cl = PJ.closed_statement(scene, nt, h, wd, p, w, mode, bound, quant)
            np.testing.assert_array_equal(got["pred"], cl["pred"])         # dec = orig: the predictions do not depend on the modes
            for t in np.nonzero(~key)[0]:
                mine, theirs = predselect.tile_sums(np.abs(got["q"][t].astype(np.int64))), predselect.tile_sums(np.abs(cl["q"][t].astype(np.int64)))
                assert (mine <= theirs).all(), (what, t)
                np.testing.assert_array_equal(mine[got["modes"][t] == 0], theirs[got["modes"][t] == 0])
                assert (mine[got["modes"][t] == 1] < theirs[got["modes"][t] == 1]).all()
        # the modes are the rule, formed anew from the candidates
        for t in np.nonzero(~key)[0]:
            orig = frames[t].astype(np.int64)
            cn = _tiles_naive(np.abs(closedloop.quantise(closedloop.x_hat(got["pred"][t], h, wd) - orig, mode, list(bound), quant)))
            cp = _tiles_naive(np.abs(closedloop.quantise(got["dec"][t - 1].astype(np.int64) - orig, mode, list(bound), quant)))
            np.testing.assert_array_equal(got["modes"][t], cp < cn, err_msg=what)
        # the patched stack: the unchanged back half forms the statement's q from it, and outside H x W nothing changed
        np.testing.assert_array_equal(closedloop.open_loop_q(got["patched"], frames, p, w, mode, list(bound), quant), got["q"], err_msg=what)
        same = got["patched"].view(np.uint32) == got["pred"].view(np.uint32)
        assert same[:, h:].all() and same[:, :, wd:].all() and same[key].all()
        # the decoder's statement from key frames + payload + modes alone
        kf = np.zeros_like(frames)
        kf[key] = frames[key]
        for layout in J.LAYOUTS if w == 3 else ("flat",):
            payload, table = closedloop.payload_of(got["q"], layout)
            dec = predselect.decode(kf, p, payload, table, layout, got["modes"], J.predictor(h, wd))
            np.testing.assert_array_equal(dec["dec"], got["dec"], err_msg=what + layout)
            np.testing.assert_array_equal(dec["patched"][~key], got["patched"][~key], err_msg=what + layout)


def test_the_jobs_use_both_modes_and_the_lossy_loop_differs_from_tz_cl1():
    """Otherwise a library that ignored the setting, or one that always took the frame in front, could pass."""
    for h, wd in J.SIZES:
        for mode, bound, quant in J.BOUNDS:
            got = PJ.statement("flicker", 7, h, wd, 0, 3, mode, bound, quant)
            m = got["modes"][~got["key"]]
            assert 0 < m.sum() < m.size, (bound, int(m.sum()), m.size)             # both modes occur
            if (h, wd) == J.SIZES[1]:
                assert all(0 < f.sum() < f.size for f in m)                        # here in every predicted frame
            cl = PJ.closed_statement("flicker", 7, h, wd, 0, 3, mode, bound, quant)
            assert (got["q"] != cl["q"]).any()
            whole = PJ.statement("translating", 7, h, wd, 0, 3, mode, bound, quant)    # random weights: the frame in front wins throughout
            assert whole["modes"][~whole["key"]].all()
        a, b = PJ.statement("flicker", 7, h, wd, 0, 3, "abs", (6.0,), "lattice"), PJ.closed_statement("flicker", 7, h, wd, 0, 3, "abs", (6.0,), "lattice")
        assert (a["dec"] != b["dec"]).any() and (a["pred"][[2, 5]] != b["pred"][[2, 5]]).any()     # the modes change what is fed back


def test_decode_refuses_bad_modes():
    from tezip_amd import closedloop, predselect
    h, wd = J.SIZES[0]
    got = PJ.statement("flicker", 7, h, wd, 0, 3, "abs", (0.0,), "greedy")
    frames = PJ.frames("flicker", 7, h, wd)
    kf = np.zeros_like(frames)
    kf[got["key"]] = frames[got["key"]]
    payload, table = closedloop.payload_of(got["q"], "flat")
    for t, v in ((0, 1), (1, 2)):
        bad = got["modes"].copy()
        bad[t, 0, 0] = v
        with pytest.raises(ValueError, match="mode"):
            predselect.decode(kf, 0, payload, table, "flat", bad, J.predictor(h, wd))


# --------------------------------------------------------------------------------------------------- pred_modes.dat
def test_pack_and_unpack_are_inverses():
    from tezip_amd import predselect
    rng = np.random.default_rng(7)
    for nt, h, w in [(7, 24, 40), (9, 61, 90), (1, 1, 1), (5, 512, 512), (3, 16, 17)]:
        th, tw = predselect.tiles_of(h, w)
        modes = rng.integers(0, 2, (nt, th, tw), dtype=np.uint8)
        data = predselect.pack(modes)
        assert data[:4] == b"TZP1" and struct.unpack("<4I", data[4:20]) == (16, nt, th, tw)
        assert len(data) == 20 + (nt * th * tw + 7) // 8
        np.testing.assert_array_equal(np.frombuffer(data[20:], np.uint8), np.packbits(modes.reshape(-1), bitorder="little"))
        back = predselect.unpack(data, nt, h, w)
        assert back.dtype == np.uint8
        np.testing.assert_array_equal(back, modes)
    assert len(predselect.pack(np.zeros((1, 32, 32), np.uint8))) - 20 == 128       # 128 bytes per 512 x 512 frame
    with pytest.raises(ValueError):
        predselect.pack(np.full((1, 2, 2), 2, np.uint8))


def test_malformed_files_are_refused(tmp_path):
    from tezip_amd import predselect
    nt, h, w = 7, 24, 40                                                   # 7 * 2 * 3 = 42 tiles: 6 bytes, 6 pad bits
    modes = np.zeros((nt, 2, 3), np.uint8)
    modes[1, 1, 2] = modes[6, 1, 2] = 1
    good = predselect.pack(modes)
    np.testing.assert_array_equal(predselect.unpack(good, nt, h, w), modes)
    cases = {
        "truncated": [good[:10], good[:20], good[:-1], b""],
        "too long": [good + b"\0"],
        "wrong magic": [b"TZP2" + good[4:], b"\0" * len(good)],
        "implies": [good[:4] + struct.pack("<4I", 8, nt, 2, 3) + good[20:], good[:4] + struct.pack("<4I", 16, nt + 1, 2, 3) + good[20:],
                    good[:4] + struct.pack("<4I", 16, nt, 3, 2) + good[20:]],
        "pad bit": [good[:-1] + bytes([good[-1] | 0x04]), good[:-1] + bytes([good[-1] | 0x80])],
    }
    for needle, datas in cases.items():
        for data in datas:
            with pytest.raises(ValueError, match=needle):
                predselect.unpack(data, nt, h, w)
    with pytest.raises(ValueError, match="implies"):                       # the dimensions do not fit the trailer
        predselect.unpack(good, nt, h + 16, w)
    with pytest.raises(ValueError, match="is missing"):
        predselect.read(str(tmp_path), nt, h, w)
    assert predselect.write(str(tmp_path), modes) == len(good)
    np.testing.assert_array_equal(predselect.read(str(tmp_path), nt, h, w), modes)
    (tmp_path / predselect.FILE).write_bytes(good[:-2])
    with pytest.raises(ValueError, match="truncated"):
        predselect.read(str(tmp_path), nt, h, w)


# ------------------------------------------------------------------------------------------------------- the marks
def test_marks_in_every_parser():
    from tezip_amd import closedloop, decompress, predselect
    assert predselect.MARKS == (49, 50, 52, 53, 56, 57)
    for m in predselect.MARKS:
        assert predselect.is_select(m) and predselect.closed_mark(m) == m - 32 and closedloop.is_closed(m - 32) and not closedloop.is_closed(m)
    for m in (1, 2, 4, 5, 8, 9) + closedloop.MARKS + (33, 34, 36, 40, 48, 51, 54, 55, 58, 81):
        assert not predselect.is_select(m) and predselect.closed_mark(m) == m
    nt, H, W = 3, 4, 6
    n = nt * H * W * 3
    for one in predselect.MARKS:
        decompress.check_stream((one, nt, H, W, 3), 0, n, n)
        with pytest.raises(ValueError, match="closed-loop"):
            decompress.check_stream((one, nt, H, W, 1), 0, n // 3, n)
    for one in (33, 34, 36, 40, 48, 51, 54, 55, 58, 81):
        with pytest.raises(ValueError, match="unsupported stack shape"):
            decompress.check_stream((one, nt, H, W, 3), 0, n, n)


@pytest.mark.parametrize("coder", ["huff", "huffr", "huffd"])
def test_huffman_parsers_accept_the_marks_of_their_layouts(coder):
    import importlib
    from tezip_amd import closedloop
    fmt = importlib.import_module("tezip_amd." + coder)
    nt, H, W = 3, 4, 6
    q = np.random.default_rng(3).integers(-9, 10, (nt, H, W, 3)).astype(np.int16)
    for one, layout in ((49, "flat"), (52, "channel"), (56, "plane")):
        payload, table = closedloop.payload_of(q, layout)
        data = fmt.encode_file(payload, table, (one, nt, H, W, 3), 0)
        p = fmt.parse(data, nt * H * W * 3)
        assert p.shape == (one, nt, H, W, 3)
        got, _ = fmt.decode_file(data, nt * H * W * 3)
        np.testing.assert_array_equal(closedloop.q_of(got, p.table, q.shape, layout), q)
    payload, table = closedloop.payload_of(q, "flat")
    for one in (50, 53, 57, 33, 48, 51):
        with pytest.raises(ValueError, match="unsupported stack shape"):
            fmt.parse(fmt.encode_file(payload, table, (one, nt, H, W, 3), 0))


def test_sidecar_and_check_pred(tmp_path):
    from tezip_amd import decompress, predselect, sidecar
    cfg, wts = J.model()
    nt, h, w = 7, 24, 40
    modes = np.zeros((nt, 2, 3), np.uint8)
    modes[2, 0, 1] = 1
    a = tmp_path / "a"
    a.mkdir()
    doc = sidecar.write(str(a), 1, wts, 24, 40, (nt, h, w, 0), loop="closed", pred="select")
    assert doc["pred"] == "select" and doc["loop"] == "closed" and sidecar.pred_of(sidecar.read(str(a))) == "select"
    with pytest.raises(ValueError, match="is missing"):
        decompress.early_pred_modes(str(a))
    with pytest.raises(ValueError, match="is missing"):
        decompress.check_pred(str(a), 49, nt, h, w)
    predselect.write(str(a), modes)
    np.testing.assert_array_equal(decompress.early_pred_modes(str(a)), modes)
    np.testing.assert_array_equal(decompress.check_pred(str(a), 52, nt, h, w), modes)
    with pytest.raises(ValueError, match="prediction as select, entropy.dat's trailer as net"):
        decompress.check_pred(str(a), 17, nt, h, w)
    b = tmp_path / "b"
    b.mkdir()
    doc = sidecar.write(str(b), 1, wts, 24, 40, (nt, h, w, 0), loop="closed")
    assert "pred" not in doc and sidecar.pred_of(sidecar.read(str(b))) == "net"
    assert decompress.early_pred_modes(str(b)) is None and decompress.check_pred(str(b), 17, nt, h, w) is None
    with pytest.raises(ValueError, match="prediction as net, entropy.dat's trailer as select"):
        decompress.check_pred(str(b), 49, nt, h, w)
    assert sidecar.pred_of(None) is None and decompress.early_pred_modes(str(tmp_path)) is None
    with pytest.raises(sidecar.SidecarMismatch):
        sidecar.pred_of({"pred": "net"})
    with pytest.raises(SystemExit) as e:
        decompress.pred_modes_or_exit(str(b), 49, nt, h, w)
    assert e.value.code == 2


# ------------------------------------------------------------------------------------------------ the flag's refusals
def test_check_flags():
    from tezip_amd import predselect
    assert predselect.check_flags("net", "open") is None and predselect.check_flags("net", "closed") is None
    assert predselect.check_flags("select", "closed") is None
    assert predselect.check_flags("select", "open") == predselect.NEEDS_CLOSED and "add --loop closed" in predselect.NEEDS_CLOSED
    assert "--pred takes one of" in predselect.check_flags("both", "closed")


def _cli(argv):
    from tezip_amd import tezip
    return tezip.build_parser().parse_args(argv)


_JOB = ["-c", "m", "d", "o", "-p", "0", "-w", "3", "-m", "abs", "-b", "0"]


@pytest.mark.parametrize("argv,needle", [
    (["-u", "m", "d", "o", "--pred", "select"], "valid with -c"),
    (["-u", "m", "d", "o", "--pred", "net"], "valid with -c"),
    (["-l", "m", "d", "--pred", "select"], "valid with -c"),
    (_JOB + ["--pred", "select"], "add --loop closed"),
    (_JOB + ["--pred", "select", "--loop", "open"], "add --loop closed"),
    (["-c", "m", "d", "o", "-p", "0", "-t", "0.01", "-m", "abs", "-b", "0", "--loop", "closed", "--pred", "select"], "-t"),
    (["-c", "m", "d", "o", "-p", "0", "--sweep", "-m", "abs", "-b", "0", "--loop", "closed", "--pred", "select"], "--sweep"),
    (_JOB + ["--gray", "--loop", "closed", "--pred", "select"], "--gray"),
    (["-c", "m", "d", "o", "-p", "0", "-w", "3", "--target-psnr", "40", "--loop", "closed", "--pred", "select"], "--target-psnr"),
    (["-c", "m", "d", "o", "-p", "0", "-w", "3", "--target-ratio", "4", "--coder", "huffd", "--loop", "closed", "--pred", "select"], "--target-ratio"),
    (["-c", "m", "d", "o", "-p", "0", "-w", "3", "-m", "abs", "--frame-bounds", "f.json", "--loop", "closed", "--pred", "select"], "--frame-bounds"),
    (["-c", "m", "d", "o", "-p", "0", "-w", "3", "-m", "abs", "--bound-map", "m.npy", "--loop", "closed", "--pred", "select"], "--bound-map"),
    (["-c", "m", "d", "o", "-p", "0", "-w", "3", "-m", "abs", "-b", "2", "--loop", "closed", "--pred", "select"], "--quant lattice"),
])
def test_cli_refuses_before_a_gpu_is_touched(argv, needle, capsys, tmp_path, monkeypatch):
    from tezip_amd import _lib, tezip
    monkeypatch.setattr(tezip, "probe_gpu", lambda force: pytest.fail("a GPU was probed"))
    monkeypatch.setattr(_lib, "load", lambda *a, **kw: pytest.fail("the library was loaded"), raising=False)
    out = tmp_path / "o"
    argv = [str(out) if a == "o" else a for a in argv]
    with pytest.raises(SystemExit) as e:
        tezip.main(_cli(argv))
    assert e.value.code == 2
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    assert len(lines) == 1 and lines[0].startswith("ERROR:") and needle in lines[0], lines
    assert not out.exists()


def test_cli_refuses_a_sharded_select_job(capsys, monkeypatch):
    from tezip_amd import tezip
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setattr(tezip, "probe_gpu", lambda force: pytest.fail("a GPU was probed"))
    with pytest.raises(SystemExit) as e:
        tezip.main(_cli(_JOB + ["--loop", "closed", "--pred", "select"]))
    assert e.value.code == 2
    out = capsys.readouterr().out
    assert out.startswith("ERROR:") and "sharded" in out


def test_pred_net_changes_nothing_in_the_parsed_job_and_select_travels(monkeypatch):
    from tezip_amd import compress, tezip
    calls = []
    monkeypatch.setattr(tezip, "probe_gpu", lambda force: True)
    monkeypatch.setattr(compress, "run", lambda *a, **kw: calls.append((a, kw)))
    tezip.main(_cli(_JOB))
    tezip.main(_cli(_JOB + ["--pred", "net"]))
    assert calls[0] == calls[1] and "PRED" not in calls[0][1]
    closed = _JOB + ["--loop", "closed", "--sdelta", "auto", "--coder", "huffd", "--report", "--digests"]
    tezip.main(_cli(closed))
    tezip.main(_cli(closed + ["--pred", "net"]))
    assert calls[2] == calls[3] and "PRED" not in calls[2][1] and calls[2][1]["LOOP"] == "closed"
    tezip.main(_cli(closed + ["--pred", "select"]))
    a, kw = calls[4]
    assert a == calls[2][0] and kw == dict(calls[2][1], PRED="select")


def test_compress_run_refuses_select_without_the_closed_loop(capsys, tmp_path):
    from tezip_amd import compress
    with pytest.raises(SystemExit) as e:
        compress.run("m", "d", str(tmp_path / "o"), 0, 3, None, "abs", [0.0], True, False, True, PRED="select")
    assert e.value.code == 2
    out = capsys.readouterr().out
    assert out.startswith("ERROR:") and "add --loop closed" in out and not (tmp_path / "o").exists()
