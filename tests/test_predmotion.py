"""Motion-compensated tiles TZ-PM1 (tezip_amd/predmotion.py) without a GPU: the search, the rule and the loop from first principles
(a per-tile, per-vector loop that shares nothing with the statement's vectorised search), what the jobs of tests/predmotion_jobs.py
must contain for the GPU tests to mean something, the L1 property of a lossless job against TZ-PS1 and TZ-CL1, the patched stack,
pred_modes.dat in the format TZP2, the marks, and the flag's refusals.  tests/test_gpu_predmotion.py holds the library to this
statement bit for bit."""
import struct

import numpy as np
import pytest

import closedloop_jobs as J
import predmotion_jobs as MJ


def _brute(prev, orig):
    """Per tile the best vector and its SAD by lexicographic order of (SAD, |dy| + |dx|, dy, dx), two loops over tiles and two over
    vectors -> vectors (TH, TW, 2), sad (TH, TW), tied (TH, TW): whether a second vector reaches the smallest SAD."""
    h, w = orig.shape[:2]
    th, tw = -(-h // 16), -(-w // 16)
    prev, orig = prev.astype(np.int64), orig.astype(np.int64)
    vec, sad, tied = np.zeros((th, tw, 2), np.int8), np.zeros((th, tw), np.int64), np.zeros((th, tw), bool)
    for i in range(th):
        for j in range(tw):
            ys, xs = np.arange(16 * i, min(16 * i + 16, h)), np.arange(16 * j, min(16 * j + 16, w))
            tile = orig[np.ix_(ys, xs)]
            found = []
            for dy in range(-7, 8):
                for dx in range(-7, 8):
                    yy, xx = np.minimum(np.maximum(ys + dy, 0), h - 1), np.minimum(np.maximum(xs + dx, 0), w - 1)
                    found.append((int(np.abs(prev[np.ix_(yy, xx)] - tile).sum()), abs(dy) + abs(dx), dy, dx))
            found.sort()
            vec[i, j], sad[i, j], tied[i, j] = found[0][2:], found[0][0], found[0][0] == found[1][0]
    return vec, sad, tied


def _gather(prev, vec):
    """x_mc sample by sample: three loops."""
    h, w = prev.shape[:2]
    out = np.zeros_like(prev)
    for y in range(h):
        for x in range(w):
            dy, dx = (int(c) for c in vec[y // 16, x // 16])
            out[y, x] = prev[min(max(y + dy, 0), h - 1), min(max(x + dx, 0), w - 1)]
    return out


def _tiles_naive(a):
    h, w = a.shape[:2]
    return np.array([[int(a[16 * i: 16 * i + 16, 16 * j: 16 * j + 16].sum()) for j in range(-(-w // 16))] for i in range(-(-h // 16))])


def _reads_clamped(vec, modes, h, w):
    """(TH, TW) bool: mode-1 tiles whose vector takes a sample from a clamped coordinate."""
    th, tw = modes.shape
    out = np.zeros((th, tw), bool)
    for i in range(th):
        for j in range(tw):
            dy, dx = (int(c) for c in vec[i, j])
            y1, x1 = min(16 * i + 16, h) - 1, min(16 * j + 16, w) - 1
            out[i, j] = modes[i, j] == 1 and (16 * i + dy < 0 or y1 + dy > h - 1 or 16 * j + dx < 0 or x1 + dx > w - 1)
    return out


# --------------------------------------------------------------------------------------- the statement, from first principles
@pytest.mark.parametrize("scene", MJ.SCENES)
@pytest.mark.parametrize("h,wd", MJ.SIZES)
@pytest.mark.parametrize("nt,p,w", MJ.TRIPLES)
def test_the_statement_against_first_principles(nt, p, w, h, wd, scene):
    from tezip_amd import closedloop, predmotion
    frames = MJ.frames(scene, nt, h, wd)
    for mode, bound, quant in MJ.BOUNDS:
        what = "%s %s %g %s" % (scene, mode, bound[0], quant)
        got = MJ.statement(scene, nt, h, wd, p, w, mode, bound, quant)
        key = got["key"]
        np.testing.assert_array_equal(key, closedloop.key_mask(nt, p, w))
        assert not got["modes"][key].any() and got["modes"].max() <= 1 and not got["vectors"][got["modes"] == 0].any()
        E = min(255, int(np.floor(bound[0])))
        assert np.abs(got["dec"].astype(np.int64) - frames.astype(np.int64)).max() <= E, what
        for t in np.nonzero(~key)[0]:
            orig, prev = frames[t].astype(np.int64), got["dec"][t - 1]
            vec, sad, _ = _brute(prev, frames[t])
            x_mc, x_net = _gather(prev, vec).astype(np.int64), closedloop.x_hat(got["pred"][t], h, wd)
            assert (np.abs(x_mc - orig).sum(axis=2).reshape(h, wd).sum() == sad.sum()), what
            cn = _tiles_naive(np.abs(closedloop.quantise(x_net - orig, mode, list(bound), quant)))
            cm = _tiles_naive(np.abs(closedloop.quantise(x_mc - orig, mode, list(bound), quant)))
            m = cm < cn                                                                   # a tie goes to the network
            np.testing.assert_array_equal(got["modes"][t], m, err_msg=what)
            np.testing.assert_array_equal(got["vectors"][t], np.where(m[..., None], vec, 0), err_msg=what)
            x = np.where(np.repeat(np.repeat(m, 16, 0), 16, 1)[:h, :wd, None], x_mc, x_net)
            q = closedloop.quantise(x - orig, mode, list(bound), quant)
            np.testing.assert_array_equal(got["q"][t], q, err_msg=what)
            np.testing.assert_array_equal(got["dec"][t], np.clip(x - q, 0, 255), err_msg=what)
        # the patched stack: the unchanged back half forms the statement's q from it, and outside H x W nothing changed
        np.testing.assert_array_equal(closedloop.open_loop_q(got["patched"], frames, p, w, mode, list(bound), quant), got["q"], err_msg=what)
        same = got["patched"].view(np.uint32) == got["pred"].view(np.uint32)
        assert same[:, h:].all() and same[:, :, wd:].all() and same[key].all()
        # the decoder's statement from key frames + payload + modes + vectors alone
        kf = np.zeros_like(frames)
        kf[key] = frames[key]
        for layout in MJ.LAYOUTS if w == 3 else ("flat",):
            payload, table = closedloop.payload_of(got["q"], layout)
            dec = predmotion.decode(kf, p, payload, table, layout, got["modes"], got["vectors"], J.predictor(h, wd))
            np.testing.assert_array_equal(dec["dec"], got["dec"], err_msg=what + layout)
            np.testing.assert_array_equal(dec["patched"][~key], got["patched"][~key], err_msg=what + layout)


def test_the_network_is_fed_the_decoded_frame_and_exact_motion_is_found():
    """A hand-made predictor of zeros loses every tile; a texture moved by (+3, -5) is found at (-3, +5) in every interior tile."""
    from tezip_amd import closedloop, predmotion
    rng = np.random.default_rng(3)
    big = rng.integers(30, 226, (80, 100, 3), dtype=np.uint8)
    frames = np.stack([big[20 - 3 * t: 20 - 3 * t + 48, 20 + 5 * t: 20 + 5 * t + 64] for t in range(4)])   # frame t (y, x) = frame t-1 (y - 3, x + 5)
    fed = []

    class Zero:
        def c0(self, hp, wp):
            return np.zeros((hp, wp, 3), np.float32)

        def next(self, frame):
            fed.append(np.array(frame))
            return np.zeros_like(frame)

    for bound, quant in (([0.0], "greedy"), ([6.0], "lattice")):
        del fed[:]
        got = predmotion.encode(frames, 0, 4, "abs", bound, quant, Zero())
        nk = np.nonzero(~got["key"])[0]
        assert got["modes"][nk].all()
        assert (got["vectors"][nk][:, 1, 1:3] == (-3, 5)).all()                            # interior tiles: exact
        if bound[0] == 0:
            assert not got["q"][nk][:, 16:32, 16:48].any()
        for f, t in zip(fed, nk):
            np.testing.assert_array_equal(f, closedloop.u8_to_f32(got["dec"][t - 1], 48, 64))


def test_the_key_orders_by_sad_then_length_then_dy_then_dx():
    from tezip_amd import predmotion
    flat = np.full((16, 16, 3), 90, np.uint8)
    np.testing.assert_array_equal(predmotion.search(flat, flat)[0, 0], (0, 0))               # all 225 tie in SAD: the shortest
    k = predmotion.keys_of(flat, flat)[:, 0, 0]
    assert k.max() < 2 ** 30 and len(set(k.tolist())) == 225 and k.min() == 7 * 16 + 7
    assert (195840 * 4096 + 14 * 256 + 14 * 16 + 14) < 2 ** 30
    prev = flat.copy()
    prev[:, 8:] = 200                                                                       # a vertical edge: dy is free, dx is not
    orig = flat.copy()
    orig[:, 6:] = 200                                                                       # ... moved 2 to the left
    np.testing.assert_array_equal(predmotion.search(prev, orig)[0, 0], (0, 2))
    prev = np.zeros((16, 16, 3), np.uint8)
    prev[8, 8] = 255                                                                        # a dot ...
    orig = np.zeros_like(prev)
    orig[7, 8] = orig[9, 8] = 255                                                           # ... seen above and below: (-1, 0) and (1, 0) tie
    keys = predmotion.keys_of(prev, orig)[:, 0, 0]
    assert (keys >> 12)[6 * 15 + 7] == (keys >> 12)[8 * 15 + 7] == (keys >> 12).min()
    np.testing.assert_array_equal(predmotion.search(prev, orig)[0, 0], (-1, 0))                          # the smaller dy


# ------------------------------------------------------------------------------------------ what the jobs must contain
def test_the_jobs_contain_every_case_of_the_definition():
    """Otherwise a library that ignored part of the definition could pass the GPU tests."""
    seen = dict(mode0=0, mode1_zero=0, displaced=0, extreme=0, clamped=0, tied=0)
    for scene in MJ.SCENES:
        for h, wd in MJ.SIZES:
            got = MJ.statement(scene, 7, h, wd, 0, 3, *MJ.BOUNDS[0])
            fr = MJ.frames(scene, 7, h, wd)
            for t in np.nonzero(~got["key"])[0]:
                m, v = got["modes"][t], got["vectors"][t]
                seen["mode0"] += int((m == 0).sum())
                seen["mode1_zero"] += int(((m == 1) & ~v.any(axis=-1)).sum())
                seen["displaced"] += int(v.any(axis=-1).sum())
                seen["extreme"] += int((np.abs(v).max(axis=-1) == 7).sum())
                seen["clamped"] += int(_reads_clamped(v, m, h, wd).sum())
                seen["tied"] += int((_brute(got["dec"][t - 1], fr[t])[2] & (m == 1)).sum())   # a tie the stored vector shows
    assert all(n > 0 for n in seen.values()), seen
    ext = MJ.statement("shift7", 7, 61, 90, 0, 3, *MJ.BOUNDS[0])
    nk = ~ext["key"]
    assert (ext["vectors"][nk][:, 1:3, 1:5] == (-7, 7)).all() and not ext["q"][nk][:, 16:48, 16:80].any()   # interior tiles: exact at the extreme


# -------------------------------------------------------------------------------------------------- the lossless property
@pytest.mark.parametrize("scene", MJ.SCENES)
@pytest.mark.parametrize("h,wd", MJ.SIZES)
def test_l1_property_of_a_lossless_job(scene, h, wd):
    from tezip_amd import predselect
    for nt, p, w in MJ.TRIPLES:
        job = (scene, nt, h, wd, p, w) + MJ.BOUNDS[0]
        pm, ps, cl = MJ.statement(*job), MJ.select_statement(*job), MJ.closed_statement(*job)
        np.testing.assert_array_equal(pm["dec"], MJ.frames(scene, nt, h, wd))
        np.testing.assert_array_equal(pm["pred"], cl["pred"])                                # dec = orig: no dependence on modes or vectors
        for t in np.nonzero(~pm["key"])[0]:
            a, b, c = (predselect.tile_sums(np.abs(s["q"][t].astype(np.int64))) for s in (pm, ps, cl))
            assert (a <= b).all() and (b <= c).all(), (job, t)
            np.testing.assert_array_equal(a[pm["modes"][t] == 0], c[pm["modes"][t] == 0])
            assert (ps["modes"][t] <= pm["modes"][t]).all()                                  # a tile select took, motion takes too


# ------------------------------------------------------------------------------------------------------- pred_modes.dat
def _random_tiles(rng, nt, th, tw):
    modes = rng.integers(0, 2, (nt, th, tw), dtype=np.uint8)
    vectors = rng.integers(-7, 8, (nt, th, tw, 2)).astype(np.int8) * modes[..., None].astype(np.int8)
    return modes, vectors


def test_pack_and_unpack_are_inverses():
    from tezip_amd import predmotion, predselect
    rng = np.random.default_rng(7)
    for nt, h, w in [(7, 24, 40), (9, 61, 90), (1, 1, 1), (5, 512, 512), (3, 16, 17)]:
        th, tw = predselect.tiles_of(h, w)
        modes, vectors = _random_tiles(rng, nt, th, tw)
        data = predmotion.pack(modes, vectors)
        nbits = (nt * th * tw + 7) // 8
        assert data[:4] == b"TZP2" and struct.unpack("<5I", data[4:24]) == (16, nt, th, tw, 7)
        assert len(data) == 24 + nbits + int(modes.sum())
        assert data[24: 24 + nbits] == predselect.pack(modes)[20:]                           # TZ-PS1's mode bits
        v = vectors[modes == 1].astype(int) + 7
        np.testing.assert_array_equal(np.frombuffer(data[24 + nbits:], np.uint8), v[:, 0] * 16 + v[:, 1])
        back_m, back_v = predmotion.unpack(data, nt, h, w)
        assert back_m.dtype == np.uint8 and back_v.dtype == np.int8
        np.testing.assert_array_equal(back_m, modes)
        np.testing.assert_array_equal(back_v, vectors)
    one = np.ones((1, 2, 2), np.uint8)
    for bad_m, bad_v in ((one * 2, np.zeros((1, 2, 2, 2), np.int8)), (one, np.full((1, 2, 2, 2), 8, np.int8)), (one, np.zeros((1, 2, 2), np.int8)),
                         (one * 0, np.ones((1, 2, 2, 2), np.int8))):
        with pytest.raises(ValueError):
            predmotion.pack(bad_m, bad_v)


def test_malformed_files_are_refused(tmp_path):
    from tezip_amd import predmotion, predselect
    nt, h, w = 7, 24, 40                                                   # 42 tiles: 6 bytes of bits, 6 pad bits; two vectors
    modes = np.zeros((nt, 2, 3), np.uint8)
    vectors = np.zeros((nt, 2, 3, 2), np.int8)
    modes[1, 1, 2] = modes[6, 1, 2] = 1
    vectors[1, 1, 2], vectors[6, 1, 2] = (-7, 3), (7, -7)
    good = predmotion.pack(modes, vectors)
    assert len(good) == 24 + 6 + 2 and good[-2:] == bytes([0 * 16 + 10, 14 * 16 + 0])
    hdr = lambda *d: good[:4] + struct.pack("<5I", *d) + good[24:]           # noqa: E731
    cases = {
        "truncated": [good[:10], good[:24], good[:-1], good[:27], b""],
        "too long": [good + b"\0"],
        "wrong magic": [b"TZP1" + good[4:], predselect.pack(modes), b"\0" * len(good)],
        "search radius": [hdr(16, nt, 2, 3, 8), hdr(16, nt, 2, 3, 0)],
        "implies": [hdr(8, nt, 2, 3, 7), hdr(16, nt + 1, 2, 3, 7), hdr(16, nt, 3, 2, 7)],
        "pad bit": [good[:29] + bytes([good[29] | 0x04]) + good[30:], good[:29] + bytes([good[29] | 0x80]) + good[30:]],
        "nibble of 15": [good[:-1] + b"\xf0", good[:-1] + b"\x0f", good[:-2] + b"\xff" + good[-1:]],
    }
    for needle, datas in cases.items():
        for data in datas:
            with pytest.raises(ValueError, match=needle):
                predmotion.unpack(data, nt, h, w)
    with pytest.raises(ValueError, match="implies"):
        predmotion.unpack(good, nt, h + 16, w)
    with pytest.raises(ValueError, match="wrong magic"):                   # and the reverse: a TZP2 file under a select mark
        predselect.unpack(good, nt, h, w)
    with pytest.raises(ValueError, match="is missing"):
        predmotion.read(str(tmp_path), nt, h, w)
    assert predmotion.write(str(tmp_path), modes, vectors) == len(good)
    got = predmotion.read(str(tmp_path), nt, h, w)
    np.testing.assert_array_equal(got[0], modes)
    np.testing.assert_array_equal(got[1], vectors)


def test_decode_refuses_bad_modes_and_vectors():
    from tezip_amd import closedloop, predmotion
    h, wd = MJ.SIZES[0]
    got = MJ.statement("flicker", 7, h, wd, 0, 3, *MJ.BOUNDS[0])
    frames = MJ.frames("flicker", 7, h, wd)
    kf = np.zeros_like(frames)
    kf[got["key"]] = frames[got["key"]]
    payload, table = closedloop.payload_of(got["q"], "flat")
    zero = tuple(np.argwhere(got["modes"][1] == 0)[0])
    for bad_m, bad_v, needle in (((0, 0, 0, 1), None, "mode"), (None, (0, 0, 0, 0, 1), "mode 0"), (None, (1,) + zero + (1, 1), "mode 0"),
                                 (None, (1,) + tuple(np.argwhere(got["modes"][1] == 1)[0]) + (0, 8), "outside")):
        m, v = got["modes"].copy(), got["vectors"].copy()
        if bad_m:
            m[bad_m[:3]] = bad_m[3]
        if bad_v:
            v[bad_v[:4]] = bad_v[4]
        with pytest.raises(ValueError, match=needle):
            predmotion.decode(kf, 0, payload, table, "flat", m, v, J.predictor(h, wd))


# ------------------------------------------------------------------------------------------------------- the marks
def test_marks():
    from tezip_amd import closedloop, decompress, predmotion, predselect
    assert predmotion.MARKS == (81, 82, 84, 85, 88, 89)
    nt, H, W = 3, 4, 6
    n = nt * H * W * 3
    for m in predmotion.MARKS:
        assert predmotion.is_motion(m) and predmotion.pred_of_mark(m) == "motion"
        assert predmotion.select_mark(m) == m - 32 and predselect.is_select(m - 32) and predmotion.closed_mark(m) == m - 64
        assert closedloop.is_closed(m - 64) and not closedloop.is_closed(m) and not predselect.is_select(m)
        # without predmotion's mapping the decoder does not know the mark: it is no closed and no select mark
        with pytest.raises(ValueError, match="unsupported stack shape"):
            decompress.check_stream((m, nt, H, W, 3), 0, n, n)
        decompress.check_stream((predmotion.select_mark(m), nt, H, W, 3), 0, n, n)
    for m in (1, 2, 4, 5, 8, 9) + closedloop.MARKS + predselect.MARKS + (65, 80, 83, 86, 87, 90, 113):
        assert not predmotion.is_motion(m) and predmotion.select_mark(m) == m and predmotion.closed_mark(m) == predselect.closed_mark(m)
    assert [predmotion.pred_of_mark(m) for m in (1, 17, 49, 81)] == ["net", "net", "select", "motion"]


@pytest.mark.parametrize("coder", ["huff", "huffr", "huffd"])
def test_huffman_parsers_accept_the_marks_of_their_layouts(coder):
    import importlib
    from tezip_amd import closedloop
    fmt = importlib.import_module("tezip_amd." + coder)
    nt, H, W = 3, 4, 6
    q = np.random.default_rng(3).integers(-9, 10, (nt, H, W, 3)).astype(np.int16)
    for one, layout in ((81, "flat"), (84, "channel"), (88, "plane")):
        payload, table = closedloop.payload_of(q, layout)
        data = fmt.encode_file(payload, table, (one, nt, H, W, 3), 0)
        p = fmt.parse(data, nt * H * W * 3)
        assert p.shape == (one, nt, H, W, 3)
        got, _ = fmt.decode_file(data, nt * H * W * 3)
        np.testing.assert_array_equal(closedloop.q_of(got, p.table, q.shape, layout), q)
    payload, table = closedloop.payload_of(q, "flat")
    for one in (82, 85, 89, 65, 80, 83):
        with pytest.raises(ValueError, match="unsupported stack shape"):
            fmt.parse(fmt.encode_file(payload, table, (one, nt, H, W, 3), 0))
    with pytest.raises(ValueError, match="unsupported stack shape"):
        fmt.parse(fmt.encode_file(closedloop.payload_of(q[..., :1], "flat")[0], table, (81, nt, H, W, 1), 0))


def test_sidecar_and_check_pred(tmp_path):
    from tezip_amd import decompress, predmotion, predselect, sidecar
    cfg, wts = J.model()
    nt, h, w = 7, 24, 40
    modes = np.zeros((nt, 2, 3), np.uint8)
    vectors = np.zeros((nt, 2, 3, 2), np.int8)
    modes[2, 0, 1], vectors[2, 0, 1] = 1, (4, -7)
    a = tmp_path / "a"
    a.mkdir()
    doc = sidecar.write(str(a), 1, wts, 24, 40, (nt, h, w, 0), loop="closed", pred="motion")
    assert doc["pred"] == "motion" and doc["loop"] == "closed" and sidecar.pred_of(sidecar.read(str(a))) == "motion"
    with pytest.raises(ValueError, match="is missing"):
        decompress.early_pred_modes(str(a))
    with pytest.raises(ValueError, match="is missing"):
        decompress.check_pred(str(a), 81, nt, h, w)
    predmotion.write(str(a), modes, vectors)
    kind, got_m, got_v = decompress.stream_pred(str(a), 84, nt, h, w)
    assert kind == "motion"
    np.testing.assert_array_equal(got_m, modes)
    np.testing.assert_array_equal(got_v, vectors)
    np.testing.assert_array_equal(decompress.early_pred_modes(str(a)), modes)
    np.testing.assert_array_equal(decompress.check_pred(str(a), 84, nt, h, w), modes)
    for one, have in ((17, "net"), (49, "select")):
        with pytest.raises(ValueError, match="prediction as motion, entropy.dat's trailer as %s" % have):
            decompress.check_pred(str(a), one, nt, h, w)
    predselect.write(str(a), modes)                                        # a TZP1 file under the motion mark
    with pytest.raises(ValueError, match="wrong magic"):
        decompress.check_pred(str(a), 81, nt, h, w)
    with pytest.raises(ValueError, match="wrong magic"):
        decompress.early_pred_modes(str(a))
    b = tmp_path / "b"
    b.mkdir()
    sidecar.write(str(b), 1, wts, 24, 40, (nt, h, w, 0), loop="closed", pred="select")
    predmotion.write(str(b), modes, vectors)                               # and the reverse
    with pytest.raises(ValueError, match="wrong magic"):
        decompress.check_pred(str(b), 49, nt, h, w)
    with pytest.raises(ValueError, match="prediction as select, entropy.dat's trailer as motion"):
        decompress.check_pred(str(b), 81, nt, h, w)
    with pytest.raises(SystemExit) as e:
        decompress.stream_pred_or_exit(str(b), 81, nt, h, w)
    assert e.value.code == 2
    c = tmp_path / "c"
    c.mkdir()
    sidecar.write(str(c), 1, wts, 24, 40, (nt, h, w, 0), loop="closed", pred="select")
    predselect.write(str(c), modes)
    kind, got_m, got_v = decompress.stream_pred(str(c), 49, nt, h, w)
    assert kind == "select" and got_v is None
    np.testing.assert_array_equal(got_m, modes)
    assert decompress.stream_pred(str(tmp_path), 17, nt, h, w) == ("net", None, None)
    with pytest.raises(sidecar.SidecarMismatch):
        sidecar.pred_of({"pred": "both"})


# ------------------------------------------------------------------------------------------------ the flag's refusals
def test_check_flags_leaves_net_and_select_alone():
    from tezip_amd import predmotion, predselect
    assert predmotion.PREDS == ("net", "select", "motion") and predselect.PREDS == ("net", "select")
    for pred in ("net", "select", "both"):
        for loop in ("open", "closed"):
            assert predmotion.check_flags(pred, loop) == predselect.check_flags(pred, loop)
    assert predmotion.check_flags("motion", "closed") is None
    assert predmotion.check_flags("motion", "open") == predmotion.NEEDS_CLOSED and "add --loop closed" in predmotion.NEEDS_CLOSED


def _cli(argv):
    from tezip_amd import tezip
    return tezip.build_parser().parse_args(argv)


_JOB = ["-c", "m", "d", "o", "-p", "0", "-w", "3", "-m", "abs", "-b", "0"]
_PM = ["--loop", "closed", "--pred", "motion"]


@pytest.mark.parametrize("argv,needle", [
    (["-u", "m", "d", "o", "--pred", "motion"], "valid with -c"),
    (["-l", "m", "d", "--pred", "motion"], "valid with -c"),
    (_JOB + ["--pred", "motion"], "add --loop closed"),
    (_JOB + ["--pred", "motion", "--loop", "open"], "add --loop closed"),
    (["-c", "m", "d", "o", "-p", "0", "-t", "0.01", "-m", "abs", "-b", "0"] + _PM, "-t"),
    (["-c", "m", "d", "o", "-p", "0", "--sweep", "-m", "abs", "-b", "0"] + _PM, "--sweep"),
    (_JOB + ["--gray"] + _PM, "--gray"),
    (["-c", "m", "d", "o", "-p", "0", "-w", "3", "--target-psnr", "40"] + _PM, "--target-psnr"),
    (["-c", "m", "d", "o", "-p", "0", "-w", "3", "--target-ratio", "4", "--coder", "huffd"] + _PM, "--target-ratio"),
    (["-c", "m", "d", "o", "-p", "0", "-w", "3", "-m", "abs", "--frame-bounds", "f.json"] + _PM, "--frame-bounds"),
    (["-c", "m", "d", "o", "-p", "0", "-w", "3", "-m", "abs", "--bound-map", "m.npy"] + _PM, "--bound-map"),
    (["-c", "m", "d", "o", "-p", "0", "-w", "3", "-m", "abs", "-b", "2"] + _PM, "--quant lattice"),
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


def test_cli_refuses_a_sharded_motion_job(capsys, monkeypatch):
    from tezip_amd import tezip
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setattr(tezip, "probe_gpu", lambda force: pytest.fail("a GPU was probed"))
    with pytest.raises(SystemExit) as e:
        tezip.main(_cli(_JOB + _PM))
    assert e.value.code == 2
    out = capsys.readouterr().out
    assert out.startswith("ERROR:") and "sharded" in out


def test_net_and_select_jobs_are_parsed_as_before_and_motion_travels(monkeypatch):
    from tezip_amd import compress, tezip
    calls = []
    monkeypatch.setattr(tezip, "probe_gpu", lambda force: True)
    monkeypatch.setattr(compress, "run", lambda *a, **kw: calls.append((a, kw)))
    closed = _JOB + ["--loop", "closed", "--sdelta", "auto", "--coder", "huffd", "--report", "--digests"]
    for extra in ([], ["--pred", "net"], ["--pred", "select"], ["--pred", "motion"]):
        tezip.main(_cli(closed + extra))
    assert calls[0] == calls[1] and "PRED" not in calls[0][1] and calls[0][1]["LOOP"] == "closed"
    assert calls[2][0] == calls[0][0] and calls[2][1] == dict(calls[0][1], PRED="select")
    assert calls[3][0] == calls[0][0] and calls[3][1] == dict(calls[0][1], PRED="motion")


def test_compress_run_refuses_motion_without_the_closed_loop(capsys, tmp_path):
    from tezip_amd import compress
    with pytest.raises(SystemExit) as e:
        compress.run("m", "d", str(tmp_path / "o"), 0, 3, None, "abs", [0.0], True, False, True, PRED="motion")
    assert e.value.code == 2
    out = capsys.readouterr().out
    assert out.startswith("ERROR:") and "add --loop closed" in out and not (tmp_path / "o").exists()
