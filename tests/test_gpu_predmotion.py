"""Motion-compensated tiles TZ-PM1 on a MI355X (tz_set_pred_motion, tz_pred_modes, tz_pred_vectors, tz_put_pred_modes,
tz_put_pred_vectors, k_pm_select, k_pm_step, k_pm_recon): the library held bit for bit to the slow statement
(tezip_amd/predmotion.py with the C oracle's PredNet; tests/test_predmotion.py holds that statement to first principles and shows
that the jobs contain every case of the definition) -- mode bytes, vectors, the prediction stack with the chosen tiles expressed in
it, payload and table in every layout, the decoded stack -- at 24 x 40 (every tile on a frame edge, rows a 4-byte multiple) and
61 x 90 (pads to 64 x 96, rows of 270 bytes, ragged edge tiles); past one grid of workgroups; with the setting off; the refusals of
the C ABI; and the command line end to end."""
import json
import os

import numpy as np
import pytest

import closedloop_jobs as J
import predmotion_jobs as MJ
import predselect_jobs as PJ

pytestmark = pytest.mark.gpu

TZ_ERR_INVALID, TZ_ERR_STATE = -1, -4


@pytest.fixture(scope="module")
def contexts():
    """One context per (H, W, contract), model loaded and prepared with four batch slots."""
    from tezip_amd import _lib
    made = {}

    def get(h, w, contract=0):
        if (h, w, contract) not in made:
            cfg, wts = J.model()
            c = _lib.Context(0)
            if contract:
                c.set_contract(contract)
            c.load_model(cfg, wts)
            c.prepare(_lib.pad8(h), _lib.pad8(w), 4)
            made[h, w, contract] = c
        c = made[h, w, contract]
        _reset(c)
        return c
    yield get
    for c in made.values():
        c.close()


def _reset(ctx):
    ctx.set_pred_motion(0)
    ctx.set_pred_select(False)
    ctx.set_quantiser(0)
    ctx.set_delta_stride(0)
    ctx.set_delta_plane(0)


def _layout(ctx, layout):
    ctx.set_delta_stride(0)
    ctx.set_delta_plane(0)
    if layout == "channel":
        ctx.set_delta_stride(1)
    elif layout == "plane":
        ctx.set_delta_plane(1)


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _same_predictions(ctx, want, h, w, what):
    """the resident stack is the statement's patched one inside H x W (key slots hold C0 on both sides of the test: not compared)"""
    got = ctx.get_predictions()
    nk = ~want["key"]
    np.testing.assert_array_equal(_bits(got[nk][:, :h, :w]), _bits(want["patched"][nk][:, :h, :w]), err_msg=what)


def _job_equals_statement(ctx, scene, nt, h, w, p, win, layouts, contract=0, bounds=MJ.BOUNDS):
    from tezip_amd import closedloop
    frames = np.ascontiguousarray(MJ.frames(scene, nt, h, w))
    for mode, bound, quant in bounds:
        what = "%s %dx%dx%d p%d w%d %s %g %s" % (scene, nt, h, w, p, win, mode, bound[0], quant)
        want = MJ.statement(scene, nt, h, w, p, win, mode, bound, quant, contract)
        ctx.set_quantiser(quant)
        ctx.set_pred_motion(7)
        _layout(ctx, "flat")
        key = ctx.rollout_closed(frames, p, win, mode, list(bound))
        assert ctx.pool_held()[0] == 0
        np.testing.assert_array_equal(key, want["key"], err_msg=what)
        modes, vectors = ctx.pred_modes(), ctx.pred_vectors()
        assert modes.dtype == np.uint8 and modes.shape == want["modes"].shape
        assert vectors.dtype == np.int8 and vectors.shape == want["vectors"].shape
        np.testing.assert_array_equal(modes, want["modes"], err_msg=what)                  # byte for byte
        np.testing.assert_array_equal(vectors, want["vectors"], err_msg=what)
        _same_predictions(ctx, want, h, w, what)
        for layout in layouts:
            _layout(ctx, layout)
            payload, table, delta = ctx.encode(mode, list(bound), True, want_delta=True)
            want_payload, want_table = closedloop.payload_of(want["q"], layout)
            np.testing.assert_array_equal(delta, want["q"], err_msg=what + " " + layout)
            np.testing.assert_array_equal(table, want_table, err_msg=what + " " + layout)
            np.testing.assert_array_equal(np.asarray(payload).reshape(-1), want_payload, err_msg=what + " " + layout)
        # the decoder: key stack, payload, modes and vectors alone
        kf = np.zeros_like(frames)
        kf[want["key"]] = frames[want["key"]]
        for layout in layouts:
            _layout(ctx, layout)
            payload, table = closedloop.payload_of(want["q"], layout)
            ctx.put_pred_modes(want["modes"])
            ctx.put_pred_vectors(want["vectors"])
            dkey = ctx.rollout_decode_closed(kf, p, payload, table)
            assert ctx.pool_held()[0] == 0
            np.testing.assert_array_equal(dkey, want["key"], err_msg=what + " " + layout)
            np.testing.assert_array_equal(ctx.decoded_get(0, nt), want["dec"], err_msg=what + " decoder " + layout)
            _same_predictions(ctx, want, h, w, what + " decoder " + layout)
    _reset(ctx)


@pytest.mark.parametrize("scene", MJ.SCENES)
@pytest.mark.parametrize("h,w", MJ.SIZES)
@pytest.mark.parametrize("nt,p,win", MJ.TRIPLES)
def test_library_equals_the_statement(contexts, nt, p, win, h, w, scene):
    _job_equals_statement(contexts(h, w), scene, nt, h, w, p, win, MJ.LAYOUTS)


@pytest.mark.parametrize("contract", [1, 2])
def test_both_arithmetic_contracts(contexts, contract):
    h, w = MJ.SIZES[1]
    ctx = contexts(h, w, contract)
    assert ctx.get_contract() == contract
    _job_equals_statement(ctx, "flicker", 7, h, w, 0, 3, ("flat",), contract=contract)
    assert ctx.rollout_contract() == contract


# ------------------------------------------------------------------------------------------------ the whole launch
# k_pm_* start min(tiles, PM_GRID = 128) workgroups a frame, one tile a trip: tiles = TH * TW.  The smallest count above that is
# 129 = 3 * 43: 3 tile rows (H in 33 .. 48) of 43 tiles (W in 673 .. 688), where workgroup 0 takes a second trip (tile 128: tile row
# 2, tile 42, the last one).  48 x 676 has rows of a 4-byte multiple and a last tile of 4 columns; 33 x 673 has rows of 2019 bytes,
# one row in the last tile row and one column in the last tile.
WHOLE = [(48, 676), (33, 673)]
WHOLE_JOB = (4, 0, 3)
WHOLE_BOUNDS = [MJ.BOUNDS[0], MJ.BOUNDS[2]]


def _tiles(h, w):
    return -(-h // 16) * -(-w // 16)


def test_the_whole_launch_shapes_cross_the_grid():
    assert [_tiles(h, w) for h, w in WHOLE] == [129, 129]
    assert _tiles(32, 688) <= 128 and _tiles(48, 672) <= 128                  # one tile row or one tile less: one trip


@pytest.mark.parametrize("h,w", WHOLE)
def test_past_one_grid_of_workgroups(contexts, h, w):
    nt, p, win = WHOLE_JOB
    ctx = contexts(h, w)
    _job_equals_statement(ctx, "flicker", nt, h, w, p, win, ("flat",), bounds=WHOLE_BOUNDS)
    want = MJ.statement("flicker", nt, h, w, p, win, *WHOLE_BOUNDS[0])
    nk = ~want["key"]
    assert want["modes"][nk][:, 2, 42].all() and want["vectors"][nk][:, 2, 42].any()   # the second trip's tile: bytes it must write
    assert 0 < want["modes"][nk].sum() < want["modes"][nk].size


# ------------------------------------------------------------------------------------------------- off is off
def test_closed_and_select_jobs_with_motion_off(contexts):
    """tz_set_pred_motion(0) right behind a motion rollout: the closed job and the select job give the bytes of their existing
    statements (tests/closedloop_jobs.py, tests/predselect_jobs.py) with the launches they had."""
    from tezip_amd import closedloop
    h, w = MJ.SIZES[1]
    nt, p, win = 7, 0, 3
    ctx = contexts(h, w)
    frames = np.ascontiguousarray(PJ.frames("flicker", nt, h, w))
    for mode, bound, quant in J.BOUNDS:
        for select in (False, True):
            want = (PJ.statement if select else PJ.closed_statement)("flicker", nt, h, w, p, win, mode, bound, quant, 0)
            ctx.set_quantiser(quant)
            ctx.set_pred_select(False)
            ctx.set_pred_motion(7)
            ctx.rollout_closed(frames, p, win, mode, list(bound))
            ctx.set_pred_motion(0)
            assert ctx.get_pred_motion() == 0
            ctx.set_pred_select(select)
            ctx.prof_enable(True)
            ctx.prof_reset()
            ctx.rollout_closed(frames, p, win, mode, list(bound))
            n_quant = ctx.prof_get()["quant"][1]
            ctx.prof_enable(False)
            assert n_quant == ((1 if select else 0) if bound[0] == 0 else 2), (bound, select, n_quant)
            assert ctx.lib.tz_pred_vectors(ctx.h, None, 0) == TZ_ERR_STATE
            if select:
                np.testing.assert_array_equal(ctx.pred_modes(), want["modes"])
            payload, table, delta = ctx.encode(mode, list(bound), True, want_delta=True)
            want_payload, want_table = closedloop.payload_of(want["q"], "flat")
            np.testing.assert_array_equal(delta, want["q"])
            np.testing.assert_array_equal(np.asarray(payload).reshape(-1), want_payload)
            np.testing.assert_array_equal(table, want_table)
            kf = np.zeros_like(frames)
            kf[want["key"]] = frames[want["key"]]
            ctx.put_pred_vectors(np.full((nt, 4, 6, 2), 3, np.int8))               # put, but motion is off: not read
            if select:
                ctx.put_pred_modes(want["modes"])
            ctx.rollout_decode_closed(kf, p, want_payload, want_table)
            np.testing.assert_array_equal(ctx.decoded_get(0, nt), want["dec"])
    _reset(ctx)


def test_state_and_invalid(contexts):
    import ctypes as C
    from tezip_amd import _lib, closedloop
    h, w = MJ.SIZES[0]
    nt, p, win = 7, 0, 3
    ctx = contexts(h, w)
    lib = ctx.lib
    frames = np.ascontiguousarray(MJ.frames("flicker", nt, h, w))
    for r in (1, 6, 8, -7):
        assert lib.tz_set_pred_motion(ctx.h, r) == TZ_ERR_INVALID
    assert lib.tz_set_pred_motion(None, 7) == TZ_ERR_INVALID and ctx.get_pred_motion() == 0
    # one second candidate a tile: motion excludes selection and the other way round
    ctx.set_pred_select(True)
    assert lib.tz_set_pred_motion(ctx.h, 7) == TZ_ERR_INVALID and "tz_set_pred_select" in lib.tz_last_error(ctx.h).decode()
    assert ctx.get_pred_motion() == 0
    ctx.set_pred_select(False)
    ctx.set_pred_motion(7)
    assert lib.tz_set_pred_select(ctx.h, 1) == TZ_ERR_INVALID and "tz_set_pred_motion" in lib.tz_last_error(ctx.h).decode()
    assert ctx.get_pred_select() == 0 and ctx.get_pred_motion() == 7
    # tz_pred_vectors without a motion rollout: the open loop, the closed loop alone, the select loop
    vec = np.zeros(nt * 2 * 3 * 2, np.int8)
    ctx.rollout(frames, p, win)                                               # the open loop ignores the setting
    assert lib.tz_pred_vectors(ctx.h, vec.ctypes.data, vec.size) == TZ_ERR_STATE
    ctx.set_pred_motion(0)
    ctx.rollout_closed(frames, p, win, "abs", [0.0])
    assert lib.tz_pred_vectors(ctx.h, vec.ctypes.data, vec.size) == TZ_ERR_STATE
    ctx.set_pred_select(True)
    ctx.rollout_closed(frames, p, win, "abs", [0.0])
    assert lib.tz_pred_vectors(ctx.h, vec.ctypes.data, vec.size) == TZ_ERR_STATE
    ctx.set_pred_select(False)
    # a motion rollout serves motion jobs alone, and the other way round
    table = np.zeros(_lib.TZ_MAX_TABLE, np.int16)
    pay = np.zeros(frames.size, np.int16)
    tlen = C.c_int(0)
    encode = lambda: lib.tz_encode(ctx.h, 0, 0.0, 0.0, 1, pay.ctypes.data, table.ctypes.data, C.byref(tlen), None)   # noqa: E731
    for ran_under in (7, 0):
        ctx.set_pred_motion(ran_under)
        ctx.rollout_closed(frames, p, win, "abs", [0.0])
        assert encode() == 0
        ctx.set_pred_motion(7 - ran_under)
        assert encode() == TZ_ERR_STATE
        msg = lib.tz_last_error(ctx.h).decode()
        assert "tz_encode" in msg and "tz_set_pred_motion" in msg and ("with" if ran_under else "without") + " motion" in msg, msg
        ctx.set_pred_motion(ran_under)
        assert encode() == 0
    ctx.set_pred_motion(7)
    ctx.rollout_closed(frames, p, win, "abs", [0.0])
    modes = np.zeros(nt * 2 * 3, np.uint8)
    assert lib.tz_pred_modes(ctx.h, modes.ctypes.data, modes.size) == 0       # tz_pred_modes serves a motion rollout
    assert lib.tz_pred_vectors(ctx.h, vec.ctypes.data, vec.size - 1) == TZ_ERR_INVALID
    assert lib.tz_pred_vectors(ctx.h, vec.ctypes.data, vec.size) == 0
    want = MJ.statement("flicker", nt, h, w, p, win, "abs", (0.0,), "greedy", 0)
    np.testing.assert_array_equal(modes.reshape(nt, 2, 3), want["modes"])
    np.testing.assert_array_equal(vec.reshape(nt, 2, 3, 2), want["vectors"])
    # the decoder's vectors
    kf = np.zeros_like(frames)
    kf[want["key"]] = frames[want["key"]]
    payload, tb = closedloop.payload_of(want["q"], "flat")
    payload = np.ascontiguousarray(payload)
    decode = lambda: lib.tz_rollout_decode_closed(ctx.h, kf.ctypes.data, nt, h, w, p, payload.ctypes.data, payload.size,   # noqa: E731
                                                  tb.ctypes.data, len(tb), None)
    put_v = lambda v, n=None: lib.tz_put_pred_vectors(ctx.h, v.ctypes.data, v.size if n is None else n)   # noqa: E731
    assert lib.tz_put_pred_modes(ctx.h, modes.ctypes.data, modes.size) == 0
    for value in (8, -8, 127, -128):
        bad = vec.copy()
        bad[9] = value
        assert put_v(bad) == TZ_ERR_INVALID                                   # a component outside -7 .. 7: at once
        assert "-7 .. 7" in lib.tz_last_error(ctx.h).decode()
    assert decode() == TZ_ERR_INVALID                                         # ... leaves nothing put
    assert put_v(vec, vec.size - 2) == 0 and decode() == TZ_ERR_INVALID       # a wrong n: from the rollout
    assert "vector components" in lib.tz_last_error(ctx.h).decode()
    tile0 = int(np.flatnonzero(((want["modes"] == 0) & ~want["key"][:, None, None]).reshape(-1))[0])   # a tile of mode 0 in a predicted frame
    bad = vec.copy()
    bad[2 * tile0 + 1] = -2
    assert put_v(bad) == 0 and decode() == TZ_ERR_INVALID
    assert "mode 0" in lib.tz_last_error(ctx.h).decode()
    bad = vec.copy()
    bad[2 * (3 * 6 + 1)] = 1                                                  # frame 3 is a key frame
    assert put_v(bad) == 0 and decode() == TZ_ERR_INVALID
    assert "key frame 3" in lib.tz_last_error(ctx.h).decode()
    assert ctx.pool_held()[0] == 0
    assert put_v(vec) == 0 and decode() == 0
    np.testing.assert_array_equal(ctx.decoded_get(0, nt), frames)
    _reset(ctx)


# ------------------------------------------------------------------------------------------------ the command line
NT, H, W = 7, 24, 40
JOB = ["-p", "0", "-w", "3"]
PM = ["--loop", "closed", "--pred", "motion"]


@pytest.fixture(scope="module")
def job(tmp_path_factory):
    """model directory, image directory, names and frames (the flicker scene), on disk once"""
    from PIL import Image
    from tezip_amd import weights
    root = tmp_path_factory.mktemp("predmotion_cli")
    frames = np.ascontiguousarray(MJ.frames("flicker", NT, H, W))
    cfg, wts = J.model()
    mdir = str(root / "model")
    weights.save_model(mdir, cfg, wts, 24, 40)
    ddir = root / "data"
    ddir.mkdir()
    names = ["f_%03d.png" % t for t in range(NT)]
    for t, n in enumerate(names):
        Image.fromarray(frames[t]).save(ddir / n)
    return mdir, str(ddir), names, frames


def _tezip(argv, capsys):
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


def _files(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d))}


def _pred_line(want):
    nk = ~want["key"]
    m, v = want["modes"][nk], want["vectors"][nk]
    return "pred: motion (TZ-PM1), %d of %d tiles from the frame in front (%.1f %%), %d displaced" % (
        m.sum(), m.size, 100.0 * m.sum() / m.size, v.any(axis=-1).sum())


def test_cli_lossless_round_trip_flipped_vector_and_malformed_files(tmp_path, job, capsys, monkeypatch):
    from tezip_amd import closedloop, decompress, predmotion, predselect, zstd
    mdir, ddir, names, frames = job
    comp, dec = str(tmp_path / "comp"), str(tmp_path / "dec")
    status, out = _tezip(["-c", mdir, ddir, comp] + JOB + ["-m", "abs", "-b", "0"] + PM + ["--digests", "--report"], capsys)
    assert status == 0, out
    want = MJ.statement("flicker", NT, H, W, 0, 3, "abs", (0.0,), "greedy", 0)
    nk = ~want["key"]
    m, v = want["modes"][nk], want["vectors"][nk]
    lines = out.splitlines()
    line = _pred_line(want)
    assert lines.count(line) == 1 and lines.index(line) == lines.index("loop: closed (TZ-CL1)") + 1, out
    assert sorted(os.listdir(comp)) == ["entropy.dat", "filename.txt", "frame_digests.json", "key_frame.dat", "pred_modes.dat", "quality.json",
                                        "tezip_amd.json"]
    doc = json.load(open(os.path.join(comp, "tezip_amd.json")))
    assert doc["pred"] == "motion" and doc["loop"] == "closed"
    stored = open(os.path.join(comp, "pred_modes.dat"), "rb").read()
    assert stored == predmotion.pack(want["modes"], want["vectors"])
    payload, table, shape, warm_up = decompress.parse_stream(zstd.decompress(open(os.path.join(comp, "entropy.dat"), "rb").read()))
    assert shape == (81, NT, H, W, 3)
    np.testing.assert_array_equal(payload, closedloop.payload_of(want["q"], "flat")[0])
    quality = json.load(open(os.path.join(comp, "quality.json")))
    assert quality["pred_motion"] == {"tiles": int(m.size), "prev_tiles": int(m.sum()), "displaced_tiles": int(v.any(axis=-1).sum())}
    assert quality["lossless"] and "pred_select" not in quality
    sizes = sum(os.path.getsize(os.path.join(comp, n)) for n in ("filename.txt", "key_frame.dat", "entropy.dat", "pred_modes.dat"))
    assert quality["stored_bytes"] == sizes and "ratio: %.4f" % (frames.size / sizes) in lines
    for env in ({}, {"TEZIP_NO_STREAMING": "1"}):
        for k, val in env.items():
            monkeypatch.setenv(k, val)
        d = dec + "".join(env)
        status, out = _tezip(["-u", mdir, comp, d, "--verify", "require"], capsys)
        assert status == 0 and "verified: %d frames" % NT in out, out
        np.testing.assert_array_equal(_images(d, names), frames)             # byte for byte
        status, out = _tezip(["-u", mdir, comp, d + "_r", "--frames", "1:3"], capsys)
        assert status == 2 and "--frames" in out
    monkeypatch.delenv("TEZIP_NO_STREAMING")
    # one changed vector byte (the first chosen tile's dx, still inside 0 .. 14): the digests catch it
    path = os.path.join(comp, "pred_modes.dat")
    at = 24 + (NT * 2 * 3 + 7) // 8
    flipped = bytearray(stored)
    flipped[at] += 1 if flipped[at] & 15 < 14 else -1
    open(path, "wb").write(bytes(flipped))
    d = str(tmp_path / "dec_flip")
    status, out = _tezip(["-u", mdir, comp, d], capsys)
    assert status == 3 and names[int(np.argwhere(want["modes"])[0][0])] in out, out      # the frame of the first chosen tile
    assert not os.path.exists(d) or os.listdir(d) == []
    # malformed files: one ERROR line, status 2
    radius = stored[:20] + (8).to_bytes(4, "little") + stored[24:]
    for data, needle in ((stored[:-1], "truncated"), (stored[:at - 2], "truncated"), (stored + b"\0", "too long"),
                         (predselect.pack(want["modes"]), "magic"), (radius, "search radius"), (stored[:at] + b"\xf3" + stored[at + 1:], "nibble of 15"),
                         (stored[:at - 1] + bytes([stored[at - 1] | 0x80]) + stored[at:], "pad bit"), (None, "missing")):
        if data is None:
            os.remove(path)
        else:
            open(path, "wb").write(data)
        d = str(tmp_path / ("dec_" + needle.replace(" ", "_")))
        status, out = _tezip(["-u", mdir, comp, d], capsys)
        errors = [ln for ln in out.splitlines() if ln.startswith("ERROR:")]
        assert status == 2 and len(errors) == 1 and needle in errors[0], out
        assert not os.path.exists(d) or os.listdir(d) == []
    # a sidecar that contradicts the mark
    open(path, "wb").write(stored)
    side = os.path.join(comp, "tezip_amd.json")
    for pred, says in ((None, "net"), ("select", "select")):
        other = dict(doc)
        del other["pred"]
        if pred:
            other["pred"] = pred
            open(path, "wb").write(predselect.pack(want["modes"]))           # (what such a sidecar's early check wants to see)
        json.dump(other, open(side, "w"))
        status, out = _tezip(["-u", mdir, comp, str(tmp_path / ("dec_x_" + says))], capsys)
        assert status == 2 and "prediction as %s, entropy.dat's trailer as motion" % says in out, out
    open(path, "wb").write(stored)
    os.remove(side)                                                          # no sidecar: the trailer alone decides
    d = str(tmp_path / "dec_y")
    status, out = _tezip(["-u", mdir, comp, d, "--verify", "require"], capsys)
    assert status == 0, out
    np.testing.assert_array_equal(_images(d, names), frames)
    open(path, "wb").write(predselect.pack(want["modes"]))                   # a TZP1 file under the motion mark
    status, out = _tezip(["-u", mdir, comp, str(tmp_path / "dec_z")], capsys)
    assert status == 2 and "wrong magic" in out, out


def test_cli_select_stream_with_a_tzp2_file_is_refused(tmp_path, job, capsys):
    from tezip_amd import predmotion
    mdir, ddir, names, frames = job
    comp = str(tmp_path / "comp")
    status, out = _tezip(["-c", mdir, ddir, comp] + JOB + ["-m", "abs", "-b", "0", "--loop", "closed", "--pred", "select"], capsys)
    assert status == 0, out
    want = MJ.statement("flicker", NT, H, W, 0, 3, "abs", (0.0,), "greedy", 0)
    predmotion.write(comp, want["modes"], want["vectors"])
    status, out = _tezip(["-u", mdir, comp, str(tmp_path / "dec")], capsys)
    assert status == 2 and "wrong magic" in out, out


def test_cli_lattice_bound_with_gpu_coders(tmp_path, job, capsys):
    mdir, ddir, names, frames = job
    comp, dec = str(tmp_path / "comp"), str(tmp_path / "dec")
    status, out = _tezip(["-c", mdir, ddir, comp] + JOB + ["-m", "abs", "-b", "6", "--quant", "lattice"] + PM +
                         ["--digests", "--coder", "huffd", "--sdelta", "auto", "--key-coder", "huff"], capsys)
    assert status == 0, out
    from tezip_amd import huffd
    assert huffd.parse(np.fromfile(os.path.join(comp, "entropy.dat"), np.uint8)).shape[0] in (81, 84, 88)
    want = MJ.statement("flicker", NT, H, W, 0, 3, "abs", (6.0,), "lattice", 0)
    assert _pred_line(want) in out.splitlines()
    status, out = _tezip(["-u", mdir, comp, dec, "--verify", "require"], capsys)
    assert status == 0 and "verified: %d frames" % NT in out, out
    got = _images(dec, names)
    assert np.abs(got.astype(int) - frames.astype(int)).max() <= 6
    np.testing.assert_array_equal(got, want["dec"])
    # a changed vector byte is caught here too
    path = os.path.join(comp, "pred_modes.dat")
    data = bytearray(open(path, "rb").read())
    at = 24 + (NT * 2 * 3 + 7) // 8
    data[at] += 1 if data[at] & 15 < 14 else -1
    open(path, "wb").write(bytes(data))
    status, out = _tezip(["-u", mdir, comp, str(tmp_path / "dec_flip")], capsys)
    assert status == 3, out


def test_cli_pred_net_writes_the_files_of_no_flag(tmp_path, job, capsys):
    mdir, ddir, names, frames = job
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    args = JOB + ["-m", "abs", "-b", "2", "--quant", "lattice", "--loop", "closed", "--report"]
    status, out_a = _tezip(["-c", mdir, ddir, a] + args, capsys)
    assert status == 0, out_a
    status, out_b = _tezip(["-c", mdir, ddir, b] + args + ["--pred", "net"], capsys)
    assert status == 0, out_b
    assert _files(a) == _files(b) and out_a == out_b
    assert "pred_modes.dat" not in os.listdir(a) and "pred" not in json.load(open(os.path.join(a, "tezip_amd.json"))) and "pred:" not in out_a
