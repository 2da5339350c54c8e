"""Per-tile selection TZ-PS1 on a MI355X (tz_set_pred_select, tz_pred_modes, tz_put_pred_modes, k_ps_select, k_ps_step, k_ps_recon):
the library held bit for bit to the slow statement (tezip_amd/predselect.py with the C oracle's PredNet; tests/test_predselect.py
holds that statement to first principles) -- mode bytes, the prediction stack with the chosen tiles expressed in it, payload and
table in every layout, the decoded stack -- at 24 x 40 (1.5 x 2.5 tiles, unpadded, the 4-byte path) and 61 x 90 (pads to 64 x 96,
rows of 270 bytes: byte by byte), on the translating scene (random weights: the frame in front wins every tile) and on the flicker
scene (both modes); past one grid of workgroups; and the command line end to end."""
import json
import os

import numpy as np
import pytest

import closedloop_jobs as J
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


def _job_equals_statement(ctx, scene, nt, h, w, p, win, layouts, contract=0, bounds=PJ.BOUNDS):
    from tezip_amd import closedloop
    frames = np.ascontiguousarray(PJ.frames(scene, nt, h, w))
    for mode, bound, quant in bounds:
        what = "%s %dx%dx%d p%d w%d %s %g %s" % (scene, nt, h, w, p, win, mode, bound[0], quant)
        want = PJ.statement(scene, nt, h, w, p, win, mode, bound, quant, contract)
        ctx.set_quantiser(quant)
        ctx.set_pred_select(True)
        _layout(ctx, "flat")
        key = ctx.rollout_closed(frames, p, win, mode, list(bound))
        assert ctx.pool_held()[0] == 0
        np.testing.assert_array_equal(key, want["key"], err_msg=what)
        modes = ctx.pred_modes()
        assert modes.dtype == np.uint8 and modes.shape == want["modes"].shape
        np.testing.assert_array_equal(modes, want["modes"], err_msg=what)                  # byte for byte
        _same_predictions(ctx, want, h, w, what)
        for layout in layouts:
            _layout(ctx, layout)
            payload, table, delta = ctx.encode(mode, list(bound), True, want_delta=True)
            want_payload, want_table = closedloop.payload_of(want["q"], layout)
            np.testing.assert_array_equal(delta, want["q"], err_msg=what + " " + layout)
            np.testing.assert_array_equal(table, want_table, err_msg=what + " " + layout)
            np.testing.assert_array_equal(np.asarray(payload).reshape(-1), want_payload, err_msg=what + " " + layout)
        # the decoder: key stack, payload and modes alone
        kf = np.zeros_like(frames)
        kf[want["key"]] = frames[want["key"]]
        for layout in layouts:
            _layout(ctx, layout)
            payload, table = closedloop.payload_of(want["q"], layout)
            ctx.put_pred_modes(want["modes"])
            dkey = ctx.rollout_decode_closed(kf, p, payload, table)
            assert ctx.pool_held()[0] == 0
            np.testing.assert_array_equal(dkey, want["key"], err_msg=what + " " + layout)
            np.testing.assert_array_equal(ctx.decoded_get(0, nt), want["dec"], err_msg=what + " decoder " + layout)
            _same_predictions(ctx, want, h, w, what + " decoder " + layout)
    _reset(ctx)


@pytest.mark.parametrize("scene", PJ.SCENES)
@pytest.mark.parametrize("h,w", PJ.SIZES)
@pytest.mark.parametrize("nt,p,win", PJ.TRIPLES)
def test_library_equals_the_statement(contexts, nt, p, win, h, w, scene):
    _job_equals_statement(contexts(h, w), scene, nt, h, w, p, win, PJ.LAYOUTS)


@pytest.mark.parametrize("contract", [1, 2])
def test_both_arithmetic_contracts(contexts, contract):
    h, w = PJ.SIZES[1]
    ctx = contexts(h, w, contract)
    assert ctx.get_contract() == contract
    _job_equals_statement(ctx, "flicker", 7, h, w, 0, 3, ("flat",), contract=contract)
    assert ctx.rollout_contract() == contract


# ------------------------------------------------------------------------------------------------ the whole launch
# k_ps_* start min(strips, PS_GRID = 64) workgroups a frame, a strip being 4 tiles of one tile row: strips = TH * ceil(TW / 4).
# The smallest frames with more strips than that have TH * ceil(TW / 4) = 65 = 13 * 5: 13 tile rows (H in 193 .. 208) of 17 tiles
# (W in 257 .. 272), where workgroup 0 takes a second trip (strip 64: tile row 12, tiles 16 .. 19 of which one exists).
# 200 x 260 is the 4-byte path with no padding rows; 193 x 257 the byte path, one row in the last tile row and one column in the
# last tile.  Both pad to 200 x 264 and share a context.
WHOLE = [(200, 260), (193, 257)]
WHOLE_JOB = (4, 0, 3)
WHOLE_BOUNDS = [PJ.BOUNDS[0], PJ.BOUNDS[2]]


def _strips(h, w):
    th, tw = -(-h // 16), -(-w // 16)
    return th * -(-tw // 4)


def test_the_whole_launch_shapes_cross_the_grid():
    assert [_strips(h, w) for h, w in WHOLE] == [65, 65]
    assert _strips(192, 272) <= 64 and _strips(208, 256) <= 64               # one tile row or one tile less: one trip


@pytest.mark.parametrize("h,w", WHOLE)
def test_past_one_grid_of_workgroups(contexts, h, w):
    nt, p, win = WHOLE_JOB
    ctx = contexts(h, w)
    _job_equals_statement(ctx, "flicker", nt, h, w, p, win, ("flat",), bounds=WHOLE_BOUNDS)
    want = PJ.statement("flicker", nt, h, w, p, win, *WHOLE_BOUNDS[0])
    last = want["modes"][~want["key"]][:, 12, 16]                            # the second trip's tile
    assert last.shape == (2,) and last.all()                               # ... takes the frame in front: a byte the trip must write
    both = want["modes"][~want["key"]]
    assert 0 < both.sum() < both.size


# ------------------------------------------------------------------------------------------------- off is off
def test_unchanged_launches_with_selection_off(contexts):
    """tz_set_pred_select(0): the closed-loop job gives the bytes of tests/closedloop_jobs.py's statement, with the launches of
    the closed loop alone (no k_ps_* under the quantiser's profiler slot), also right behind a select rollout."""
    from tezip_amd import closedloop
    h, w = PJ.SIZES[1]
    nt, p, win = 7, 0, 3
    ctx = contexts(h, w)
    frames = np.ascontiguousarray(J.frames(nt, h, w))
    for mode, bound, quant in J.BOUNDS:
        want = J.statement(nt, h, w, p, win, mode, bound, quant, 0)
        ctx.set_quantiser(quant)
        ctx.set_pred_select(True)
        ctx.rollout_closed(frames, p, win, mode, list(bound))
        ctx.set_pred_select(False)
        assert ctx.get_pred_select() == 0
        ctx.prof_enable(True)
        ctx.prof_reset()
        ctx.rollout_closed(frames, p, win, mode, list(bound))
        n_quant = ctx.prof_get()["quant"][1]
        ctx.prof_enable(False)
        assert n_quant == (0 if bound[0] == 0 else 2), (bound, n_quant)      # k_cl_step once per step of a lossy loop, nothing else
        assert ctx.lib.tz_pred_modes(ctx.h, None, 0) == TZ_ERR_STATE
        payload, table, delta = ctx.encode(mode, list(bound), True, want_delta=True)
        want_payload, want_table = closedloop.payload_of(want["q"], "flat")
        np.testing.assert_array_equal(delta, want["q"])
        np.testing.assert_array_equal(np.asarray(payload).reshape(-1), want_payload)
        np.testing.assert_array_equal(table, want_table)
        kf = np.zeros_like(frames)
        kf[want["key"]] = frames[want["key"]]
        ctx.put_pred_modes(np.ones((nt, 4, 6), np.uint8))                     # put, but selection is off: not read
        ctx.rollout_decode_closed(kf, p, want_payload, want_table)
        np.testing.assert_array_equal(ctx.decoded_get(0, nt), want["dec"])
    _reset(ctx)


def test_state_and_invalid(contexts):
    import ctypes as C
    from tezip_amd import _lib
    h, w = PJ.SIZES[0]
    nt, p, win = 7, 0, 3
    ctx = contexts(h, w)
    lib = ctx.lib
    frames = np.ascontiguousarray(PJ.frames("flicker", nt, h, w))
    assert lib.tz_set_pred_select(ctx.h, 2) == TZ_ERR_INVALID and lib.tz_set_pred_select(None, 1) == TZ_ERR_INVALID
    out = np.zeros(nt * 2 * 3, np.uint8)
    ctx.rollout(frames, p, win)                                               # the open loop ignores the setting
    ctx.set_pred_select(True)
    key, _ = ctx.rollout(frames, p, win)
    assert lib.tz_pred_modes(ctx.h, out.ctypes.data, out.size) == TZ_ERR_STATE
    payload, table, _ = ctx.encode("abs", [0.0], True)
    ctx.set_pred_select(False)
    payload2, table2, _ = ctx.encode("abs", [0.0], True)
    np.testing.assert_array_equal(np.asarray(payload), np.asarray(payload2))
    # a select rollout serves select jobs alone, and the other way round
    table = np.zeros(_lib.TZ_MAX_TABLE, np.int16)
    pay = np.zeros(frames.size, np.int16)
    tlen = C.c_int(0)
    encode = lambda: lib.tz_encode(ctx.h, 0, 0.0, 0.0, 1, pay.ctypes.data, table.ctypes.data, C.byref(tlen), None)   # noqa: E731
    for ran_under in (True, False):
        ctx.set_pred_select(ran_under)
        ctx.rollout_closed(frames, p, win, "abs", [0.0])
        assert encode() == 0
        ctx.set_pred_select(not ran_under)
        assert encode() == TZ_ERR_STATE
        msg = lib.tz_last_error(ctx.h).decode()
        assert "tz_encode" in msg and "tz_set_pred_select" in msg and ("with" if ran_under else "without") + " per-tile" in msg, msg
        ctx.set_pred_select(ran_under)
        assert encode() == 0
    ctx.set_pred_select(True)
    ctx.rollout_closed(frames, p, win, "abs", [0.0])
    assert lib.tz_pred_modes(ctx.h, out.ctypes.data, out.size - 1) == TZ_ERR_INVALID
    assert lib.tz_pred_modes(ctx.h, out.ctypes.data, out.size) == 0
    # the decoder's modes
    want = PJ.statement("flicker", nt, h, w, p, win, "abs", (0.0,), "greedy", 0)
    np.testing.assert_array_equal(out.reshape(nt, 2, 3), want["modes"])
    from tezip_amd import closedloop
    kf = np.zeros_like(frames)
    kf[want["key"]] = frames[want["key"]]
    payload, tb = closedloop.payload_of(want["q"], "flat")
    payload = np.ascontiguousarray(payload)
    decode = lambda: lib.tz_rollout_decode_closed(ctx.h, kf.ctypes.data, nt, h, w, p, payload.ctypes.data, payload.size,   # noqa: E731
                                                  tb.ctypes.data, len(tb), None)
    bad = out.copy()
    bad[7] = 2
    assert lib.tz_put_pred_modes(ctx.h, bad.ctypes.data, bad.size) == TZ_ERR_INVALID                # a byte above 1
    assert decode() == TZ_ERR_INVALID                                                                # ... leaves nothing put
    assert lib.tz_put_pred_modes(ctx.h, out.ctypes.data, out.size - 1) == 0 and decode() == TZ_ERR_INVALID   # a wrong n
    assert "mode bytes" in lib.tz_last_error(ctx.h).decode()
    bad = out.copy()
    bad[3 * 6 + 1] = 1                                                                               # frame 3 is a key frame
    assert lib.tz_put_pred_modes(ctx.h, bad.ctypes.data, bad.size) == 0 and decode() == TZ_ERR_INVALID
    assert "key frame 3" in lib.tz_last_error(ctx.h).decode()
    assert ctx.pool_held()[0] == 0
    assert lib.tz_put_pred_modes(ctx.h, out.ctypes.data, out.size) == 0 and decode() == 0
    np.testing.assert_array_equal(ctx.decoded_get(0, nt), frames)
    _reset(ctx)


# ------------------------------------------------------------------------------------------------ the command line
NT, H, W = 7, 24, 40
JOB = ["-p", "0", "-w", "3"]


@pytest.fixture(scope="module")
def job(tmp_path_factory):
    """model directory, image directory, names and frames (the flicker scene), on disk once"""
    from PIL import Image
    from tezip_amd import weights
    root = tmp_path_factory.mktemp("predselect_cli")
    frames = np.ascontiguousarray(PJ.frames("flicker", NT, H, W))
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


def test_cli_lossless_round_trip_flipped_bit_and_truncation(tmp_path, job, capsys, monkeypatch):
    from tezip_amd import decompress, predselect, zstd
    mdir, ddir, names, frames = job
    comp, dec = str(tmp_path / "comp"), str(tmp_path / "dec")
    status, out = _tezip(["-c", mdir, ddir, comp] + JOB + ["-m", "abs", "-b", "0", "--loop", "closed", "--pred", "select", "--digests",
                                                           "--report"], capsys)
    assert status == 0, out
    want = PJ.statement("flicker", NT, H, W, 0, 3, "abs", (0.0,), "greedy", 0)
    m = want["modes"][~want["key"]]
    lines = out.splitlines()
    line = "pred: select (TZ-PS1), %d of %d tiles from the frame in front (%.1f %%)" % (m.sum(), m.size, 100.0 * m.sum() / m.size)
    assert lines.count(line) == 1 and lines.index(line) == lines.index("loop: closed (TZ-CL1)") + 1, out
    assert sorted(os.listdir(comp)) == ["entropy.dat", "filename.txt", "frame_digests.json", "key_frame.dat", "pred_modes.dat", "quality.json",
                                        "tezip_amd.json"]
    doc = json.load(open(os.path.join(comp, "tezip_amd.json")))
    assert doc["pred"] == "select" and doc["loop"] == "closed"
    stored = open(os.path.join(comp, "pred_modes.dat"), "rb").read()
    assert stored == predselect.pack(want["modes"])
    payload, table, shape, warm_up = decompress.parse_stream(zstd.decompress(open(os.path.join(comp, "entropy.dat"), "rb").read()))
    assert shape == (49, NT, H, W, 3)
    np.testing.assert_array_equal(payload, predselect.closedloop.payload_of(want["q"], "flat")[0])
    quality = json.load(open(os.path.join(comp, "quality.json")))
    assert quality["pred_select"] == {"tiles": int(m.size), "prev_tiles": int(m.sum())} and quality["lossless"]
    sizes = sum(os.path.getsize(os.path.join(comp, n)) for n in ("filename.txt", "key_frame.dat", "entropy.dat", "pred_modes.dat"))
    assert quality["stored_bytes"] == sizes and "ratio: %.4f" % (frames.size / sizes) in lines
    for env in ({}, {"TEZIP_NO_STREAMING": "1"}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        d = dec + "".join(env)
        status, out = _tezip(["-u", mdir, comp, d, "--verify", "require"], capsys)
        assert status == 0 and "verified: %d frames" % NT in out, out
        np.testing.assert_array_equal(_images(d, names), frames)             # byte for byte
        status, out = _tezip(["-u", mdir, comp, d + "_r", "--frames", "1:3"], capsys)
        assert status == 2 and "--frames" in out
    monkeypatch.delenv("TEZIP_NO_STREAMING")
    # one flipped bit at a non-key frame (frame 1, tile 0): the digests catch it
    path = os.path.join(comp, "pred_modes.dat")
    flipped = bytearray(stored)
    flipped[20] ^= 1 << 6
    open(path, "wb").write(bytes(flipped))
    d = str(tmp_path / "dec_flip")
    status, out = _tezip(["-u", mdir, comp, d], capsys)
    assert status == 3 and names[1] in out, out
    assert not os.path.exists(d) or os.listdir(d) == []
    # a truncated file, a wrong magic, a set pad bit, a missing file: one ERROR line, status 2
    for data, needle in ((stored[:-1], "truncated"), (b"TZP0" + stored[4:], "magic"), (stored[:-1] + bytes([stored[-1] | 0x80]), "pad bit"),
                         (None, "missing")):
        if data is None:
            os.remove(path)
        else:
            open(path, "wb").write(data)
        d = str(tmp_path / ("dec_" + needle.replace(" ", "_")))
        status, out = _tezip(["-u", mdir, comp, d], capsys)
        lines = [ln for ln in out.splitlines() if ln.startswith("ERROR:")]
        assert status == 2 and len(lines) == 1 and needle in lines[0], out
        assert not os.path.exists(d) or os.listdir(d) == []
    # a sidecar that contradicts the mark
    open(path, "wb").write(stored)
    side = os.path.join(comp, "tezip_amd.json")
    del doc["pred"]
    json.dump(doc, open(side, "w"))
    status, out = _tezip(["-u", mdir, comp, str(tmp_path / "dec_x")], capsys)
    assert status == 2 and "prediction as net, entropy.dat's trailer as select" in out, out
    os.remove(side)                                                          # no sidecar: the trailer alone decides
    d = str(tmp_path / "dec_y")
    status, out = _tezip(["-u", mdir, comp, d, "--verify", "require"], capsys)
    assert status == 0, out
    np.testing.assert_array_equal(_images(d, names), frames)


def test_cli_lattice_bound_with_gpu_coders(tmp_path, job, capsys):
    mdir, ddir, names, frames = job
    comp, dec = str(tmp_path / "comp"), str(tmp_path / "dec")
    status, out = _tezip(["-c", mdir, ddir, comp] + JOB + ["-m", "abs", "-b", "6", "--quant", "lattice", "--loop", "closed", "--pred", "select",
                                                           "--digests", "--coder", "huffd", "--sdelta", "auto", "--key-coder", "huff"], capsys)
    assert status == 0, out
    from tezip_amd import huffd
    assert huffd.parse(np.fromfile(os.path.join(comp, "entropy.dat"), np.uint8)).shape[0] in (49, 52, 56)
    want = PJ.statement("flicker", NT, H, W, 0, 3, "abs", (6.0,), "lattice", 0)
    status, out = _tezip(["-u", mdir, comp, dec, "--verify", "require"], capsys)
    assert status == 0 and "verified: %d frames" % NT in out, out
    got = _images(dec, names)
    assert np.abs(got.astype(int) - frames.astype(int)).max() <= 6
    np.testing.assert_array_equal(got, want["dec"])


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
