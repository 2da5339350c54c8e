"""Closed-loop prediction TZ-CL1 on a MI355X (tz_rollout_closed, tz_rollout_decode_closed, k_cl_step, k_cl_recon): the library held
bit for bit to the slow statement (tezip_amd/closedloop.py with the C oracle's PredNet; tests/test_closedloop.py holds that
statement to first principles) on the same jobs -- key mask, predictions, payload and table in every layout, the decoded stack --
with one window per batch and several, more windows than batch slots, TZ-PA2, staged frames and a resident payload."""
import numpy as np
import pytest

import closedloop_jobs as J

pytestmark = pytest.mark.gpu

TZ_ERR_STATE, TZ_ERR_UNSUPPORTED = -4, -6


@pytest.fixture(scope="module")
def contexts():
    """One context per (H, W, max_batch), model loaded and prepared."""
    from tezip_amd import _lib
    made = {}

    def get(h, w, max_batch):
        if (h, w, max_batch) not in made:
            cfg, wts = J.model()
            c = _lib.Context(0)
            c.load_model(cfg, wts)
            c.prepare(_lib.pad8(h), _lib.pad8(w), max_batch)
            made[h, w, max_batch] = c
        c = made[h, w, max_batch]
        _reset(c)
        return c
    yield get
    for c in made.values():
        c.close()


def _reset(ctx):
    ctx.set_quantiser(0)
    ctx.set_frame_bounds(None)
    ctx.set_bound_map(None)
    ctx.set_payload_channels(3)
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
    got = ctx.get_predictions()
    nk = ~want["key"]
    np.testing.assert_array_equal(_bits(got[nk][:, :h, :w]), _bits(want["pred"][nk][:, :h, :w]), err_msg=what)
    return got


def _idle(ctx):
    assert ctx.pool_held()[0] == 0


def _job_equals_statement(ctx, nt, h, w, p, win, layouts, contract=0):
    from tezip_amd import closedloop
    frames = np.ascontiguousarray(J.frames(nt, h, w))
    for mode, bound, quant in J.BOUNDS:
        what = "%dx%dx%d p%d w%d %s %g %s" % (nt, h, w, p, win, mode, bound[0], quant)
        want = J.statement(nt, h, w, p, win, mode, bound, quant, contract)
        ctx.set_quantiser(quant)
        _layout(ctx, "flat")
        key = ctx.rollout_closed(frames, p, win, mode, list(bound))
        _idle(ctx)
        np.testing.assert_array_equal(key, want["key"], err_msg=what)
        assert ctx.rollout_loop() == 1
        _same_predictions(ctx, want, h, w, what)
        kf = np.zeros_like(frames)
        kf[want["key"]] = frames[want["key"]]
        for layout in layouts:
            _layout(ctx, layout)
            payload, table, delta = ctx.encode(mode, list(bound), True, want_delta=True)
            _idle(ctx)
            want_payload, want_table = closedloop.payload_of(want["q"], layout)
            np.testing.assert_array_equal(delta, want["q"], err_msg=what + " " + layout)
            np.testing.assert_array_equal(table, want_table, err_msg=what + " " + layout)
            np.testing.assert_array_equal(np.asarray(payload).reshape(-1), want_payload, err_msg=what + " " + layout)
        for layout in layouts:   # (the encoder's predictions are gone after the first of these)
            _layout(ctx, layout)
            payload, table = closedloop.payload_of(want["q"], layout)
            dkey = ctx.rollout_decode_closed(kf, p, payload, table)
            _idle(ctx)
            np.testing.assert_array_equal(dkey, want["key"], err_msg=what + " " + layout)
            np.testing.assert_array_equal(ctx.decoded_get(0, nt), want["dec"], err_msg=what + " " + layout)
            _same_predictions(ctx, want, h, w, what + " decoder " + layout)
            assert ctx.rollout_loop() == 0
    _reset(ctx)


@pytest.mark.parametrize("max_batch", [1, 4])
@pytest.mark.parametrize("h,w", J.SIZES)
@pytest.mark.parametrize("nt,p,win", J.TRIPLES)
def test_library_equals_the_statement(contexts, nt, p, win, h, w, max_batch):
    # every layout on the jobs with two steps per window, flat on the others
    layouts = J.LAYOUTS if win == 3 else ("flat",)
    _job_equals_statement(contexts(h, w, max_batch), nt, h, w, p, win, layouts)


def test_more_windows_than_batch_slots(contexts):
    h, w = J.SIZES[1]
    _job_equals_statement(contexts(h, w, 2), 9, h, w, 0, 2, ("flat", "plane"))     # four windows, two slots


def test_tz_pa2_on_both_sides(contexts):
    ctx = contexts(256, 256, 1)
    assert ctx.get_contract() == 2
    _job_equals_statement(ctx, 3, 256, 256, 0, 2, ("flat",), contract=0)
    assert ctx.rollout_contract() == 2


def test_staged_frames_and_resident_payload(contexts):
    from tezip_amd import closedloop
    h, w = J.SIZES[1]
    nt, p, win = 7, 1, 2
    ctx = contexts(h, w, 4)
    frames = np.ascontiguousarray(J.frames(nt, h, w))
    want = J.statement(nt, h, w, p, win, "abs", (6.0,), "lattice", 0)
    ctx.set_quantiser("lattice")
    _layout(ctx, "channel")
    ctx.frames_begin(nt, h, w)
    ctx.frames_put(0, frames[:3])
    ctx.frames_put(3, frames[3:])
    np.testing.assert_array_equal(ctx.rollout_closed(None, p, win, "abs", [6.0]), want["key"])
    _, table, _ = ctx.encode("abs", [6.0], True, payload="resident")
    want_payload, want_table = closedloop.payload_of(want["q"], "channel")
    np.testing.assert_array_equal(table, want_table)
    np.testing.assert_array_equal(ctx.payload_get(0, want_payload.size), want_payload)
    q = ctx.encode_quality("resident", table)          # the decoder's tail on the final predictions: what -u writes
    assert int(q["max_abs"].max()) == int(np.abs(want["dec"].astype(int) - frames.astype(int)).max()) <= 6
    np.testing.assert_array_equal(q["sse"], ((want["dec"].astype(np.int64) - frames) ** 2).reshape(nt, -1).sum(1))
    kf = np.zeros_like(frames)
    kf[want["key"]] = frames[want["key"]]
    ctx.frames_begin(nt, h, w)
    ctx.frames_put(0, kf)
    ctx.payload_begin(want_payload.size)
    ctx.payload_put(0, want_payload[:1000])
    ctx.payload_put(1000, want_payload[1000:])
    np.testing.assert_array_equal(ctx.rollout_decode_closed(None, p, None, table), want["key"])
    np.testing.assert_array_equal(ctx.decoded_get(0, nt), want["dec"])
    np.testing.assert_array_equal(ctx.decoded_get(2, 3), want["dec"][2:5])
    from tezip_amd import digest
    np.testing.assert_array_equal(ctx.decoded_digests(0, nt), [digest.frame_digest(f) for f in want["dec"]])
    _idle(ctx)
    _reset(ctx)


def test_device_stacks(contexts):
    import torch
    h, w = J.SIZES[1]
    nt, p, win = 7, 0, 3
    ctx = contexts(h, w, 4)
    frames = np.ascontiguousarray(J.frames(nt, h, w))
    want = J.statement(nt, h, w, p, win, "abs", (2.0,), "lattice", 0)
    ctx.set_quantiser("lattice")
    np.testing.assert_array_equal(ctx.rollout_closed(torch.from_numpy(frames.copy()).cuda(), p, win, "abs", [2.0]), want["key"])
    _same_predictions(ctx, want, h, w, "device frames")
    from tezip_amd import closedloop
    payload, table = closedloop.payload_of(want["q"], "flat")
    kf = np.zeros_like(frames)
    kf[want["key"]] = frames[want["key"]]
    ctx.rollout_decode_closed(torch.from_numpy(kf).cuda(), p, torch.from_numpy(np.array(payload)).cuda(), table)
    np.testing.assert_array_equal(ctx.decoded_get(0, nt), want["dec"])
    _reset(ctx)


def test_a_no_op_cannot_pass(contexts):
    """The closed predictions are not the open-loop ones, and the lossy loop feeds the decoded frame, not the original."""
    h, w = J.SIZES[0]
    nt, p, win = 7, 0, 3
    ctx = contexts(h, w, 4)
    frames = np.ascontiguousarray(J.frames(nt, h, w))
    key, _ = ctx.rollout(frames, p, win)
    open_pred = ctx.get_predictions().copy()
    assert ctx.rollout_loop() == 0
    want_open = J.open_loop(nt, h, w, p, win, 0)
    nk = ~key
    np.testing.assert_array_equal(_bits(open_pred[nk]), _bits(want_open["pred"][nk]))
    ctx.rollout_closed(frames, p, win, "abs", [0.0])
    lossless = ctx.get_predictions().copy()
    ctx.set_quantiser("lattice")
    ctx.rollout_closed(frames, p, win, "abs", [6.0])
    lossy = ctx.get_predictions().copy()
    differs = lambda a, b: [t for t in range(nt) if nk[t] and (_bits(a[t, :h, :w]) != _bits(b[t, :h, :w])).any()]  # noqa: E731
    second = [t for t in range(nt) if nk[t] and nk[t - 1]]                  # the frames whose input depends on the loop
    assert differs(lossless, open_pred) == second and second
    assert differs(lossy, lossless) == second
    _reset(ctx)


def test_state_and_unsupported(contexts):
    from tezip_amd import _lib
    h, w = J.SIZES[0]
    nt, p, win = 7, 0, 3
    ctx = contexts(h, w, 4)
    lib = ctx.lib
    frames = np.ascontiguousarray(J.frames(nt, h, w))
    key = np.zeros(nt, np.uint8)
    closed = lambda window, mode, b0, b1=0.0: lib.tz_rollout_closed(ctx.h, frames.ctypes.data, nt, h, w, p, window, mode, b0, b1,  # noqa: E731
                                                                  key.ctypes.data)
    # what the closed loop does not serve
    assert closed(win, 0, 6.0) == TZ_ERR_UNSUPPORTED                         # lossy under the greedy quantiser
    assert "lattice" in lib.tz_last_error(ctx.h).decode()
    assert closed(win, 0, 0.4) == 0 and ctx.rollout_loop() == 1              # the greedy identity is the lossless loop
    ctx.set_quantiser("lattice")
    for mode, b0, b1 in ((1, 0.1, 0.0), (2, 6.0, 0.1), (3, 0.1, 0.0)):
        assert closed(win, mode, b0, b1) == TZ_ERR_UNSUPPORTED, mode
    assert closed(0, 0, 6.0) == TZ_ERR_UNSUPPORTED and closed(0, 0, 0.0) == TZ_ERR_UNSUPPORTED
    assert closed(win, 4, 6.0) == -1 and closed(win, 0, float("nan")) == -1 and closed(-1, 0, 6.0) == -1
    assert lib.tz_rollout_closed(None, frames.ctypes.data, nt, h, w, p, win, 0, 0.0, 0.0, None) == -1
    assert lib.tz_rollout_loop(None) == -1
    fresh = _lib.Context(0)
    assert lib.tz_rollout_loop(fresh.h) == TZ_ERR_STATE                      # no rollout yet
    fresh.close()
    assert closed(win, 0, 0.9) == 0                                          # the lattice identity
    ctx.set_frame_bounds([6.0] * nt)
    assert closed(win, 0, 6.0) == TZ_ERR_UNSUPPORTED
    ctx.set_frame_bounds(None)
    ctx.set_payload_channels(1)
    assert closed(win, 0, 6.0) == TZ_ERR_UNSUPPORTED
    kf = np.zeros_like(frames)
    kf[[0, 3, 6]] = frames[[0, 3, 6]]
    pay = np.zeros(frames.size, np.int16)
    assert lib.tz_rollout_decode_closed(ctx.h, kf.ctypes.data, nt, h, w, p, pay.ctypes.data, pay.size, None, -1, None) == TZ_ERR_UNSUPPORTED
    ctx.set_payload_channels(3)
    assert lib.tz_rollout_decode_closed(ctx.h, kf.ctypes.data, nt, h, w, p, pay.ctypes.data, pay.size - 1, None, -1, None) == -1
    _idle(ctx)
    # a stamped rollout serves its own job alone
    assert closed(win, 0, 6.0) == 0 and ctx.rollout_loop() == 1
    table = np.zeros(_lib.TZ_MAX_TABLE, np.int16)
    out = np.zeros(frames.size, np.int16)
    rec = np.zeros(nt, _lib.QUALITY_DTYPE)
    size = np.zeros(3, _lib.SIZE_DTYPE)
    import ctypes as C
    tlen = C.c_int(0)
    calls = {
        "tz_encode": lambda m, b0, b1: lib.tz_encode(ctx.h, m, b0, b1, 1, out.ctypes.data, table.ctypes.data, C.byref(tlen), None),
        "tz_encode_delta": lambda m, b0, b1: lib.tz_encode_delta(ctx.h, m, b0, b1, out.ctypes.data),
        "tz_bound_probe": lambda m, b0, b1: lib.tz_bound_probe(ctx.h, m, b0, b1, rec.ctypes.data),
        "tz_size_probe": lambda m, b0, b1: lib.tz_size_probe(ctx.h, m, b0, b1, 1, 2, size.ctypes.data),
        "tz_sdelta_probe": lambda m, b0, b1: lib.tz_sdelta_probe(ctx.h, m, b0, b1, 1, 2, size.ctypes.data),
    }
    for name, call in calls.items():
        assert call(0, 6.0, 0.0) == 0, name                                  # the loop's own job
        for m, b0, b1 in ((0, 2.0, 0.0), (0, 0.0, 0.0), (1, 6.0, 0.0)):      # another bound, another mode
            assert call(m, b0, b1) == TZ_ERR_STATE, (name, m, b0)
            msg = lib.tz_last_error(ctx.h).decode()
            assert name in msg and "closed loop" in msg and "mode 0, bound 6 " in msg and "quantiser 1" in msg, msg
        ctx.set_quantiser("greedy")                                          # another quantiser
        assert call(0, 6.0, 0.0) == TZ_ERR_STATE, name
        ctx.set_quantiser("lattice")
        ctx.set_frame_bounds([6.0] * nt)
        assert call(0, 6.0, 0.0) == TZ_ERR_STATE and "tz_set_frame_bounds" in lib.tz_last_error(ctx.h).decode(), name
        ctx.set_frame_bounds(None)
        ctx.set_bound_map(np.full((h, w), 6, np.uint8))
        assert call(0, 6.0, 0.0) == TZ_ERR_STATE and "tz_set_bound_map" in lib.tz_last_error(ctx.h).decode(), name
        ctx.set_bound_map(None)
        ctx.set_payload_channels(1)
        assert call(0, 6.0, 0.0) == TZ_ERR_STATE and "tz_set_payload_channels" in lib.tz_last_error(ctx.h).decode(), name
        ctx.set_payload_channels(3)
        assert call(0, 6.0, 0.0) == 0, name
        _idle(ctx)
    assert ctx.rollout_loop() == 1                                           # nothing of this changed the rollout
    _reset(ctx)


def test_open_loop_bytes_come_back(contexts):
    h, w = J.SIZES[1]
    nt, p, win = 7, 0, 3
    ctx = contexts(h, w, 4)
    frames = np.ascontiguousarray(J.frames(nt, h, w))
    ctx.set_quantiser("lattice")

    def open_job():
        key, _ = ctx.rollout(frames, p, win)
        payload, table, _ = ctx.encode("abs", [6.0], True)
        return key.copy(), np.asarray(payload).copy(), table.copy()

    before = open_job()
    ctx.rollout_closed(frames, p, win, "abs", [6.0])
    closed_payload, closed_table, _ = ctx.encode("abs", [6.0], True)
    closed_payload = np.asarray(closed_payload).copy()
    after = open_job()
    assert ctx.rollout_loop() == 0
    for a, b in zip(before, after):
        np.testing.assert_array_equal(a, b)
    assert (closed_payload != before[1]).any()
    payload, table, _ = ctx.encode("abs", [2.0], True)                        # and the open rollout serves any bound again
    assert table is not None
    _idle(ctx)
    _reset(ctx)
