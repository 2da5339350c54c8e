"""TZ-CLF1 on a MI355X (tz_rollout_closed_frames, tz_loop_frame_bounds, tz_loop_search_trace, k_clf_probe, k_clf_step): the library
held bit for bit to the slow statement (tezip_amd/closedframes.py with the C oracle's PredNet; tests/test_closedframes.py holds
that statement to first principles) -- key mask, predictions, the bounds found, every sum of the search, payload and table in
every layout under tz_set_frame_bounds(found), the decoded stack -- for given bounds and for the search, with one window per batch
and several, more windows than batch slots, TZ-PA2, the widest sums, an unaligned frame buffer, poisoned scratch, and every rule
of the entry point and of its stamp."""
import os
import subprocess
import sys

import numpy as np
import pytest

import closedframes_jobs as F
import closedloop_jobs as J

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TZ_ERR_INVALID, TZ_ERR_STATE, TZ_ERR_UNSUPPORTED = -1, -4, -6
NOT_RUN = 2 ** 64 - 1


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
    ctx.set_pred_select(False)
    ctx.set_pred_motion(0)


def _layout(ctx, layout):
    ctx.set_delta_stride(0)
    ctx.set_delta_plane(0)
    if layout == "channel":
        ctx.set_delta_stride(1)
    elif layout == "plane":
        ctx.set_delta_plane(1)


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _idle(ctx):
    assert ctx.pool_held()[0] == 0


def _trace(want):
    return np.array(want["trace"], dtype=np.uint64)


def _rollout_equals(ctx, frames, p, win, want, what, bounds=None, limit=0):
    """One tz_rollout_closed_frames against the statement: key mask, predictions, bounds, sse, trace."""
    nt, h, w = frames.shape[:3]
    ctx.set_frame_bounds(None)
    key = ctx.rollout_closed_frames(frames, p, win, bounds=bounds, sse_limit=limit)
    _idle(ctx)
    np.testing.assert_array_equal(key, want["key"], err_msg=what)
    assert ctx.rollout_loop() == 1
    got = ctx.get_predictions()
    nk = ~want["key"]
    np.testing.assert_array_equal(_bits(got[nk][:, :h, :w]), _bits(want["pred"][nk][:, :h, :w]), err_msg=what)
    fb, sse = ctx.loop_frame_bounds()
    _idle(ctx)
    np.testing.assert_array_equal(fb, want["bounds"], err_msg=what)
    np.testing.assert_array_equal(sse, np.array(want["sse"], dtype=np.uint64), err_msg=what)
    if bounds is None:
        np.testing.assert_array_equal(ctx.loop_search_trace(), _trace(want), err_msg=what)
    else:
        with pytest.raises(Exception):
            ctx.loop_search_trace()
    return fb, got


def _job_equals(ctx, frames, p, win, want, what, layouts):
    """The back half under tz_set_frame_bounds(found) and the decoder, against the statement."""
    from tezip_amd import closedloop
    nt = len(frames)
    ctx.set_frame_bounds(want["bounds"])
    payloads = {}
    for layout in layouts:
        _layout(ctx, layout)
        payload, table, delta = ctx.encode("abs", [0.0], True, want_delta=True)
        _idle(ctx)
        want_payload, want_table = closedloop.payload_of(want["q"], layout)
        np.testing.assert_array_equal(delta, want["q"], err_msg=what + " " + layout)
        np.testing.assert_array_equal(table, want_table, err_msg=what + " " + layout)
        np.testing.assert_array_equal(np.asarray(payload).reshape(-1), want_payload, err_msg=what + " " + layout)
        payloads[layout] = (want_payload, want_table)
    ctx.set_frame_bounds(None)
    kf = np.zeros_like(frames)
    kf[want["key"]] = frames[want["key"]]
    for layout in layouts:
        _layout(ctx, layout)
        dkey = ctx.rollout_decode_closed(kf, p, *payloads[layout])
        _idle(ctx)
        np.testing.assert_array_equal(dkey, want["key"], err_msg=what + " " + layout)
        np.testing.assert_array_equal(ctx.decoded_get(0, nt), want["dec"], err_msg=what + " decoder " + layout)
        assert ctx.rollout_loop() == 0
    _layout(ctx, "flat")


def _whole_job(ctx, nt, h, w, p, win, layouts, targets=F.TARGETS, contract=0, spread=True):
    frames = np.ascontiguousarray(F.frames(nt, h, w))
    ctx.set_quantiser("lattice")
    what = "%dx%dx%d p%d w%d" % (nt, h, w, p, win)
    want = F.with_bounds(nt, h, w, p, win, tuple(F.given(nt)), contract)
    _rollout_equals(ctx, frames, p, win, want, what + " given", bounds=F.given(nt))
    _job_equals(ctx, frames, p, win, want, what + " given", layouts)
    for db in targets:
        want = F.searched(nt, h, w, p, win, db, contract)
        if spread:
            F.check_spread(want)
        _rollout_equals(ctx, frames, p, win, want, what + " %g dB" % db, limit=F.limit_of(db, h, w))
        _job_equals(ctx, frames, p, win, want, what + " %g dB" % db, layouts)
    _reset(ctx)


@pytest.mark.parametrize("max_batch", [1, 4])
@pytest.mark.parametrize("h,w", F.SIZES)
@pytest.mark.parametrize("nt,p,win", F.TRIPLES)
def test_library_equals_the_statement(contexts, nt, p, win, h, w, max_batch):
    layouts = J.LAYOUTS if win == 3 else ("flat",)
    _whole_job(contexts(h, w, max_batch), nt, h, w, p, win, layouts)


def test_more_windows_than_batch_slots(contexts):
    h, w = F.SIZES[1]
    _whole_job(contexts(h, w, 2), 9, h, w, 0, 2, ("flat", "plane"))     # four windows, two slots


def test_a_search_replays_as_given_bounds(contexts):
    h, w = F.SIZES[1]
    nt, p, win, db = 7, 0, 3, 30.0
    ctx = contexts(h, w, 4)
    ctx.set_quantiser("lattice")
    frames = np.ascontiguousarray(F.frames(nt, h, w))
    want = F.searched(nt, h, w, p, win, db, 0)
    found, pred_a = _rollout_equals(ctx, frames, p, win, want, "search", limit=F.limit_of(db, h, w))
    pred_a = pred_a.copy()
    ctx.set_frame_bounds(found)
    pay_a, table_a, _ = ctx.encode("abs", [0.0], True)
    pay_a = np.asarray(pay_a).copy()
    ctx.set_frame_bounds(None)
    ctx.rollout_closed_frames(frames, p, win, bounds=found)
    fb, sse = ctx.loop_frame_bounds()
    np.testing.assert_array_equal(fb, found)
    assert not sse.any()
    nk = ~want["key"]
    np.testing.assert_array_equal(_bits(ctx.get_predictions()[nk]), _bits(pred_a[nk]))
    ctx.set_frame_bounds(found)
    pay_b, table_b, _ = ctx.encode("abs", [0.0], True)
    np.testing.assert_array_equal(np.asarray(pay_b), pay_a)
    np.testing.assert_array_equal(table_b, table_a)
    _idle(ctx)
    _reset(ctx)


def test_uniform_bounds_and_zeros_are_the_closed_job(contexts):
    """Bounds of 6 everywhere give tz_rollout_closed's job under abs 6; zeros (and 0.9) its lossless job."""
    h, w = F.SIZES[1]
    nt, p, win = 8, 1, 3
    ctx = contexts(h, w, 4)
    ctx.set_quantiser("lattice")
    frames = np.ascontiguousarray(F.frames(nt, h, w))
    for b in (6.0, 0.0, 0.9):
        ctx.set_frame_bounds(None)
        key = ctx.rollout_closed(frames, p, win, "abs", [b])
        pred = ctx.get_predictions().copy()
        pay, table, _ = ctx.encode("abs", [b], True)
        pay = np.asarray(pay).copy()
        key2 = ctx.rollout_closed_frames(frames, p, win, bounds=[b] * nt)
        np.testing.assert_array_equal(key, key2)
        np.testing.assert_array_equal(_bits(ctx.get_predictions()[~key]), _bits(pred[~key]))
        fb, _ = ctx.loop_frame_bounds()
        np.testing.assert_array_equal(fb, np.where(key, 0.0, b))
        ctx.set_frame_bounds(fb)
        pay2, table2, _ = ctx.encode("abs", [0.0], True)
        np.testing.assert_array_equal(np.asarray(pay2), pay)
        np.testing.assert_array_equal(table2, table)
        _idle(ctx)
    _reset(ctx)


def test_tz_pa2(contexts):
    ctx = contexts(256, 256, 1)
    assert ctx.get_contract() == 2
    _whole_job(ctx, 3, 256, 256, 0, 2, ("flat",), targets=(36.0,), contract=0, spread=False)   # (one searched frame)
    ctx.set_quantiser("lattice")
    ctx.rollout_closed_frames(np.ascontiguousarray(F.frames(3, 256, 256)), 0, 2, sse_limit=F.limit_of(36.0, 256, 256))
    assert ctx.rollout_contract() == 2
    _reset(ctx)


def test_the_widest_sums(contexts):
    """512 x 512: the search's sums against numpy on the library's own predictions (no oracle rollout is needed: frame 1 is
    predicted from a key frame).  Every round of the search, the result and what the frame decodes to."""
    from tezip_amd import closedframes
    h = w = 512
    nt, p, win, db = 3, 0, 2, 30.0
    ctx = contexts(h, w, 1)
    ctx.set_quantiser("lattice")
    frames = np.array(F.frames(nt, h, w))
    limit = F.limit_of(db, h, w)
    # frame 1 is predicted from key frame 0 whatever it holds itself: make it lie 100 off its prediction everywhere, so that the
    # first round (E = 127 leaves such a delta to the decoder as it is) sums 512 * 512 * 3 * 100^2 = 7.9e9 > 2^32
    ctx.rollout_closed(frames, p, win, "abs", [0.0])
    x = (ctx.get_predictions()[1][:h, :w] * np.float32(255.0)).astype(np.int64)
    frames[1] = np.where(x < 128, x + 100, x - 100).astype(np.uint8)
    key = ctx.rollout_closed_frames(frames, p, win, sse_limit=limit)
    _idle(ctx)
    np.testing.assert_array_equal(key, [True, False, True])
    np.testing.assert_array_equal((ctx.get_predictions()[1][:h, :w] * np.float32(255.0)).astype(np.int64), x)
    orig = frames[1].astype(np.int64)
    rounds = []
    lo, hi = 0, 511
    while hi - lo > 1:
        mid = (lo + hi) // 2
        rounds.append(closedframes.sse_of(x, orig, mid))
        lo, hi = (mid, hi) if rounds[-1] <= limit else (lo, mid)
    assert 0 < lo < 510 and max(rounds) > 2 ** 32                     # (a sum that 32 bits would not hold)
    trace = ctx.loop_search_trace()
    assert [int(v) for v in trace[:, 1]] == rounds + [NOT_RUN] * (9 - len(rounds))
    assert (trace[:, 0] == NOT_RUN).all() and (trace[:, 2] == NOT_RUN).all()
    fb, sse = ctx.loop_frame_bounds()
    assert list(fb) == [0.0, lo / 2.0, 0.0] and int(sse[1]) == closedframes.sse_of(x, orig, lo) and not sse[0] and not sse[2]
    ctx.set_frame_bounds(fb)
    _, _, delta = ctx.encode("abs", [0.0], True, want_delta=True)
    q, _ = closedframes.decode_under(x, orig, lo // 2)
    np.testing.assert_array_equal(delta[1], q)
    _idle(ctx)
    _reset(ctx)


def test_frames_off_the_16_byte_boundary(contexts):
    import devmem
    h, w = F.SIZES[1]
    nt, p, win, db = 7, 0, 3, 36.0
    ctx = contexts(h, w, 4)
    ctx.set_quantiser("lattice")
    frames = np.ascontiguousarray(F.frames(nt, h, w))
    want = F.searched(nt, h, w, p, win, db, 0)
    for off in (3, 8):
        view, intact = devmem.view(frames, off)
        _rollout_equals(ctx, view, p, win, want, "offset %d" % off, limit=F.limit_of(db, h, w))
        assert intact()
    view, intact = devmem.view(frames, 5)
    _rollout_equals(ctx, view, p, win, F.with_bounds(nt, h, w, p, win, tuple(F.given(nt)), 0), "offset 5 given", bounds=F.given(nt))
    assert intact()
    _reset(ctx)


def test_staged_frames(contexts):
    h, w = F.SIZES[1]
    nt, p, win, db = 8, 1, 3, 30.0
    ctx = contexts(h, w, 4)
    ctx.set_quantiser("lattice")
    frames = np.ascontiguousarray(F.frames(nt, h, w))
    ctx.frames_begin(nt, h, w)
    ctx.frames_put(0, frames[:3])
    ctx.frames_put(3, frames[3:])
    want = F.searched(nt, h, w, p, win, db, 0)
    key = ctx.rollout_closed_frames(None, p, win, sse_limit=F.limit_of(db, h, w))
    np.testing.assert_array_equal(key, want["key"])
    np.testing.assert_array_equal(ctx.loop_frame_bounds()[0], want["bounds"])
    np.testing.assert_array_equal(ctx.loop_search_trace(), _trace(want))
    _idle(ctx)
    _reset(ctx)


def test_entry_point_rules(contexts):
    from tezip_amd import _lib
    h, w = F.SIZES[0]
    nt, p, win = 7, 0, 3
    ctx = contexts(h, w, 4)
    lib = ctx.lib
    frames = np.ascontiguousarray(F.frames(nt, h, w))
    key = np.zeros(nt, np.uint8)
    good = np.array(F.given(nt), np.float64)

    def call(bounds=good, limit=0, window=win):
        return lib.tz_rollout_closed_frames(ctx.h, frames.ctypes.data, nt, h, w, p, window, None if bounds is None else bounds.ctypes.data,
                                            limit, key.ctypes.data)

    msg = lambda: lib.tz_last_error(ctx.h).decode()  # noqa: E731
    assert call() == TZ_ERR_UNSUPPORTED and "tz_set_quantiser" in msg()                 # the greedy quantiser
    ctx.set_quantiser("lattice")
    assert call() == 0 and ctx.rollout_loop() == 1
    assert call(None, 0) == TZ_ERR_INVALID and "neither" in msg()                        # exactly one of the two
    assert call(good, 5) == TZ_ERR_INVALID and "both" in msg()
    for bad in (-1.0, float("nan"), float("inf")):
        b = good.copy()
        b[2] = bad
        assert call(b) == TZ_ERR_INVALID and "frame 2" in msg(), bad
    assert call(window=0) == TZ_ERR_UNSUPPORTED and call(window=-1) == TZ_ERR_INVALID
    assert lib.tz_rollout_closed_frames(None, frames.ctypes.data, nt, h, w, p, win, good.ctypes.data, 0, None) == TZ_ERR_INVALID
    assert lib.tz_rollout_closed_frames(ctx.h, frames.ctypes.data, 1, h, w, p, win, good.ctypes.data, 0, None) == TZ_ERR_INVALID
    ctx.set_frame_bounds([6.0] * nt)
    assert call() == TZ_ERR_UNSUPPORTED and "tz_set_frame_bounds" in msg()
    ctx.set_frame_bounds(None)
    ctx.set_bound_map(np.full((h, w), 6, np.uint8))
    assert call() == TZ_ERR_UNSUPPORTED and "tz_set_bound_map" in msg()
    ctx.set_bound_map(None)
    ctx.set_payload_channels(1)
    assert call() == TZ_ERR_UNSUPPORTED and "tz_set_payload_channels" in msg()
    ctx.set_payload_channels(3)
    ctx.set_pred_select(True)
    assert call() == TZ_ERR_UNSUPPORTED and "tz_set_pred_select" in msg()
    ctx.set_pred_select(False)
    ctx.set_pred_motion(7)
    assert call() == TZ_ERR_UNSUPPORTED and "tz_set_pred_motion" in msg()
    ctx.set_pred_motion(0)
    _idle(ctx)
    # the getters: another kind of rollout is TZ_ERR_STATE
    out, sse, tr = np.zeros(nt), np.zeros(nt, np.uint64), np.zeros(9 * nt, np.uint64)
    fresh = _lib.Context(0)
    assert lib.tz_loop_frame_bounds(fresh.h, out.ctypes.data, sse.ctypes.data, nt) == TZ_ERR_STATE
    assert lib.tz_loop_search_trace(fresh.h, tr.ctypes.data, tr.size) == TZ_ERR_STATE
    fresh.close()
    assert lib.tz_loop_frame_bounds(None, None, None, 0) == TZ_ERR_INVALID and lib.tz_loop_search_trace(None, None, 0) == TZ_ERR_INVALID
    ctx.rollout(frames, p, win)
    assert lib.tz_loop_frame_bounds(ctx.h, out.ctypes.data, sse.ctypes.data, nt) == TZ_ERR_STATE
    ctx.rollout_closed(frames, p, win, "abs", [6.0])
    assert lib.tz_loop_frame_bounds(ctx.h, out.ctypes.data, sse.ctypes.data, nt) == TZ_ERR_STATE and "tz_rollout_closed_frames" in msg()
    assert lib.tz_loop_search_trace(ctx.h, tr.ctypes.data, tr.size) == TZ_ERR_STATE
    assert call() == 0
    assert lib.tz_loop_frame_bounds(ctx.h, out.ctypes.data, sse.ctypes.data, nt) == nt and not sse.any()
    assert lib.tz_loop_frame_bounds(ctx.h, None, None, 0) == nt
    assert lib.tz_loop_frame_bounds(ctx.h, out.ctypes.data, None, nt - 1) == TZ_ERR_INVALID
    assert lib.tz_loop_search_trace(ctx.h, tr.ctypes.data, tr.size) == TZ_ERR_STATE      # given bounds: no search ran
    assert call(None, 1000) == 0
    assert lib.tz_loop_search_trace(ctx.h, tr.ctypes.data, tr.size) == 9 * nt
    assert lib.tz_loop_search_trace(ctx.h, tr.ctypes.data, tr.size - 1) == TZ_ERR_INVALID
    ctx.rollout_decode_closed(np.where(np.array([1, 0, 0, 1, 0, 0, 1], bool)[:, None, None, None], frames, 0).astype(np.uint8), p,
                              np.zeros(frames.size, np.int16), None)
    assert lib.tz_loop_frame_bounds(ctx.h, out.ctypes.data, sse.ctypes.data, nt) == TZ_ERR_STATE
    _idle(ctx)
    _reset(ctx)


def test_a_stamped_rollout_serves_its_own_job_alone(contexts):
    import ctypes as C
    from tezip_amd import _lib
    h, w = F.SIZES[0]
    nt, p, win = 7, 0, 3
    ctx = contexts(h, w, 4)
    lib = ctx.lib
    ctx.set_quantiser("lattice")
    frames = np.ascontiguousarray(F.frames(nt, h, w))
    ctx.rollout_closed_frames(frames, p, win, bounds=F.given(nt))
    stamp, _ = ctx.loop_frame_bounds()
    table = np.zeros(_lib.TZ_MAX_TABLE, np.int16)
    out = np.zeros(frames.size, np.int16)
    rec = np.zeros(nt, _lib.QUALITY_DTYPE)
    size = np.zeros(3, _lib.SIZE_DTYPE)
    tlen = C.c_int(0)
    calls = {
        "tz_encode": lambda m, b0: lib.tz_encode(ctx.h, m, b0, 0.0, 1, out.ctypes.data, table.ctypes.data, C.byref(tlen), None),
        "tz_encode_delta": lambda m, b0: lib.tz_encode_delta(ctx.h, m, b0, 0.0, out.ctypes.data),
        "tz_bound_probe": lambda m, b0: lib.tz_bound_probe(ctx.h, m, b0, 0.0, rec.ctypes.data),
        "tz_size_probe": lambda m, b0: lib.tz_size_probe(ctx.h, m, b0, 0.0, 1, 2, size.ctypes.data),
        "tz_sdelta_probe": lambda m, b0: lib.tz_sdelta_probe(ctx.h, m, b0, 0.0, 1, 2, size.ctypes.data),
    }

    def refused(name, call, m=0, b0=0.0):
        assert call(m, b0) == TZ_ERR_STATE, name
        msg = lib.tz_last_error(ctx.h).decode()
        assert name in msg and "tz_rollout_closed_frames" in msg, msg

    other = stamp.copy()
    other[1] += 0.5
    for name, call in calls.items():
        ctx.set_frame_bounds(stamp)
        assert call(0, 0.0) == 0 and call(0, 6.0) == 0, name            # the stamp's job: b0 is not read
        refused(name, call, m=1)                                        # another mode
        ctx.set_quantiser("greedy")
        refused(name, call)
        ctx.set_quantiser("lattice")
        ctx.set_frame_bounds(None)                                      # no frame bounds: a uniform job is another job
        refused(name, call)
        refused(name, call, b0=6.0)
        for b in (other, stamp[:-1], np.concatenate([stamp, [0.0]])):   # another vector
            ctx.set_frame_bounds(b)
            refused(name, call)
        ctx.set_frame_bounds(stamp)
        ctx.set_payload_channels(1)
        refused(name, call)
        ctx.set_payload_channels(3)
        assert call(0, 0.0) == 0, name
        _idle(ctx)
    hist, edge = np.zeros(1 << 16, np.uint64), np.zeros(2, np.int16)
    begin = lambda m, b0: lib.tz_encode_begin(ctx.h, m, b0, 0.0, 1, hist.ctypes.data, edge.ctypes.data)  # noqa: E731
    assert begin(1, 0.1) == TZ_ERR_STATE and "tz_rollout_closed_frames" in lib.tz_last_error(ctx.h).decode()
    assert begin(0, 0.0) == TZ_ERR_UNSUPPORTED                          # (the stamp's job: sharded entries take one bound)
    ctx.set_frame_bounds(None)
    assert begin(0, 6.0) == TZ_ERR_STATE
    assert ctx.rollout_loop() == 1
    # the rule for a uniform stamp is what it was: tz_rollout_closed's rollout refuses frame bounds
    ctx.rollout_closed(frames, p, win, "abs", [6.0])
    assert calls["tz_encode"](0, 6.0) == 0
    ctx.set_frame_bounds([6.0] * nt)
    assert calls["tz_encode"](0, 6.0) == TZ_ERR_STATE and "tz_set_frame_bounds" in lib.tz_last_error(ctx.h).decode()
    _idle(ctx)
    _reset(ctx)


_POISON_SCRIPT = """
import sys
import numpy as np
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import closedframes_jobs as F
import closedloop_jobs as J
from tezip_amd import _lib
h, w = F.SIZES[1]
nt, p, win, db = 7, 0, 3, 36.0
cfg, wts = J.model()
ctx = _lib.Context(0)
ctx.load_model(cfg, wts)
ctx.prepare(_lib.pad8(h), _lib.pad8(w), 4)
ctx.set_quantiser("lattice")
frames = np.ascontiguousarray(F.frames(nt, h, w))
want = F.searched(nt, h, w, p, win, db, 0)
for rep in range(2):      # (the second call reuses pool blocks the first one filled)
    ctx.set_frame_bounds(None)
    key = ctx.rollout_closed_frames(frames, p, win, sse_limit=F.limit_of(db, h, w))
    fb, sse = ctx.loop_frame_bounds()
    assert (key == want["key"]).all() and (fb == want["bounds"]).all() and [int(s) for s in sse] == want["sse"]
    assert (ctx.loop_search_trace() == np.array(want["trace"], dtype=np.uint64)).all()
    ctx.set_frame_bounds(fb)
    _, _, delta = ctx.encode("abs", [0.0], True, want_delta=True)
    assert (delta == want["q"]).all()
ctx.close()
print("poison ok")
"""


def test_same_results_under_poison(tmp_path):
    """TEZIP_POISON fills every device buffer handed out before its use (tests/test_gpu_poison.py): the sums of the search
    start from zeros the rollout writes itself, whatever the pool's blocks held."""
    script = tmp_path / "poison_job.py"
    script.write_text(_POISON_SCRIPT % (ROOT, os.path.join(ROOT, "tests")))
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, str(script)], cwd=ROOT, capture_output=True, text=True,
                       env=dict(os.environ, TEZIP_POISON="0xA5"), timeout=330)
    assert r.returncode == 0 and "poison ok" in r.stdout, r.stdout + r.stderr
