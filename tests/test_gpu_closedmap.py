"""TZ-CLM1 on a MI355X (tz_rollout_closed_map, k_clm_step, k_psm_step): the library held bit for bit to the slow statement
(tezip_amd/closedmap.py with the C oracle's PredNet; tests/test_closedmap.py holds that statement to first principles) -- key mask,
predictions, modes, delta, payload and table in every layout under the same map, the decoded stack -- for the network alone and
for per-tile selection, at the sizes that take k_clm_step's three forms, with one window per batch and several, more windows than
batch slots, TZ-PA2, an unaligned frame buffer, poisoned scratch, and every rule of the entry point and of its stamp."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import closedloop_jobs as J
import closedmap_jobs as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TZ_ERR_INVALID, TZ_ERR_STATE, TZ_ERR_UNSUPPORTED = -1, -4, -6


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


def _rollout_equals(ctx, frames, p, win, want, what, select):
    """One tz_rollout_closed_map under the map in force against the statement: key mask, predictions, modes."""
    h, w = frames.shape[1:3]
    key = ctx.rollout_closed_map(frames, p, win)
    _idle(ctx)
    np.testing.assert_array_equal(key, want["key"], err_msg=what)
    assert ctx.rollout_loop() == 1
    nk = ~want["key"]
    final = want["patched"] if select else want["pred"]
    np.testing.assert_array_equal(_bits(ctx.get_predictions()[nk][:, :h, :w]), _bits(final[nk][:, :h, :w]), err_msg=what)
    if select:
        np.testing.assert_array_equal(ctx.pred_modes(), want["modes"], err_msg=what)


def _job_equals(ctx, frames, p, win, want, what, layouts, select):
    """The back half under the same map and the decoder, against the statement."""
    from tezip_amd import closedloop
    nt = len(frames)
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
    ctx.set_bound_map(None)                                     # the decoder never sees a bound
    kf = np.zeros_like(frames)
    kf[want["key"]] = frames[want["key"]]
    for layout in layouts:
        _layout(ctx, layout)
        if select:
            ctx.put_pred_modes(want["modes"])
        dkey = ctx.rollout_decode_closed(kf, p, *payloads[layout])
        _idle(ctx)
        np.testing.assert_array_equal(dkey, want["key"], err_msg=what + " " + layout)
        np.testing.assert_array_equal(ctx.decoded_get(0, nt), want["dec"], err_msg=what + " decoder " + layout)
        assert ctx.rollout_loop() == 0
    _layout(ctx, "flat")


def _whole_job(ctx, scene, nt, h, w, p, win, layouts, select, which="map", contract=0):
    frames = np.ascontiguousarray(M.frames(scene, nt, h, w))
    want = M.statement(scene, nt, h, w, p, win, which, select, contract)
    what = "%s %dx%dx%d p%d w%d %s%s" % (scene, nt, h, w, p, win, which, " select" if select else "")
    ctx.set_quantiser("lattice")
    ctx.set_pred_select(select)
    ctx.set_bound_map(M.MAPS[which](h, w))
    _rollout_equals(ctx, frames, p, win, want, what, select)
    _job_equals(ctx, frames, p, win, want, what, layouts, select)
    _reset(ctx)
    return want


@pytest.mark.parametrize("max_batch", [1, 4])
@pytest.mark.parametrize("h,w", M.SIZES)
@pytest.mark.parametrize("nt,p,win", M.TRIPLES)
def test_library_equals_the_statement(contexts, nt, p, win, h, w, max_batch):
    layouts = J.LAYOUTS if win == 3 else ("flat",)
    if (nt, p, win) != (9, 0, 4):
        M.check_map_matters("translating", nt, h, w, p, win, False, 0)
    _whole_job(contexts(h, w, max_batch), "translating", nt, h, w, p, win, layouts, False)


@pytest.mark.parametrize("max_batch", [1, 4])
@pytest.mark.parametrize("h,w", M.SIZES)
@pytest.mark.parametrize("nt,p,win", M.TRIPLES)
def test_selection_equals_the_statement(contexts, nt, p, win, h, w, max_batch):
    layouts = J.LAYOUTS if win == 3 else ("flat",)
    want = _whole_job(contexts(h, w, max_batch), "flicker", nt, h, w, p, win, layouts, True)
    assert M.check_mixed(want) == M.PREV_TILES[h, w][nt, p, win]


@pytest.mark.parametrize("select", [False, True])
def test_rows_of_a_padded_frame(contexts, select):
    """20 x 32 pads to 24 x 32 with W a multiple of 16: k_clm_step walks the crop row by row on 16-byte accesses."""
    h, w = M.ROWS_SIZE
    _whole_job(contexts(h, w, 4), "flicker" if select else "translating", 7, h, w, 0, 3, ("flat",), select)


@pytest.mark.parametrize("select", [False, True])
def test_more_windows_than_batch_slots(contexts, select):
    h, w = M.SIZES[1]
    _whole_job(contexts(h, w, 2), "flicker" if select else "translating", 9, h, w, 0, 2, ("flat", "plane"), select)   # four windows, two slots


@pytest.mark.parametrize("select", [False, True])
@pytest.mark.parametrize("h,w", M.SIZES)
def test_uniform_and_zero_maps_are_the_closed_job(contexts, h, w, select):
    """A map of k everywhere gives tz_rollout_closed's job under abs k -- predictions, modes and payload -- and a map of zeros its
    lossless job."""
    nt, p, win = 8, 1, 3
    ctx = contexts(h, w, 4)
    ctx.set_quantiser("lattice")
    ctx.set_pred_select(select)
    frames = np.ascontiguousarray(M.frames("flicker" if select else "translating", nt, h, w))
    for k in (6, 0, 255):
        ctx.set_bound_map(None)
        key = ctx.rollout_closed(frames, p, win, "abs", [float(k)])
        pred = ctx.get_predictions().copy()
        modes = ctx.pred_modes().copy() if select else None
        pay, table, _ = ctx.encode("abs", [float(k)], True)
        pay = np.asarray(pay).copy()
        ctx.set_bound_map(M.uniform(h, w, k))
        key2 = ctx.rollout_closed_map(frames, p, win)
        _idle(ctx)
        np.testing.assert_array_equal(key, key2)
        np.testing.assert_array_equal(_bits(ctx.get_predictions()[~key]), _bits(pred[~key]), err_msg=str(k))
        if select:
            np.testing.assert_array_equal(ctx.pred_modes(), modes, err_msg=str(k))
        pay2, table2, _ = ctx.encode("abs", [0.0], True)
        np.testing.assert_array_equal(np.asarray(pay2), pay, err_msg=str(k))
        np.testing.assert_array_equal(table2, table)
        _idle(ctx)
    _reset(ctx)


def test_a_zero_map_takes_the_lossless_schedule(contexts):
    """No step kernel runs: the quantiser's profiler slot counts no launch during the rollout."""
    h, w = M.SIZES[0]
    nt, p, win = 7, 0, 3
    ctx = contexts(h, w, 4)
    ctx.set_quantiser("lattice")
    frames = np.ascontiguousarray(M.frames("translating", nt, h, w))
    ctx.prof_enable(True)
    for which, launches in (("zero", 0), ("map", win - 1)):
        ctx.set_bound_map(M.MAPS[which](h, w))
        ctx.prof_reset()
        ctx.rollout_closed_map(frames, p, win)
        assert ctx.prof_get()["quant"][1] == launches, which
    ctx.prof_enable(False)
    want = M.statement("translating", nt, h, w, p, win, "zero", False, 0)
    ctx.set_bound_map(M.MAPS["zero"](h, w))
    ctx.rollout_closed_map(frames, p, win)
    _, _, delta = ctx.encode("abs", [0.0], True, want_delta=True)
    np.testing.assert_array_equal(delta, want["q"])
    _reset(ctx)


def test_tz_pa2(contexts):
    h = w = 256
    ctx = contexts(h, w, 1)
    assert ctx.get_contract() == 2
    _whole_job(ctx, "translating", 3, h, w, 0, 2, ("flat",), False)
    ctx.set_quantiser("lattice")
    ctx.set_bound_map(M.the_map(h, w))
    ctx.rollout_closed_map(np.ascontiguousarray(M.frames("translating", 3, h, w)), 0, 2)
    assert ctx.rollout_contract() == 2
    _reset(ctx)


@pytest.mark.parametrize("select", [False, True])
def test_frames_off_the_16_byte_boundary(contexts, select):
    """The unpadded size, whose aligned stack takes the 16-byte form: off its boundary the scalar form gives the same bytes."""
    import devmem
    h, w = M.SIZES[0]
    nt, p, win = 7, 0, 3
    ctx = contexts(h, w, 4)
    scene = "flicker" if select else "translating"
    frames = np.ascontiguousarray(M.frames(scene, nt, h, w))
    want = M.statement(scene, nt, h, w, p, win, "map", select, 0)
    ctx.set_quantiser("lattice")
    ctx.set_pred_select(select)
    ctx.set_bound_map(M.the_map(h, w))
    for off in (3, 8):
        view, intact = devmem.view(frames, off)
        _rollout_equals(ctx, view, p, win, want, "offset %d" % off, select)
        assert intact()
        _, _, delta = ctx.encode("abs", [0.0], True, want_delta=True)
        np.testing.assert_array_equal(delta, want["q"])
    _reset(ctx)


def test_staged_frames(contexts):
    h, w = M.SIZES[1]
    nt, p, win = 8, 1, 3
    ctx = contexts(h, w, 4)
    ctx.set_quantiser("lattice")
    ctx.set_bound_map(M.the_map(h, w))
    frames = np.ascontiguousarray(M.frames("translating", nt, h, w))
    ctx.frames_begin(nt, h, w)
    ctx.frames_put(0, frames[:3])
    ctx.frames_put(3, frames[3:])
    want = M.statement("translating", nt, h, w, p, win, "map", False, 0)
    key = ctx.rollout_closed_map(None, p, win)
    np.testing.assert_array_equal(key, want["key"])
    _, _, delta = ctx.encode("abs", [0.0], True, want_delta=True)
    np.testing.assert_array_equal(delta, want["q"])
    _, table, _ = ctx.encode("abs", [0.0], True, payload="resident")
    rec = ctx.encode_map_check("resident", table)                  # the existing check kernel works on the stamped rollout
    assert not rec["violations"].any() and not rec["max_excess"].any()
    _idle(ctx)
    _reset(ctx)


def test_entry_point_rules(contexts):
    h, w = M.SIZES[0]
    nt, p, win = 7, 0, 3
    ctx = contexts(h, w, 4)
    lib = ctx.lib
    frames = np.ascontiguousarray(M.frames("translating", nt, h, w))
    key = np.zeros(nt, np.uint8)

    def call(window=win, n=nt):
        return lib.tz_rollout_closed_map(ctx.h, frames.ctypes.data, n, h, w, p, window, key.ctypes.data)

    msg = lambda: lib.tz_last_error(ctx.h).decode()  # noqa: E731
    assert call() == TZ_ERR_UNSUPPORTED and "tz_set_quantiser" in msg()                  # the greedy quantiser
    ctx.set_quantiser("lattice")
    assert call() == TZ_ERR_STATE and "tz_set_bound_map" in msg()                        # no map in force
    ctx.set_bound_map(np.full((h, w + 8), 6, np.uint8))
    assert call() == TZ_ERR_INVALID and "tz_set_bound_map" in msg()                      # a map of another size
    ctx.set_bound_map(M.the_map(h, w))
    assert call() == 0 and ctx.rollout_loop() == 1
    ctx.set_quantiser("greedy")
    assert call() == TZ_ERR_UNSUPPORTED and "tz_set_quantiser" in msg()
    ctx.set_quantiser("lattice")
    assert call(window=0) == TZ_ERR_UNSUPPORTED and call(window=-1) == TZ_ERR_INVALID and call(n=1) == TZ_ERR_INVALID
    assert lib.tz_rollout_closed_map(None, frames.ctypes.data, nt, h, w, p, win, None) == TZ_ERR_INVALID
    ctx.set_payload_channels(1)
    assert call() == TZ_ERR_UNSUPPORTED and "tz_set_payload_channels" in msg()
    ctx.set_payload_channels(3)
    ctx.set_pred_motion(7)
    assert call() == TZ_ERR_UNSUPPORTED and "tz_set_pred_motion" in msg()
    ctx.set_pred_motion(0)
    # frame bounds and a map exclude each other at the setters: with bounds in force the entry point names them, not the missing map
    assert lib.tz_set_frame_bounds(ctx.h, np.full(nt, 6.0).ctypes.data, nt) == TZ_ERR_INVALID
    ctx.set_bound_map(None)
    ctx.set_frame_bounds([6.0] * nt)
    assert call() == TZ_ERR_UNSUPPORTED and "tz_set_frame_bounds" in msg()
    ctx.set_frame_bounds(None)
    # tz_rollout_closed under a map is refused as it was
    ctx.set_bound_map(M.the_map(h, w))
    assert lib.tz_rollout_closed(ctx.h, frames.ctypes.data, nt, h, w, p, win, 0, C.c_double(6.0), C.c_double(0.0), key.ctypes.data) == TZ_ERR_UNSUPPORTED
    assert "tz_set_bound_map" in msg()
    assert call() == 0
    _idle(ctx)
    _reset(ctx)


def test_a_stamped_rollout_serves_its_own_job_alone(contexts):
    from tezip_amd import _lib
    h, w = M.SIZES[0]
    nt, p, win = 7, 0, 3
    ctx = contexts(h, w, 4)
    lib = ctx.lib
    ctx.set_quantiser("lattice")
    frames = np.ascontiguousarray(M.frames("translating", nt, h, w))
    stamp = M.the_map(h, w)
    ctx.set_bound_map(stamp)
    ctx.rollout_closed_map(frames, p, win)
    table = np.zeros(_lib.TZ_MAX_TABLE, np.int16)
    out = np.zeros(frames.size, np.int16)
    rec = np.zeros(nt, _lib.QUALITY_DTYPE)
    size = np.zeros(3, _lib.SIZE_DTYPE)
    tlen = C.c_int(0)
    calls = {
        "tz_encode": lambda m, b0: lib.tz_encode(ctx.h, m, b0, 0.0, 1, out.ctypes.data, table.ctypes.data, C.byref(tlen), None),
        "tz_encode_delta": lambda m, b0: lib.tz_encode_delta(ctx.h, m, b0, 0.0, out.ctypes.data),
        "tz_bound_probe": lambda m, b0: lib.tz_bound_probe(ctx.h, m, b0, 0.0, rec.ctypes.data),
        "tz_sdelta_probe": lambda m, b0: lib.tz_sdelta_probe(ctx.h, m, b0, 0.0, 1, 2, size.ctypes.data),
    }

    def refused(name, call, m=0, b0=0.0):
        assert call(m, b0) == TZ_ERR_STATE, name
        msg = lib.tz_last_error(ctx.h).decode()
        assert name in msg and "tz_rollout_closed_map" in msg, msg

    for name, call in calls.items():
        ctx.set_bound_map(stamp)
        assert call(0, 0.0) == 0 and call(0, 6.0) == 0, name            # the stamp's job: b0 is not read
        refused(name, call, m=1)                                        # another mode
        ctx.set_quantiser("greedy")
        refused(name, call)
        ctx.set_quantiser("lattice")
        ctx.set_bound_map(None)                                         # no map: a uniform job is another job
        refused(name, call)
        refused(name, call, b0=6.0)
        for other in (M.rolled(h, w), M.uniform(h, w, 6), M.uniform(h + 8, w, 6)):   # the map was replaced
            ctx.set_bound_map(other)
            refused(name, call)
        ctx.set_bound_map(stamp.copy())                                 # the same bytes again serve
        ctx.set_payload_channels(1)
        refused(name, call)
        ctx.set_payload_channels(3)
        assert call(0, 0.0) == 0, name
        _idle(ctx)
    # the entries that serve no bound map at all say so once the stamp's rule is met, and the stamp's rule comes first
    hist, edge = np.zeros(1 << 16, np.uint64), np.zeros(2, np.int16)
    for name, call in (("tz_encode_begin", lambda m, b0: lib.tz_encode_begin(ctx.h, m, b0, 0.0, 1, hist.ctypes.data, edge.ctypes.data)),
                       ("tz_size_probe", lambda m, b0: lib.tz_size_probe(ctx.h, m, b0, 0.0, 1, 2, size.ctypes.data))):
        ctx.set_bound_map(stamp)
        refused(name, call, m=1, b0=0.1)
        assert call(0, 0.0) == TZ_ERR_UNSUPPORTED, name
        ctx.set_bound_map(None)
        refused(name, call, b0=6.0)
        ctx.set_bound_map(M.rolled(h, w))
        refused(name, call)
    assert ctx.rollout_loop() == 1
    # the rule for a uniform stamp is what it was: tz_rollout_closed's rollout refuses a map
    ctx.set_bound_map(None)
    ctx.rollout_closed(frames, p, win, "abs", [6.0])
    assert calls["tz_encode"](0, 6.0) == 0
    ctx.set_bound_map(M.uniform(h, w, 6))
    assert calls["tz_encode"](0, 6.0) == TZ_ERR_STATE and "tz_rollout_closed_map" not in lib.tz_last_error(ctx.h).decode()
    # and a map rollout run with selection serves a select job alone
    ctx.set_bound_map(stamp)
    ctx.set_pred_select(True)
    ctx.rollout_closed_map(frames, p, win)
    assert calls["tz_encode"](0, 0.0) == 0
    ctx.set_pred_select(False)
    assert calls["tz_encode"](0, 0.0) == TZ_ERR_STATE
    _idle(ctx)
    _reset(ctx)


_POISON_SCRIPT = """
import sys
import numpy as np
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import closedloop_jobs as J
import closedmap_jobs as M
from tezip_amd import _lib
h, w = M.SIZES[1]
nt, p, win = 7, 0, 3
cfg, wts = J.model()
ctx = _lib.Context(0)
ctx.load_model(cfg, wts)
ctx.prepare(_lib.pad8(h), _lib.pad8(w), 4)
ctx.set_quantiser("lattice")
ctx.set_bound_map(M.the_map(h, w))
for select, scene in ((False, "translating"), (True, "flicker")):
    frames = np.ascontiguousarray(M.frames(scene, nt, h, w))
    want = M.statement(scene, nt, h, w, p, win, "map", select, 0)
    ctx.set_pred_select(select)
    for rep in range(2):      # (the second call reuses pool blocks the first one filled)
        key = ctx.rollout_closed_map(frames, p, win)
        assert (key == want["key"]).all()
        if select:
            assert (ctx.pred_modes() == want["modes"]).all()
        _, _, delta = ctx.encode("abs", [0.0], True, want_delta=True)
        assert (delta == want["q"]).all()
        assert ctx.pool_held()[0] == 0
ctx.close()
print("poison ok")
"""


def test_same_results_under_poison(tmp_path):
    """TEZIP_POISON fills every device buffer handed out before its use (tests/test_gpu_poison.py): the loop reads nothing it did
    not write, whatever the pool's blocks held."""
    script = tmp_path / "poison_job.py"
    script.write_text(_POISON_SCRIPT % (ROOT, os.path.join(ROOT, "tests")))
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, str(script)], cwd=ROOT, capture_output=True, text=True,
                       env=dict(os.environ, TEZIP_POISON="0xA5"), timeout=330)
    assert r.returncode == 0 and "poison ok" in r.stdout, r.stdout + r.stderr
