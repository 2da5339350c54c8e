"""The predictor and the codec at the largest frame size tz_model_prepare accepts (run with -m gpu on a MI355X).

tz_model_prepare refuses a frame when some level's widest plane, npx_l * max(4 R_l, 2 S_l, 8) floats, reaches 2^30: the
fast convolution kernels address inside one frame's plane with 32-bit byte offsets.  These tests hold the guard at its
exact edges and run the frames just inside it -- where a signed product, a sign extension or a wrapped 32-bit offset
would show -- against the C oracle on crops of the frame (tests/crop_oracle.py), bit for bit:
  * PredNet (3,48,96,192): level 1's 192 gate columns bind, 4728 x 4728 is the largest square (E_1, the widest plane a
    32-bit-addressed kernel reads, ends 1.5 MB under 2^31 bytes);
  * a model with R < S, (3,64,64) / R (3,16,16): level 1's error maps bind, 5792 x 5792 is the largest square and E_1's
    byte offsets pass 2^31 near the middle row of the frame;
  * (3,64): 4096 x 4096 holds exactly 2^30 floats at level 1 and is refused.
"""
import re

import numpy as np
import pytest

import crop_oracle as CO
from oracle import coracle
from tezip_amd.prednet import PredNetConfig

pytestmark = pytest.mark.gpu

MODELS = {
    "default": PredNetConfig(),
    "r_lt_s": PredNetConfig(stack_sizes=(3, 64, 64), R_stack_sizes=(3, 16, 16)),
    "two_level": PredNetConfig(stack_sizes=(3, 64)),
}


# ---------------------------------------------------------------------------- the rule, restated
def _widest(cfg, l):
    return max(4 * cfg.R_stack_sizes[l], 2 * cfg.stack_sizes[l], 8)


def _step(cfg):
    return max(8, 1 << (cfg.nb_layers - 1))


def _accepts(cfg, hp, wp):
    return all((hp >> l) * (wp >> l) * _widest(cfg, l) < (1 << 30) for l in range(cfg.nb_layers))


def _limit_px(cfg):
    """The figure the refusal message reports: the largest frame, in level-0 pixels, the binding level allows."""
    return min((((1 << 30) - 1) // _widest(cfg, l)) << (2 * l) for l in range(cfg.nb_layers))


def _largest_square(cfg):
    s = _step(cfg)
    n = int(_limit_px(cfg) ** 0.5) // s * s + 2 * s
    while not _accepts(cfg, n, n):
        n -= s
    return n


def _largest_strip(cfg):
    s = _step(cfg)
    w = _limit_px(cfg) // s // s * s + 2 * s
    while not _accepts(cfg, s, w):
        w -= s
    return w


def test_the_restated_rule_gives_the_documented_edges():
    d, r, t = MODELS["default"], MODELS["r_lt_s"], MODELS["two_level"]
    assert _limit_px(d) == 22369620
    assert (_largest_square(d), _largest_strip(d)) == (4728, 2796200)
    assert _accepts(d, 4096, 4096) and not _accepts(d, 4736, 4736) and not _accepts(d, 8, 2796208)
    assert 2364 * 2364 * 192 == 1072991232 < (1 << 30)
    assert _largest_square(r) == 5792 and not _accepts(r, 5800, 5800)
    assert not _accepts(t, 4096, 4096) and 2048 * 2048 * 256 == 1 << 30 and _accepts(t, 4088, 4096)
    # which plane binds: the default model's level-1 gate columns, the R < S model's level-1 error maps
    assert _widest(d, 1) == 4 * 48 and _widest(r, 1) == 2 * 64


def _ctx():
    from tezip_amd import _lib
    return _lib.Context(0)


def _mem_used():
    import torch
    free, total = torch.cuda.mem_get_info(0)
    return (total - free) / 2 ** 30


@pytest.mark.parametrize("name", sorted(MODELS))
def test_prepare_accepts_the_largest_frames_and_refuses_the_next(name):
    """The largest legal square and one-tile strip are accepted; the next legal size of each -- and the documented edges
    -- is refused with TZ_ERR_UNSUPPORTED before anything is allocated, with the Python rule's limit figure in the message;
    the context stays usable after every refusal."""
    from tezip_amd._lib import TezipError
    cfg = MODELS[name]
    s = _step(cfg)
    sq, strip = _largest_square(cfg), _largest_strip(cfg)
    refused = [(sq + s, sq + s), (s, strip + s)]
    accepted = [(sq, sq), (s, strip)]
    if name == "default":
        accepted.append((4096, 4096))
        refused.append((4728, 4736))
    if name == "r_lt_s":
        refused.append((5800, 5792))
    if name == "two_level":
        refused.append((4096, 4096))
        accepted.append((4088, 4096))
    wts = cfg.init_weights(seed=3, bias_scale=0.25)
    c = _ctx()
    try:
        c.load_model(cfg, wts)
        for hp, wp in accepted:
            assert _accepts(cfg, hp, wp)
            c.prepare(hp, wp, 1)
        for hp, wp in refused:
            assert not _accepts(cfg, hp, wp)
            with pytest.raises(TezipError) as ei:
                c.prepare(hp, wp, 1)
            msg = str(ei.value)
            assert ei.value.status == -6 and "32-bit" in msg, msg   # TZ_ERR_UNSUPPORTED
            assert int(re.search(r"up to about (\d+) pixels", msg).group(1)) == _limit_px(cfg), msg
            assert "%dx%d" % (hp, wp) in msg, msg
            # usable: a small frame prepares and predicts as the oracle does
            c.prepare(16, 16, 1)
            net = coracle.CPredNet(wts, cfg.stack_sizes, cfg.R_stack_sizes, 16, 16)
            np.testing.assert_array_equal(c.predict_c0(), net.c0())
    finally:
        c.close()


# ---------------------------------------------------------------------------- the predictor at the limit
def _e1_row_past_2_31(cfg, hp, wp):
    """The level-0 row at which level 1's error-map plane (2 S_1 floats per pixel) passes 2^31 bytes."""
    return 2 * ((1 << 31) // ((wp >> 1) * 2 * cfg.stack_sizes[1] * 4))


CASES = {"default_square": ("default", 4728, 4728), "default_strip": ("default", 8, 2796200),
         "r_lt_s_square": ("r_lt_s", 5792, 5792)}


@pytest.mark.parametrize("case", list(CASES))
def test_predictor_at_the_frame_size_limit(case):
    """Three random frames through a context prepared for batches of 2 (the second item's planes start past 2^32 bytes
    into their buffers), under TZ-PA1 and TZ-PA2, with the fast kernels and with the general ones: the two dispatches
    agree bit for bit on the whole frame, PA1 and PA2 are the same function to 2e-5, and c0 and every prediction equal
    the C oracle bit for bit on crops at both corners (and, for the R < S model, across the row where E_1's byte offset
    passes 2^31).  The fast kernel families are asserted by the profiler counts, so that a dispatch change cannot
    quietly route these sizes round them."""
    name, hp, wp = CASES[case]
    cfg = MODELS[name]
    assert _accepts(cfg, hp, wp) and not _accepts(cfg, hp + _step(cfg), wp + _step(cfg))
    wts = cfg.init_weights(seed=29, bias_scale=0.25)
    rng = np.random.default_rng(31)
    frames = (rng.integers(0, 256, (3, hp, wp, 3), dtype=np.uint8).astype(np.float32) / np.float32(255))
    L = cfg.nb_layers
    crops = {"top_left": CO.corner(hp, wp, L, "tl", 128, CO.margin(1)),
             "bottom_right": CO.corner(hp, wp, L, "br", 128, CO.margin(1))}
    if name == "r_lt_s":
        y = _e1_row_past_2_31(cfg, hp, wp)
        assert 2900 > y > 2880 and (y // 2) * (wp // 2) * 128 * 4 < (1 << 31) <= (y // 2 + 1) * (wp // 2) * 128 * 4
        crops["e1_past_2_31"] = CO.plan(hp, wp, L, (y - 32, y + 32), (wp // 2 - 64, wp // 2 + 64), CO.margin(1))
        assert all(crops["e1_past_2_31"].artificial())
    c = _ctx()
    preds = {}
    try:
        c.load_model(cfg, wts)
        c.prepare(hp, wp, max_batch=2)
        for contract in (1, 2):
            c.set_contract(contract)
            c0 = c.predict_c0()
            c.prof_enable(True)
            c.prof_reset()
            fast = c.predict_next(frames)
            p = c.prof_get()
            c.set_conv_impl(0)
            try:
                general = c.predict_next(frames)
            finally:
                c.set_conv_impl(1)
                c.prof_enable(False)
            n = {k: v[1] for k, v in p.items()}
            print("%s PA%d launches: %s; device memory in use %.1f GiB" % (case, contract, {
                k: n[k] for k in ("wino_pa2", "conv16_lds_dma", "convlat_small_grid", "conv16b_level0", "conv_small_valu",
                                  "conv3x3_general")}, _mem_used()))
            if contract == 2:
                assert n["wino_pa2"] > 0 and n["conv3x3_general"] == 0, n
            else:
                assert n["conv16_lds_dma"] + n["convlat_small_grid"] > 0 and n["wino_pa2"] == 0, n
            assert n["conv16b_level0"] + n["conv_small_valu"] > 0, n
            if name == "default":
                assert n["conv16b_level0"] > 0 and n["conv_small_valu"] > 0, n
            assert np.array_equal(fast, general), "PA%d: the fast kernels and the general kernels differ" % contract
            del general
            for cname, crop in crops.items():
                co = CO.CropOracle(cfg, wts, crop, contract)
                CO.assert_matches(c0, co.c0(), crop, CO.margin(0), "%s PA%d c0 %s" % (case, contract, cname))
                for i in range(len(frames)):
                    CO.assert_matches(fast[i], co.next(frames[i]), crop, CO.margin(1),
                                      "%s PA%d frame %d %s" % (case, contract, i, cname))
            preds[contract] = fast
        for i in range(len(frames)):
            assert np.abs(preds[1][i] - preds[2][i]).max() < 2e-5
    finally:
        c.close()


# ---------------------------------------------------------------------------- a whole job at the limit
def _job_frames(nt, h, w, seed):
    rng = np.random.default_rng(seed)
    yy = np.arange(h, dtype=np.float32)[:, None]
    xx = np.arange(w, dtype=np.float32)[None, :]
    out = np.empty((nt, h, w, 3), np.uint8)
    for t in range(nt):
        base = 120 + 60 * np.sin((xx + 2 * t) / 37.0) + 40 * np.cos((yy - t) / 29.0)
        noise = rng.integers(-3, 4, (h, w, 3), dtype=np.int16)
        for ch, (a, b) in enumerate([(1.0, 0.0), (0.7, 30.0), (-0.5, 255.0)]):
            out[t, :, :, ch] = np.clip(np.rint(a * base + b) + noise[:, :, ch], 0, 255).astype(np.uint8)
    return out


@pytest.fixture(scope="module")
def job():
    """PredNet (3,48,96,192) prepared for 4728 x 4728, five frames of a smooth moving pattern with noise."""
    cfg = MODELS["default"]
    wts = cfg.init_weights(seed=123)
    c = _ctx()
    c.load_model(cfg, wts)
    c.prepare(4728, 4728, max_batch=2)
    yield c, cfg, wts, _job_frames(5, 4728, 4728, 7)
    c.close()


@pytest.mark.parametrize("mode,bound", [("abs", [0.0]), ("abs", [2.0]), ("pwrel", [0.05])])
def test_a_whole_job_at_the_frame_size_limit(job, mode, bound):
    """nt 5, warm-up 1, window 3 at 4728 x 4728 under the default contract (TZ-PA2): the key mask; the predictions against
    an oracle rollout on the bottom-right crop; the delta tap against the oracle's delta and error bound on the device's
    own predictions, frame by frame; payload and table against the oracle's back half; the decoder's rollout and tail
    (lossless bit-exact, lossy = the oracle's reconstruction of the quantised delta, within the bound); and the quality
    records against numpy's int64 statistics of the decoded frames."""
    c, cfg, wts, frames = job
    nt, h, w = frames.shape[:3]
    key, _ = c.rollout(frames, 1, 3)
    assert key.tolist() == [True, True, False, False, True]
    assert c.rollout_contract() == 2
    pred = c.get_predictions()
    crop = CO.corner(h, w, cfg.nb_layers, "br", 128, CO.margin(2))
    co = CO.CropOracle(cfg, wts, crop, 2)
    for d, ref in enumerate(co.rollout(coracle.u8_to_f32_frame(frames[1], h, w), 2), 1):
        CO.assert_matches(pred[1 + d], ref, crop, CO.margin(d), "%s %r depth %d" % (mode, bound, d))
    payload, table, delta = c.encode(mode, bound, True, want_delta=True)
    for i in range(nt):
        if key[i]:
            assert not delta[i].any(), "key frame %d" % i
        else:
            want = coracle.error_bound_frame(frames[i], coracle.delta_frame(pred[i], frames[i]), mode, bound)
            np.testing.assert_array_equal(delta[i], want, err_msg="delta frame %d" % i)
    ref_payload, ref_table = coracle.encode_tail(delta, True)
    np.testing.assert_array_equal(table, ref_table)
    assert np.array_equal(payload, ref_payload)
    del ref_payload
    payload = np.array(payload)
    q = c.encode_quality(payload, table)
    keys = np.where(key[:, None, None, None], frames, 0).astype(np.uint8)
    assert (c.rollout_decode(keys, 1) == key).all()
    dec = np.array(c.decode(payload, table))
    if bound == [0.0]:
        assert np.array_equal(dec, frames)
    else:
        for i in range(nt):
            want = frames[i] if key[i] else coracle.reconstruct_frame(pred[i], None, delta[i])
            np.testing.assert_array_equal(dec[i], want, err_msg="decoded frame %d" % i)
        err = np.abs(dec.astype(np.int16) - frames.astype(np.int16))
        assert int(err.max()) <= (bound[0] + 1 if mode == "abs" else bound[0] * 255 + 2)
    d = (dec.astype(np.int64) - frames.astype(np.int64)).reshape(nt, -1)
    want = np.stack([(d * d).sum(1), np.abs(d).max(1), (d != 0).sum(1)], axis=1)
    got = np.stack([q["sse"].astype(np.int64), q["max_abs"].astype(np.int64), q["n_changed"].astype(np.int64)], axis=1)
    np.testing.assert_array_equal(got, want)
    print("job %s %r: device memory in use %.1f GiB" % (mode, bound, _mem_used()))


def test_dwp_rollout_at_the_frame_size_limit(job):
    """A dynamic-window rollout at 4728 x 4728 (k_sse / k_sse_decide over 22 M-pixel frames): its decisions replayed in
    float64 from the device's own predictions (compress.py:245-263)."""
    c, cfg, wts, frames = job
    nt, h, w = frames.shape[:3]
    fe_pad = h * w * 3
    _, probe = c.rollout(frames, 1, None, 1e9, want_mse=True)
    thr = float(min(probe[3], probe[4])) * (1 - 1e-6)   # some frame past depth 1 is rejected
    key, mse = c.rollout(frames, 1, None, thr, want_mse=True)
    pred = c.get_predictions()
    run, k0, expect = 0.0, 2, [0, 1]
    for idx in range(2, nt):
        if key[idx] and not (idx == nt - 1 and mse[idx] <= thr):
            assert mse[idx] > thr
            expect.append(idx)
            k0, run = idx + 1, 0.0
            continue
        run += coracle.sse_frame(frames[idx], pred[idx])
        stop = run / ((idx - k0 + 1) * fe_pad)
        assert stop == pytest.approx(mse[idx], rel=1e-9) and stop <= thr
    assert key.nonzero()[0].tolist() == expect
    assert len(expect) > 2   # the threshold did reject a frame
