"""The oldest operator seams -- tz_delta_encode, tz_error_bound, tz_reconstruct (and tz_decode_delta through it), tz_window_sse,
tz_remap / tz_unmap, tz_byte_shuffle / tz_byte_unshuffle -- on DEVICE buffers at every alignment a caller may pass.

A host array reaches the kernels through a pool block, which is 16-byte aligned; a device pointer is passed on as it is.  So
only a device buffer can take a kernel off its vector form, or into it with a pointer that form was not made for.  Every
buffer of every case here is a devmem.view: x at a chosen distance behind a 16-byte boundary, 64 bytes of 0x5A on both sides,
and every case asserts that the guards still hold.  What is expected comes from the C oracle (oracle/coracle.py) and is
compared bit for bit.

The tables below are the cases; tests/test_seam_cases.py checks without a GPU that they cover what they claim and that the
expected values are not vacuous.

TERMS: the address terms of each seam's dispatch (tz_codec.hip; DESIGN.md, "Wide accesses of the operator seams"), as
buffer -> (bytes per element, the alignments some vector form asks of the buffer).

OFFSETS: per seam, the byte offsets of its buffers behind a 16-byte boundary (a buffer that is not named sits on it):
  * every buffer aligned;
  * each buffer alone off by ONE ELEMENT;
  * all buffers off, by different amounts;
  * for every term (buffer, A): the buffer alone at the smallest offset that fails A and passes the narrower terms of the
    same buffer -- and at every larger power of two below A, where the narrower forms are entered at their least alignment;
  * tz_reconstruct's `out` at +1, +2 and +3: where k_recon's dword store is wrong by the letter.
"""
import numpy as np
import pytest

from oracle import coracle
from oracle import oracle as O

import devmem

pytestmark = pytest.mark.gpu

TERMS = {
    # k_delta_flat: float4 loads of pred, uint2 loads of orig, short8 stores
    "delta_encode": {"pred": (4, (16,)), "orig": (1, (8,)), "out": (2, (16,))},
    # k_q_tiles `grouped` (pred is NULL and tmp pool scratch for the stand-alone operator): uint3 loads of orig, uint2 of diff
    "error_bound": {"orig": (1, (4,)), "diff": (2, (8,))},
    # k_recon_flat: float4 pred, short8 diff, uint2 key, uint2 out; k_recon: dword stores of out
    "reconstruct": {"pred": (4, (16,)), "key": (1, (8,)), "diff": (2, (16,)), "out": (1, (4, 8))},
    # k_sse: element accesses only
    "window_sse": {"orig": (1, ()), "pred": (4, ())},
}

OFFSETS = {
    "delta_encode": [
        {},
        {"pred": 4}, {"pred": 8}, {"pred": 12},
        {"orig": 1}, {"orig": 2}, {"orig": 4},
        {"out": 2}, {"out": 4}, {"out": 8},
        {"orig": 8},                                     # the flat form with orig at its least alignment
        {"pred": 12, "orig": 5, "out": 6},
    ],
    "error_bound": [
        {},
        {"orig": 1}, {"orig": 2},
        {"diff": 2}, {"diff": 4},
        {"orig": 4}, {"diff": 8}, {"orig": 12, "diff": 8},   # the grouped form at its least alignment
        {"orig": 3, "diff": 6},
    ],
    "reconstruct": [
        {},
        {"pred": 4}, {"pred": 8}, {"pred": 12},
        {"key": 1}, {"key": 2}, {"key": 4},
        {"diff": 2}, {"diff": 4}, {"diff": 8},
        {"out": 1}, {"out": 2}, {"out": 3}, {"out": 4},
        {"key": 8, "out": 8},                            # the flat form with key and out at their least alignment
        {"pred": 4, "key": 1, "diff": 6, "out": 3},
        {"pred": 8, "key": 7, "diff": 10, "out": 12},    # the general form, dword stores
    ],
    "window_sse": [
        {},
        {"orig": 1}, {"pred": 4},
        {"orig": 3, "pred": 12},
    ],
}

# (frames, H, W, the mask of the call or None).  Unpadded: 8 x 8 (one vector group per 8 elements, no tail), 16 x 24; padded:
# 13 x 11 -> 16 x 16, 5 x 7 -> 8 x 8 (the general form, and n % 4 != 0 in k_recon).  One case per seam has a masked frame.
FRAME_SHAPES = {
    "delta_encode": [(2, 8, 8, None), (3, 16, 24, (0, 1, 0)), (2, 13, 11, None), (1, 5, 7, None)],     # zero_mask
    "reconstruct": [(3, 8, 8, (1, 0, 1)), (2, 16, 24, (0, 1)), (2, 13, 11, (1, 0)), (3, 5, 7, (0, 1, 0))],   # key_mask
    "window_sse": [(2, 8, 8, None), (2, 16, 24, None), (2, 13, 11, None), (1, 5, 7, None)],
    # quantiser chains: 8 x 8 one chunk; 5 x 4 HW % 4 == 0, less than a chunk; 13 x 11 HW % 4 != 0; 72 x 64 = 4608 elements,
    # two tiles: k_q_chain / k_q_bstitch run, and the smooth walk's runs cross the tile boundary.  skip_mask
    "error_bound": [(1, 8, 8, None), (2, 5, 4, None), (2, 13, 11, None), (3, 72, 64, (0, 1, 0))],
}

# all four modes at one bound that merges runs, and abs 0.3 (E < 0.5: only equal neighbours share a run)
MERGING_BOUNDS = [("abs", [2.0]), ("rel", [0.1]), ("absrel", [3.0, 0.1]), ("pwrel", [0.02])]
BOUNDS = MERGING_BOUNDS + [("abs", [0.3])]

LUT_SIZES = [1, 7, 8, 9, 4095, 4097]

REMAP_ALIGNMENT = "tezip_hip status -1: remap buffers must be 16-byte aligned"
SHUFFLE_ALIGNMENT = "tezip_hip status -1: byte-shuffle buffers must be 16-byte aligned"
SDELTA_ALIGNMENT = "tezip_hip status -1: spatial_delta buffers must be 16-byte aligned"      # FLAT_ALIGNMENT of test_gpu_layouts.py
SHUFFLE_MULTIPLE ="tezip_hip status -1: byte shuffle needs a multiple of 8 elements"


def pad8(v):
    return (v + 7) // 8 * 8


def label(off):
    return " ".join("%s+%d" % kv for kv in sorted(off.items())) or "aligned"


# ------------------------------------------------------------------------------------------- data and what is expected of it
def edge_predictions():
    """float32 predictions on whose value the truncation of compress.py:307 turns: exactly 0 and 1, and for every k in
    [1, 255) the three neighbours around k / 255 -- their float32 products with 255 sit one ulp on either side of k."""
    p = np.float32(np.arange(1, 255, dtype=np.float32) / np.float32(255))
    lo, hi = np.nextafter(p, np.float32(0)), np.nextafter(p, np.float32(2))
    return np.concatenate([np.array([0.0, 1.0], np.float32), np.stack([lo, p, hi], axis=1).reshape(-1)]).astype(np.float32)


def frames_u8(rng, nf, h, w):
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    out = []
    for t in range(nf):
        base = 120 + 60 * np.sin((xx + 2 * t) / 5.0) + 40 * np.cos((yy - t) / 4.0)
        img = np.stack([base, base * 0.7 + 30, 255 - base * 0.5], axis=-1) + rng.normal(0, 3.0, (h, w, 3))
        out.append(np.clip(np.round(img), 0, 255).astype(np.uint8))
    return np.stack(out)


def predictions(rng, nf, h, w):
    """(nf, Hp, Wp, 3) float32 in [0, 1], the pad region non-zero; the edge values dealt over the cropped part."""
    pred = rng.random((nf, pad8(h), pad8(w), 3), dtype=np.float32)
    edge = edge_predictions()
    crop = pred[:, :h, :w].reshape(-1).copy()
    where = rng.permutation(crop.size)[: min(edge.size, crop.size)]
    crop[where] = edge[: where.size]
    pred[:, :h, :w] = crop.reshape(nf, h, w, 3)
    return pred


def delta_data(nf, h, w, mask):
    rng = np.random.default_rng([1, nf, h, w])
    pred, orig = predictions(rng, nf, h, w), rng.integers(0, 256, (nf, h, w, 3), dtype=np.uint8)
    zero = None if mask is None else np.array(mask, np.uint8)
    want = np.stack([coracle.delta_frame(pred[i], orig[i], bool(zero is not None and zero[i])) for i in range(nf)])
    return pred, orig, zero, want


def bound_data(nf, h, w):
    """Originals and the `smooth` walk of test_gpu_parity.py: a delta stack whose neighbours differ by 0 or 1 mostly."""
    rng = np.random.default_rng([2, nf, h, w])
    orig = frames_u8(rng, nf, h, w)
    diff = np.clip(np.round(np.cumsum(rng.normal(0, 0.7, (nf, h * w, 3)), axis=1)), -255, 255).reshape(nf, h, w, 3).astype(np.int16)
    return orig, diff


def bound_expected(orig, diff, mask, mode, bound):
    return np.stack([diff[i] if mask is not None and mask[i] else coracle.error_bound_frame(orig[i], diff[i], mode, bound)
                     for i in range(orig.shape[0])])


def recon_data(nf, h, w, mask):
    """Deltas of +-300 against bases in [0, 255]: the sum leaves [0, 255] on both sides."""
    rng = np.random.default_rng([3, nf, h, w])
    pred, key = predictions(rng, nf, h, w), rng.integers(0, 256, (nf, h, w, 3), dtype=np.uint8)
    diff = rng.integers(-300, 301, (nf, h, w, 3)).astype(np.int16)
    km = np.array(mask, np.uint8)
    want = np.stack([coracle.reconstruct_frame(pred[i], key[i] if km[i] else None, diff[i]) for i in range(nf)])
    return pred, key, km, diff, want


def sse_data(nf, h, w):
    rng = np.random.default_rng([4, nf, h, w])
    pred, orig = predictions(rng, nf, h, w), rng.integers(0, 256, (nf, h, w, 3), dtype=np.uint8)
    return orig, pred, np.array([coracle.sse_frame(orig[i], pred[i]) for i in range(nf)])


def lut_data(n):
    """Symbols as the encoder has them (1600 - a spatial delta), their table, the ranks; and ranks with values that no table
    entry answers (they pass through)."""
    rng = np.random.default_rng([5, n])
    y = (1600 - np.clip(np.round(rng.normal(0, 6, n)), -255, 255)).astype(np.int16)
    table = O.build_table(y)
    ranks = O.remap_enc(y, table)
    loose = ranks.copy()
    loose[:: 3] = np.resize([-3, len(table) + 2, len(table) - 1, 2111, 2112], loose[:: 3].size)
    return y, table, ranks, loose


def identity_lut():
    return (np.arange(65536, dtype=np.int64) - 32768).astype(np.int16)


def enc_lut(table):
    lut = identity_lut()
    lut[np.asarray(table).astype(np.int64) + 32768] = np.arange(len(table))
    return lut


def byte_planes(x):
    b = np.ascontiguousarray(x, np.int16).reshape(-1).view(np.uint8)
    return np.concatenate([b[0::2], b[1::2]])


# ------------------------------------------------------------------------------------------------------------ the seams
@pytest.fixture(scope="module")
def ctx():
    from tezip_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


class Views:
    """The device views of one call: put(name, x, offsets) -> the view; check() asserts every guard."""

    def __init__(self, what):
        self.what, self.guards = what, []

    def put(self, name, x, off):
        v, intact = devmem.view(x, off.get(name, 0))
        self.guards.append((name, intact))
        return v

    def check(self):
        for name, intact in self.guards:
            assert intact(), "guard bytes of %s written, %s" % (name, self.what)


@pytest.mark.parametrize("nf,h,w,mask", FRAME_SHAPES["delta_encode"], ids=lambda v: str(v).replace(" ", ""))
def test_delta_encode(ctx, nf, h, w, mask):
    pred, orig, zero, want = delta_data(nf, h, w, mask)
    for off in OFFSETS["delta_encode"]:
        what = "tz_delta_encode %dx%dx%d %s" % (nf, h, w, label(off))
        vs = Views(what)
        out = vs.put("out", devmem.fill(want.shape, np.int16), off)
        ctx.delta_encode(vs.put("pred", pred, off), vs.put("orig", orig, off), zero, out=out)
        ctx.synchronize()
        np.testing.assert_array_equal(devmem.host(out), want, what)
        vs.check()


@pytest.mark.parametrize("nf,h,w,mask", FRAME_SHAPES["error_bound"], ids=lambda v: str(v).replace(" ", ""))
def test_error_bound_in_place(ctx, nf, h, w, mask):
    orig, diff = bound_data(nf, h, w)
    skip = None if mask is None else np.array(mask, np.uint8)
    for mode, bound in BOUNDS:
        want = bound_expected(orig, diff, skip, mode, bound)
        for off in OFFSETS["error_bound"]:
            what = "tz_error_bound %s %r %dx%dx%d %s" % (mode, bound, nf, h, w, label(off))
            vs = Views(what)
            d = vs.put("diff", diff, off)
            ctx.error_bound(vs.put("orig", orig, off), d, mode, bound, skip)
            ctx.synchronize()
            np.testing.assert_array_equal(devmem.host(d), want, what)
            vs.check()


@pytest.mark.parametrize("nf,h,w,mask", FRAME_SHAPES["reconstruct"], ids=lambda v: str(v).replace(" ", ""))
def test_reconstruct(ctx, nf, h, w, mask):
    pred, key, km, diff, want = recon_data(nf, h, w, mask)
    for off in OFFSETS["reconstruct"]:
        what = "tz_reconstruct %dx%dx%d %s" % (nf, h, w, label(off))
        vs = Views(what)
        out = vs.put("out", devmem.fill(want.shape, np.uint8), off)
        ctx.reconstruct(vs.put("pred", pred, off), vs.put("key", key, off), km, vs.put("diff", diff, off), out=out)
        ctx.synchronize()
        np.testing.assert_array_equal(devmem.host(out), want, what)
        vs.check()


@pytest.mark.parametrize("nf,h,w,mask", FRAME_SHAPES["window_sse"], ids=lambda v: str(v).replace(" ", ""))
def test_window_sse(ctx, nf, h, w, mask):
    orig, pred, want = sse_data(nf, h, w)
    for off in OFFSETS["window_sse"]:
        what = "tz_window_sse %dx%dx%d %s" % (nf, h, w, label(off))
        vs = Views(what)
        got = ctx.window_sse(vs.put("orig", orig, off), vs.put("pred", pred, off))
        assert got.tolist() == want.tolist(), what                 # the same summation order: the same bits
        vs.check()


def _refused(call, text, vs, out):
    from tezip_amd import _lib
    with pytest.raises(_lib.TezipError) as e:
        call()
    assert str(e.value) == text and e.value.status == -1, vs.what
    assert (devmem.host(out).reshape(-1).view(np.uint8) == devmem.GUARD_BYTE).all(), "a refused call wrote, " + vs.what
    vs.check()


@pytest.mark.parametrize("n", LUT_SIZES)
def test_remap_unmap_and_byte_planes(ctx, n):
    y, table, ranks, loose = lut_data(n)
    calls = [("tz_remap", lambda i, o: ctx.remap(i, table, out=o), y, coracle.lut_apply(y, enc_lut(table))),
             ("tz_unmap", lambda i, o: ctx.unmap(i, table, offset=False, out=o), loose, O.remap_dec(loose, table)),
             ("tz_unmap + offset", lambda i, o: ctx.unmap(i, table, offset=True, out=o), loose,
              (1600 - O.remap_dec(loose, table).astype(np.int32)).astype(np.int16)),
             ("tz_byte_unshuffle", lambda i, o: ctx.byte_unshuffle(i, out=o), byte_planes(ranks), ranks)]
    if n % 8 == 0:
        calls.append(("tz_byte_shuffle", lambda i, o: ctx.byte_shuffle(i, out=o), ranks, byte_planes(ranks)))
    for name, call, src, want in calls:
        vs = Views("%s n %d" % (name, n))
        out = vs.put("out", devmem.fill(want.shape, want.dtype), {})
        call(vs.put("in", src, {}), out)
        ctx.synchronize()
        np.testing.assert_array_equal(devmem.host(out), want, vs.what)
        vs.check()
        # off the 16-byte grid by one element, the input and then the output: refused, nothing written
        text = REMAP_ALIGNMENT if "map" in name else SHUFFLE_ALIGNMENT
        for off in ({"in": src.dtype.itemsize}, {"out": want.dtype.itemsize}):
            vs = Views("%s n %d %s" % (name, n, label(off)))
            out = vs.put("out", devmem.fill(want.shape, want.dtype), off)
            _refused(lambda: call(vs.put("in", src, off), out), text, vs, out)
    if n % 8:
        vs = Views("tz_byte_shuffle n %d" % n)
        out = vs.put("out", devmem.fill(2 * n, np.uint8), {})
        _refused(lambda: ctx.byte_shuffle(vs.put("in", ranks, {}), out=out), SHUFFLE_MULTIPLE, vs, out)


# ------------------------------------------------------------------------------------------------------- the whole paths
NT, H, W, WINDOW = 6, 16, 16, 2       # unpadded, a multiple of 16 elements: aligned buffers take the decoder's fused tail


def _model_context():
    from tezip_amd import _lib
    from tezip_amd.prednet import PredNetConfig
    cfg = PredNetConfig(stack_sizes=(3, 16, 32))
    c = _lib.Context(0)
    c.load_model(cfg, cfg.init_weights(seed=4, bias_scale=0.2))
    c.prepare(H, W, 4)
    return c


@pytest.fixture(scope="module")
def job():
    """One encoded sequence: the frames, the key mask and key stack, the payload and its table, the quantised delta stack."""
    from tezip_amd import synth
    frames = np.ascontiguousarray(synth.translating_scene(NT, H, W, seed=3))
    enc = _model_context()
    try:
        key = enc.rollout(frames, 0, WINDOW)[0]
        payload, table, _ = enc.encode("abs", [2.0], True)
        delta = np.array(enc.encode_delta("abs", [2.0]))
        vs = Views("tz_encode_delta out+2")
        out = vs.put("out", devmem.fill(delta.shape, np.int16), {"out": 2})
        enc.encode_delta("abs", [2.0], out=out)
        enc.synchronize()
        delta_dev = devmem.host(out)
        vs.check()
    finally:
        enc.close()
    key_stack = np.where(key[:, None, None, None], frames, 0).astype(np.uint8)
    return {"frames": frames, "key": key, "key_stack": key_stack, "payload": np.array(payload), "table": table, "delta": delta,
            "delta_dev": delta_dev}


def test_encode_delta_into_a_device_buffer_off_the_grid(job):
    assert np.abs(job["delta"]).max() > 0
    np.testing.assert_array_equal(job["delta_dev"], job["delta"])


def test_encode_refuses_a_device_payload_off_the_grid(job):
    """The payload is written by the remap (with a table) or by the spatial delta (without one; the fused passes step aside
    for a buffer off the grid): neither has an element-wise form, the call is refused and the buffer untouched."""
    enc = _model_context()
    try:
        enc.rollout(job["frames"], 0, WINDOW)
        for mode, bound, entropy, text in (("abs", [2.0], True, REMAP_ALIGNMENT), ("abs", [2.0], False, SDELTA_ALIGNMENT),
                                           ("abs", [0.0], False, SDELTA_ALIGNMENT)):
            vs = Views("tz_encode %s %r entropy %r payload+2" % (mode, bound, entropy))
            out = vs.put("payload", devmem.fill(job["payload"].shape, np.int16), {"payload": 2})
            _refused(lambda: enc.encode(mode, bound, entropy, payload=out), text, vs, out)
        vs = Views("tz_encode payload aligned")
        out = vs.put("payload", devmem.fill(job["payload"].shape, np.int16), {})
        enc.encode("abs", [2.0], True, payload=out)
        enc.synchronize()
        np.testing.assert_array_equal(devmem.host(out), job["payload"])
        vs.check()
    finally:
        enc.close()


def test_decode_from_and_into_device_buffers_off_the_grid(job):
    dec = _model_context()
    try:
        dec.prof_enable(True)
        dec.rollout_decode(job["key_stack"], 0)
        dec.prof_reset()
        want = np.array(dec.decode(job["payload"], job["table"]))
        prof = dec.prof_get()
        assert (int(prof["undelta_scan"][1]), int(prof["reconstruct"][1])) == (1, 0)        # the fused tail
        assert int(np.abs(want.astype(int) - job["frames"].astype(int)).max()) <= 2
        vs = Views("tz_decode payload+2 frames_out+1")
        out = vs.put("out", devmem.fill(want.shape, np.uint8), {"out": 1})
        dec.prof_reset()
        dec.decode(vs.put("payload", job["payload"], {"payload": 2}), job["table"], out=out)
        dec.synchronize()
        prof = dec.prof_get()
        assert (int(prof["undelta_scan"][1]), int(prof["reconstruct"][1])) == (1, 1)        # scan + reconstruct
        np.testing.assert_array_equal(devmem.host(out), want, vs.what)
        vs.check()
    finally:
        dec.close()


def test_decode_delta_reconstructs_into_device_buffers_off_the_grid(job):
    """tz_decode_delta is tz_reconstruct on the context's predictions and key frames: deltas that clamp on both sides, `out`
    at +1, +2 and +3 bytes, against the oracle's reconstruct of the predictions the context holds."""
    rng = np.random.default_rng(7)
    delta = rng.integers(-300, 301, job["frames"].shape).astype(np.int16)
    dec = _model_context()
    try:
        key = dec.rollout_decode(job["key_stack"], 0)
        assert key.any() and not key.all()
        pred = dec.get_predictions()
        want = np.stack([coracle.reconstruct_frame(pred[i], job["key_stack"][i] if key[i] else None, delta[i]) for i in range(NT)])
        assert (want == 0).any() and (want == 255).any()
        np.testing.assert_array_equal(dec.decode_delta(delta), want)
        for off in ({}, {"out": 1}, {"out": 2}, {"out": 3}, {"delta": 2}, {"delta": 8, "out": 4}, {"delta": 6, "out": 3}):
            vs = Views("tz_decode_delta " + label(off))
            out = vs.put("out", devmem.fill(want.shape, np.uint8), off)
            dec.decode_delta(vs.put("delta", delta, off), out=out)
            dec.synchronize()
            np.testing.assert_array_equal(devmem.host(out), want, vs.what)
            vs.check()
    finally:
        dec.close()
