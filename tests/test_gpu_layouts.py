"""The three payload layouts of the codec's lossless back half -- flat (3 channels, delta against the element in front), gray
(1 channel) and channel stride (3 channels, delta against the element three in front) -- pinned below the bytes: which
launches serve each entry point (per-class launch counts of the profiler), the TZD64 digests of what they produce, the seam
functions at the sizes where their kernels change form, and the text of every refusal.  The launch counts and digests are
those of the commit before the layouts were put behind one host path (tests/golden/layout_launches_parent.json, written by
tests/golden/make_layout_launches.py); the seams are compared with the numpy statements."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "layout_launches_parent.json")
NBINS = 2111
# name in the fixture -> tz_prof_name
CLASSES = {"delta": "delta", "quant": "quant", "spatial_delta_hist": "spatial_delta_hist", "lut": "lut_remap", "scan": "undelta_scan",
           "recon": "reconstruct", "carry": "undelta_carry", "quality": "quality", "digest": "digest", "QSERIAL": "quant_serial_chains"}
LAYOUTS = {"flat": (3, 0), "gray": (1, 0), "stride": (3, 1)}      # (tz_set_payload_channels, tz_set_delta_stride)
# 16 x 16: unpadded and a multiple of 16 elements, the flat decoder takes its fused walk; 13 x 11: padded to 16 x 16, every
# layout takes scan + reconstruct
SIZES = {"16x16": (16, 16), "13x11": (13, 11)}
NT, WARM_UP, WINDOW, RANGE = 6, 1, 2, (3, 2)
CASES = [(l, s) for l in LAYOUTS for s in SIZES]
GRAY_DELTA_OUT = "tezip_hip status -1: tz_encode: no delta_out with a one-channel payload"


def pad8(v):
    return (v + 7) // 8 * 8


def _model():
    from tezip_amd.prednet import PredNetConfig
    cfg = PredNetConfig(stack_sizes=(3, 16, 32))
    return cfg, cfg.init_weights(seed=4, bias_scale=0.2)


def _frames(layout, h, w):
    from tezip_amd import synth
    f = np.ascontiguousarray(synth.translating_scene(NT, h, w, seed=3))
    return np.ascontiguousarray(np.repeat(f[..., :1], 3, axis=-1)) if layout == "gray" else f


def _context(layout, h, w):
    from tezip_amd import _lib
    cfg, wts = _model()
    c = _lib.Context(0)
    c.load_model(cfg, wts)
    c.prepare(pad8(h), pad8(w), 4)
    channels, stride = LAYOUTS[layout]
    c.set_payload_channels(channels)
    c.set_delta_stride(stride)
    c.prof_enable(True)
    return c


def _digest(x):
    from tezip_amd import digest
    return "none" if x is None else "%016x" % digest.frame_digest(np.ascontiguousarray(x).reshape(-1).view(np.uint8))


def _counted(ctx, call):
    """call() between prof_reset and prof_get -> (its result, the launch count of every class of CLASSES)."""
    ctx.prof_reset()
    result = call()
    prof = ctx.prof_get()
    return result, {k: int(prof[name][1]) for k, name in CLASSES.items()}


def record(layout, size):
    """What one case pins: {step: {"launches": {class: count}, digests ...}}."""
    from tezip_amd import _lib
    h, w = SIZES[size]
    frames = _frames(layout, h, w)
    first, count = RANGE
    out = {}
    enc = _context(layout, h, w)
    try:
        key = enc.rollout(frames, WARM_UP, WINDOW)[0]
        for step, (mode, bound, entropy) in (("encode_lossless", ("abs", [0.0], True)), ("encode_abs2", ("abs", [2.0], True)),
                                             ("encode_no_entropy", ("abs", [2.0], False))):
            (payload, table, _), launches = _counted(enc, lambda: enc.encode(mode, bound, entropy))
            out[step] = {"launches": launches, "payload": _digest(payload), "table": _digest(table)}
        if layout == "gray":
            with pytest.raises(_lib.TezipError) as e:
                enc.encode("abs", [2.0], True, want_delta=True)
            assert str(e.value) == GRAY_DELTA_OUT
        else:
            (p, t, delta), launches = _counted(enc, lambda: enc.encode("abs", [2.0], True, want_delta=True))
            out["encode_delta_out"] = {"launches": launches, "payload": _digest(p), "table": _digest(t), "delta": _digest(delta)}
        payload, table, _ = enc.encode("abs", [2.0], True)
        q, launches = _counted(enc, lambda: enc.encode_quality(payload, table))
        out["encode_quality"] = {"launches": launches, "quality": _digest(q)}
    finally:
        enc.close()
    key_stack = np.where(key[:, None, None, None], frames, 0).astype(np.uint8)
    dec = _context(layout, h, w)
    try:
        dec.rollout_decode(key_stack, WARM_UP)
        got, launches = _counted(dec, lambda: dec.decode(payload, table))
        out["decode"] = {"launches": launches, "frames": _digest(got)}
        whole = np.array(got)
        dec.rollout_decode_range(key_stack, WARM_UP, first, count)
        got, launches = _counted(dec, lambda: dec.decode_range(payload, table, first, count))
        out["decode_range"] = {"launches": launches, "frames": _digest(got)}
        np.testing.assert_array_equal(got, whole[first: first + count])
        assert int(np.abs(whole.astype(int) - frames.astype(int)).max()) <= 2
    finally:
        dec.close()
    return out


@pytest.fixture(scope="module")
def parent():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("layout,size", CASES, ids=["%s-%s" % c for c in CASES])
def test_launches_and_digests_are_the_parents(parent, layout, size):
    got = record(layout, size)
    want = parent["%s-%s" % (layout, size)]
    assert sorted(got) == sorted(want)
    for step in sorted(want):
        assert got[step] == want[step], "%s %s: %s" % (layout, size, step)


# ------------------------------------------------------------------------------------------------------------- the seams
SEAM_SIZES = [1, 2, 3, 4, 7, 8, 9, 24, 25, 49, 4097]
STRIDE3_HOST_COVERED = {1, 2, 3, 4, 7, 8, 49, 4097}       # test_gpu_sdelta.py: host buffers, aligned and off the grid


@pytest.fixture(scope="module")
def ctx():
    from tezip_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _stack(n, seed):
    rng = np.random.default_rng(seed)
    x = rng.integers(-32768, 32768, n, dtype=np.int16)
    if n > 64:
        x[n // 3: n // 3 + n // 4] = rng.integers(-12, 13, n // 4)
    return x


def _counts(y):
    inside = y[(y >= 0) & (y < NBINS)].astype(np.int64)
    return np.bincount(inside, minlength=NBINS).astype(np.uint64)


class _Host:
    """Buffers that start 2 bytes off the 16-byte grid, in host memory."""
    name = "host"

    def put(self, x):
        hold = np.empty(x.size + 8, np.int16)
        k = ((2 - hold.ctypes.data) % 16) // 2        # hold[k] sits 2 bytes behind a 16-byte boundary
        hold[k: k + x.size] = x
        return hold[k: k + x.size]

    def out(self, n):
        return self.put(np.full(n, 0x5A5A, np.int16))

    def hist(self):
        return np.full(NBINS, 3, np.uint64), np.uint64(3)

    def get(self, ctx, t):
        return np.array(t)


class _Device(_Host):
    """The same in device memory, with guard elements around the output."""
    name = "device"

    def put(self, x):
        import torch
        t = torch.full((x.size + 16,), 0x5A5A, dtype=torch.int16, device="cuda")
        t[1: 1 + x.size].copy_(torch.from_numpy(x))
        torch.cuda.synchronize()
        self.whole = t
        return t[1: 1 + x.size]

    def hist(self):
        import torch
        t = torch.full((NBINS,), 3, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        return t, np.uint64(3)

    def get(self, ctx, t):
        ctx.synchronize()
        return t.cpu().numpy().astype(np.uint64) if t.element_size() == 8 else t.cpu().numpy()

    def guards_intact(self, n):
        o = self.whole.cpu().numpy()
        return o[0] == 0x5A5A and (o[1 + n:] == 0x5A5A).all()


def _forward(ctx, sd, gp, mem, kind, x, carry, offset, with_hist):
    """One spatial-delta seam call against its numpy statement.  kind: "flat", "gray", 1 or 3 (tz_spatial_delta_stride)."""
    what = "%s %s n %d carry %r offset %d hist %r" % (kind, mem.name, x.size, carry is not None, offset, with_hist)
    hist, h0 = mem.hist() if with_hist else (None, None)
    if kind == "gray":
        n = x.size // 3
        want = gp.spatial_delta(np.ascontiguousarray(x.reshape(-1, 3)[:, 0]), None if carry is None else int(carry[0]))
        want = (1600 - want.astype(np.int64)).astype(np.int16) if offset else want
        src, out = mem.put(x), mem.out(n)
        ctx.spatial_delta_gray(src, offset, carry=None if carry is None else int(carry[0]), hist=hist, out=out)
    else:
        n = x.size
        stride = 1 if kind == "flat" else kind
        want = sd.encode(x, stride, offset, None if carry is None else carry[:stride])
        src, out = mem.put(x), mem.out(n)
        if stride == 1 and isinstance(mem, _Device):     # k_sdelta has no scalar form: device buffers off the grid are refused
            from tezip_amd import _lib
            with pytest.raises(_lib.TezipError) as e:
                if kind == "flat":
                    ctx.spatial_delta(src, offset, out=out)
                else:
                    ctx.spatial_delta_stride(src, 1, offset, out=out)
            assert str(e.value) == FLAT_ALIGNMENT, what
            return
        if kind == "flat":
            ctx.spatial_delta(src, offset, carry=None if carry is None else int(carry[0]), hist=hist, out=out)
        else:
            ctx.spatial_delta_stride(src, stride, offset, carry=None if carry is None else carry[:stride], hist=hist, out=out)
    np.testing.assert_array_equal(mem.get(ctx, out), want, what)
    if isinstance(mem, _Device):
        assert mem.guards_intact(n), "guard elements written, " + what
    if with_hist:
        np.testing.assert_array_equal(mem.get(ctx, hist) - h0, _counts(want), "histogram, " + what)   # the counts are ADDED


def _inverse(ctx, sd, mem, kind, s, carry):
    what = "undelta %s %s n %d carry %r" % (kind, mem.name, s.size, carry is not None)
    stride = 1 if kind == "flat" else kind
    want = sd.decode(s, stride, False, None if carry is None else carry[:stride])
    src, out = mem.put(s), mem.out(s.size)
    if kind == "flat":
        ctx.spatial_undelta(src, carry=None if carry is None else int(carry[0]), out=out)
    else:
        ctx.spatial_undelta_stride(src, stride, carry=None if carry is None else carry[:stride], out=out)
    np.testing.assert_array_equal(mem.get(ctx, out), want, what)
    if isinstance(mem, _Device):
        assert mem.guards_intact(s.size), "guard elements written, " + what


CARRY = np.array([-77, 30000, -32768], np.int16)
FLAT_ALIGNMENT = "tezip_hip status -1: spatial_delta buffers must be 16-byte aligned"


@pytest.mark.parametrize("n", SEAM_SIZES)
def test_seams_at_the_sizes_where_the_kernels_change_form(ctx, n):
    from tezip_amd import graypayload as gp, sdelta as sd
    x, x3 = _stack(n, n), _stack(3 * n, 1000 + n)            # gray: n pixels of three channels
    rng = np.random.default_rng(n)
    d = rng.integers(-255, 256, n).astype(np.int16)           # a delta stack as the encoder has it: a table applies
    for mem in (_Host(), _Device()):
        for kind in ("flat", "gray", 1, 3):
            if kind == 3 and mem.name == "host" and n in STRIDE3_HOST_COVERED:
                continue
            for carry in (None, CARRY):
                for with_hist in (False, True):
                    for offset in (0, 1):
                        _forward(ctx, sd, gp, mem, kind, x3 if kind == "gray" else x, carry, offset, with_hist)
                if kind != "gray":
                    _inverse(ctx, sd, mem, kind, x, carry)
        # the prefix carry: the decoded elements in front of payload[n0], from the symbols as stored and through a table
        for stride in (1, 3):
            n0 = n // stride * stride
            if n0 == 0 or (stride == 3 and mem.name == "host" and n in (3, 24)):     # (covered by test_gpu_sdelta.py)
                continue
            what = "carry stride %d %s n0 %d" % (stride, mem.name, n0)
            np.testing.assert_array_equal(ctx.undelta_carry_stride(mem.put(sd.encode(x, stride, False)), n0, stride), x[n0 - stride: n0], what)
            payload, table = sd.payload_from_delta(d, True, stride)
            np.testing.assert_array_equal(ctx.undelta_carry_stride(mem.put(payload), n0, stride, table), d[n0 - stride: n0], what + " table")
            if stride == 1:
                assert ctx.undelta_carry(mem.put(sd.encode(x, 1, False)), n0) == int(x[n0 - 1]), what
                assert ctx.undelta_carry(mem.put(payload), n0, table) == int(d[n0 - 1]), what + " table"


# ----------------------------------------------------------------------------------------------------------- the refusals
GRAY_TEXT = ("tezip_hip status -6: %s does not serve a one-channel payload (tz_set_payload_channels(1)): sharded gray jobs are "
             "not supported")
STRIDE_TEXT = ("tezip_hip status -6: %s does not serve the channel-stride spatial delta (tz_set_delta_stride(1)): sharded jobs "
               "and one-element carries are flat only")


def test_refusal_messages_of_the_flat_only_entry_points():
    from tezip_amd import _lib
    h, w = SIZES["13x11"]
    frames = _frames("gray", h, w)
    c = _context("flat", h, w)
    try:
        c.rollout(frames, WARM_UP, WINDOW)
        payload, table, _ = c.encode("abs", [2.0], True)
        calls = ((lambda: c.encode_begin("abs", [2.0], True), "tz_encode_begin"),
                 (lambda: c.encode_finish(None, None), "tz_encode_finish"),
                 (lambda: c.encode_delta("abs", [2.0]), "tz_encode_delta"),
                 (lambda: c.decode_delta(np.zeros(frames.shape, np.int16)), "tz_decode_delta"))
        carry_call = (lambda: c.undelta_carry(payload, 3, table), "tz_undelta_carry")
        for channels, stride, text, served in ((1, 0, GRAY_TEXT, True), (3, 1, STRIDE_TEXT, False), (1, 1, GRAY_TEXT, False)):
            c.set_payload_channels(channels)
            c.set_delta_stride(stride)
            for call, name in calls:
                with pytest.raises(_lib.TezipError) as e:
                    call()
                assert str(e.value) == text % name and e.value.status == -6
            # tz_undelta_carry serves a one-channel payload (its carry is one element) and refuses the stride mode alone
            if served:
                carry_call[0]()
            else:
                with pytest.raises(_lib.TezipError) as e:
                    carry_call[0]()
                assert str(e.value) == STRIDE_TEXT % carry_call[1] and e.value.status == -6
        c.set_payload_channels(1)
        c.set_delta_stride(0)
        with pytest.raises(_lib.TezipError) as e:
            c.encode("abs", [2.0], True, want_delta=True)
        assert str(e.value) == GRAY_DELTA_OUT
        c.set_payload_channels(3)
        c.encode_delta("abs", [2.0])                                            # flat: served as ever
    finally:
        c.close()
