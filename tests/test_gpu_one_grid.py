"""The opt-in codec paths past one grid of lanes, on a MI355X.

Nearly every kernel of tezip_amd/csrc/tz_codec.hip is launched with a capped grid and walks its work in a grid-stride loop.
On its second trip a lane forms its frame index, its frame-start flag, its channel rotation and the elements in front of its
first anew, reads zero_mask[f] and P[3 f + c] again and keeps adding to its histogram.  The gray layout, the channel-stride
layout, the lattice quantiser TZ-QL1, the per-frame bounds, tz_bound_err with the probes and the key coders were tested at
64 x 64-class shapes only, where no lane takes a second trip.  Here every one of them runs at the smallest shape that crosses
its cap, against the slow statements the project already has (tezip_amd/lattice.py, graypayload.py, sdelta.py, target.py,
keycoder.py, keycoderg.py, the C oracle's greedy quantiser), integers and bytes throughout, once from host arrays and once
from device tensors that start one element behind their allocation.  tests/test_one_grid_shapes.py (CPU) holds the caps
against the source and every shape below against its conditions.

Out of scope: k_size_count, k_size_bits, k_huffr_count and k_huffd_count cap at 2048 x 256 runs of 256 elements, which is
134 M elements; a test past that cap does not fit a few seconds.

One condition of the whole jobs is met as far as their shapes allow: a key frame among the frames behind the boundary with a
predicted frame behind it leaves the gray job (18 frames, frame 16 at the boundary) ONE predicted frame that starts behind
the boundary, frame 17, and the colour job frame 23 and the part of frame 21 behind symbol 2^22.  The tests assert that the
quantiser changes deltas behind the boundary in every predicted frame that reaches there (two in the colour job).

Under the greedy quantiser the gray and the channel-stride layout have no fused pass (k_q_fill_sym serves the flat layout
alone, and tests/test_gpu_configs.py takes it past its 1024 workgroups): the jobs here run k_q_fill, k_sdelta_gray and
k_sdelta_s3 over the whole job instead."""
import functools

import numpy as np
import pytest

import test_gpu_gray as TG
import test_gpu_keycoder as TK
import test_gpu_keycoderg as TKG
import test_gpu_lattice as TL
import test_gpu_target as TT

pytestmark = pytest.mark.gpu

# symbols (elements, pixels, bytes) one launch reaches before a lane takes its second trip
ONE_TRIP = 1 << 22       # grid_for(): kCUs * kBlocksPerCU = 2048 workgroups x 256 lanes x 8 symbols; the histogram fronts: HB_GRID = 512
#                          workgroups x HB_THREADS = 1024 lanes x 8 symbols; k_bound_err: 2048 tiles of BE_TILE = 2048 elements
RECON_TRIP = 1 << 21     # k_recon / k_recon_gray, general form: grid_for(n / 4 + 1, 256) = 2048 x 256 lanes x 4 diff elements
KEY_TRIP = 1 << 20       # k_key_hist / k_key_resid: key_grid() = 256 workgroups x 256 lanes x units of 16 bytes, per key frame
KEYGRAY_TRIP = 3 << 20   # k_key_gray: 256 workgroups x 256 lanes x units of 48 bytes, per key frame
NBINS = 2111


@pytest.fixture(scope="module")
def ctx():
    from tezip_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _flat(a):
    """a shared, read-only reference array as a 1-d host tensor (a copy: torch wraps only what it may write)"""
    import torch
    return torch.from_numpy(a.reshape(-1).copy())


# ====================================================================================== 1. the stand-alone seams
# ---------------------------------------------------------------------------------- k_lattice<false>, k_lattice<true>
LAT_SHAPE = (28, 251, 251)        # fe = 189 003 = 3 (mod 8): groups of 8 straddle the frame ends; frames 23 .. 27 start behind 2^22
LAT_SKIP = 25                     # the skipped frame, a quantised neighbour on each side
LAT_NARROW, LAT_WIDE, LAT_CONST = 24, 26, 27          # rel: ranges 40 (tolerance 0.8: the identity), 160 (3.2) and a constant slab (0)
LAT_EXTREMES = (23, 24, 26, 27)                       # +-255 in the first and last element
LAT_BOUNDS = [(2.0, 7.5, 1.0, 63.5, 3.5)[f % 5] for f in range(22)] + [3.0, 0.0, 300.0, 9.0, 0.5, 2.5]
LAT_CASES = {"abs": ("abs", [2.5]), "rel": ("rel", [0.02]), "absrel": ("absrel", [3.0, 0.05]), "pwrel": ("pwrel", [0.05]),
             "frames": ("abs", [0.0])}


def lattice_skip():
    skip = np.zeros(LAT_SHAPE[0], np.uint8)
    skip[LAT_SKIP] = 1
    return skip


@functools.lru_cache(maxsize=None)
def lattice_stacks():
    """orig (uint8), diff (int16) of LAT_SHAPE x 3; read-only"""
    nf, h, w = LAT_SHAPE
    rng = np.random.default_rng(2201)
    diff = rng.integers(-255, 256, (nf, h, w, 3), dtype=np.int16)
    orig = rng.integers(0, 256, diff.shape, dtype=np.uint8)
    orig[LAT_NARROW] = np.clip(orig[LAT_NARROW], 100, 140)
    orig[LAT_WIDE] = np.clip(orig[LAT_WIDE], 0, 160)
    orig[LAT_CONST, :, :, 1] = 77
    for f in LAT_EXTREMES:
        diff[f, 0, 0, 0], diff[f, -1, -1, 2] = (-255, 255) if f % 2 else (255, -255)
    orig.setflags(write=False)
    diff.setflags(write=False)
    return orig, diff


@functools.lru_cache(maxsize=None)
def lattice_want(case):
    from tezip_amd import lattice
    orig, diff = lattice_stacks()
    mode, value = LAT_CASES[case]
    want = lattice.quantise_stack(orig, diff, mode, value, lattice_skip(), bounds=LAT_BOUNDS if case == "frames" else None)
    want.setflags(write=False)
    return want


@pytest.mark.parametrize("case", sorted(LAT_CASES))
def test_lattice_seam_past_one_grid(ctx, case):
    import torch
    orig, diff = lattice_stacks()
    want = lattice_want(case)
    mode, value = LAT_CASES[case]
    skip = lattice_skip()

    def run(o, d):
        if case == "frames":
            ctx.lattice_bound_frames(o, d, LAT_BOUNDS, skip)
        else:
            ctx.lattice_bound(o, d, mode, value, skip)

    got = diff.copy()
    run(orig, got)
    np.testing.assert_array_equal(got, want, err_msg="host, %s" % case)
    _, to = TL._on_device(orig.copy(), 1, torch.uint8)
    whole, td = TL._on_device(diff.copy(), 1, torch.int16)
    torch.cuda.synchronize()
    run(to, td)
    ctx.synchronize()
    np.testing.assert_array_equal(td.cpu().numpy(), want, err_msg="device, one element behind the allocation, %s" % case)
    assert not whole[:1].any().item() and not whole[1 + diff.size:].any().item()


# ---------------------------------------------------------------------------------------------- k_sdelta_gray<HIST>
SDG_NPIX = ONE_TRIP + 8 * 3 + 5       # three whole groups and five single pixels behind the first trip
SDG_CARRY = -77


@functools.lru_cache(maxsize=None)
def sdelta_gray_stack():
    """(SDG_NPIX, 3) int16 in [-255, 255]; channels 1 and 2 hold other values, which must not matter"""
    rng = np.random.default_rng(2202)
    d3 = rng.integers(-255, 256, (SDG_NPIX, 3), dtype=np.int16)
    d3[0, 0], d3[-1, 0] = 255, -255
    d3.setflags(write=False)
    return d3


@functools.lru_cache(maxsize=None)
def sdelta_gray_want(carry, offset):
    from oracle import coracle
    from tezip_amd import graypayload
    y, counts = TG._want_sdelta(graypayload, sdelta_gray_stack(), carry, offset)
    np.testing.assert_array_equal(coracle.histogram(y, NBINS).astype(np.uint64), counts)
    return y, counts


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("carry", [None, SDG_CARRY], ids=["start", "carry"])
def test_spatial_delta_gray_past_one_grid(ctx, carry, offset):
    import torch
    d3 = sdelta_gray_stack()
    want, counts = sdelta_gray_want(carry, offset)
    n1, n3 = SDG_NPIX, SDG_NPIX * 3
    src = torch.zeros(n3 + 16, dtype=torch.int16, device="cuda")
    src[1: 1 + n3].copy_(_flat(d3))
    for hist_on in (False, True):
        what = "carry %r offset %d histogram %s" % (carry, offset, hist_on)
        hist = np.full(NBINS, 3, np.uint64) if hist_on else None            # the counts are ADDED
        got = ctx.spatial_delta_gray(d3, offset, carry=carry, hist=hist)
        np.testing.assert_array_equal(got, want, err_msg="host, " + what)
        if hist_on:
            np.testing.assert_array_equal(hist - np.uint64(3), counts, err_msg="host histogram, " + what)
        out = torch.full((n1 + 16,), 0x5A5A, dtype=torch.int16, device="cuda")
        dhist = torch.zeros(NBINS, dtype=torch.int64, device="cuda") if hist_on else None
        torch.cuda.synchronize()
        ctx.spatial_delta_gray(src[1: 1 + n3], offset, carry=carry, hist=dhist, out=out[1: 1 + n1])
        ctx.synchronize()
        o = out.cpu().numpy()
        np.testing.assert_array_equal(o[1: 1 + n1], want, err_msg="device, " + what)
        assert o[0] == 0x5A5A and (o[1 + n1:] == 0x5A5A).all(), "guard elements written, " + what
        if hist_on:
            np.testing.assert_array_equal(dhist.cpu().numpy().astype(np.uint64), counts, err_msg="device histogram, " + what)


# ------------------------------------------------------------------------------ k_recon_gray_flat, k_recon_gray
RECON_CASES = {   # frames, H, W, key frames
    "flat": (67, 256, 256, (0, 65)),        # unpadded, 65 536 pixels a frame: frame 64 starts AT pixel 2^22, 65 is a key frame, 66 predicted
    "general": (36, 251, 253, (0, 34)),     # inside 256 x 256, 63 503 pixels a frame: frames 34 (a key frame) and 35 start behind 2^21
}


def recon_trip(name):
    return ONE_TRIP if name == "flat" else RECON_TRIP


@functools.lru_cache(maxsize=None)
def recon_case(name):
    """pred (f32, padded), key (uint8), key mask, d (int16, one per pixel) and what they reconstruct to"""
    from tezip_amd import graypayload
    nf, h, w, keys = RECON_CASES[name]
    rng = np.random.default_rng(2203 + nf)
    pred = rng.random((nf, TG.pad8(h), TG.pad8(w), 3), dtype=np.float32)
    pred.reshape(-1)[rng.integers(0, pred.size, 64)] = 1.0
    key = rng.integers(0, 256, (nf, h, w, 3), dtype=np.uint8)          # channels 1 and 2 of the key stack are never read
    d = rng.integers(-255, 256, (nf, h, w), dtype=np.int16)
    d.reshape(-1)[::7] = 300                                             # below 0 whatever the base
    d.reshape(-1)[3::11] = -300                                          # above 255 whatever the base
    mask = [int(f in keys) for f in range(nf)]
    want = TG._want_recon(graypayload, pred, key, mask, d)
    for a in (pred, key, d, want):
        a.setflags(write=False)
    return pred, key, mask, d, want


@pytest.mark.parametrize("name", sorted(RECON_CASES))
def test_reconstruct_gray_past_one_grid(ctx, name):
    """host arrays are staged on aligned buffers: the flat form where the frames are unpadded.  One element behind the
    allocation no buffer is aligned: the general form, there past its own cap in both shapes."""
    import torch
    pred, key, mask, d, want = recon_case(name)
    nf, h, w = d.shape
    n1, n3 = d.size, d.size * 3
    got = ctx.reconstruct_gray(pred, key, mask, d)
    np.testing.assert_array_equal(got, want, err_msg="host")
    for s in (0, 1):
        t_pred = torch.zeros(pred.size + 16, dtype=torch.float32, device="cuda")
        t_pred[s: s + pred.size].copy_(_flat(pred))
        t_key = torch.zeros(n3 + 16, dtype=torch.uint8, device="cuda")
        t_key[s: s + n3].copy_(_flat(key))
        t_d = torch.zeros(n1 + 16, dtype=torch.int16, device="cuda")
        t_d[s: s + n1].copy_(_flat(d))
        out = torch.full((n3 + 64,), 0x5A, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ctx.reconstruct_gray(t_pred[s: s + pred.size], t_key[s: s + n3], mask, t_d[s: s + n1].view(nf, h, w), out=out[s: s + n3])
        ctx.synchronize()
        o = out.cpu().numpy()
        np.testing.assert_array_equal(o[s: s + n3], want.reshape(-1), err_msg="device, shift %d" % s)
        assert (o[:s] == 0x5A).all() and (o[s + n3:] == 0x5A).all(), "guard bytes written at shift %d" % s


# ---------------------------------------------------------------------------------------------- k_bound_err<V, GR>
BE_CASE = (27, 251 * 251 * 3, (25,))     # 5 103 081 elements = 2492 tiles: two tiles a workgroup; frame 25 (all zero) starts and ends behind
#                                          2^22, in second tiles (f * 189 003 mod 4096 = 2387, 2974), and frame 26 follows it
BE_OFFSETS = ((0, 0, 0), (1, 1, 1), (1, 2, 2))   # aligned; a head of 7 elements in front of the vectors; no common alignment: V = false


@functools.lru_cache(maxsize=None)
def bound_err_stacks(channels):
    from tezip_amd import target
    nframes, fe, zero = BE_CASE
    orig, d, q = TT._stacks(nframes, fe, seed=2204, zero_frames=zero)
    if channels == 1:
        orig = np.repeat(orig[:, 0::3], 3, axis=1)                       # three equal channels
    want = target.errors_of(orig, d, q, channels=channels)
    for a in (orig, d, q, want):
        a.setflags(write=False)
    return orig, d, q, want


@pytest.mark.parametrize("channels", [3, 1])
def test_bound_err_past_one_grid(ctx, channels):
    import torch
    nframes, fe, zero = BE_CASE
    orig, d, q, want = bound_err_stacks(channels)
    n = nframes * fe
    try:
        ctx.set_payload_channels(channels)
        np.testing.assert_array_equal(TT._records(ctx.bound_err(orig, d, q, nframes, fe)), want, err_msg="host")
        for off_o, off_d, off_q in BE_OFFSETS:
            to = torch.zeros(n + 16, dtype=torch.uint8, device="cuda")
            td = torch.zeros(n + 16, dtype=torch.int16, device="cuda")
            tq = torch.zeros(n + 16, dtype=torch.int16, device="cuda")
            to[off_o: off_o + n] = _flat(orig).cuda()
            td[off_d: off_d + n] = _flat(d).cuda()
            tq[off_q: off_q + n] = _flat(q).cuda()
            torch.cuda.synchronize()
            got = ctx.bound_err(to[off_o: off_o + n], td[off_d: off_d + n], tq[off_q: off_q + n], nframes, fe)
            np.testing.assert_array_equal(TT._records(got), want, err_msg="offsets %r" % ((off_o, off_d, off_q),))
    finally:
        ctx.set_payload_channels(3)


# ------------------------------------------------------------------------------------- k_key_hist, k_key_resid
KEY_SHAPE = (2, 592, 592)                # 1 051 392 bytes a frame: the smallest square past 2^20
KEY_PREDS = [[p, p] for p in range(4)] + [[3, 0], [1, 2]]


@functools.lru_cache(maxsize=None)
def key_stack():
    stack = TK._stack(*KEY_SHAPE, seed=2205)
    stack.setflags(write=False)
    return stack


def test_key_residuals_and_counts_past_one_grid(ctx):
    import torch
    from tezip_amd import keycoder
    stack = key_stack()
    k, h, w = KEY_SHAPE
    n = stack.size
    dev = torch.zeros(n + 16, dtype=torch.uint8, device="cuda")
    dev[1: 1 + n].copy_(_flat(stack))
    resid = {(j, p): keycoder.residual(stack[j], p) for j in range(k) for p in range(4)}
    for preds in KEY_PREDS:
        want = np.concatenate([resid[j, p] for j, p in enumerate(preds)])
        got = ctx.keys_residual_buf(stack, preds)
        assert got.dtype == np.int16
        np.testing.assert_array_equal(got, want, err_msg="host, residuals %r" % (preds,))
        sym = torch.zeros(n + 16, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        ctx.keys_residual_buf(dev[1: 1 + n].view(k, h, w, 3), preds, out=sym[1: 1 + n])
        torch.cuda.synchronize()
        res = sym.cpu().numpy()
        np.testing.assert_array_equal(res[1: 1 + n], want, err_msg="device, residuals %r" % (preds,))
        assert res[0] == 0 and not res[1 + n:].any()
    ctx.frames_begin(k, h, w)
    ctx.frames_put(0, stack)
    want_counts = keycoder.predictor_counts(stack)
    for idx in ([0, 1], [1]):
        counts = ctx.keys_counts(idx)
        np.testing.assert_array_equal(counts, want_counts[idx], err_msg="k_key_hist against numpy, frames %r" % (idx,))
        assert (counts.reshape(len(idx), 4, 256).sum(axis=2) == h * w * 3).all()


# ------------------------------------------------------------------------------------------------------ k_key_gray
KEYGRAY_SHAPE = (3, 1032, 1024)          # 3 170 304 bytes a frame, 3 145 728 of them on the first trip
KEYGRAY_PIXEL = (1031, 517, 1)           # frame 1: one sample of the last row, which starts at byte 3 167 232


@functools.lru_cache(maxsize=None)
def keygray_stack():
    """frame 0 gray, frame 1 gray (the test changes one sample of it), frame 2 coloured"""
    k, h, w = KEYGRAY_SHAPE
    stack = TKG.gray_stack(k, h, w, 2206)
    stack[2] = TKG.colour_stack(1, h, w, 2207)[0]
    stack.setflags(write=False)
    return stack


def test_gray_flags_past_one_grid(ctx):
    from tezip_amd import keycoderg
    stack = keygray_stack()
    k, h, w = KEYGRAY_SHAPE
    ctx.frames_begin(k, h, w)
    ctx.frames_put(0, stack)
    assert keycoderg.gray_flags(stack).tolist() == [True, True, False]
    assert ctx.keys_gray([0, 1, 2]).tolist() == [True, True, False]
    one = stack[1:2].copy()
    y, x, c = KEYGRAY_PIXEL
    one[0, y, x, c] ^= 0x80
    ctx.frames_put(1, one)
    assert keycoderg.gray_flags(one).tolist() == [False]
    assert ctx.keys_gray([0, 1, 2]).tolist() == [True, False, False]
    assert ctx.keys_gray([1]).tolist() == [False] and ctx.keys_gray([0]).tolist() == [True]


# ================================================================================================ 2. the whole jobs
def _colour_frames():
    from tezip_amd import synth
    return synth.translating_scene(24, 256, 256)          # fe = 196 608: frame 21 crosses symbol 2^22, frames 22 and 23 start behind it


def _gray_frames():
    from tezip_amd import synth
    return synth.moving_blobs(18, 512, 512)               # 262 144 symbols a frame: frame 16 starts AT the boundary, 17 behind it


JOBS = {"colour": (_colour_frames, 1, 3), "gray": (_gray_frames, 1, 3)}       # frames, warm_up, window: key frames 0, 1, 4, 7, ..
JOB_SHAPES = {"colour": (24, 256, 256), "gray": (18, 512, 512)}
LAYOUTS = {"colour_flat": ("colour", 3, 0), "colour_channel": ("colour", 3, 1), "gray_gray": ("gray", 1, 0)}   # job, payload channels, delta stride
GREEDY_LAYOUTS = ["colour_channel", "gray_gray"]      # (the flat greedy job past its caps is tests/test_gpu_configs.py's and test_gpu_fullsize.py's)
BOUND_CASES = {"abs2": ("abs", [2.0], False), "rel": ("rel", [0.02], False), "pwrel": ("pwrel", [0.05], False), "frames": ("abs", [99.0], True)}


def job_keys(name):
    """the key mask the rollout must give (compress.py:183-268: the warm-up frames, then every window-th frame)"""
    nt = JOB_SHAPES[name][0]
    _, p, window = JOBS[name]
    return [f < p or (f - p) % window == 0 for f in range(nt)]


def job_bounds(name):
    """one abs bound per frame; the late predicted frames (20, 21, 23 resp. 14, 15, 17) differ from one another"""
    nt = JOB_SHAPES[name][0]
    key = job_keys(name)
    b = [9.0 if key[f] else (2.0, 7.5, 3.5, 63.5, 1.0, 5.0)[f % 6] for f in range(nt)]
    b[2], b[3] = 0.0, 0.3
    return b


class _Job:
    def __init__(self, name):
        from tezip_amd import _lib, frametarget
        make, self.p, self.window = JOBS[name]
        self.name = name
        self.frames = make()
        self.nt, self.h, self.w = self.frames.shape[:3]
        assert (self.nt, self.h, self.w) == JOB_SHAPES[name]
        self.enc = _lib.Context(0)
        self.dec = None
        self.key = TT._rollout(self.enc, self.frames, self.p, self.window)
        assert self.key.tolist() == job_keys(name)
        if name == "colour":
            TT._nontrivial(self.enc, self.frames, self.key)
        self.skip = np.array(frametarget.fixed_frames(self.key, self.p), np.uint8)
        self.delta = self.enc.encode_delta("abs", [0.0]).copy()          # the job's deltas, unquantised
        self.pred = self.enc.get_predictions().copy()
        self.bounds = job_bounds(name)
        self.memo = {}
        for a in (self.frames, self.delta, self.pred):
            a.setflags(write=False)

    def late(self, channels):
        """the predicted frames with symbols behind the trip boundary"""
        fsym = self.h * self.w * channels
        return [f for f in range(self.nt) if not self.skip[f] and (f + 1) * fsym > ONE_TRIP]

    def quantised(self, quant, case):
        """the slow statement of the quantiser over the job's delta stack"""
        if (quant, case) not in self.memo:
            from oracle import coracle
            from tezip_amd import lattice
            mode, value, per_frame = BOUND_CASES[case]
            if quant == "lattice":
                q = lattice.quantise_stack(self.frames, self.delta, mode, value, self.skip, bounds=self.bounds if per_frame else None)
            else:
                q = self.delta.copy()
                for f in range(self.nt):
                    if not self.skip[f]:
                        q[f] = coracle.error_bound_frame(self.frames[f], self.delta[f], mode, [self.bounds[f]] if per_frame else value)
            q.setflags(write=False)
            self.memo[quant, case] = q
        return self.memo[quant, case]

    def decoded(self, q, channels):
        """what a decoder makes of the quantised stack: clip(trunc(pred * 255) - q, 0, 255), the key frames kept"""
        from tezip_amd import graypayload
        if "base" not in self.memo:
            self.memo["base"] = (self.pred[:, :self.h, :self.w] * np.float32(255.0)).astype(np.int64)   # trunc(f32(pred * 255)), as k_recon
        base = self.memo["base"]
        if channels == 1:
            out = graypayload.reconstruct(base[..., 0], q[..., 0])
        else:
            out = np.clip(base - q.astype(np.int64), 0, 255).astype(np.uint8)
        out[self.key] = self.frames[self.key]
        return out

    def decoder(self, channels):
        from tezip_amd import _lib
        if self.dec is None:
            cfg, wts = TT._model()
            self.dec = _lib.Context(0)
            self.dec.load_model(cfg, wts)
            self.dec.prepare(_lib.pad8(self.h), _lib.pad8(self.w), max_batch=4)
            self.dec.set_payload_channels(channels)
            key_stack = np.where(self.key[:, None, None, None], self.frames, 0).astype(np.uint8)
            assert self.dec.rollout_decode(key_stack, self.p).tolist() == self.key.tolist()
        return self.dec

    def close(self):
        self.enc.close()
        if self.dec is not None:
            self.dec.close()


@pytest.fixture(scope="module")
def jobs():
    made = {}

    def get(name):
        if name not in made:
            made[name] = _Job(name)
        return made[name]
    yield get
    for j in made.values():
        j.close()


def _set(job, channels, stride, quant, bounds):
    job.enc.set_payload_channels(channels)
    job.enc.set_delta_stride(stride)
    job.enc.set_quantiser(quant)
    job.enc.set_frame_bounds(bounds)


def _bites_behind_the_boundary(job, q, channels, what):
    """the quantiser changes deltas behind the trip boundary in every predicted frame that reaches there, in the colour job
    two of them; a key frame lies behind the boundary, a predicted frame follows it, and no fixed frame changes"""
    fsym = job.h * job.w * channels
    late = job.late(channels)
    key_late = [f for f in range(job.nt) if job.key[f] and f * fsym >= ONE_TRIP]
    assert key_late and key_late[0] + 1 in late, (what, key_late, late)
    assert len(late) >= (2 if job.name == "colour" else 1), (what, late)
    dq, dd = (q if channels == 3 else q[..., 0]).reshape(-1), (job.delta if channels == 3 else job.delta[..., 0]).reshape(-1)
    for f in late:
        lo = max(f * fsym, ONE_TRIP)
        assert (dq[lo: (f + 1) * fsym] != dd[lo: (f + 1) * fsym]).any(), "%s changes nothing behind the boundary in frame %d" % (what, f)
    assert not any((q[f] != job.delta[f]).any() for f in range(job.nt) if job.skip[f])


@pytest.mark.parametrize("case", sorted(BOUND_CASES))
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_lattice_front_past_one_grid(jobs, layout, case):
    name, channels, stride = LAYOUTS[layout]
    job = jobs(name)
    ctx = job.enc
    mode, value, per_frame = BOUND_CASES[case]
    q = job.quantised("lattice", case)
    _bites_behind_the_boundary(job, q, channels, "lattice %s" % case)
    try:
        _set(job, channels, stride, 1, job.bounds if per_frame else None)
        for entropy in (True, False):
            what = "%s %s entropy %s" % (layout, case, entropy)
            want_p, want_t = TL._slow_payload(q, channels, stride, entropy)
            (payload, table, _), n = TL._launches(ctx, lambda: ctx.encode(mode, value, entropy))
            np.testing.assert_array_equal(np.asarray(payload).reshape(-1), want_p, err_msg=what)
            if entropy:
                np.testing.assert_array_equal(table, want_t, err_msg=what)
            else:
                assert table is None
            assert (n["delta"], n["spatial_delta_hist"], n["quant_serial_chains"]) == (1, 0, 0), (what, n)     # the fused front
            if channels == 3:     # the delta tap is the quantised stack, and the payload beside it the same payload
                p2, t2, tap = ctx.encode(mode, value, entropy, want_delta=True)
                np.testing.assert_array_equal(tap, q, err_msg=what)
                np.testing.assert_array_equal(np.asarray(p2).reshape(-1), want_p, err_msg=what)
    finally:
        TL._reset(ctx)


@pytest.mark.parametrize("case", sorted(BOUND_CASES))
@pytest.mark.parametrize("layout", GREEDY_LAYOUTS)
def test_greedy_quantiser_past_one_grid(jobs, layout, case):
    """tz_encode under the greedy quantiser has no fused pass in these layouts: k_delta_flat, the quantiser's chain with k_q_fill
    (a wave per chunk of 64 pixels on at most 1024 workgroups: three trips in the colour job, nine in the gray one), then
    k_sdelta_s3 resp. k_sdelta_gray over the whole job"""
    name, channels, stride = LAYOUTS[layout]
    job = jobs(name)
    ctx = job.enc
    mode, value, per_frame = BOUND_CASES[case]
    q = job.quantised("greedy", case)
    _bites_behind_the_boundary(job, q, channels, "greedy %s" % case)
    try:
        _set(job, channels, stride, 0, job.bounds if per_frame else None)
        for entropy in (True, False):
            what = "%s %s entropy %s" % (layout, case, entropy)
            want_p, want_t = TL._slow_payload(q, channels, stride, entropy)
            payload, table, _ = ctx.encode(mode, value, entropy)
            np.testing.assert_array_equal(np.asarray(payload).reshape(-1), want_p, err_msg=what)
            if entropy:
                np.testing.assert_array_equal(table, want_t, err_msg=what)
            else:
                assert table is None
    finally:
        TL._reset(ctx)


DECODE_CASES = [(layout, "lattice") for layout in sorted(LAYOUTS)] + [(layout, "greedy") for layout in GREEDY_LAYOUTS]


@pytest.mark.parametrize("layout,quant", DECODE_CASES)
def test_decode_past_one_grid(jobs, layout, quant):
    """every payload of the two tests above through tz_decode on a decoder's rollout"""
    name, channels, stride = LAYOUTS[layout]
    job = jobs(name)
    ctx = job.enc
    dec = job.decoder(channels)
    try:
        dec.set_delta_stride(stride)
        for case in sorted(BOUND_CASES):
            mode, value, per_frame = BOUND_CASES[case]
            _set(job, channels, stride, int(quant == "lattice"), job.bounds if per_frame else None)
            want = job.decoded(job.quantised(quant, case), channels)
            for entropy in (True, False):
                payload, table, _ = ctx.encode(mode, value, entropy)
                got = dec.decode(payload, table)
                np.testing.assert_array_equal(got, want, err_msg="%s %s %s entropy %s" % (layout, quant, case, entropy))
            err = np.abs(want.astype(np.int64) - job.frames).reshape(job.nt, -1).max(axis=1)
            assert err[job.late(channels)].min() > 0 and not err[job.skip != 0].any()
    finally:
        TL._reset(ctx)
        dec.set_delta_stride(0)


@pytest.mark.parametrize("layout,quant", [("gray_gray", "greedy"), ("gray_gray", "lattice"), ("colour_flat", "lattice"), ("colour_channel", "lattice")])
def test_probes_past_one_grid(jobs, layout, quant):
    name, channels, stride = LAYOUTS[layout]
    job = jobs(name)
    ctx = job.enc
    try:
        for case in sorted(BOUND_CASES):
            mode, value, per_frame = BOUND_CASES[case]
            _set(job, channels, stride, int(quant == "lattice"), job.bounds if per_frame else None)
            got = TT._records(ctx.bound_probe(mode, value))
            payload, table, _ = ctx.encode(mode, value, True)
            want = TT._records(ctx.encode_quality(payload, table))
            np.testing.assert_array_equal(got, want, err_msg="%s %s %s" % (layout, quant, case))
            assert want[job.late(channels), 0].min() > 0 and not want[job.skip != 0].any()
    finally:
        TL._reset(ctx)
