"""The closed loop under one abs bound per pixel (`tezip.py -c --loop closed --quant lattice -m abs --loop-map FILE`;
tz_rollout_closed_map; NOT a reference feature), definition TZ-CLM1 -- the slow statement of it in numpy, the specification the GPU
is tested against, the refusals and the stdout line.

M is an H x W uint8 map of the images' own size, read by boundmap.load: M[y, x] is the abs tolerance of all three channels of pixel
(y, x) in every frame the loop quantises.  TZ-CLM1 is TZ-CL1 (tezip_amd/closedloop.py) except for the quantiser of a non-key frame:

  key mask, groups, fixed frames (frame 0, warm-up, key frames: stored exactly), the feeding rule, x = trunc(f32(pred * 255)), the
  mark and the decoder: TZ-CL1's.
  quantiser     d = x - orig, q = Q_{M[p]}(d) with TZ-QL1 (tezip_amd/lattice.py): E = M[p], s = 2E + 1,
                q = clamp(sign(d) * ((|d| + E) div s) * s, -255, 255); E = 0 is the identity.  dec[t] = clamp(x - q, 0, 255) is fed
                to step t + 1.
  selection     with --pred select it is TZ-PS1 (tezip_amd/predselect.py) with that Q: cost_c = sum |Q_{M[p]}(x_c - orig)| over
                the tile, mode 1 iff cost_prev < cost_net (a tie goes to the network), x = m ? dec[t-1] : x_net, chosen tiles
                patched into the prediction stack as predselect.pv; pred_modes.dat is TZP1, unchanged.  --pred motion is refused.

What follows, each point held by tests/test_closedmap.py:

  the bound     |dec - orig| <= M[p] at every sample of every frame: with k = (|d| + E) div s, |d| - E <= k * s <= |d| + E, so
                |q - d| <= E before the clamp; the clamp to +-255 only acts where |d| <= 255 < k * s, where it moves q towards d;
                and x - q lies within E of orig, which is inside 0..255, so the clamp of dec cannot move it away from orig.
  exact pixels  M[p] = 0: q = d, dec = orig.
  uniform map   M = k everywhere is closedloop.encode under abs k with the lattice quantiser, byte for byte (the same formula at
                every sample); likewise predselect.encode with selection.  M = 0 everywhere is the lossless closed job.
  the back half q is a pure function of (final pred, orig, M): boundmap.quantise(x_hat(final pred) - orig, M, skip, "lattice") on
                the open loop's deltas (group firsts zeroed) gives the loop's q again, so the unchanged tz_encode under
                tz_set_bound_map forms the stream.  Under selection the final predictions are the patched ones.
  the decoder   never sees a bound: closedloop.decode / predselect.decode decode the stream to the loop's dec, unchanged.

The kernels divide by the per-pixel s with one float reciprocal shared by the pixel's three channels; div_shortcut states that
formula and tests/test_closedmap.py holds it to integer division at every (numerator, E) the quantiser can meet.

This module is pure numpy; the predictor is passed in, as for closedloop.encode."""
import numpy as np

from . import boundmap, closedloop, lattice, predselect

DEFINITION = "TZ-CLM1"
FLAG = "--loop-map"


def check_flags(loop_map, loop, quant, mode, bound, pred=None, compressing=True, sweep=False, sharded=False, gray=False, threshold=None,
                target_psnr=None, target_ratio=None, per_frame=False, frame_bounds=None, bound_map=None, loop_psnr=None, loop_bounds=None):
    """The refusals of --loop-map that tezip.py and a direct caller of compress.run share: None, or the message.  loop_map is only
    asked whether it is there (load() reads it).  Without the flag nothing is refused here."""
    if loop_map is None:
        return None
    if not compressing:
        return "%s is valid with -c (--compress) only (-u decodes such a job without a flag)" % FLAG
    if loop != "closed":
        return "%s sets the bounds of a closed loop: add --loop closed" % FLAG
    if quant != "lattice":
        return "%s needs a quantiser that is a function of one sample: add --quant lattice" % FLAG
    if pred == "motion":
        return "%s cannot be combined with --pred motion (motion-compensated tiles under a map are out of scope: use --pred select)" % FLAG
    for on, other, why in ((bound_map is not None, "--bound-map", "that is the open loop's map; %s gives the closed loop's" % FLAG),
                           (loop_psnr is not None, "--loop-psnr", "a job takes one bound per frame or one per pixel"),
                           (loop_bounds is not None, "--loop-bounds", "a job takes one bound per frame or one per pixel"),
                           (target_psnr is not None, "--target-psnr", "a target needs a rollout per candidate"),
                           (target_ratio is not None, "--target-ratio", "a target needs a rollout per candidate"),
                           (per_frame, "--per-frame", "that is the open loop's search"),
                           (frame_bounds is not None, "--frame-bounds", "a job takes one bound per frame or one per pixel"),
                           (gray, "--gray", "the loop decodes three channels"),
                           (threshold is not None, "-t", "the closed loop runs fixed windows: use -w"),
                           (sweep, "--sweep", "run the job you want with -w")):
        if on:
            return "%s cannot be combined with %s (%s)" % (FLAG, other, why)
    if sharded:
        return "%s is not available for a sharded job (WORLD_SIZE > 1): run it on one GPU" % FLAG
    if bound:
        return "%s takes the place of -b" % FLAG
    if mode != "abs":
        return "%s gives abs bounds: it goes with -m abs and takes the place of -b" % FLAG
    return None


def load(spec, H=None, W=None):
    """--loop-map FILE / LOOP_MAP: what boundmap.load accepts, or a 2-D uint8 array.  A ValueError names the file and the rule."""
    if isinstance(spec, (str, bytes)) or hasattr(spec, "__fspath__"):
        return boundmap.load(spec, H, W)
    m = np.ascontiguousarray(spec)
    if m.dtype != np.uint8 or m.ndim != 2 or m.size == 0:
        raise ValueError("bound map LOOP_MAP is a %s array of shape %s: a map is a 2-D uint8 array, one abs tolerance 0..255 per pixel"
                         % (m.dtype, tuple(m.shape)))
    problem = check_size(m, H, W, "LOOP_MAP")
    if problem:
        raise ValueError(problem)
    return m


def check_size(m, H, W, spec="LOOP_MAP"):
    return boundmap.check_size(m, H, W, spec if isinstance(spec, str) else "LOOP_MAP")


def stdout_line(m):
    return "loop map: %dx%d, abs %d..%d, %.1f %% of pixels exact (%s)" % (m.shape[0], m.shape[1], int(m.min()), int(m.max()),
                                                                          100.0 * float((m == 0).sum()) / m.size, DEFINITION)


# ---------------------------------------------------------------------------------------------------- the slow statement
def _map(M, h, w):
    M = np.asarray(M)
    if M.dtype != np.uint8 or M.shape != (h, w):
        raise ValueError("the map must be a %d x %d uint8 array, got %s%r" % (h, w, M.dtype, M.shape))
    return M.astype(np.float64)[..., None]


def quantise(d, M):
    """Q of TZ-CLM1 on the (H, W, 3) deltas of one frame: TZ-QL1 with E = M[pixel] -> int64."""
    d = np.asarray(d)
    return lattice.quantise_e(d, _map(M, d.shape[0], d.shape[1]))


def choose(x_net, x_prev, orig, M):
    """The modes (TH, TW) uint8 of one frame under the map: 1 iff cost_prev < cost_net."""
    cost_net = predselect.tile_sums(np.abs(quantise(x_net - orig, M)))
    cost_prev = predselect.tile_sums(np.abs(quantise(x_prev - orig, M)))
    return (cost_prev < cost_net).astype(np.uint8)


def encode(frames, p, w, M, predictor, select=False):
    """The encoder's loop.  frames, p, w, predictor as closedloop.encode; M the H x W uint8 map.  Returns dict(key, pred, q int16,
    dec uint8) as closedloop.encode; with select also patched and modes as predselect.encode (pred: the NETWORK's predictions)."""
    frames = np.asarray(frames, np.uint8)
    nt, h, wd, _ = frames.shape
    _map(M, h, wd)
    hp, wp = closedloop.pad8(h), closedloop.pad8(wd)
    key, gfirst = closedloop.key_mask(nt, p, w), closedloop.group_first(nt, p, w)
    c0 = np.asarray(predictor.c0(hp, wp), np.float32)
    pred = np.empty((nt, hp, wp, 3), np.float32)
    q = np.zeros((nt, h, wd, 3), np.int64)
    dec = np.zeros_like(frames)
    modes = np.zeros((nt,) + predselect.tiles_of(h, wd), np.uint8)
    for t in range(nt):
        orig = frames[t].astype(np.int64)
        if key[t]:
            pred[t] = c0
            dec[t] = frames[t]
            q[t] = 0 if gfirst[t] else closedloop.x_hat(c0, h, wd) - orig   # (a warm-up frame 1..p-1: unquantised, decodes to the original)
            continue
        pred[t] = np.asarray(predictor.next(closedloop.u8_to_f32(dec[t - 1], hp, wp)), np.float32)
        x = closedloop.x_hat(pred[t], h, wd)
        if select:
            x_prev = dec[t - 1].astype(np.int64)
            modes[t] = choose(x, x_prev, orig, M)
            x = np.where(predselect.per_sample(modes[t], h, wd), x_prev, x)
        q[t] = quantise(x - orig, M)
        dec[t] = np.clip(x - q[t], 0, 255).astype(np.uint8)
    out = dict(key=key, pred=pred, q=q.astype(np.int16), dec=dec)
    if select:
        patched = pred.copy()
        for t in np.nonzero(~key)[0]:
            patched[t] = predselect.patch(pred[t], dec[t - 1], modes[t])
        out.update(patched=patched, modes=modes)
    return out


def open_loop_q(pred, frames, p, w, M):
    """What the OPEN-loop formulas under the map (delta, zeroed group firsts, boundmap.quantise with the lattice on every frame that
    is not skipped) give on a prediction stack -- on the loop's final predictions this is encode()'s q."""
    frames = np.asarray(frames, np.uint8)
    nt, h, wd, _ = frames.shape
    gfirst = closedloop.group_first(nt, p, w)
    skip = gfirst.copy()
    skip[:p] = True
    d = np.zeros((nt, h, wd, 3), np.int64)
    for t in range(nt):
        if not gfirst[t]:
            d[t] = closedloop.x_hat(pred[t], h, wd) - frames[t].astype(np.int64)
    return boundmap.quantise(d, np.asarray(M, np.uint8), skip, "lattice")


# ---------------------------------------------------------------------------------------------------- the kernels' division
def div_shortcut(n, E, ulp=0):
    """(n + E) div (2E + 1) as the kernels form it, n = |d|: one float32 reciprocal r of s = 2E + 1 per pixel, shared by its three
    channels, then trunc((f32(n + E) + 0.5f) * r) per sample.  n + E + 0.5 is at least 0.5 away from every multiple of s, a relative
    margin of 0.5 / 765 = 6.5e-4 against the 2.4e-7 of two roundings, so any reciprocal within one ulp serves: `ulp` in (-1, 0, 1)
    moves r that far from the correctly rounded 1 / s, which covers the hardware's approximate reciprocal."""
    n, E = np.asarray(n, np.int64), np.asarray(E, np.int64)
    r = np.float32(1.0) / (2 * E + 1).astype(np.float32)
    if ulp:
        r = np.nextafter(r, np.float32(np.inf if ulp > 0 else -np.inf), dtype=np.float32)
    return (((n + E).astype(np.float32) + np.float32(0.5)) * r).astype(np.int64)
