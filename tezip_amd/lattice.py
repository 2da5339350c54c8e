"""The lattice quantiser of a lossy job (`tezip.py -c --quant lattice`; NOT a reference feature), definition TZ-QL1 -- the slow
statement of it in numpy, integers throughout but for the float64 tolerance.

The reference's quantiser (compress.py:23-70) is a greedy walk that merges runs of neighbouring deltas which fit into one 2E
window.  TZ-QL1 is a uniform mid-tread quantiser with the same guarantee per sample and no neighbours: for a delta d and the
tolerance e >= 0 (a float64 formed exactly as the greedy quantiser forms it: abs |b0|; rel (max - min of the slab) * b0; absrel
the smaller of the two; pwrel orig * b0 per element; under per-frame bounds bounds[f])

    E = min(255, floor(e))          s = 2E + 1
    q = clamp( sign(d) * ((|d| + E) div s) * s , -255, 255 )

  * |q - d| <= E <= e for d in [-255, 255]: the lattice point is within E of d, and the clamp projects onto an interval that
    contains d, so it cannot increase the error;
  * |q| <= 255, so the spatial delta of the payload stays in [-510, 510];
  * e < 1 is the identity (s = 1); E = 255 maps every d in [-255, 255] to 0;
  * the payload carries q itself (a multiple of the step), not an index: the decoder never sees a bound, and `-u` decodes such a
    job as it decodes any other.
The formula is defined for every int16 d (the bound on the error holds inside [-255, 255], the encoder's domain).  Negative and
NaN tolerances are refused where the greedy quantiser refuses them.

`python -m tezip_amd.lattice STACK.npy [warm_up]` prints, for an (nt, H, W[, 3]) uint8 stack with the previous frame as the
stand-in predictor, the payload bytes of both quantisers at abs 2 and abs 6, flat and at the channel stride."""
import numpy as np

MODES = ("abs", "rel", "absrel", "pwrel")
QUANTS = ("greedy", "lattice")
DEFINITION = "TZ-QL1"
STDOUT_LINE = "quant: lattice (TZ-QL1)"


def tolerance(orig, mode, value):
    """The float64 tolerance of one (frame, channel) slab as compress.py:28-48 forms it: a scalar, or per element for pwrel."""
    if mode not in MODES:
        raise ValueError("unknown mode %r" % (mode,))
    b0 = float(value[0])
    if np.isnan(b0) or (mode == "absrel" and np.isnan(float(value[1]))):
        raise ValueError("error bound is NaN")
    if mode in ("rel", "pwrel") and b0 < 0:
        raise ValueError("%s bound must be >= 0" % mode)
    if mode == "absrel" and float(value[1]) < 0:
        raise ValueError("absrel bound must be >= 0")
    if mode == "abs":
        return abs(b0)
    bf = np.asarray(orig).astype(np.int64)
    if mode == "pwrel":
        with np.errstate(invalid="ignore"):
            return bf.astype(np.float64) * b0
    rng = float(bf.max() - bf.min()) if bf.size else 0.0
    if mode == "rel":
        return rng * b0
    a, r = abs(b0), rng * float(value[1])
    return a if a < r else r


def step_radius(e):
    """E = min(255, floor(e)) as int64 (scalar or array); e >= 0, +inf allowed; a NaN (0 * inf) counts as no tolerance."""
    e = np.nan_to_num(np.asarray(e, np.float64), nan=0.0, posinf=np.inf)
    return np.minimum(255.0, np.floor(e)).astype(np.int64)


def quantise_e(diff, e):
    """TZ-QL1 with the tolerance(s) e (a scalar, or an array that broadcasts against diff) -> int64 array like diff."""
    d = np.asarray(diff).astype(np.int64)
    E = step_radius(e)
    s = 2 * E + 1
    q = np.sign(d) * ((np.abs(d) + E) // s) * s
    return np.where(E == 0, d, np.clip(q, -255, 255))   # (E == 0 leaves every int16 d as it is, inside the domain or not)


def quantise(orig, diff, mode, value):
    """One (frame, channel) slab, in the shape of oracle.error_bound: orig / diff integer arrays of the same shape; returns an
    int64 array like diff."""
    return quantise_e(diff, tolerance(orig, mode, value))


def quantise_stack(orig, diff, mode, value, skip=None, bounds=None):
    """The whole (nt, H, W, 3) stack, per frame and channel as compress.py:316-319 walks it.  skip[f] != 0: frame f is left as
    it is.  bounds (one abs tolerance per frame, finite and >= 0): in place of (mode, value).  Returns int16."""
    o, d = np.asarray(orig), np.asarray(diff)
    if d.ndim != 4 or o.shape != d.shape:
        raise ValueError("orig and diff must be (nt, H, W, C) stacks of one shape, got %r and %r" % (o.shape, d.shape))
    if bounds is not None:
        b = np.asarray(bounds, np.float64)
        if b.shape != (len(d),) or not np.isfinite(b).all() or (b < 0).any():
            raise ValueError("bounds must be %d finite numbers >= 0" % len(d))
    out = d.astype(np.int16).copy()
    for f in range(len(d)):
        if skip is not None and skip[f]:
            continue
        for c in range(d.shape[3]):
            q = quantise_e(d[f, :, :, c], float(b[f])) if bounds is not None else quantise(o[f, :, :, c], d[f, :, :, c], mode, value)
            out[f, :, :, c] = q
    return out


def order0_bytes(symbols):
    """The order-0 cost of a symbol array in bytes (what an ideal memoryless coder spends), rounded up."""
    counts = np.bincount(np.asarray(symbols).reshape(-1).astype(np.int64) & 0xFFFF)
    counts = counts[counts > 0].astype(np.float64)
    n = counts.sum()
    return int(np.ceil(float(-(counts * np.log2(counts / n)).sum()) / 8.0))


def previous_frame_deltas(frames, warm_up=0):
    """The stand-in predictor of the measurements: frame t is predicted by frame t - 1; frames 0 .. warm_up are stored exactly
    (delta 0, never quantised).  -> (int16 delta stack, skip mask)."""
    f = np.asarray(frames)
    if f.ndim == 3:
        f = np.repeat(f[..., None], 3, axis=-1)
    d = np.zeros(f.shape, np.int16)
    d[1:] = f[:-1].astype(np.int16) - f[1:].astype(np.int16)
    skip = np.zeros(len(f), np.uint8)
    skip[:warm_up + 1] = 1
    d[skip != 0] = 0
    return f, d, skip


def greedy(orig, diff, mode, value):
    """The reference's quantiser (compress.py:23-70) on one slab, for the comparison this module prints: a run grows while the
    windows [d - e, d + e] of its elements share a point, and takes the truncated middle of what they share.  (The tests hold
    the table against the project's oracle instead.)"""
    d = np.asarray(diff).astype(np.int64)
    e = np.broadcast_to(np.asarray(tolerance(orig, mode, value), np.float64), d.shape).reshape(-1)
    if not (e != 0).any():
        return d
    flat, out = d.reshape(-1), d.reshape(-1).copy()
    hi, lo, head = np.inf, -np.inf, 0
    for i in range(flat.size):
        u, l = flat[i] + e[i], flat[i] - e[i]
        if min(hi, u) - max(lo, l) < 0.0:
            out[head:i] = int((hi + lo) / 2)
            hi, lo, head = np.inf, -np.inf, i
        hi, lo = min(hi, u), max(lo, l)
    if flat.size:
        out[head:] = int((hi + lo) / 2)
    return out.reshape(d.shape)


def greedy_stack(orig, diff, mode, value, skip, error_bound):
    """The reference's quantiser over the stack, per frame and channel (error_bound: `greedy` above or a twin of it)."""
    out = np.asarray(diff).astype(np.int16).copy()
    for f in range(len(out)):
        if skip[f]:
            continue
        for c in range(out.shape[3]):
            out[f, :, :, c] = error_bound(orig[f, :, :, c], diff[f, :, :, c], mode, value)
    return out


def table_rows(frames, error_bound, bounds=(2.0, 6.0), warm_up=0):
    """[(abs, quantiser, flat zstd-9, flat o0, channel zstd-9, channel o0, PSNR of the predicted frames)] for a uint8 stack:
    bytes of the predicted frames' payload, o0 = its order-0 cost."""
    from . import sdelta, zstd
    f, d, skip = previous_frame_deltas(frames, warm_up)
    rows = []
    for b in bounds:
        for name in QUANTS:
            q = (greedy_stack(f, d, "abs", [b], skip, error_bound) if name == "greedy" else quantise_stack(f, d, "abs", [b], skip))
            err = np.clip(f.astype(np.int64) + d - q, 0, 255) - f
            sse = float((err[skip == 0] ** 2).sum())
            psnr = float("inf") if sse == 0 else 10.0 * np.log10(err[skip == 0].size * 65025.0 / sse)
            cells = []
            for stride in (1, 3):   # the payload of the predicted frames (frames 0 .. warm_up are stored exactly in every job)
                y = sdelta.encode(q[warm_up + 1:], stride, True)
                cells += [len(zstd.compress(y.tobytes(), 9)), order0_bytes(y)]
            rows.append((b, name, cells[0], cells[1], cells[2], cells[3], psnr))
    return rows


def main(argv=None):
    import sys
    argv = sys.argv[1:] if argv is None else argv
    if not 1 <= len(argv) <= 2:
        print(__doc__)
        return 2
    print("| abs | quantiser | flat zstd-9 | flat o0 | channel zstd-9 | channel o0 | PSNR of predicted frames, dB |")
    print("|---|---|---|---|---|---|---|")
    for row in table_rows(np.load(argv[0]), greedy, warm_up=int(argv[1]) if len(argv) > 1 else 0):
        print("| %g | %s | %d | %d | %d | %d | %.2f |" % row)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
