"""One abs bound per pixel (`tezip.py -c -m abs --bound-map FILE`; NOT a reference feature), definition TZ-BM1 -- the slow
statement of it in numpy, the loader of the map, and the check of a restored directory without a GPU.

M is an H x W uint8 map of the source frames' own (unpadded) size: M[y, x] is the abs tolerance, an integer 0..255, of all three
channels of pixel (y, x) in every frame the encoder quantises.  Frame 0, warm-up and key frames are stored exactly, as ever.

  greedy   per quantised frame and channel the chain of H * W deltas in row-major order, E_i = (double)M[i], Du = d + E_i,
           Dl = d - E_i, and the walk of compress.py:55-67 unchanged, truncation of (u + l) / 2 toward zero included: the
           reference's pwrel walk with the tolerance vector replaced by M (error_bound(M, diff, "pwrel", (1.0,)), bit for bit).
  lattice  TZ-QL1 (tezip_amd/lattice.py) with e = M[p] per sample.

What follows: |q - d| <= M[p] at every sample (a run's value lies in [l, u], a subset of every member's [d_i - M_i, d_i + M_i];
the ends are integers, so truncation cannot leave the interval), hence |decoded - orig| <= M[p]; a pixel with M = 0 is restored
exactly; a map that is k everywhere gives byte for byte the job `-m abs -b k`; a map of zeros gives the lossless job.

`python -m tezip_amd.boundmap MAP IMAGE_DIR RESTORED_DIR` checks the images of RESTORED_DIR against those of IMAGE_DIR under
MAP: exit status 0, or 3 with one line per frame that breaks its map."""
import os
import sys

import numpy as np

from . import lattice

DEFINITION = "TZ-BM1"
QUANTS = lattice.QUANTS
EXIT_BROKEN = 3
HELD_LINE = "bound map: held in every frame"

NEEDS_COMPRESS = "--bound-map is valid with -c (--compress) only (-u decodes such a job without a flag)"
NO_SWEEP = "--bound-map cannot be combined with --sweep"
NOT_SHARDED = "--bound-map is not available for a sharded job (WORLD_SIZE > 1): run it on one GPU"
NEEDS_ABS = "--bound-map goes with -m abs and takes the place of -b, --frame-bounds, --target-psnr, --target-ratio and --per-frame"


def _image(path):
    """the decoder compress.load_images uses"""
    from PIL import Image, UnidentifiedImageError
    try:
        return np.array(Image.open(path))
    except (OSError, UnidentifiedImageError, ValueError) as e:
        raise ValueError("bound map %s cannot be read: %s" % (path, e))


def load(path, H=None, W=None):
    """The map of `path`: a .npy holding a 2-D uint8 array, or an image with one channel or three equal ones.  H, W (when given):
    the size it must have.  A ValueError names the file and the rule."""
    path = os.fspath(path)
    if path.lower().endswith(".npy"):
        try:
            m = np.load(path, allow_pickle=False)
        except (OSError, ValueError) as e:
            raise ValueError("bound map %s cannot be read: %s" % (path, e))
        if m.dtype != np.uint8 or m.ndim != 2:
            raise ValueError("bound map %s holds a %s array of shape %s: a map is a 2-D uint8 array, one abs tolerance 0..255 per pixel"
                             % (path, m.dtype, tuple(m.shape)))
    else:
        m = _image(path)
        if m.dtype != np.uint8:
            raise ValueError("bound map %s decodes to %s samples: a map holds 8-bit samples, one abs tolerance 0..255 per pixel" % (path, m.dtype))
        if m.ndim == 3 and m.shape[2] == 3 and (m[..., 0] == m[..., 1]).all() and (m[..., 0] == m[..., 2]).all():
            m = m[..., 0]
        if m.ndim != 2:
            raise ValueError("bound map %s has colour: a map is a single-channel image, or one whose three channels are equal everywhere" % path)
    m = np.ascontiguousarray(m, np.uint8)
    if m.size == 0:
        raise ValueError("bound map %s is empty" % path)
    problem = check_size(m, H, W, path)
    if problem:
        raise ValueError(problem)
    return m


def check_size(m, H, W, path="BOUND_MAP"):
    """None, or the message: a map has the images' own size"""
    if H is not None and W is not None and m.shape != (H, W):
        return "bound map %s is %d x %d for images of %d x %d: a map has the images' own size" % (path, m.shape[0], m.shape[1], H, W)
    return None


def check_flags(bound_map, mode, bound, target_psnr, target_ratio, per_frame, frame_bounds, sharded):
    """The refusals tezip.py and a direct caller of compress.run share: None, or the message."""
    if bound_map is None:
        return None
    if sharded:
        return NOT_SHARDED
    if mode != "abs" or bound or target_psnr is not None or target_ratio is not None or per_frame or frame_bounds is not None:
        return NEEDS_ABS
    return None


def stats(m):
    """what tezip_amd.json records"""
    return {"max": int(m.max()), "exact_pixels": int((m == 0).sum())}


def stdout_line(m):
    return "bound map: %dx%d, abs %d..%d, %.1f %% of pixels exact" % (m.shape[0], m.shape[1], int(m.min()), int(m.max()),
                                                                       100.0 * float((m == 0).sum()) / m.size)


def broken_line(i, name, n):
    return "ERROR: frame %d (%s) exceeds its bound map at %d samples" % (i, name, n)


def _greedy_chain(d, e):
    """compress.py:55-67 on one chain of integer deltas d with the float64 tolerances e -> int64"""
    du, dl = d.astype(np.float64) + e, d.astype(np.float64) - e
    out = d.astype(np.int64).copy()
    u, l, head = np.inf, -np.inf, 0
    for i in range(len(d)):
        if min(u, du[i]) - max(l, dl[i]) < 0.0:
            out[head:i] = int((u + l) / 2)   # int(): truncation toward zero, as the reference's int64 store
            u, l, head = np.inf, -np.inf, i
        if du[i] < u:
            u = du[i]
        if l < dl[i]:
            l = dl[i]
    if len(d):
        out[head:] = int((u + l) / 2)
    return out


def quantise(diff, M, skip=None, quant="greedy"):
    """The numpy statement of both quantisers under the map M (H x W uint8) on an (nt, H, W, C) integer delta stack; skip[f] != 0:
    frame f is left as it is.  Returns int16."""
    d = np.asarray(diff)
    M = np.asarray(M)
    if quant not in QUANTS:
        raise ValueError("unknown quantiser %r" % (quant,))
    if d.ndim != 4 or M.dtype != np.uint8 or M.shape != d.shape[1:3]:
        raise ValueError("diff must be an (nt, H, W, C) stack and M an H x W uint8 map, got %r and %s%r" % (d.shape, M.dtype, M.shape))
    out = d.astype(np.int16).copy()
    e = M.reshape(-1).astype(np.float64)
    for f in range(len(d)):
        if skip is not None and skip[f]:
            continue
        if quant == "lattice":
            out[f] = lattice.quantise_e(d[f], e.reshape(M.shape)[..., None])
            continue
        if not M.any():    # no tolerance anywhere: the reference returns its input (compress.py:24)
            continue
        for c in range(d.shape[3]):
            out[f, :, :, c] = _greedy_chain(d[f, :, :, c].reshape(-1).astype(np.int64), e).reshape(M.shape)
    return out


def check(orig, decoded, M):
    """Per frame of two (nt, H, W, 3) uint8 stacks: {"violations": samples with |decoded - orig| > M, "max_excess":
    max(|e| - M, 0)} -- what tz_map_check gives."""
    o, x, M = np.asarray(orig), np.asarray(decoded), np.asarray(M)
    if o.shape != x.shape or o.ndim != 4 or M.shape != o.shape[1:3]:
        raise ValueError("two (nt, H, W, C) stacks of one shape and an H x W map, got %r, %r and %r" % (o.shape, x.shape, M.shape))
    excess = np.abs(x.astype(np.int64) - o.astype(np.int64)) - M.astype(np.int64)[None, :, :, None]
    return [{"violations": int((excess[f] > 0).sum()), "max_excess": int(max(excess[f].max(), 0)) if excess[f].size else 0}
            for f in range(len(o))]


def _rgb(path):
    a = _image(path)
    if a.ndim == 2:
        a = np.repeat(a[..., None], 3, axis=-1)
    if a.ndim != 3 or a.shape[2] != 3 or a.dtype != np.uint8:
        raise ValueError("%s is not an 8-bit RGB or grayscale image" % path)
    return a


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    if len(argv) != 3:
        print(__doc__)
        return 2
    map_path, src, dst = argv
    names = sorted(os.listdir(src)) if os.path.isdir(src) else []
    if not names:
        print("ERROR:", src, "is an empty or non-existent directory")
        return 2
    try:
        first = _rgb(os.path.join(src, names[0]))
        M = load(map_path, first.shape[0], first.shape[1])
        broken = 0
        for i, name in enumerate(names):
            if not os.path.exists(os.path.join(dst, name)):
                print("ERROR: %s has no image %s" % (dst, name))
                return 2
            rec = check(_rgb(os.path.join(src, name))[None], _rgb(os.path.join(dst, name))[None], M)[0]
            if rec["violations"]:
                print(broken_line(i, name, rec["violations"]))
                broken += 1
    except ValueError as e:
        print("ERROR:", e)
        return 2
    if broken:
        return EXIT_BROKEN
    print(HELD_LINE)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
