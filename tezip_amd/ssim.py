"""Structural similarity of two frame stacks (`tezip.py -c --report --ssim`; not in the reference).

PSNR says how large the error of a lossy job is, not where it sits: a run of small errors along an edge and the same error
spread as noise have the same PSNR.  SSIM compares the frames window by window -- mean, variance and covariance -- and is
the second figure a lossy-compression evaluation quotes.  The per-frame records come from the library (k_ssim in
csrc/tz_codec.hip: tz_ssim_frames, tz_encode_ssim); this module is the slow numpy statement of the same definition, the
statement the kernel is tested against, and turns records into the figures a user reads.  Pure numpy: no GPU is needed.

The definition, TZ-SSIM-1.  For two uint8 frames a, b of shape (H, W, 3), each channel on its own:

    windows   8 x 8 pixels at every origin (y, x) with y % 4 == 0, x % 4 == 0, y + 8 <= H, x + 8 <= W: per channel
              ((H-8)//4 + 1) * ((W-8)//4 + 1) windows when H, W >= 8, else none; a frame has three times as many.  Up to 3
              rows at the bottom and 3 columns at the right edge (H % 4, W % 4) lie in no window and are NOT compared.
    moments   exact integers over the window's 64 samples: s1 = sum a, s2 = sum b, sa = sum a^2, sb = sum b^2, s12 = sum ab
    factors   the usual SSIM with C1 = (0.01 * 255)^2, C2 = (0.03 * 255)^2 and the population variance, multiplied through
              by 64^2 and by 100 so that every constant is an integer (int64; all four below 2^53 in magnitude; d1, d2 > 0):
                  n1 = 200 * s1 * s2 + 2663424                       d1 = 100 * (s1^2 + s2^2) + 2663424
                  n2 = 200 * (64 * s12 - s1 * s2) + 23970816         d2 = 100 * (64 * (sa + sb) - s1^2 - s2^2) + 23970816
    value     in float64 and in exactly this order: p = double(n1) * double(n2), q = double(d1) * double(d2), r = p / q,
              Q = llrint(r * 4294967296.0), round half to even.  There is no other floating-point operation, and all four
              are correctly rounded IEEE operations, so Q is one integer everywhere.
    record    per frame (tz_frame_ssim, 24 bytes): int64 sum_q32 = sum of Q over the frame's windows, int64 min_q32 = the
              smallest Q (0 when there is no window), uint32 windows, uint32 reserved = 0.  Sum and minimum of integers
              do not depend on how a GPU cuts the frame, so the record is a function of the two frames.
    figures   frame SSIM = sum_q32 / (windows * 2^32); the frame's worst window = min_q32 / 2^32; the sequence's SSIM =
              (sum of the sums) / (sum of the windows * 2^32) -- not a mean of frame values, as with PSNR --; None (JSON
              null) where windows == 0.

`python -m tezip_amd.ssim DIR_A DIR_B` compares two image directories on the CPU (the way to check the images a `-u` wrote
against the sources): images are paired by sorted file name, a single-channel image is widened to RGB; one line per frame,
then `SSIM:` and `SSIM_min:` for the sequence; exit status 2 when the counts or sizes differ."""
import glob
import os
import sys

import numpy as np

SSIM_DTYPE = np.dtype([("sum_q32", "<i8"), ("min_q32", "<i8"), ("windows", "<u4"), ("reserved", "<u4")])   # tz_frame_ssim
WIN, STEP = 8, 4
K1, K2 = 2663424, 23970816        # 100 * 64^2 * (0.01 * 255)^2 and 100 * 64^2 * (0.03 * 255)^2
ONE = 1 << 32


def window_grid(H, W):
    """(rows, columns) of window origins of one channel of an H x W frame."""
    if H < WIN or W < WIN:
        return 0, 0
    return (H - WIN) // STEP + 1, (W - WIN) // STEP + 1


def window_count(H, W):
    """Windows of one H x W x 3 frame (three channels)."""
    ny, nx = window_grid(H, W)
    return 3 * ny * nx


def _window_sums(x, ny, nx):
    """x: (H, W, 3) int64 -> (ny, nx, 3): the sum of x over every window, through 4 x 4 cell sums."""
    cells = x[: (ny + 1) * STEP, : (nx + 1) * STEP].reshape(ny + 1, STEP, nx + 1, STEP, 3).sum(axis=(1, 3))
    return cells[:-1, :-1] + cells[:-1, 1:] + cells[1:, :-1] + cells[1:, 1:]


def window_q(a, b):
    """Q of every window of two (H, W, 3) uint8 frames: int64 (rows, columns, 3); the frames must have windows."""
    ny, nx = window_grid(a.shape[0], a.shape[1])
    a = a.astype(np.int64)
    b = b.astype(np.int64)
    s1, s2 = _window_sums(a, ny, nx), _window_sums(b, ny, nx)
    sa, sb, s12 = _window_sums(a * a, ny, nx), _window_sums(b * b, ny, nx), _window_sums(a * b, ny, nx)
    n1 = 200 * s1 * s2 + K1
    n2 = 200 * (64 * s12 - s1 * s2) + K2
    d1 = 100 * (s1 * s1 + s2 * s2) + K1
    d2 = 100 * (64 * (sa + sb) - s1 * s1 - s2 * s2) + K2
    p = n1.astype(np.float64) * n2.astype(np.float64)
    q = d1.astype(np.float64) * d2.astype(np.float64)
    r = p / q
    return np.rint(r * 2.0 ** 32).astype(np.int64)


def frame_records(a, b):
    """The tz_frame_ssim records of two uint8 stacks (nt, H, W, 3) (or two frames (H, W, 3)): SSIM_DTYPE[nt]."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != np.uint8 or b.dtype != np.uint8:
        raise TypeError("frames are uint8, got %s and %s" % (a.dtype, b.dtype))
    if a.ndim == 3:
        a, b = a[None], b[None]
    if a.shape != b.shape or a.ndim != 4 or a.shape[3] != 3:
        raise ValueError("two stacks of one shape (nt, H, W, 3), got %r and %r" % (a.shape, b.shape))
    out = np.zeros(len(a), SSIM_DTYPE)
    n = window_count(a.shape[1], a.shape[2])
    out["windows"] = n
    if n:
        for f in range(len(a)):
            q = window_q(a[f], b[f])
            out["sum_q32"][f] = q.sum(dtype=np.int64)
            out["min_q32"][f] = q.min()
    return out


def _fields(records):
    r = np.asarray(records)
    if r.dtype.names:
        return r["sum_q32"].astype(np.int64), r["min_q32"].astype(np.int64), r["windows"].astype(np.int64)
    r = np.asarray(r, np.int64)
    if r.ndim != 2 or r.shape[1] < 3:
        raise ValueError("ssim records must be SSIM_DTYPE or (nt, 3) (sum_q32, min_q32, windows), got shape %r" % (r.shape,))
    return r[:, 0], r[:, 1], r[:, 2]


def figures(records):
    """{"ssim", "ssim_min": the sequence's figures, "per_frame": [{"ssim", "ssim_min"}]}; None where there is no window."""
    sums, mins, wins = _fields(records)
    per = [{"ssim": int(s) / (int(w) * ONE) if w else None, "ssim_min": int(m) / ONE if w else None}   # (int / int: correctly rounded)
           for s, m, w in zip(sums, mins, wins)]
    total = int(wins.sum())
    have = wins > 0
    return {"ssim": sum(int(s) for s in sums) / (total * ONE) if total else None,
            "ssim_min": int(mins[have].min()) / ONE if total else None,
            "per_frame": per}


def _text(v):
    return "n/a" if v is None else "%.6f" % v


def stdout_line(ssim, ssim_min):
    """The line -c --report --ssim prints behind the report's three."""
    return "SSIM: n/a" if ssim is None else "SSIM: %.6f (worst window %.6f)" % (ssim, ssim_min)


def read_images(data_dir):
    """(sorted file names, uint8 (nt, H, W, 3)) of an image directory; a single-channel image is widened to RGB.  Raises
    ValueError for an empty directory, a file that is no image or images of more than one size."""
    from PIL import Image
    paths = sorted(glob.glob(os.path.join(data_dir, "*")))
    if not paths:
        raise ValueError("%s is an empty or non-existent directory" % data_dir)
    frames = []
    for p in paths:
        try:
            with Image.open(p) as img:
                frames.append(np.asarray(img.convert("RGB")))
        except (OSError, ValueError) as e:
            raise ValueError("%s cannot be read as an image (%s)" % (p, e))
        if frames[-1].shape != frames[0].shape:
            raise ValueError("%s is %r, %s is %r" % (p, frames[-1].shape[:2], paths[0], frames[0].shape[:2]))
    return [os.path.basename(p) for p in paths], np.stack(frames)


def compare_dirs(dir_a, dir_b):
    """(names of dir_a, records) of the images of two directories paired by sorted file name."""
    names_a, a = read_images(dir_a)
    names_b, b = read_images(dir_b)
    if len(names_a) != len(names_b):
        raise ValueError("%s holds %d images, %s holds %d" % (dir_a, len(names_a), dir_b, len(names_b)))
    if a.shape != b.shape:
        raise ValueError("%s holds %d x %d images, %s %d x %d" % (dir_a, a.shape[1], a.shape[2], dir_b, b.shape[1], b.shape[2]))
    return names_a, frame_records(a, b)


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m tezip_amd.ssim", description="TZ-SSIM-1 of two image directories (no GPU)")
    ap.add_argument("dir_a", metavar="DIR_A")
    ap.add_argument("dir_b", metavar="DIR_B")
    arg = ap.parse_args(argv)
    try:
        names, rec = compare_dirs(arg.dir_a, arg.dir_b)
    except (OSError, ValueError) as e:
        print("ERROR:", e)
        return 2
    fig = figures(rec)
    for name, f in zip(names, fig["per_frame"]):
        print("%s: SSIM %s (worst window %s)" % (name, _text(f["ssim"]), _text(f["ssim_min"])))
    print("SSIM: %s" % _text(fig["ssim"]))
    print("SSIM_min: %s" % _text(fig["ssim_min"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
