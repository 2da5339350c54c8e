"""The C oracle on a crop of a frame (a plain module for the tests; pytest does not collect it).

One predictor step starts from the initial state and every operation in it is local with zero padding at the frame edge,
so the oracle run on a crop reproduces the whole frame's result bit for bit except near the crop's ARTIFICIAL edges (the
sides where the crop stops inside the frame).  That lets the tests check frames far larger than the oracle could run
whole (tests/test_gpu_frame_limit.py): the oracle's cost follows the crop, not the frame.

A crop is legal when
  * its origin is a multiple of 64, so the 2x2 pooling grids and the Winograd F(2x2, 3x3) output tiles of every level
    fall on the same lines as in the whole frame;
  * its height and width divide by 8 and by 2^(levels-1), as a prepared frame must;
  * on every side that is not artificial it runs to the real frame edge.

How far the artificial edges reach into the result (measured by tests/test_crop_oracle.py, the margins below hold it):
c0 up to 7 px, one step up to 31 px, a rollout of depth d (each prediction fed on the previous crop prediction) about
31 d px.
"""
import numpy as np

from oracle import coracle

ORIGIN = 64


def margin(depth):
    """Pixels trimmed from each artificial side: depth 0 = c0, depth d >= 1 = d steps of a rollout."""
    return 8 if depth == 0 else 32 * depth


class Crop:
    """Rows [y0, y1) and columns [x0, x1) of an (hp, wp) padded frame."""

    def __init__(self, hp, wp, y0, y1, x0, x1, levels):
        step = max(8, 1 << (levels - 1))
        assert y0 % ORIGIN == 0 and x0 % ORIGIN == 0, "crop origin (%d, %d) is not on the %d grid" % (y0, x0, ORIGIN)
        assert 0 <= y0 < y1 <= hp and 0 <= x0 < x1 <= wp, (y0, y1, x0, x1, hp, wp)
        assert (y1 - y0) % step == 0 and (x1 - x0) % step == 0, "crop %dx%d does not divide by %d" % (y1 - y0, x1 - x0, step)
        self.hp, self.wp, self.y0, self.y1, self.x0, self.x1, self.levels = hp, wp, y0, y1, x0, x1, levels

    @property
    def h(self):
        return self.y1 - self.y0

    @property
    def w(self):
        return self.x1 - self.x0

    def artificial(self):
        """(top, bottom, left, right): True where the crop stops inside the frame."""
        return self.y0 > 0, self.y1 < self.hp, self.x0 > 0, self.x1 < self.wp

    def cut(self, a):
        """The crop of a (..., hp, wp, C) array."""
        return a[..., self.y0:self.y1, self.x0:self.x1, :]

    def compared(self, m):
        """(rows, cols) slices, in crop coordinates, of what stays after trimming m pixels from the artificial sides."""
        t, b, l, r = self.artificial()
        rows = slice(m if t else 0, self.h - m if b else self.h)
        cols = slice(m if l else 0, self.w - m if r else self.w)
        assert rows.start < rows.stop and cols.start < cols.stop, "margin %d leaves nothing of a %dx%d crop" % (m, self.h, self.w)
        return rows, cols

    def __repr__(self):
        return "crop rows [%d, %d) cols [%d, %d) of %dx%d" % (self.y0, self.y1, self.x0, self.x1, self.hp, self.wp)


def plan(hp, wp, levels, rows, cols, m):
    """The smallest legal crop of an (hp, wp) frame that holds rows [rows[0], rows[1]) x cols [cols[0], cols[1]) after m
    pixels are trimmed from its artificial sides."""
    step = max(8, 1 << (levels - 1))

    def axis(a, b, n):
        lo = max(0, a - m) // ORIGIN * ORIGIN
        hi = b + m
        if hi >= n:
            return lo, n
        hi = lo + -(-(hi - lo) // step) * step
        return (lo, hi) if hi < n else (lo, n)

    y0, y1 = axis(rows[0], rows[1], hp)
    x0, x1 = axis(cols[0], cols[1], wp)
    return Crop(hp, wp, y0, y1, x0, x1, levels)


def corner(hp, wp, levels, which, size, m):
    """A crop that holds the size x size corner 'tl' or 'br' of the frame after trimming m."""
    if which == "tl":
        return plan(hp, wp, levels, (0, min(size, hp)), (0, min(size, wp)), m)
    return plan(hp, wp, levels, (max(0, hp - size), hp), (max(0, wp - size), wp), m)


class CropOracle:
    """coracle.CPredNet for one model and contract on the crop's size."""

    def __init__(self, cfg, weights, crop, contract):
        self.crop = crop
        self.net = coracle.CPredNet(weights, cfg.stack_sizes, cfg.R_stack_sizes, crop.h, crop.w).set_contract(contract)

    def c0(self):
        return self.net.c0()

    def next(self, frame_full):
        """One step on the crop of a whole (hp, wp, 3) float32 frame."""
        return self.net.next(np.ascontiguousarray(self.crop.cut(frame_full)))

    def rollout(self, frame_full, depth):
        """Predictions of depth 1..depth from one whole frame, each fed on the previous crop prediction."""
        out, cur = [], np.ascontiguousarray(self.crop.cut(frame_full))
        for _ in range(depth):
            cur = self.net.next(cur)
            out.append(cur)
        return out


def assert_matches(got_full, ref_crop, crop, m, what=""):
    """got_full: an (hp, wp, C) array of the whole frame (or the crop itself); ref_crop: the oracle's result on the crop.
    Bit equality outside m pixels of the artificial sides."""
    got = crop.cut(got_full) if got_full.shape[:2] == (crop.hp, crop.wp) else got_full
    assert got.shape == ref_crop.shape, (got.shape, ref_crop.shape)
    rows, cols = crop.compared(m)
    g, r = got[rows, cols], ref_crop[rows, cols]
    if not np.array_equal(g, r):
        bad = np.argwhere(g != r)
        y, x = bad[0][:2]
        raise AssertionError("%s: %d values differ on %r (margin %d); first at frame pixel (%d, %d): %r vs %r" % (
            what, len(bad), crop, m, crop.y0 + rows.start + y, crop.x0 + cols.start + x, g[y, x], r[y, x]))


def reach(full, ref_crop, crop):
    """How far, in pixels from the nearest artificial side, the crop result differs from the whole frame's: 0 = nowhere."""
    d = np.any(crop.cut(full) != ref_crop, axis=-1)
    ys, xs = np.nonzero(d)
    if len(ys) == 0:
        return 0
    t, b, l, r = crop.artificial()
    big = np.full(len(ys), 1 << 30)
    dist = np.minimum.reduce([ys if t else big, crop.h - 1 - ys if b else big, xs if l else big,
                              crop.w - 1 - xs if r else big])
    assert (dist < (1 << 30)).all(), "the crop differs from the whole frame with no artificial side: %r" % crop
    return int(dist.max()) + 1
