"""The case table of tests/test_gpu_seam_alignment.py, checked without a GPU: that the byte offsets cover what the table's
header claims -- mechanically, from TERMS --, and that what the GPU test expects is not vacuous: the data reach the edges
they are meant to reach, and two statements of every operation (the C oracle and the numpy one) agree on them."""
import numpy as np
import pytest

from oracle import coracle
from oracle import oracle as O

import test_gpu_seam_alignment as S

SEAMS = sorted(S.TERMS)


@pytest.mark.parametrize("seam", SEAMS)
def test_offsets_are_legal_and_cover_the_rules(seam):
    terms, cases = S.TERMS[seam], S.OFFSETS[seam]
    assert sorted(S.FRAME_SHAPES) == SEAMS and sorted(S.OFFSETS) == SEAMS
    assert len({S.label(c) for c in cases}) == len(cases), "a case twice"
    for off in cases:
        for buf, o in off.items():
            assert buf in terms and 0 < o < 16 and o % terms[buf][0] == 0, (seam, off)    # aligned to the element type
    assert {} in cases, "every buffer aligned"
    for buf, (elem, _) in terms.items():
        assert any(off.get(buf, 0) == 0 for off in cases) and any(off.get(buf, 0) for off in cases), (seam, buf)
        assert {buf: elem} in cases, "%s: %s alone off by one element" % (seam, buf)
    assert any(len(off) == len(terms) and len(set(off.values())) == len(terms) for off in cases), "all off by different amounts"


@pytest.mark.parametrize("seam", SEAMS)
def test_every_predicate_term_fails_alone_at_its_smallest_offset(seam):
    terms, cases = S.TERMS[seam], S.OFFSETS[seam]
    for buf, (elem, aligns) in terms.items():
        for a in aligns:
            narrower = [b for b in aligns if b < a]
            # the offsets at which this term fails and every narrower term of the same buffer holds
            failing = [o for o in range(elem, 16, elem) if o % a and all(o % b == 0 for b in narrower)]
            assert failing, (seam, buf, a)
            assert {buf: failing[0]} in cases, "%s: no case fails %s & %d alone at +%d" % (seam, buf, a - 1, failing[0])
            # ... and the vector forms behind the narrower terms are entered at every alignment up to this one
            p = elem
            while p < a:
                assert {buf: p} in cases, (seam, buf, a, p)
                p *= 2


def test_the_offsets_the_issue_names():
    for seam, off in (("error_bound", {"diff": 8}), ("error_bound", {"orig": 1}), ("error_bound", {"orig": 2}), ("error_bound", {"orig": 4}),
                      ("delta_encode", {"orig": 4}), ("reconstruct", {"out": 4}), ("delta_encode", {"out": 8}), ("reconstruct", {"diff": 8}),
                      ("delta_encode", {"pred": 4}), ("delta_encode", {"pred": 8}), ("delta_encode", {"pred": 12}),
                      ("reconstruct", {"out": 1}), ("reconstruct", {"out": 2}), ("reconstruct", {"out": 3})):
        assert off in S.OFFSETS[seam], (seam, off)


def test_shapes_are_the_smallest_of_every_kernel_form():
    for seam in ("delta_encode", "reconstruct", "window_sse"):
        hw = [(h, w) for _, h, w, _ in S.FRAME_SHAPES[seam]]
        assert hw == [(8, 8), (16, 24), (13, 11), (5, 7)]
        assert [(S.pad8(h), S.pad8(w)) for h, w in hw[2:]] == [(16, 16), (8, 8)]
    assert (3 * 5 * 7 * 3) % 4 != 0                                   # k_recon's tail group
    hw = [h * w for _, h, w, _ in S.FRAME_SHAPES["error_bound"]]
    assert hw[0] == 64 and hw[1] % 4 == 0 and hw[1] < 64 and hw[2] % 4 != 0 and hw[3] == 4608 and 4096 < hw[3] <= 2 * 4096
    for seam in ("delta_encode", "reconstruct", "error_bound"):
        masks = [m for _, _, _, m in S.FRAME_SHAPES[seam] if m is not None]
        assert masks and all(1 <= nf <= 3 and (m is None or len(m) == nf) for nf, _, _, m in S.FRAME_SHAPES[seam])
        assert any(0 in m and 1 in m for m in masks)
    assert all(0 in m and 1 in m for _, _, _, m in S.FRAME_SHAPES["reconstruct"])       # both key-mask values, every shape
    assert max(nf * h * w * 3 for shapes in S.FRAME_SHAPES.values() for nf, h, w, _ in shapes) == 3 * 72 * 64 * 3
    assert S.LUT_SIZES == [1, 7, 8, 9, 4095, 4097]
    assert [b for b in S.BOUNDS if b[0] == "abs"] == [("abs", [2.0]), ("abs", [0.3])]
    assert sorted(m for m, _ in S.MERGING_BOUNDS) == ["abs", "absrel", "pwrel", "rel"]


def _trunc255(p):
    return (np.asarray(p, np.float32) * np.float32(255.0)).astype(np.int64)          # compress.py:307: a float32 product


def test_edge_predictions_sit_one_ulp_on_either_side_of_an_integer():
    e = S.edge_predictions()
    assert e.dtype == np.float32 and e[0] == 0.0 and e[1] == 1.0 and _trunc255(e[:2]).tolist() == [0, 255]
    lo, p, hi = e[2:].reshape(-1, 3).T
    k = np.arange(1, 255)
    assert (np.nextafter(lo, np.float32(2)) == p).all() and (np.nextafter(p, np.float32(2)) == hi).all()
    # neighbouring floats, and the truncated product turns between them: k - 1 below k / 255, k above it
    assert (_trunc255(lo) == k - 1).all() and (_trunc255(hi) == k).all() and np.isin(_trunc255(p) - k, (-1, 0)).all()
    assert (np.abs(lo.astype(np.float64) * 255 - k) < 2e-5).all() and (np.abs(hi.astype(np.float64) * 255 - k) < 4e-5).all()


@pytest.mark.parametrize("nf,h,w,mask", S.FRAME_SHAPES["delta_encode"], ids=lambda v: str(v).replace(" ", ""))
def test_delta_data(nf, h, w, mask):
    pred, orig, zero, want = S.delta_data(nf, h, w, mask)
    crop = pred[:, :h, :w]
    edge = S.edge_predictions()
    assert (crop == 0.0).any() and (crop == 1.0).any() and np.isin(crop, edge[2:]).sum() >= min(edge.size, crop.size) - 2
    assert pred.shape == (nf, S.pad8(h), S.pad8(w), 3) and want.dtype == np.int16 and want.shape == orig.shape
    ref = O.delta_group(pred, orig, zero_first=False)
    for i in range(nf):
        if zero is not None and zero[i]:
            assert not want[i].any() and ref[i].any()
        else:
            np.testing.assert_array_equal(want[i], ref[i])
            assert want[i].any() and (want[i] != orig[i]).any()
    if zero is not None:
        assert zero.any() and not zero.all()


@pytest.mark.parametrize("nf,h,w,mask", S.FRAME_SHAPES["error_bound"], ids=lambda v: str(v).replace(" ", ""))
def test_bound_data(nf, h, w, mask):
    orig, diff = S.bound_data(nf, h, w)
    skip = None if mask is None else np.array(mask, np.uint8)
    assert diff.dtype == np.int16 and np.abs(diff).max() <= 255
    for mode, bound in S.BOUNDS:
        want = S.bound_expected(orig, diff, skip, mode, bound)
        assert want.dtype == np.int16 and want.shape == diff.shape
        for i in range(nf):
            if skip is not None and skip[i]:
                np.testing.assert_array_equal(want[i], diff[i])
                assert (coracle.error_bound_frame(orig[i], diff[i], mode, bound) != diff[i]).any() or (mode, bound) not in S.MERGING_BOUNDS
                continue
            for c in range(3):
                np.testing.assert_array_equal(want[i][..., c], O.error_bound(orig[i][..., c], diff[i][..., c], mode, bound),
                                              "%s %r frame %d channel %d" % (mode, bound, i, c))
            chains_in, chains_out = diff[i].reshape(-1, 3), want[i].reshape(-1, 3)
            if (mode, bound) in S.MERGING_BOUNDS:
                # a run took in neighbours that differed: the output is not the input, and has fewer value changes
                assert (chains_out != chains_in).any(), (mode, bound, i)
                assert (np.diff(chains_out, axis=0) != 0).sum() < (np.diff(chains_in, axis=0) != 0).sum()
            else:
                np.testing.assert_array_equal(chains_out, chains_in)       # E < 0.5 merges equal neighbours only
            if h * w > 4096 and (mode, bound) == ("abs", [2.0]):
                # a run crosses the boundary between the two tiles: one value on both sides of it, over deltas that differ
                crossing = (chains_out[4095] == chains_out[4096]) & (chains_in[4095] != chains_in[4096])
                assert crossing.any() or (chains_out[4090:4102] == chains_out[4095]).all(axis=0).any(), i


@pytest.mark.parametrize("nf,h,w,mask", S.FRAME_SHAPES["reconstruct"], ids=lambda v: str(v).replace(" ", ""))
def test_recon_data(nf, h, w, mask):
    pred, key, km, diff, want = S.recon_data(nf, h, w, mask)
    base = np.where(km[:, None, None, None] != 0, key.astype(np.int64), _trunc255(pred[:, :h, :w]))
    v = base - diff
    assert (v < 0).any() and (v > 255).any() and ((v > 0) & (v < 255)).any()              # clamps at 0 and at 255, and not always
    np.testing.assert_array_equal(want, O.reconstruct_int(base, diff))
    for i in range(nf):
        assert (want[i] != key[i]).any()
    assert (want == 0).any() and (want == 255).any()


@pytest.mark.parametrize("nf,h,w,mask", S.FRAME_SHAPES["window_sse"], ids=lambda v: str(v).replace(" ", ""))
def test_sse_data(nf, h, w, mask):
    orig, pred, want = S.sse_data(nf, h, w)
    hp, wp = S.pad8(h), S.pad8(w)
    for i in range(nf):
        x = np.zeros((hp, wp, 3))
        x[:h, :w] = orig[i].astype(np.float32) / np.float32(255)
        sq = (x - pred[i].astype(np.float64)) ** 2
        # two statements of compress.py:246 (the oracle's fixed summation order against numpy's): equal to rounding
        np.testing.assert_allclose(want[i], sq.sum(), rtol=1e-12)
        if (hp, wp) != (h, w):
            assert sq.sum() - sq[:h, :w].sum() > 1e-3 * sq.sum()       # the pad region of pred counts, against x = 0


@pytest.mark.parametrize("n", S.LUT_SIZES)
def test_lut_data(n):
    y, table, ranks, loose = S.lut_data(n)
    assert y.dtype == ranks.dtype == loose.dtype == np.int16 and y.size == n
    np.testing.assert_array_equal(coracle.lut_apply(y, S.enc_lut(table)), ranks)        # the C statement against the numpy one
    assert (ranks != y).all() and ranks.max() < len(table)
    dec = O.remap_dec(loose, table)
    np.testing.assert_array_equal(coracle.lut_apply(loose, O.unmap_lut(table).astype(np.int16)), dec)
    np.testing.assert_array_equal(O.remap_dec(ranks, table), y)
    if n >= 7:
        assert (dec != loose).any() and ((loose < 0) | (loose >= len(table))).any()     # mapped values and values that pass through
    planes = S.byte_planes(ranks)
    u = ranks.astype(np.int64) & 0xFFFF
    np.testing.assert_array_equal(planes, np.concatenate([u & 0xFF, u >> 8]).astype(np.uint8))
    assert planes.size == 2 * n
