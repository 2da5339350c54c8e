"""The shapes of tests/test_gpu_one_grid.py against the caps they are meant to cross, without a GPU.

The trip sizes of that file are derived from constants in tezip_amd/csrc/tz_codec.hip; this file reads the source as text and
asserts them, so that whoever changes a cap is told to move the shapes.  Then, by arithmetic, every shape of the GPU file
crosses its trip size under the conditions that make the second trip of a lane worth testing (frame starts behind the
boundary, ragged frame ends, the skipped / zero / key frame's position), and the slow statements alone, on the GPU file's own
seeded inputs, show that each case bites there."""
import os
import re

import numpy as np
import pytest

import test_gpu_one_grid as G
from conftest import ROOT

SOURCE = os.path.join(ROOT, "tezip_amd", "csrc", "tz_codec.hip")
MOVE = "a launch cap of tz_codec.hip changed: move the shapes of tests/test_gpu_one_grid.py past the new cap"


@pytest.fixture(scope="module")
def source():
    with open(SOURCE) as f:
        return f.read()


# ------------------------------------------------------------------------------------------------------ 0. the caps
def test_the_caps_are_the_ones_the_trip_sizes_come_from(source):
    for text in ("static constexpr int kBlocksPerCU = 8;", "static constexpr int kCUs = 256;",
                 "static constexpr int HB_THREADS = 1024, HB_GRID = 2 * kCUs;", "static constexpr int BE_TILE = 256 * 8;",
                 "size_t cap = (size_t)kCUs * kBlocksPerCU;"):
        assert source.count(text) == 1, (text, MOVE)
    key_grid = re.search(r"static dim3 key_grid\(size_t fe, int nkeys\) \{\s*return dim3\(\(unsigned\)std::min<size_t>\(\(fe / 16 \+ 2 \+ 255\) / 256, 256\), "
                         r"\(unsigned\)nkeys\);", source)
    assert key_grid, MOVE
    gray = re.search(r"hipLaunchKernelGGL\(k_key_gray, dim3\(\(unsigned\)std::min<size_t>\(\(fe / 48 \+ 2 \+ 255\) / 256, 256\), \(unsigned\)nkeys\), "
                     r"dim3\(256\)", source)
    assert gray, MOVE
    # the launches whose grids the trip sizes describe
    for text in ("k_lattice<true>, dim3(grid_for(items, 256)), dim3(256)", "k_lattice<false>, dim3(grid_for(items, 256)), dim3(256)",
                 "const dim3 grid(d_hist ? std::min(HB_GRID, grid_for(n8, HB_THREADS)) : grid_for(n8, 256)), block(d_hist ? HB_THREADS : 256);",
                 "gray ? k_recon_gray_flat : k_recon_flat, dim3(grid_for(n / 8, 256)), dim3(256)",
                 "k_recon_gray, dim3(grid_for(n / 4 + 1, 256)), dim3(256)",
                 "size_t G = std::min<size_t>((size_t)grid_for(tiles, 1), tiles);",
                 "k_key_hist, key_grid(fe, nkeys), dim3(256)", "k_key_resid, key_grid((size_t)H * W * 3, nkeys), dim3(256)"):
        assert text in source, (text, MOVE)
    cus, per_cu, hb_threads, hb_grid, be_tile = 256, 8, 1024, 2 * 256, 256 * 8
    assert G.ONE_TRIP == cus * per_cu * 256 * 8 == hb_grid * hb_threads * 8 == cus * per_cu * be_tile == 1 << 22
    assert G.RECON_TRIP == cus * per_cu * 256 * 4 == 1 << 21
    assert G.KEY_TRIP == 256 * 256 * 16 == 1 << 20
    assert G.KEYGRAY_TRIP == 256 * 256 * 48 == 3 << 20


# ------------------------------------------------------------------------------------------------ 1. the lattice seam
def test_lattice_seam_shape():
    nf, h, w = G.LAT_SHAPE
    fe = h * w * 3
    assert nf * fe > G.ONE_TRIP and fe % 8 != 0
    late = [f for f in range(nf) if f * fe >= G.ONE_TRIP + 8]          # (+ 8: whatever the head in front of the vector groups)
    assert len(late) >= 3 and late == list(range(late[0], nf))
    assert G.LAT_SKIP in late[1:-1], "the skipped frame has a quantised neighbour on each side, both behind the boundary"
    assert all(f in late for f in (G.LAT_NARROW, G.LAT_WIDE, G.LAT_CONST) + G.LAT_EXTREMES)
    # a group of 8 straddles a frame end on the second trip whether the stack is aligned (head 0) or one element off (head 7)
    for head in (0, 7):
        assert any((f * fe - head) % 8 for f in late)
    assert len(G.LAT_BOUNDS) == nf
    b = [G.LAT_BOUNDS[f] for f in late if f != G.LAT_SKIP]
    assert 0.0 in b and 0.5 in b and max(b) >= 255.0
    assert all(G.LAT_BOUNDS[f] != G.LAT_BOUNDS[f - 1] for f in late)


@pytest.mark.parametrize("case", sorted(G.LAT_CASES))
def test_lattice_seam_cases_bite_behind_the_boundary(case):
    from tezip_amd import lattice
    nf, h, w = G.LAT_SHAPE
    fe = h * w * 3
    orig, diff = G.lattice_stacks()
    want = G.lattice_want(case)
    assert want.dtype == np.int16 and want.shape == diff.shape
    changed = [f for f in range(nf) if (want[f] != diff[f]).any()]
    late = [f for f in changed if f * fe >= G.ONE_TRIP + 8]
    assert len(late) >= 2 and G.LAT_SKIP not in changed, (case, changed)
    for f in G.LAT_EXTREMES:
        assert abs(int(diff[f, 0, 0, 0])) == 255 and int(diff[f, 0, 0, 0]) == -int(diff[f, -1, -1, 2])
    mode, value = G.LAT_CASES[case]
    E = lambda f, c: int(lattice.step_radius(lattice.tolerance(orig[f, :, :, c], mode, value)))   # noqa: E731
    if case == "rel":      # the tolerances of the late frames differ from their predecessors'
        assert [E(f, 0) for f in (23, G.LAT_NARROW, G.LAT_WIDE, G.LAT_CONST)] == [5, 0, 3, 5] and E(G.LAT_CONST, 1) == 0
        assert not (want[G.LAT_NARROW] != diff[G.LAT_NARROW]).any() and not (want[G.LAT_CONST, :, :, 1] != diff[G.LAT_CONST, :, :, 1]).any()
    if case == "absrel":
        assert [E(f, 0) for f in (23, G.LAT_NARROW, G.LAT_WIDE)] == [3, 2, 3] and E(G.LAT_CONST, 1) == 0
    if case == "frames":
        for f in range(nf):
            assert (want[f] != diff[f]).any() == (G.LAT_BOUNDS[f] >= 1.0 and f != G.LAT_SKIP), f
        assert not np.delete(want, [f for f in range(nf) if G.LAT_BOUNDS[f] < 255.0 or f == G.LAT_SKIP], axis=0).any()   # bound >= 255: all 0
    if case == "abs":
        assert np.abs(want.astype(np.int64) - diff).max() == 2


# ------------------------------------------------------------------------------------------ the gray spatial delta
def test_spatial_delta_gray_shape_and_statement():
    assert G.SDG_NPIX > G.ONE_TRIP and (G.SDG_NPIX - G.ONE_TRIP) % 8 == 5 and (G.SDG_NPIX - G.ONE_TRIP) // 8 >= 1
    d3 = G.sdelta_gray_stack()
    assert d3.shape == (G.SDG_NPIX, 3) and (d3[:, 0] != d3[:, 1]).any()
    seen = set()
    for carry in (None, G.SDG_CARRY):
        for offset in (0, 1):
            y, counts = G.sdelta_gray_want(carry, offset)
            assert y.size == G.SDG_NPIX
            seen.add(y.tobytes())
            if offset:
                assert int(counts.sum()) == y.size
            # what only a second trip makes: the symbols behind the boundary are their own, not a repeat of the first trip's
            assert (y[G.ONE_TRIP: G.ONE_TRIP + 29] != y[:29]).any()
    assert len(seen) == 4


# ---------------------------------------------------------------------------------------------- the gray reconstruct
@pytest.mark.parametrize("name", sorted(G.RECON_CASES))
def test_reconstruct_gray_shapes_and_statement(name):
    nf, h, w, keys = G.RECON_CASES[name]
    trip = G.recon_trip(name)
    fpix = h * w
    assert nf * fpix > trip
    if name == "flat":      # unpadded, whole groups of 8: the flat form's conditions
        assert h % 8 == 0 and w % 8 == 0 and fpix % 8 == 0
    else:
        assert h % 2 == 1 and w % 2 == 1 and fpix % 4 != 0
    late_keys = [f for f in keys if f * fpix >= trip]
    assert late_keys and late_keys[0] + 1 < nf and late_keys[0] + 1 not in keys, "a key frame behind the boundary, a predicted frame behind it"
    # the same key frame lies behind the general form's cap, which the device run one element off the alignment takes
    assert late_keys[0] * fpix >= G.RECON_TRIP
    pred, key, mask, d, want = G.recon_case(name)
    assert want.shape == (nf, h, w, 3) and [f for f in range(nf) if mask[f]] == list(keys)
    for f in (late_keys[0], late_keys[0] + 1):                            # both clamps fire behind the boundary
        assert want[f].min() == 0 and want[f].max() == 255
    f = late_keys[0]
    assert (want[f, ..., 0].astype(np.int64) == np.clip(key[f, ..., 0].astype(np.int64) - d[f], 0, 255)).all()
    assert (want[f + 1, ..., 0].astype(np.int64) != np.clip(key[f + 1, ..., 0].astype(np.int64) - d[f + 1], 0, 255)).any()


# ---------------------------------------------------------------------------------------------------- k_bound_err
@pytest.mark.parametrize("channels", [3, 1])
def test_bound_err_shape_and_statement(channels):
    nframes, fe, zero = G.BE_CASE
    n = nframes * fe
    be_tile, cap = 2048, 2048
    assert n > G.ONE_TRIP and fe % be_tile != 0 and fe % 3 == 0
    assert all(f * fe >= G.ONE_TRIP and f + 1 < nframes for f in zero), "an all-zero frame behind the boundary, a frame behind it"
    for head in (0, 7):     # tzk_bound_err's grid: no workgroup takes one tile, and a frame end lies in a second tile
        tiles = (n - head + be_tile - 1) // be_tile
        assert tiles > cap
        per_block = (tiles + cap - 1) // cap * be_tile
        assert per_block == 2 * be_tile
        assert any((f * fe - head) % per_block >= be_tile for f in range(1, nframes))
        assert any((f * fe - head) % per_block >= be_tile for f in zero + tuple(f + 1 for f in zero))
    # the offsets of the device runs: vectors on aligned stacks, vectors behind a head, and no vectors
    kinds = []
    for off_o, off_d, off_q in G.BE_OFFSETS:
        h = (8 - off_o) & 7
        kinds.append((((2 * off_d + 2 * h) | (2 * off_q + 2 * h)) & 15 == 0, h))
    assert kinds == [(True, 0), (True, 7), (False, 7)]
    orig, d, q, want = G.bound_err_stacks(channels)
    r = orig.astype(np.int64) + d - q
    late = [f for f in range(nframes) if f * fe >= G.ONE_TRIP]
    assert (r[late] < 0).any() and (r[late] > 255).any()                 # both clamps fire
    assert all(tuple(want[f]) == (0, 0, 0) for f in zero) and all(want[f, 0] > 0 for f in range(nframes) if f not in zero)
    assert len({tuple(rec) for rec in want.tolist()}) == nframes - len(zero) + 1, "no two frames share a record"
    if channels == 1:
        from tezip_amd import graypayload, target
        assert graypayload.is_gray(orig.reshape(nframes, -1, 3)) and (want != target.errors_of(orig, d, q)).any()


# ------------------------------------------------------------------------------------------------- the key coders
def test_key_coder_shapes_and_statements():
    from tezip_amd import keycoder, keycoderg
    k, h, w = G.KEY_SHAPE
    fe = h * w * 3
    assert k == 2 and h == w and fe > G.KEY_TRIP + 16 and (h - 1) * (h - 1) * 3 <= G.KEY_TRIP, "the smallest square past the cap"
    assert sorted({p for preds in G.KEY_PREDS for p in preds}) == [0, 1, 2, 3] and all(len(p) == k for p in G.KEY_PREDS)
    stack = G.key_stack()
    counts = keycoder.predictor_counts(stack)
    for j in range(k):      # the bytes only a second trip reads have a distribution of their own: dropping them changes the counts
        tail = stack[j].reshape(-1)[G.KEY_TRIP + 16:]
        first = stack[j].reshape(-1)[:tail.size]
        assert (np.bincount(tail, minlength=256) != np.bincount(first, minlength=256)).any()
        assert (stack[j, :8] != stack[j, -8:]).any()
        assert int(counts[j, 0].sum()) == fe
    assert (counts[0] != counts[1]).any()
    k, h, w = G.KEYGRAY_SHAPE
    fe = h * w * 3
    y, x, c = G.KEYGRAY_PIXEL
    assert k == 3 and fe > G.KEYGRAY_TRIP + 48
    assert y == h - 1 and (y * w + x) * 3 + c >= G.KEYGRAY_TRIP + 48 + 16, "a sample only a second trip reads"
    stack = G.keygray_stack()
    assert keycoderg.gray_flags(stack).tolist() == [True, True, False]
    one = stack[1:2].copy()
    one[0, y, x, c] ^= 0x80
    assert keycoderg.gray_flags(one).tolist() == [False]
    # the coloured frame would still read as coloured from its first trip alone; the one-sample frame would not
    assert not keycoderg.gray_flags(stack[2:3, :64]).any() and keycoderg.gray_flags(one[:, :y]).all()


# ------------------------------------------------------------------------------------------------- the whole jobs
@pytest.mark.parametrize("layout", sorted(G.LAYOUTS))
def test_whole_job_shapes(layout):
    name, channels, stride = G.LAYOUTS[layout]
    nt, h, w = G.JOB_SHAPES[name]
    _, p, window = G.JOBS[name]
    fsym = h * w * channels
    assert nt * fsym > G.ONE_TRIP and h % 8 == 0 and w % 8 == 0 and fsym % 8 == 0, "the fused front applies"
    key = G.job_keys(name)
    fixed = [key[f] or f < max(1, p) for f in range(nt)]
    assert fixed == key
    late_keys = [f for f in range(nt) if key[f] and f * fsym >= G.ONE_TRIP]
    assert late_keys and late_keys[0] + 1 < nt and not key[late_keys[0] + 1], "a key frame behind the boundary, a predicted frame behind it"
    late = [f for f in range(nt) if not key[f] and (f + 1) * fsym > G.ONE_TRIP]
    if name == "colour":
        assert (late_keys, late) == ([22], [21, 23]) and 21 * fsym < G.ONE_TRIP < 22 * fsym
    else:
        assert (late_keys, late) == ([16], [17]) and 16 * fsym == G.ONE_TRIP, "frame 16 starts exactly at the boundary"
    b = G.job_bounds(name)
    assert len(b) == nt and 0.0 in b and any(0 < v < 1 for v in b)
    around = [max(f for f in range(late[0]) if not key[f])] + late       # the last predicted frame in front of the boundary and those behind it
    assert len({b[f] for f in around}) == len(around) >= 2 and all(b[f] >= 1.0 for f in around)
    assert sorted(G.BOUND_CASES) == ["abs2", "frames", "pwrel", "rel"]
    assert {(G.BOUND_CASES[c][0], tuple(G.BOUND_CASES[c][1])) for c in ("abs2", "rel", "pwrel")} == {("abs", (2.0,)), ("rel", (0.02,)), ("pwrel", (0.05,))}

