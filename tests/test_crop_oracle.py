"""The crop oracle (tests/crop_oracle.py) against the whole-frame C oracle, on the CPU: for every model that
tests/test_gpu_frame_limit.py runs at the frame-size limit and both arithmetic contracts, c0, one step and rollouts of
depth 1..3 on a crop equal the whole frame's bit for bit outside the margins the GPU tests trim, the measured reach of the
artificial edges stays inside those margins, and the comparison fails on a single 1-ulp change."""
import numpy as np
import pytest

import crop_oracle as CO
from oracle import coracle
from tezip_amd.prednet import PredNetConfig

MODELS = {
    "default": PredNetConfig(),
    "r_lt_s": PredNetConfig(stack_sizes=(3, 64, 64), R_stack_sizes=(3, 16, 16)),
    "two_level": PredNetConfig(stack_sizes=(3, 64)),
}
HP, WP, DEPTH = 320, 320, 3


@pytest.fixture(scope="module", params=sorted(MODELS))
def whole(request):
    """Both contracts' whole-frame c0 and depth-1..3 rollout of one random frame."""
    cfg = MODELS[request.param]
    wts = cfg.init_weights(seed=17, bias_scale=0.25)
    frame = np.random.default_rng(5).integers(0, 256, (HP, WP, 3)).astype(np.float32) / np.float32(255)
    out = {}
    for contract in (1, 2):
        net = coracle.CPredNet(wts, cfg.stack_sizes, cfg.R_stack_sizes, HP, WP).set_contract(contract)
        seq, cur = [], frame
        for _ in range(DEPTH):
            cur = net.next(cur)
            seq.append(cur)
        out[contract] = (net.c0(), seq)
    return request.param, cfg, wts, frame, out


def _crops(levels):
    """name: (crop, deepest rollout compared on it)"""
    return {"bottom_right": (CO.Crop(HP, WP, 128, HP, 64, WP, levels), DEPTH),      # artificial top and left
            "top_left": (CO.Crop(HP, WP, 0, 192, 0, 256, levels), DEPTH),           # artificial bottom and right
            "interior": (CO.Crop(HP, WP, 64, 256, 64, 256, levels), 2)}             # four artificial sides


@pytest.mark.parametrize("contract", [1, 2])
def test_crop_equals_the_whole_frame_outside_the_margin(whole, contract):
    name, cfg, wts, frame, out = whole
    c0, seq = out[contract]
    reaches = {}
    crops = _crops(cfg.nb_layers)
    for cname, (crop, depth) in crops.items():
        co = CO.CropOracle(cfg, wts, crop, contract)
        got = [co.c0()] + co.rollout(frame, depth)
        for d, (ref_full, g) in enumerate(zip([c0] + seq, got)):
            what = "%s PA%d %s depth %d" % (name, contract, cname, d)
            CO.assert_matches(ref_full, g, crop, CO.margin(d), what)
            reaches[(cname, d)] = r = CO.reach(ref_full, g, crop)
            assert r <= CO.margin(d), "%s: the artificial edges reach %d px, margin %d" % (what, r, CO.margin(d))
    # the edges do reach into the crop (else the margins would test nothing), and their reach grows with depth
    assert all(reaches[(c, 1)] > 0 for c in crops)
    assert all(reaches[(c, d)] <= reaches[(c, d + 1)] for c, (_, depth) in crops.items() for d in range(1, depth))


def test_plan_gives_legal_crops_that_hold_the_region():
    for levels in (1, 2, 3, 4):
        for hp, wp, rows, cols, m in [(4728, 4728, (4600, 4728), (4600, 4728), 64), (4728, 4728, (0, 128), (0, 128), 32),
                                      (8, 2796200, (0, 8), (2796000, 2796200), 32), (5792, 5792, (2880, 2912), (100, 300), 32)]:
            c = CO.plan(hp, wp, levels, rows, cols, m)
            r, k = c.compared(m)
            assert c.y0 + r.start <= rows[0] and rows[1] <= c.y0 + r.stop, (c, rows)
            assert c.x0 + k.start <= cols[0] and cols[1] <= c.x0 + k.stop, (c, cols)
            assert c.h * c.w <= (rows[1] - rows[0] + 2 * m + 64 + 8) * (cols[1] - cols[0] + 2 * m + 64 + 8)
    with pytest.raises(AssertionError):
        CO.Crop(256, 256, 32, 256, 0, 256, 3)      # origin off the 64 grid
    with pytest.raises(AssertionError):
        CO.Crop(256, 256, 64, 252, 0, 256, 3)      # height does not divide by 8


@pytest.mark.parametrize("contract", [1, 2])
def test_the_comparison_fails_on_one_ulp(whole, contract):
    """One output value nudged by 1 ulp anywhere in the compared region -- next to the trimmed margin, or at the real
    frame corner -- fails the comparison; the same nudge inside the margin does not."""
    name, cfg, wts, frame, out = whole
    crop = _crops(cfg.nb_layers)["bottom_right"][0]
    ref = CO.CropOracle(cfg, wts, crop, contract).rollout(frame, 1)[0]
    dev = out[contract][1][0]
    m = CO.margin(1)
    CO.assert_matches(dev, ref, crop, m)
    for (y, x, c), caught in [((crop.y0 + m, crop.x0 + m, 0), True), ((HP - 1, WP - 1, 2), True),
                              ((crop.y0 + m, WP - 1, 1), True), ((crop.y0 + m - 1, crop.x0 + 40, 0), False)]:
        bad = dev.copy()
        bad[y, x, c] = np.nextafter(bad[y, x, c], np.float32(2))
        if caught:
            with pytest.raises(AssertionError, match="1 values differ"):
                CO.assert_matches(bad, ref, crop, m, "%s PA%d" % (name, contract))
        else:
            CO.assert_matches(bad, ref, crop, m)
