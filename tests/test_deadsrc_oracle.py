"""The lemma behind k_wino's dead-source skip (tz_prednet.hip measure_dead / launch_wino), on the C
oracle's own statement of a TZ-PA2 convolution (oracle/tz_oracle.c conv3x3_wino through coracle.conv_probe(winograd=True)):

    every Winograd chain D[i][j] starts from the literal +0; the transform of an all-zero patch is +-0; fmaf(+-0, U, +0) = +0
    for every finite U.  So behind a LEADING run of all-zero channels every chain holds exactly the +0 it would have started
    from: the convolution over all channels and the convolution over the remaining channels, with the weights sliced
    accordingly, are the same bits.

Runs on the CPU.  Compared as uint32 bit patterns: a zero of the other sign is a difference.  The data go down to 1e-30, the
weights to 1e-12 (products that are subnormal or underflow), some weights are negative, some biases are -0.

Not claimed, and shown by the last test: dead channels in the MIDDLE of K.  A chain can sit at -0 behind an underflow, and
fmaf(+0, U, -0) = +0 flips it."""
import numpy as np
import pytest

from oracle import coracle

H, W, C, CU, COUT = 12, 12, 48, 16, 16


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _case(seed, prefix, zero, ups):
    """(x, xu, w, bias): `prefix` leading channels of x are `zero` (+0.0 or -0.0) at every pixel."""
    rng = np.random.default_rng(seed)
    # magnitudes from 1e-30 to 1: 10 ** uniform(-30, 0), relu-like data (non-negative), a quarter of the pixels exactly +0
    x = (10.0 ** rng.uniform(-30, 0, (H, W, C))).astype(np.float32)
    x[rng.random((H, W, C)) < 0.25] = 0.0
    x[:, :, :prefix] = zero
    xu = (10.0 ** rng.uniform(-30, 0, (H // 2, W // 2, CU))).astype(np.float32) if ups else None
    cin = C + (CU if ups else 0)
    w = ((10.0 ** rng.uniform(-12, 0, (3, 3, cin, COUT))) * rng.choice([-1.0, 1.0], (3, 3, cin, COUT))).astype(np.float32)
    bias = rng.normal(0, 0.1, COUT).astype(np.float32)
    bias[::3] = -0.0
    bias[1::6] = 0.0
    return x, xu, w, bias


@pytest.mark.parametrize("ups", [False, True], ids=["same", "same+up"])
@pytest.mark.parametrize("zero", [0.0, -0.0], ids=["+0", "-0"])
@pytest.mark.parametrize("prefix", [16, 32])
def test_a_zero_prefix_of_the_source_can_be_left_out(prefix, zero, ups):
    x, xu, w, bias = _case(1000 + prefix + int(ups), prefix, np.float32(zero), ups)
    assert (_bits(x[:, :, :prefix]) == _bits(np.float32(zero))).all()
    assert np.isfinite(w).all() and (np.signbit(bias) & (bias == 0)).any()
    assert (x[x > 0].min() < 1e-28) and (np.abs(w).min() < 1e-11) and (w < 0).any()
    full = coracle.conv_probe(x, xu, w, bias, winograd=True)
    part = coracle.conv_probe(x[:, :, prefix:], xu, w[:, :, prefix:], bias, winograd=True)
    assert np.isfinite(full).all()
    np.testing.assert_array_equal(_bits(full), _bits(part))
    # the case is not vacuous: the remaining channels matter, and some output is a zero whose sign could have flipped
    assert not np.array_equal(_bits(full), _bits(np.broadcast_to(bias, full.shape)))


def test_all_outputs_that_hang_on_signed_zeros_survive_a_prefix():
    """Everything so small that every product underflows: the chains hold +-0 only, the outputs are the -0 / +0 the biases
    and the chains' signs make of it.  A zero prefix still changes no bit."""
    rng = np.random.default_rng(5)
    x = np.full((H, W, C), 1e-30, np.float32) * rng.uniform(0.5, 2, (H, W, C)).astype(np.float32)
    x[:, :, :32] = 0.0
    w = (-1e-20 * rng.uniform(0.5, 2, (3, 3, C, COUT))).astype(np.float32)
    bias = np.full(COUT, -0.0, np.float32)
    full = coracle.conv_probe(x, None, w, bias, winograd=True)
    part = coracle.conv_probe(x[:, :, 32:], None, w[:, :, 32:], bias, winograd=True)
    assert (full == 0).all() and np.signbit(full).any()          # some outputs ARE -0: the chains behind them sit at -0
    np.testing.assert_array_equal(_bits(full), _bits(part))


def test_counter_case_dead_channels_in_the_middle_are_not_claimed():
    """The same underflowing data with the zero block in the MIDDLE of K (channels 16..31, live channels before it): chains
    that sit at -0 behind the first block become +0 when the zero block adds fmaf(+0, U, -0).  Leaving that block out is
    therefore NOT the same bits -- which is why the predictor skips a prefix only.  Only the numbers are asserted to agree;
    the count of differing bit patterns is printed."""
    rng = np.random.default_rng(5)
    x = np.full((H, W, C), 1e-30, np.float32) * rng.uniform(0.5, 2, (H, W, C)).astype(np.float32)
    x[:, :, 16:] = 0.0                                             # live block 0, then zeros to the end
    w = (-1e-20 * rng.uniform(0.5, 2, (3, 3, C, COUT))).astype(np.float32)
    bias = np.full(COUT, -0.0, np.float32)
    keep = np.r_[0:16, 32:48]
    full = coracle.conv_probe(x, None, w, bias, winograd=True)
    # (channels 16..47 are all zero; leaving out 16..31 -- a block in the middle -- or 16..47 -- everything behind block 0)
    mid = coracle.conv_probe(x[:, :, keep], None, w[:, :, keep], bias, winograd=True)
    only0 = coracle.conv_probe(x[:, :, :16], None, w[:, :, :16], bias, winograd=True)
    np.testing.assert_array_equal(full, mid)                       # equal as numbers (-0 == +0) ...
    np.testing.assert_array_equal(full, only0)
    print("bit patterns that differ: block in the middle left out %d, everything behind block 0 left out %d of %d"
          % (int((_bits(full) != _bits(mid)).sum()), int((_bits(full) != _bits(only0)).sum()), full.size))
