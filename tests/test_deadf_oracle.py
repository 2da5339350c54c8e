"""The lemma behind k_wino's dead forget gate (tz_prednet.hip measure_deadf, tz_wino_kernels.hip.h EPI_LSTM3; DESIGN.md section
5), on the C oracle under contract 2 and in numpy float32:

    c = f * c_prev + i * g is a multiplication, a multiplication and an addition (oracle/tz_oracle.c lstm_level_c).  Where
    c_prev is +0, f * c_prev is +0 for every f in [0, 1] (a hard sigmoid is nothing else unless it is NaN), so c = (+0) + i * g
    whatever the forget gate's weights are.

Runs on the CPU.  Compared as uint32 bit patterns: a zero of the other sign is a difference."""
import numpy as np
import pytest

import deadf_models as D
from oracle import coracle

HP, WP = 24, 40


def _oracle(sp):
    cfg, w, frames = D.model(sp)
    net = coracle.CPredNet(w, cfg.stack_sizes, cfg.R_stack_sizes, sp[2], sp[3]).set_contract(2)
    out = {"pred0": net.next(frames[0])}
    out["pred"], dbg = net.next(frames[-1], debug=True)
    for l in range(cfg.nb_layers):
        out["e%d" % l], out["r%d" % l], out["c%d" % l] = dbg["e"][l], dbg["r"][l], dbg["c"][l]
    return cfg, out


@pytest.mark.parametrize("shape", [D.DEFAULT, D.M9], ids=["default", "3x80x128"])
def test_c0_is_plus_zero_in_every_word_exactly_for_zero_biases(shape):
    zero = D.c0_numpy(D.spec("zero", HP, WP, 1, shape=shape))
    for l, c in enumerate(zero):
        assert (D.bits(c) == 0).all(), l
    biased = D.c0_is_plus_zero(D.spec("bias", HP, WP, 1, shape=shape))
    assert biased and not any(biased.values()), biased


def test_the_forget_gate_reaches_no_result_where_c0_is_plus_zero():
    """Every forget-gate kernel and bias overwritten: predictions and every e / r tap (and c) of the oracle keep their bits."""
    cfg, ref = _oracle(D.spec("zero", HP, WP, 1))
    _, got = _oracle(D.spec("zero_f", HP, WP, 1))
    w0, w1 = D.model(D.spec("zero", HP, WP, 1))[1], D.model(D.spec("zero_f", HP, WP, 1))[1]
    names = [nm for nm, _ in cfg.weight_shapes()]
    differ = [nm for nm, a, b in zip(names, w0, w1) if not np.array_equal(a, b)]
    assert differ == [nm for nm in names if nm.startswith("f")], differ     # all of the forget gate and nothing else
    for k in ref:
        np.testing.assert_array_equal(D.bits(got[k]), D.bits(ref[k]), err_msg=k)
    assert all(np.abs(ref["r%d" % l]).max() > 0 for l in range(cfg.nb_layers))   # (not a model that computes nothing)


def test_with_biases_the_forget_gate_does_reach_the_result():
    """bias_scale 0.1: C0_l is not zero and the same overwrite changes r -- the comparison above cannot pass vacuously."""
    cfg, ref = _oracle(D.spec("bias", HP, WP, 1))
    _, got = _oracle(D.spec("bias_f", HP, WP, 1))
    for l in range(cfg.nb_layers):
        assert not np.array_equal(D.bits(got["r%d" % l]), D.bits(ref["r%d" % l])), l


def test_f_times_plus_zero_plus_t_is_plus_zero_plus_t():
    """numpy float32: f * (+0) + t has the bits of (+0) + t -- and those are NOT the bits of t where t is -0."""
    sub = np.float32(1e-45)                                          # the smallest subnormal
    assert sub > 0 and sub.view(np.uint32) == 1
    f = np.array([0.0, 0.5, 1.0, sub], np.float32)
    t = np.array([0.0, -0.0, sub, -sub, 3e-39, -3e-39, 1.5, -1.5, 3e38, -3e38, np.inf, -np.inf], np.float32)
    zero = np.float32(0.0)
    with np.errstate(all="ignore"):
        lhs = (f[:, None] * zero).astype(np.float32) + t[None, :]
        rhs = zero + t
    assert (D.bits(f * zero) == 0).all()
    for row in lhs:
        np.testing.assert_array_equal(D.bits(row), D.bits(rhs))
    assert D.bits(rhs)[1] == 0 and D.bits(t)[1] == 0x80000000        # (+0) + (-0) = +0: the addition is not the identity
    # ... and what the rule does not cover: a NaN forget gate, -0 as the cell state
    assert np.isnan(np.float32(np.nan) * zero)
    assert D.bits(np.float32(0.5) * np.float32(-0.0) + np.float32(-0.0)) == 0x80000000
