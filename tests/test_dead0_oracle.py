"""The lemma behind k_conv16b's dead positive half of E_0 (tz_prednet.hip measure_dead / launch_conv), on
the C oracle:

    E_0 = [relu(Ahat0_0 - x), relu(x - Ahat0_0)] and x >= +0.  Where Ahat0_0 is +-0 over the whole plane the positive half is
    +0 at every pixel of every frame, and a term fmaf(+0, w, acc) with w finite leaves a non-zero acc as it is and a zero acc
    a zero: the weights that multiply the positive half reach no result.

Runs on the CPU.  Compared as uint32 bit patterns: a zero of the other sign is a difference.  The frames hold black pixels
(x = 0: the negative half is +0 there too, and its products with negative weights are -0) and full white."""
import numpy as np
import pytest

import dead0_models as D
from oracle import coracle

HP, WP = 24, 40
NFRAMES = 4


def _run(sp):
    """Predictions of NFRAMES frames and of each prediction fed back once, and the taps of the last call."""
    cfg, w = D.model(sp)
    net = coracle.CPredNet(w, cfg.stack_sizes, cfg.R_stack_sizes, sp[2], sp[3])
    x = D.as_float(D.frames_u8(NFRAMES, sp[2], sp[3]))
    assert (x == 0).any() and (x == 1).any() and (x[1] == 0).all() and (x[2] == 1).all()
    out = {}
    for i in range(NFRAMES):
        out["pred%d" % i], dbg = net.next(x[i], debug=True)
        out["again%d" % i], dbg2 = net.next(out["pred%d" % i], debug=True)
        for l in range(cfg.nb_layers):
            out["e%d_%d" % (l, i)], out["r%d_%d" % (l, i)] = dbg["e"][l], dbg["r"][l]
            out["ae%d_%d" % (l, i)], out["ar%d_%d" % (l, i)] = dbg2["e"][l], dbg2["r"][l]
    return cfg, out


_run_cached = {}


def _ref(sp):
    if sp not in _run_cached:
        _run_cached[sp] = _run(sp)
        for v in _run_cached[sp][1].values():
            v.setflags(write=False)
    return _run_cached[sp]


@pytest.mark.parametrize("shape", [D.DEFAULT, D.R1, D.SMALL], ids=["default", "r0=1", "3x16x32"])
def test_ahat0_is_zero_on_the_whole_plane_exactly_for_zero_biases(shape):
    assert D.positive_half_is_dead(D.spec("zero", HP, WP, 1, shape=shape))
    assert not D.positive_half_is_dead(D.spec("bias", HP, WP, 1, shape=shape))


@pytest.mark.parametrize("how", ["random", "huge", "negative"])
def test_the_positive_half_weights_reach_no_result_where_ahat0_is_zero(how):
    cfg, ref = _ref(D.spec("zero", HP, WP, 1))
    _, got = _run(D.spec("zero+" + how, HP, WP, 1))
    w0, w1 = D.model(D.spec("zero", HP, WP, 1))[1], D.model(D.spec("zero+" + how, HP, WP, 1))[1]
    names = [nm for nm, _ in cfg.weight_shapes()]
    differ = [nm for nm, a, b in zip(names, w0, w1) if not np.array_equal(a, b)]
    assert sorted(differ) == sorted(nm for nm, _, _ in D.pos_rows(cfg)), differ
    for nm, c0, n in D.pos_rows(cfg):   # ... and of those kernels only the rows of the positive half
        a, b = w0[names.index(nm)], w1[names.index(nm)]
        keep = np.r_[0:c0, c0 + n:a.shape[2]]
        assert np.array_equal(a[:, :, keep], b[:, :, keep]) and (a[:, :, c0:c0 + n] != b[:, :, c0:c0 + n]).all()
    for k in ref:
        np.testing.assert_array_equal(D.bits(got[k]), D.bits(ref[k]), err_msg=k)
    # (not a model that computes nothing, and the positive half IS +0 in every word)
    assert all(np.abs(ref["r%d_0" % l]).max() > 0 for l in range(cfg.nb_layers))
    for i in range(NFRAMES):
        assert (D.bits(ref["e0_%d" % i][:, :, :3]) == 0).all()
    assert np.abs(ref["e0_0"][:, :, 3:]).max() > 0


def test_one_infinite_weight_on_a_dead_channel_changes_the_result():
    """0 x inf is a NaN the chain must keep: why measure_dead asks for finite weights."""
    cfg, ref = _ref(D.spec("zero", HP, WP, 1))
    _, got = _run(D.spec("zero+inf", HP, WP, 1))
    assert not np.array_equal(D.bits(got["e1_0"]), D.bits(ref["e1_0"]))
    assert not np.array_equal(D.bits(got["pred0"]), D.bits(ref["pred0"]))


def test_a_plane_that_is_zero_inside_but_not_on_the_border():
    """Ahat0_0 of the border model: +0 inside and on the left border, 0.036 on the right border column.  There the positive half
    is live under black pixels and the overwrite does change bits: why the whole plane is looked at."""
    sp = D.spec("border", HP, WP, 1)
    a = D.ahat0(sp)
    assert (D.bits(a[:, :-1]) == 0).all() and a[:, -1].min() > 1e-2
    assert not D.positive_half_is_dead(sp)
    _, ref = _ref(sp)
    assert ref["e0_0"][:, -1, :3].max() > 1e-2 and (D.bits(ref["e0_0"][:, :-1, :3]) == 0).all()
    _, got = _run(D.spec("border+random", HP, WP, 1))
    assert not np.array_equal(D.bits(got["e1_0"]), D.bits(ref["e1_0"]))
    assert not np.array_equal(D.bits(got["pred0"]), D.bits(ref["pred0"]))
