"""Level 0 without the dead half of the error maps (-m gpu).  E_0 is stored one half per quad, [e+ (3) 0 | e- (3) 0]; where
tz_model_prepare MEASURES that Ahat0_0 is +-0 over the whole plane (and the weights of those rows are finite), k_conv16b runs
block 0 of A_0 and of the level-0 gates with the k-step of the negative half alone (tz_prednet.hip measure_dead / launch_conv,
tz_conv_kernels.hip.h DEAD0; tests/test_dead0_oracle.py states the lemma on the C oracle).

Every case runs, through the C ABI: predict_next on frames with runs of 0 and 255 (k_err0 from key-like frames), predict_next on
those predictions (k_err0 from float frames), and a rollout of windows of three frames (the second step of a window takes its
error maps from the first step's prediction epilogue, the e0_out path).  Predictions and every level's E / R taps are compared as
BIT PATTERNS between (a) the skip on, (b) TEZIP_DEAD0=0 on a fresh model, (c) tz_set_conv_impl(0) (k_conv3x3 walks all 8 floats
of a pixel, and k_err0 forms every error map) and (d) the C oracle.  What was measured is read from the TEZIP_DEAD0_LOG=1 lines and
compared with the rule restated on the oracle's Ahat0_0 (tests/dead0_models.py)."""
import functools
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (ROOT, os.path.join(ROOT, "tests")):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

import pytest  # noqa: E402

import dead0_models as D  # noqa: E402

pytestmark = pytest.mark.gpu

ENV = ("TEZIP_DEAD0", "TEZIP_DEAD0_LOG", "TEZIP_DEADSRC", "TEZIP_DEADSRC_LOG", "TEZIP_DEADF", "TEZIP_DEADF_LOG", "TEZIP_EPART")
LOG_LINE = re.compile(r"\[tezip\] dead level 0, (A|gates): positive half of E_0 \+0 everywhere: (yes|no), its k-step left out: (yes|no)"
                      r"(?: \((.*)\))?$")
WIN = 3


def _nframes(batch):
    return batch + 1 if batch > 1 else 2   # the last predict_next call is a batch of one: the taps are the last frame's


def _tap_names(cfg, pre=""):
    return [pre + "e%d" % l for l in range(cfg.nb_layers)] + [pre + "r%d" % l for l in range(cfg.nb_layers)]


def _names(cfg):
    return ["p1", "p2", "roll"] + _tap_names(cfg) + _tap_names(cfg, "a")


def run_job(spec, impl=1, frames=None, **env):
    """The job on the GPU with `env` set while the model is loaded and prepared (the switches are read per prepare)."""
    from tezip_amd import _lib
    cfg, w = D.model(spec)
    hp, wp, batch = spec[2], spec[3], spec[4]
    x = D.as_float(D.frames_u8(_nframes(batch), hp, wp)) if frames is None else frames
    old = {k: os.environ.get(k) for k in env}
    c = _lib.Context(0)
    try:
        os.environ.update({k: str(v) for k, v in env.items()})
        c.set_conv_impl(impl)
        c.load_model(cfg, w)
        c.prepare(hp, wp, max_batch=batch)
        c.prof_enable(True)
        c.prof_reset()
        out = {"p1": c.predict_next(x)}
        for l in range(cfg.nb_layers):
            out["e%d" % l], out["r%d" % l] = c.predict_tap(0, l), c.predict_tap(1, l)
        out["p2"] = c.predict_next(out["p1"])
        for l in range(cfg.nb_layers):
            out["ae%d" % l], out["ar%d" % l] = c.predict_tap(0, l), c.predict_tap(1, l)
        u8 = D.frames_u8(batch * WIN, hp, wp, seed=7)
        key, _ = c.rollout(u8, 0, WIN)
        roll = c.get_predictions()
        roll[key] = 0                                            # (slots of key frames hold no prediction)
        out["roll"], out["key"] = roll, key
        prof = c.prof_get()
        out["n16b"], out["n3x3"] = np.array(prof["conv16b_level0"][1]), np.array(prof["conv3x3_general"][1])
        c.prof_enable(False)
    finally:
        c.close()
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return out


@functools.lru_cache(maxsize=None)
def _oracle(spec):
    """Computed once per job; shared by the cases over it and never written to.  (The oracle has no batches.)"""
    from oracle import coracle
    from oracle import oracle as O
    cfg, w = D.model(spec)
    hp, wp, batch = spec[2], spec[3], spec[4]
    net = coracle.CPredNet(w, cfg.stack_sizes, cfg.R_stack_sizes, hp, wp)
    x = D.as_float(D.frames_u8(_nframes(batch), hp, wp))
    ref = {"p1": np.empty_like(x), "p2": np.empty_like(x)}
    for i in range(len(x)):
        ref["p1"][i], d1 = net.next(x[i], debug=True)
        ref["p2"][i], d2 = net.next(ref["p1"][i], debug=True)
    for l in range(cfg.nb_layers):
        ref["e%d" % l], ref["r%d" % l], ref["ae%d" % l], ref["ar%d" % l] = d1["e"][l], d1["r"][l], d2["e"][l], d2["r"][l]

    class P:
        def c0(self, a, b):
            return net.c0()

        def next(self, f):
            return net.next(np.asarray(f, np.float32))

    u8 = D.frames_u8(batch * WIN, hp, wp, seed=7)
    ro = O.rollout(u8, 0, WIN, None, P())
    roll = np.zeros((len(u8), hp, wp, 3), np.float32)
    for start, preds in ro["groups"]:
        for i, p in enumerate(preds):
            roll[start + i] = p
    roll[ro["key"]] = 0
    ref["roll"], ref["key"] = roll, ro["key"]
    for v in ref.values():
        v.setflags(write=False)
    return ref


def _same_bits(got, want, what, cfg):
    np.testing.assert_array_equal(got["key"], want["key"], err_msg=what + ": key frames")
    for k in _names(cfg):
        np.testing.assert_array_equal(D.bits(got[k]), D.bits(want[k]), err_msg="%s: %s" % (what, k))


def _log(stderr):
    rows = {m[1]: dict(zero=m[2] == "yes", out=m[3] == "yes", why=m[4] or "")
            for m in (LOG_LINE.search(ln) for ln in stderr.splitlines()) if m}
    assert set(rows) == {"A", "gates"}, stderr[-1500:]
    return rows


def _check(spec, capfd, oracle=True, kept=None):
    """The four forms of the job give the same bits; the log says what the rule on the oracle's Ahat0_0 says; no launch is added,
    removed or moved to another kernel.  `kept`: {convolution: part of the reason its line must give for walking every k-step}."""
    cfg = D.model(spec)[0]
    capfd.readouterr()
    on = run_job(spec, TEZIP_DEAD0_LOG=1)
    rows = _log(capfd.readouterr().err)
    off = run_job(spec, TEZIP_DEAD0=0)
    assert "dead level 0" not in capfd.readouterr().err            # nothing is printed unless asked
    _same_bits(on, off, "against TEZIP_DEAD0=0", cfg)
    assert on["n16b"] == off["n16b"] > 0 and on["n3x3"] == off["n3x3"], (on["n16b"], off["n16b"], on["n3x3"], off["n3x3"])
    gen = run_job(spec, impl=0)
    assert gen["n16b"] == 0
    _same_bits(on, gen, "against tz_set_conv_impl(0)", cfg)
    if oracle:
        _same_bits(on, _oracle(spec), "against the C oracle", cfg)
    dead = D.positive_half_is_dead(spec)
    for name, row in sorted(rows.items()):
        print("%s: %r" % (name, row))
        assert row["zero"] == dead, (name, row)
        if kept and name in kept:
            assert not row["out"] and kept[name] in row["why"], (name, row)
        else:
            assert row["out"] == dead, (name, row)
            assert ("9 of 18 k-steps" in row["why"]) == row["out"], (name, row)
    return on, rows


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("hp,wp", [(16, 16), (24, 40), (64, 64)])
def test_zero_bias_model_leaves_the_positive_half_out(hp, wp, batch, capfd):
    """Keras' default initialisation (the bench's model).  16 x 16: one tile; 24 x 40: cut tiles in both directions; 64 x 64:
    sixteen tiles.  Black and white runs: x = 0 makes both halves +0, x = 1 the largest error."""
    on, rows = _check(D.spec("zero", hp, wp, batch), capfd)
    assert all(r["out"] for r in rows.values()), rows
    assert (D.bits(on["e0"][:, :, :3]) == 0).all() and np.abs(on["e0"][:, :, 3:]).max() > 0
    assert np.abs(on["r0"]).max() > 0 and np.abs(on["p2"]).max() > 0
    assert (~on["key"]).sum() == batch * (WIN - 1)


@pytest.mark.parametrize("shape,hp,wp,batch", [(D.R1, 24, 40, 3), (D.R1, 16, 16, 1), (D.SMALL, 24, 40, 1), (D.SMALL, 64, 64, 3)],
                         ids=["r0=1-24x40x3", "r0=1-16x16x1", "3x16x32-24x40x1", "3x16x32-64x64x3"])
def test_other_model_shapes(shape, hp, wp, batch, capfd):
    """A_0 at four column tiles with one-channel gates (R_0 = 1), and at one column tile (three levels): with the default model's
    three tiles every k_conv16b shape of a model with levels above level 0."""
    _, rows = _check(D.spec("zero", hp, wp, batch, shape=shape, seed=77), capfd)
    assert all(r["out"] for r in rows.values()), rows


def test_a_gray_first_level_is_not_a_model_the_library_loads():
    """stack_sizes[0] = 1 is refused by tz_model_load (frames are RGB; gray jobs are expanded to three channels first), so the
    layout's C < 3 form is reachable through no entry point; R_0 = 1 above is the gray-most model there is."""
    from tezip_amd import _lib
    from tezip_amd.prednet import PredNetConfig
    cfg = PredNetConfig(stack_sizes=(1, 16, 32))
    c = _lib.Context(0)
    try:
        with pytest.raises(_lib.TezipError, match=r"stack_sizes\[0\] must be 3"):
            c.load_model(cfg, cfg.init_weights(seed=1))
    finally:
        c.close()


@pytest.mark.parametrize("hp,wp,batch,seed", [(24, 40, 3, 123), (64, 64, 1, 31)])
def test_biased_models_walk_every_k_step(hp, wp, batch, seed, capfd):
    """bias_scale 0.1: Ahat0_0 is not zero, nothing is dead, the launches are the ones TEZIP_DEAD0=0 makes (_check: the same
    counts per kernel, the same bits) -- the layout alone changed for such a model, and the oracle and k_conv3x3 still agree."""
    on, rows = _check(D.spec("bias", hp, wp, batch, seed=seed), capfd)
    assert rows == {"A": dict(zero=False, out=False, why=""), "gates": dict(zero=False, out=False, why="")}, rows
    # the activation getter hands E_0 out in the channel order [positive (3) | negative (3)]: both halves are live here
    ref = _oracle(D.spec("bias", hp, wp, batch, seed=seed))
    for k in ("e0", "ae0"):
        assert on[k].shape == (hp, wp, 6)
        np.testing.assert_array_equal(D.bits(on[k]), D.bits(ref[k]))
        # (a channel whose Ahat0_0 the bias took to 0 has an empty positive half; no two live channels are the same)
        live = [ch for ch in range(6) if np.abs(on[k][:, :, ch]).max() > 0]
        assert any(ch < 3 for ch in live) and any(ch >= 3 for ch in live), (k, live)
        assert all(not np.array_equal(on[k][:, :, a], on[k][:, :, b]) for a in live for b in live if a < b), k


def test_a_plane_that_is_zero_inside_but_not_on_the_border(capfd):
    """Ahat0_0 is +0 everywhere but on the right border column (tests/dead0_models.py): a measurement that looked at the interior,
    or at one pixel, would call the half dead.  Asserted on the oracle's plane; the log must say that every k-step is walked."""
    spec = D.spec("border", 24, 40, 1)
    a = D.ahat0(spec)
    assert (D.bits(a[:, :-1]) == 0).all() and a[:, -1].min() > 1e-2
    on, rows = _check(spec, capfd)
    assert rows == {"A": dict(zero=False, out=False, why=""), "gates": dict(zero=False, out=False, why="")}, rows
    assert on["e0"][:, -1, :3].max() > 1e-2                          # the positive half IS live there, under the black pixels


def test_a_non_finite_weight_on_the_positive_half_keeps_both_k_steps(capfd):
    """One +inf in A_0's kernel on a channel of the positive half: A_0 walks both k-steps (0 x inf is a NaN the chain must keep),
    the gates, whose weights are finite, do not.  Compared with TEZIP_DEAD0=0 and k_conv3x3 (what the oracle's libm makes of
    the NaN is its business)."""
    _, rows = _check(D.spec("zero+inf", 24, 40, 1), capfd, oracle=False, kept={"A": "not finite"})
    assert [(rows[k]["zero"], rows[k]["out"]) for k in ("A", "gates")] == [(True, False), (True, True)], rows


def test_predict_next_holds_the_skip_off_for_frames_with_a_sign_bit(capfd):
    """tz_predict_next takes the caller's floats: a negative value makes relu(Ahat0_0 - x) positive, the half is live for that
    call, and the call walks every k-step -- the results are the oracle's.  (Frames of the codec are u8 / 255 or predictions.)"""
    spec = D.spec("zero", 24, 40, 1)
    cfg = D.model(spec)[0]
    x = D.as_float(D.frames_u8(2, 24, 40))
    x[:, 3:9, 5:30] = -0.25
    from oracle import coracle
    net = coracle.CPredNet(D.model(spec)[1], cfg.stack_sizes, cfg.R_stack_sizes, 24, 40)
    want, dbg = net.next(x[1], debug=True)
    got = run_job(spec, frames=x, TEZIP_DEAD0_LOG=1)
    assert all(r["out"] for r in _log(capfd.readouterr().err).values())
    np.testing.assert_array_equal(D.bits(got["p1"][1]), D.bits(want))
    for l in range(cfg.nb_layers):
        np.testing.assert_array_equal(D.bits(got["e%d" % l]), D.bits(dbg["e"][l]), err_msg="e%d" % l)
    assert got["e0"][:, :, :3].max() == np.float32(0.25)
