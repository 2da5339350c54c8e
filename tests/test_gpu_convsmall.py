"""k_conv_small, the level-0 prediction convolution (-m gpu; tezip_amd/csrc/tz_conv_kernels.hip.h): a thread owns four
neighbouring pixels of a row, a workgroup a tile of 16 x 64 pixels, all global accesses 16 bytes wide.  The arithmetic is the
statement it always was -- acc = bias, taps ascending, ci ascending, fmaf; relu; clip -- so it is compared in BIT PATTERNS with
tz_set_conv_impl(0) (k_conv3x3 for every convolution, k_err0 for every E_0) and with the C oracle:
  * through tz_predict_next, twice chained (no e0_out: the prediction alone);
  * through a rollout of three-frame windows whose last window is shorter, so that the windows of a batch end at different
    steps: out_idx maps batch items to frame slots that are not in batch order, the items whose window ends have e0_slot = -1
    and the others get the next step's E_0 from the epilogue -- the live quad alone for the zero-bias model (dead_half), both
    halves with Ahat0_0 loaded for bias_scale 0.1;
  * E_0 itself and the states behind the rollout (tz_predict_tap) against tz_set_conv_impl(0).
Frame sizes: 16 x 16 is smaller than the tile both ways; 24 x 40 has a partial tile and an odd count of 8-pixel halves; 64 x 64
is four whole tiles in a column; 40 x 72 has a second, 8-pixel-wide tile in x and a third, 8-row one in y.  tz_model_prepare
takes padded sizes that divide by 8 only, so there is no width that is not a multiple of 4 to try."""
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
import devmem  # noqa: E402

pytestmark = pytest.mark.gpu

WIN = 3
NT = {1: 5, 3: 8}     # frames of the rollout per batch: windows [0-2] [3-4] one after the other; [0-2] [3-5] [6-7] side by side
SIZES = [(16, 16), (24, 40), (64, 64), (40, 72)]
HALF_LINE = re.compile(r"\[tezip\] dead half, level 0: Ahat0 \+-0 over the whole plane: (yes|no)")


def _clip_model(seed):
    """bias_scale 0.1 with a prediction bias of 30 on channel 0 and 0.9 on channel 1: |conv| <= 27 max|w| max|r_0| < 27 x 0.34
    for these weights, so relu(conv + 30) is above 1 at every pixel; channel 1 is near 1."""
    cfg, w = D.model(D.spec("bias", 16, 16, 1, seed=seed))
    names = [nm for nm, _ in cfg.weight_shapes()]
    assert np.abs(w[names.index("ahat0/kernel")]).max() < 0.34
    w[names.index("ahat0/bias")][:2] = np.float32([30.0, 0.9])
    return cfg, w


MODELS = {
    "zero": lambda seed: D.model(D.spec("zero", 16, 16, 1, seed=seed)),
    "bias": lambda seed: D.model(D.spec("bias", 16, 16, 1, seed=seed)),
    "clip": _clip_model,
}


def _frames(hp, wp, batch):
    return D.as_float(D.frames_u8(batch, hp, wp)), D.frames_u8(NT[batch], hp, wp, seed=7)


def run(kind, hp, wp, batch, impl, seed=123):
    from tezip_amd import _lib
    cfg, w = MODELS[kind](seed)
    x, u8 = _frames(hp, wp, batch)
    os.environ["TEZIP_DEADHALF_LOG"] = "1"
    c = None
    try:
        c = _lib.Context(0)
        c.set_contract(2)
        c.load_model(cfg, w)
        c.prepare(hp, wp, max_batch=batch)
        c.set_conv_impl(impl)
        c.prof_enable(True)
        c.prof_reset()
        out = {"p1": c.predict_next(x)}
        out["p2"] = c.predict_next(out["p1"])
        key, _ = c.rollout(u8, 0, WIN)
        roll = c.get_predictions()
        roll[key] = 0                                            # (slots of key frames hold no prediction)
        out["roll"], out["key"] = roll, key
        for l in range(cfg.nb_layers):
            out["qe%d" % l], out["qr%d" % l] = c.predict_tap(0, l), c.predict_tap(1, l)
        out["launches"] = c.prof_get()["conv_small_valu"][1]     # (the profile class of k_conv_small: launches counted)
        return out
    finally:
        if c is not None:
            c.close()
        del os.environ["TEZIP_DEADHALF_LOG"]


@functools.lru_cache(maxsize=None)
def oracle(kind, hp, wp, batch, seed=123):
    """The C oracle's predictions of the same job: computed once, shared, never written to."""
    from oracle import coracle
    from oracle import oracle as O
    cfg, w = MODELS[kind](seed)
    net = coracle.CPredNet(w, cfg.stack_sizes, cfg.R_stack_sizes, hp, wp).set_contract(2)
    x, u8 = _frames(hp, wp, batch)
    ref = {"p1": np.empty_like(x), "p2": np.empty_like(x)}
    for i in range(len(x)):
        ref["p1"][i] = net.next(x[i])
        ref["p2"][i] = net.next(ref["p1"][i])

    class P:
        def c0(self, a, b):
            return net.c0()

        def next(self, f):
            return net.next(np.asarray(f, np.float32))

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


def check(kind, hp, wp, batch, capfd):
    capfd.readouterr()
    new = run(kind, hp, wp, batch, 1)
    half = [m[1] == "yes" for m in map(HALF_LINE.search, capfd.readouterr().err.splitlines()) if m]
    gen = run(kind, hp, wp, batch, 0)
    ref = oracle(kind, hp, wp, batch)
    np.testing.assert_array_equal(new["key"], gen["key"])
    np.testing.assert_array_equal(new["key"], ref["key"])
    assert list(np.flatnonzero(new["key"])) == list(range(0, NT[batch], WIN))     # the last window is one frame short
    # k_conv_small is what ran: once per predictor step (two tz_predict_next calls, then the steps of the rollout), and
    # never under tz_set_conv_impl(0)
    assert new.pop("launches") >= 2 + (WIN - 1) and gen.pop("launches") == 0
    for k in sorted(set(new) - {"key"}):
        np.testing.assert_array_equal(D.bits(new[k]), D.bits(gen[k]), err_msg="against tz_set_conv_impl(0): " + k)
    for k in ("p1", "p2", "roll"):
        np.testing.assert_array_equal(D.bits(new[k]), D.bits(ref[k]), err_msg="against the C oracle: " + k)
    assert len(half) == 1, half
    return new, half[0]


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("hp,wp", SIZES)
def test_zero_bias_model_stores_the_live_quad_alone(hp, wp, batch, capfd):
    new, dead_half = check("zero", hp, wp, batch, capfd)
    assert dead_half
    pos, neg = new["qe0"][..., :3], new["qe0"][..., 3:]
    assert not D.bits(pos).any() and np.abs(neg).max() > 0      # E_0 behind the rollout: [+0 | x - Ahat_0 where positive]
    assert np.abs(new["roll"]).max() > 0 and np.abs(new["p2"]).max() > 0


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("hp,wp", SIZES)
def test_biased_model_stores_both_halves(hp, wp, batch, capfd):
    new, dead_half = check("bias", hp, wp, batch, capfd)
    assert not dead_half
    assert np.abs(new["qe0"]).max() > 0


@pytest.mark.parametrize("hp,wp,batch", [(24, 40, 3), (40, 72, 1)])
def test_a_prediction_above_one_clips(hp, wp, batch, capfd):
    new, _ = check("clip", hp, wp, batch, capfd)
    for k in ("p1", "p2"):
        assert (new[k][..., 0] == 1).all(), k                    # relu(conv + 30) > 1 everywhere
        assert new[k].max() == 1, k
    pred = new["roll"][~new["key"]]
    assert (pred[..., 0] == 1).all() and pred.max() == 1


@pytest.mark.parametrize("offset", [4, 8])
@pytest.mark.parametrize("kind", ["zero", "clip"])
def test_a_callers_stack_off_the_16_byte_grid(kind, offset, capfd):
    """tz_predict_next into a caller's DEVICE stack that starts 4 or 8 bytes behind a 16-byte boundary (a device pointer is
    passed on as it is): the prediction then leaves as 4-byte stores.  The same bits as into an aligned stack, which check()
    holds to the references, and not a byte outside the stack is written."""
    from tezip_amd import _lib
    hp, wp, batch = 24, 40, 3
    cfg, w = MODELS[kind](123)
    x, _ = _frames(hp, wp, batch)
    c = _lib.Context(0)
    try:
        c.set_contract(2)
        c.load_model(cfg, w)
        c.prepare(hp, wp, max_batch=batch)
        want = c.predict_next(x)
        np.testing.assert_array_equal(D.bits(want), D.bits(oracle(kind, hp, wp, batch)["p1"]))
        out, guards_intact = devmem.view(devmem.fill(x.shape, np.float32), offset)
        c.prof_enable(True)
        c.prof_reset()
        c.predict_next(x, out=out)
        assert c.prof_get()["conv_small_valu"][1] == 1
        np.testing.assert_array_equal(D.bits(devmem.host(out)), D.bits(want))
        assert guards_intact()
    finally:
        c.close()
