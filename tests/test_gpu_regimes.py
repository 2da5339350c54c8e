"""The HIP predictor where gates saturate and sums go subnormal (-m gpu), against the C oracle BIT FOR BIT under TZ-PA1 and
TZ-PA2.  Every other network-level test runs glorot weights as init_weights draws them: predictions below 0.27, |c| <
0.37, no gate clipped, nothing subnormal -- the clamp of Ahat_0 at pixel_max, tanh's middle branch, both clips of the
hard sigmoid and subnormal operands of the MFMA chains are reached by no fused epilogue there (only by the scalar probe
kernel).  tests/regimes.py scales the weights until they are; tests/test_regimes.py asserts on the CPU that every case
here reaches its regime and that the oracle is right there.  Comparisons are of bit patterns (regimes.assert_same_bits): a
flushed subnormal and a zero of the other sign are differences."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import regimes as R  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from tezip_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _load(c, case, contract, max_batch=2):
    regime, stack, rstack, hp, wp = case
    cfg, w = R.model(regime, stack, rstack)
    c.set_contract(contract)
    c.load_model(cfg, w)
    c.prepare(hp, wp, max_batch=max_batch)
    assert c.get_contract() == contract
    return cfg


def _run(c, case, cfg):
    """What regimes.oracle() computes, on the GPU: the three random frames through a batch of two (batch invariance; the
    taps then hold the last frame, a batch of one), the two constant frames as one batch, the first prediction fed back."""
    rand, const = R.frames(case[3], case[4])
    out = {"t0": c.predict_c0(), "pred": c.predict_next(rand)}
    for l in range(cfg.nb_layers):
        out["e%d" % l], out["r%d" % l] = c.predict_tap(0, l), c.predict_tap(1, l)
    out["const"] = c.predict_next(const)
    out["again"] = c.predict_next(out["pred"][:1])[0]
    return out


def _names(cfg):
    return ["t0", "pred", "const", "again"] + ["%s%d" % (k, l) for k in "er" for l in range(cfg.nb_layers)]


def _compare(got, want, cfg, what):
    for k in _names(cfg):
        R.assert_same_bits(got[k], want[k], "%s: %s" % (what, k))


# ----------------------------------------------------------------------------------------------------- regimes x shapes
@pytest.mark.parametrize("contract", [1, 2])
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_predictor_bit_exact_in_the_regime(ctx, case, contract):
    cfg = _load(ctx, case, contract)
    _compare(_run(ctx, case, cfg), R.oracle(case, contract), cfg, "%s under TZ-PA%d against the C oracle" % (R.case_id(case), contract))


# ------------------------------------------------------------------------ every dispatch path, saturated (S16)
def _fresh(monkeypatch, **env):
    from tezip_amd import _lib
    for k in ("TEZIP_EPART", "TEZIP_WINO_IPW", "TEZIP_UNIFORM"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    return _lib.Context(0)


@pytest.mark.parametrize("contract", [1, 2])
@pytest.mark.parametrize("case", R.DISPATCH_CASES, ids=R.case_id)
def test_every_dispatch_path_gives_the_oracles_bits_when_saturated(ctx, case, contract, monkeypatch):
    """The general kernel against the LDS-DMA kernels, k_convlat never / always / where the cost model picks it, the split
    gate launches forbidden and forced, two and three column blocks per k_wino workgroup: the same epilogue arithmetic
    written out in each of them -- identical to the oracle, hence to each other."""
    want = R.oracle(case, contract)
    what = "%s under TZ-PA%d, " % (R.case_id(case), contract)
    cfg = _load(ctx, case, contract)
    try:
        for impl, lat in ((0, None), (1, None), (1, "never"), (1, "always")):
            ctx.set_conv_impl(impl, lat=lat)
            _compare(_run(ctx, case, cfg), want, cfg, what + "set_conv_impl(%d, lat=%r)" % (impl, lat))
    finally:
        ctx.set_conv_impl(1)
    if contract == 2:       # k_wino really ran (tests/test_gpu_wino.py)
        ctx.prof_enable(True)
        ctx.prof_reset()
        ctx.predict_next(R.frames(case[3], case[4])[0][:1])
        prof = ctx.prof_get()
        ctx.prof_enable(False)
        assert prof["wino_pa2"][1] > 0 and prof["conv16_lds_dma"][1] == 0, prof
    for env in ({"TEZIP_EPART": 0}, {"TEZIP_EPART": 1}, {"TEZIP_WINO_IPW": 2}, {"TEZIP_WINO_IPW": 3}):
        c = _fresh(monkeypatch, **env)
        try:
            _load(c, case, contract)
            if contract == 2 and "TEZIP_EPART" in env:
                c.prof_enable(True)
                c.prof_reset()
            got = _run(c, case, cfg)
            if contract == 2 and "TEZIP_EPART" in env:     # 5 k_wino launches a predictor call fused, 7 split; 4 calls
                n = c.prof_get()["wino_pa2"][1]
                c.prof_enable(False)
                assert n == (7 if env["TEZIP_EPART"] else 5) * 4, (env, n)
        finally:
            c.close()
        _compare(got, want, cfg, what + "%r" % (env,))


# ------------------------------------------------------------------------------------- whole jobs, full delta range
@pytest.mark.parametrize("contract", [1, 2])
@pytest.mark.parametrize("job", R.JOBS, ids=R.job_id)
def test_compress_decompress_matches_oracle_over_the_full_delta_range(ctx, job, contract):
    """rollout -> encode -> decoder replay -> decode with the saturated model on frames that go black and white: deltas of
    -255 .. +255 through the fused encodes (tests/test_regimes.py asserts >= 200 and <= -200 on the oracle), against the
    numpy oracle driving the C predictor on the same contract: key mask, table, payload, decoded frames."""
    from oracle import oracle as O
    from tezip_amd import _lib
    nt, h, w, p, window, thr, mode, bound = job
    ref = R.job_oracle(job, contract)
    frames = R.job_frames(nt, h, w)
    cfg, wts = R.model("S16")
    ctx.set_contract(contract)
    ctx.load_model(cfg, wts)
    ctx.prepare(_lib.pad8(h), _lib.pad8(w), max_batch=3)
    key, _ = ctx.rollout(frames, p, window, ref["thr"])
    np.testing.assert_array_equal(key, ref["key"])
    stack = ctx.get_predictions()
    for start, preds in ref["rollout"]["groups"]:
        for j, pr in enumerate(preds):
            if j > 0 or start < p:
                R.assert_same_bits(stack[start + j], pr, "prediction of frame %d" % (start + j))
    payload, table, _ = ctx.encode(mode, list(bound), True)
    ref_payload, ref_table, _, _ = O.parse_stream(ref["stream"])
    np.testing.assert_array_equal(table, ref_table)
    np.testing.assert_array_equal(payload, ref_payload)
    _, _, delta = ctx.encode(mode, list(bound), True, want_delta=True)       # the unfused quantiser: the same deltas
    np.testing.assert_array_equal(delta, ref["delta"])
    kd = ctx.rollout_decode(ref["key_frame"].reshape(nt, h, w, 3), p)
    np.testing.assert_array_equal(kd, ref["key"])
    dec = ctx.decode(payload, table)
    np.testing.assert_array_equal(dec, ref["decoded"])
    if bound[0] == 0:
        np.testing.assert_array_equal(dec, frames)
