"""The HIP predictor across the model shapes tz_model_load accepts (-m gpu), against the C oracle BIT FOR BIT under TZ-PA1
and TZ-PA2.  Which kernel a convolution runs on is a function of the channel counts, and the other tests run few of them:
tests/model_space.py lists models that produce the rest (tests/test_model_space.py asserts that on the CPU, and that the
oracle is right on them) -- column blocks of 5, 7, 10, 15, 16, 24, packed gates of R = 1, 2 and above level 0, five to eight
levels, 1152 input channels.  Every model through every dispatch switch; the profiler's launch counts against the families
model_space.families derives from the rules of launch_conv, so that a model meant for one kernel that silently reaches
another fails; fresh contexts under the environment switches; whole jobs; one job through the command line; and the edges
of what tz_model_load and tz_model_prepare accept.  Comparisons are of bit patterns (regimes.assert_same_bits).

The device has taps for e and r; the cell state c of the step is not kept (r = o * tanh(c) carries it)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import model_space as M  # noqa: E402
from test_gpu_regimes import _fresh  # noqa: E402

pytestmark = pytest.mark.gpu

IDS = [m[0] for m in M.MODELS]
TZ_ERR_INVALID, TZ_ERR_UNSUPPORTED = -1, -6


@pytest.fixture(scope="module")
def ctx():
    from tezip_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _load(c, mid, contract, max_batch=2):
    _, _, _, hp, wp = M.BY_ID[mid]
    cfg = M.config(M.BY_ID[mid])
    c.set_contract(contract)
    c.load_model(cfg, M.weights(mid))
    c.prepare(hp, wp, max_batch=max_batch)
    return cfg


def _run(c, mid, cfg):
    """What model_space.oracle() computes, on the GPU: the three random frames through a batch of two (batch invariance;
    the taps then hold the last frame, a batch of one), the two constant frames as one batch, the first prediction fed
    back.  The 256 x 256 model: one frame."""
    rand, const = M.frames(*M.BY_ID[mid][3:])
    if mid == M.DEFAULT_CONTRACT_MODEL:
        rand = rand[:1]
    out = {"t0": c.predict_c0(), "pred": c.predict_next(rand)}
    for l in range(cfg.nb_layers):
        out["e%d" % l], out["r%d" % l] = c.predict_tap(0, l), c.predict_tap(1, l)
    if mid != M.DEFAULT_CONTRACT_MODEL:
        out["const"] = c.predict_next(const)
        out["again"] = c.predict_next(out["pred"][:1])[0]
    return out


def _compare(got, want, what):
    assert set(got) == {k for k in want if not (k[0] == "c" and k[1:].isdigit())}, (sorted(got), sorted(want))
    for k in got:
        M.assert_same_bits(got[k], want[k], "%s: %s" % (what, k))


def _contracts(mid):
    # (the 256 x 256 model is there for contract 0: the default must pick TZ-PA2 at that size)
    return [0] if mid == M.DEFAULT_CONTRACT_MODEL else [1, 2]


def _effective(mid, contract):
    return 2 if mid == M.DEFAULT_CONTRACT_MODEL else contract


CASES = [(mid, c) for mid in IDS for c in _contracts(mid)]
CASE_IDS = ["%s-PA%d" % mc for mc in CASES]


def _profile_one_step(c, mid):
    c.prof_enable(True)
    c.prof_reset()
    c.predict_next(M.frames(*M.BY_ID[mid][3:])[0][:1])
    prof = c.prof_get()
    c.prof_enable(False)
    return {k: prof[k][1] for k in M.FAMILIES}


# ------------------------------------------------------------------------------------------ models x dispatch switches
@pytest.mark.parametrize("mid,contract", CASES, ids=CASE_IDS)
def test_predictor_bit_exact_on_the_model_through_every_switch(ctx, mid, contract):
    """The general kernel, the LDS-DMA kernels, k_convlat never / always / where the cost model picks it: the same chains
    written out in each -- identical to the oracle, hence to each other.  Then the launch counts of one predictor step:
    every family is zero or not as the rules of launch_conv say for these channel counts."""
    cfg = _load(ctx, mid, contract)
    eff = _effective(mid, contract)
    assert ctx.get_contract() == eff
    want = M.oracle(mid, eff)
    what = "%s under TZ-PA%d, " % (mid, eff)
    try:
        for impl, lat in ((1, None), (0, None), (1, "never"), (1, "always")):
            ctx.set_conv_impl(impl, lat=lat)
            _compare(_run(ctx, mid, cfg), want, what + "set_conv_impl(%d, lat=%r)" % (impl, lat))
        fam = M.families(cfg, eff)
        ctx.set_conv_impl(1)
        n = _profile_one_step(ctx, mid)
        print(mid, "TZ-PA%d" % eff, n)
        for k in ("wino_pa2", "conv16b_level0", "conv_small_valu", "conv3x3_general"):
            assert (n[k] > 0) == (k in fam), (mid, k, n, fam)
        assert (n["conv16_lds_dma"] + n["convlat_small_grid"] > 0) == ("lds" in fam), (mid, n, fam)
        assert n["wino_pa2"] in ((M.wino_launches(cfg), M.wino_launches(cfg) + len(M.epart_can_split(cfg))) if eff == 2 else (0,)), (mid, n)
        assert n["conv16b_level0"] == len(fam.get("conv16b_level0", [])) and n["conv3x3_general"] == len(fam.get("conv3x3_general", []))
        ctx.set_conv_impl(1, lat="never")       # the cost model out of the way: the LDS-DMA family is k_conv16 alone
        n = _profile_one_step(ctx, mid)
        assert n["convlat_small_grid"] == 0 and n["conv16_lds_dma"] == len(fam.get("lds", [])), (mid, n, fam)
        # (fused, or with the levels that can split in two launches where that measured faster for this batch size)
        assert n["wino_pa2"] in ((M.wino_launches(cfg), M.wino_launches(cfg) + len(M.epart_can_split(cfg))) if eff == 2 else (0,)), (mid, n)
        ctx.set_conv_impl(0)                    # everything but k_wino_ref's chains on the general kernel
        n = _profile_one_step(ctx, mid)
        assert n["conv16_lds_dma"] == n["convlat_small_grid"] == n["conv16b_level0"] == n["conv_small_valu"] == 0, (mid, n)
    finally:
        ctx.set_conv_impl(1)


# --------------------------------------------------------------------------------------- fresh contexts, env switches
def _proper_divisors(n):
    return [d for d in range(1, n) if n % d == 0]


def _env_cases():
    out = []
    for mid in ("M2", "M3", "M8"):
        cl = M.classes(M.config(M.BY_ID[mid]))
        ipw = sorted({d for c in cl.values() if c["kind"] == "gates" and not c["packed"] for d in _proper_divisors(c["ncb"])})
        for contract in (1, 2):
            out += [(mid, contract, "TEZIP_EPART", v) for v in (0, 1)]
        out += [(mid, 2, "TEZIP_WINO_IPW", d) for d in ipw]     # (k_wino runs under TZ-PA2 only)
    return out


@pytest.mark.parametrize("mid,contract,name,value", _env_cases(), ids=lambda v: str(v))
def test_fresh_context_under_an_env_switch_gives_the_oracles_bits(mid, contract, name, value, monkeypatch):
    """The split gate launches forbidden and forced; every proper divisor of the models' gate column blocks as k_wino's
    column blocks per workgroup.  Where a level can split, the forced split really launched one more k_wino per level and
    step than the fused step."""
    cfg = M.config(M.BY_ID[mid])
    c = _fresh(monkeypatch, **{name: value})
    try:
        _load(c, mid, contract)
        count = contract == 2 and name == "TEZIP_EPART"
        if count:
            c.prof_enable(True)
            c.prof_reset()
        got = _run(c, mid, cfg)
        if count:      # four predictor calls in _run
            n = c.prof_get()["wino_pa2"][1]
            c.prof_enable(False)
            split = len(M.epart_can_split(cfg)) if value else 0
            assert n == (M.wino_launches(cfg) + split) * 4, (mid, value, n, M.wino_launches(cfg), split)
    finally:
        c.close()
    _compare(got, M.oracle(mid, contract), "%s under TZ-PA%d, %s=%s" % (mid, contract, name, value))


def test_the_env_cases_split_somewhere_and_nowhere():
    assert M.epart_can_split(M.config(M.BY_ID["M2"])) == [1] and M.epart_can_split(M.config(M.BY_ID["M3"])) == [1]
    assert M.epart_can_split(M.config(M.BY_ID["M8"])) == []


# ------------------------------------------------------------------------------------------------------------ whole jobs
@pytest.mark.parametrize("window,bound", [(3, 0.0), (3, 2.0), (None, 2.0)], ids=["swp-abs0", "swp-abs2", "dwp-abs2"])
@pytest.mark.parametrize("contract", [1, 2])
@pytest.mark.parametrize("mid", M.JOB_MODELS)
def test_whole_jobs_match_the_oracle(ctx, mid, contract, window, bound):
    """rollout -> encode -> decoder replay -> decode against the numpy oracle driving the C predictor on the same contract:
    key mask, table, payload, rollout_decode's key mask, decoded frames.  Frames cropped below the padded size."""
    from oracle import oracle as O
    from tezip_amd import _lib
    nt, h, w = M.job_geometry(mid)
    _, _, _, hp, wp = M.BY_ID[mid]
    assert (h, w) != (hp, wp) and (_lib.pad8(h), _lib.pad8(w)) == (hp, wp)
    ref = M.job_oracle(mid, contract, window, bound)
    frames = M.job_frames(mid)
    _load(ctx, mid, contract, max_batch=3)
    key, _ = ctx.rollout(frames, 0, window, ref["thr"])
    np.testing.assert_array_equal(key, ref["key"])
    if window is None:
        assert 1 < int(key.sum()) < nt - 1
    payload, table, _ = ctx.encode("abs", [bound], True)
    ref_payload, ref_table, _, _ = O.parse_stream(ref["stream"])
    np.testing.assert_array_equal(table, ref_table)
    np.testing.assert_array_equal(payload, ref_payload)
    kd = ctx.rollout_decode(ref["key_frame"].reshape(nt, h, w, 3), 0)
    np.testing.assert_array_equal(kd, ref["key"])
    dec = ctx.decode(payload, table)
    np.testing.assert_array_equal(dec, ref["decoded"])
    if bound == 0:
        np.testing.assert_array_equal(dec, frames)
    else:
        assert int(np.abs(dec.astype(int) - frames.astype(int)).max()) <= bound


# ---------------------------------------------------------------------------------------------------------- command line
def _write_pngs(folder, frames):
    from PIL import Image
    folder.mkdir()
    for t in range(frames.shape[0]):
        Image.fromarray(frames[t], mode="RGB").save(folder / ("frame_%03d.png" % t))
    return str(folder)


def test_cli_one_job_with_the_five_level_model(tmp_path, capsys):
    """-c then -u of 30x44 PNGs (pads to 32x48) with the five-level model, lossless: the output is the input.  24x40 frames
    pad to 24x40, which a five-level model cannot halve four times: refused in the reference's words, whether the model
    file names another size or this one, and no output directory is left."""
    from PIL import Image
    from tezip_amd import compress, decompress, synth, weights
    cfg = M.config(M.BY_ID["M6"])
    mdir = str(tmp_path / "model")
    weights.save_model(mdir, cfg, M.weights("M6"), 32, 48)
    frames = synth.translating_scene(6, 30, 44, seed=23)
    ddir = _write_pngs(tmp_path / "data", frames)
    cdir, udir = str(tmp_path / "comp"), str(tmp_path / "out")
    compress.run(mdir, ddir, cdir, 0, 3, None, "abs", [0.0], True, False, True)
    decompress.run(mdir, cdir, udir, True, False)
    got = np.stack([np.array(Image.open(os.path.join(udir, "frame_%03d.png" % t))) for t in range(6)])
    np.testing.assert_array_equal(got, frames)
    capsys.readouterr()
    small = _write_pngs(tmp_path / "data24", synth.translating_scene(4, 24, 40, seed=24))
    mdir24 = str(tmp_path / "model24")
    weights.save_model(mdir24, cfg, M.weights("M6"), 24, 40)
    for k, model in enumerate((mdir, mdir24)):
        refused = str(tmp_path / ("refused%d" % k))
        with pytest.raises(SystemExit):
            compress.run(model, small, refused, 0, 2, None, "abs", [0.0], True, False, True)
        assert "ERROR:Image size is out of scope for this model." in capsys.readouterr().out
        assert not os.path.exists(refused)


# ------------------------------------------------------------------------------------------ edges of the accepted space
def _refused(c, stack, rstack, status, words, prepare=None):
    from tezip_amd import _lib
    from tezip_amd.prednet import PredNetConfig
    cfg = PredNetConfig(stack_sizes=stack, R_stack_sizes=rstack)
    with pytest.raises(_lib.TezipError) as e:
        c.load_model(cfg, cfg.init_weights(seed=1))
        if prepare:
            c.prepare(*prepare)
    assert e.value.status == status and words in str(e.value), (stack, rstack, str(e.value))


@pytest.mark.parametrize("stack,rstack,status,words,prepare", [
    ((3, 24), None, TZ_ERR_UNSUPPORTED, "stack_sizes[1] must be a multiple of 16", None),
    ((3, 16), (5, 16), TZ_ERR_UNSUPPORTED, "R_stack_sizes[0] must be a multiple of 16 or <= 4", None),
    ((3, 16), (3, 15), TZ_ERR_UNSUPPORTED, "R_stack_sizes[1] must be a multiple of 16 or <= 4", None),
    ((3,) + (16,) * 8, None, TZ_ERR_INVALID, "bad model description", None),
    ((1, 16), None, TZ_ERR_UNSUPPORTED, "stack_sizes[0] must be 3", None),
    ((3, 16, 16, 16, 16), None, TZ_ERR_INVALID, "Image size is out of scope for this model", (24, 40)),
], ids=["stack-24", "R-5", "R-15", "nine-levels", "stack0-1", "five-levels-24x40"])
def test_edges_of_the_accepted_space_are_refused_and_the_context_still_works(ctx, stack, rstack, status, words, prepare):
    _refused(ctx, stack, rstack, status, words, prepare)
    cfg = _load(ctx, "M1", 1)
    M.assert_same_bits(ctx.predict_next(M.frames(16, 24)[0][:1])[0], M.oracle("M1", 1)["pred"][0], "M1 after a refusal")
    assert cfg.nb_layers == 2
