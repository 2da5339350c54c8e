"""The models of tests/model_space.py on the CPU.  tests/test_gpu_model_space.py holds the HIP predictor to the C oracle bit
for bit on model shapes no other test runs; here, first, that the list really produces every dispatch value the other tests
never do (so the file keeps saying why it exists), that the C oracle computes the right function on those models (against the
independent numpy restatement oracle/prednet_np.py), and that the oracle's own rule for which convolutions TZ-PA2 evaluates as
Winograd chains is the one model_space.classes restates.

`python tests/test_model_space.py` prints the table of DESIGN.md §3."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import model_space as M  # noqa: E402

IDS = [m[0] for m in M.MODELS]


# ------------------------------------------------------------------------------------------------------------- coverage
def _plain(nt):
    return lambda c, cfg: c["ncb"] if c["kind"] in ("a", "ahat") and c["NT"] == nt else None


# quantity -> (what a convolution contributes (None: nothing), the values no other -m gpu test produces)
NEVER_RUN = {
    "ncb of an NT = 1 A / Ahat convolution": (_plain(1), {5, 7, 10}),
    "ncb of an NT = 3 A / Ahat convolution": (_plain(3), {3, 5}),
    "ncb of an NT = 4 A / Ahat convolution": (_plain(4), {2, 4, 6}),
    "gate column blocks (R / 16)": (lambda c, cfg: c["ncb"] if c["kind"] == "gates" and not c["packed"] else None,
                                    {5, 7, 8, 10, 15, 16, 24}),
    "R of packed gates": (lambda c, cfg: cfg.R_stack_sizes[c["level"]] if c["packed"] else None, {1, 2}),
    "level of packed gates": (lambda c, cfg: c["level"] if c["packed"] else None, {1, 2, 4}),
    "levels": (lambda c, cfg: cfg.nb_layers, {5, 6, 7, 8}),
    "input channels of a gate convolution": (lambda c, cfg: c["kdepth"] if c["kind"] == "gates" and c["kdepth"] > 576 else None, {1152}),
    # an R <= 4 at level >= 1: packed gates over 16-multiple E sources, Ahat_l from <= 4 channels, and the level below
    # upsampling <= 4 channels (FULLK = false with an upsampled source)
    "situations of an R <= 4 above level 0": (
        lambda c, cfg: ("packed gates, 16-multiple E" if c["kind"] == "gates" and c["packed"] and c["level"] >= 1 and c["srcs"][0] % 16 == 0 else
                        "Ahat from <= 4 channels" if c["kind"] == "ahat" and c["level"] >= 1 and c["srcs"][0] <= 4 else
                        "upsampled source of <= 4 channels" if c["kind"] == "gates" and c["ups"] and c["srcs"][1] <= 4 else None),
        {"packed gates, 16-multiple E", "Ahat from <= 4 channels", "upsampled source of <= 4 channels"}),
}


def _produced(what, models):
    get = NEVER_RUN[what][0]
    out = set()
    for stack, rstack in models:
        cfg = M.config((None, stack, rstack))
        out |= {get(c, cfg) for c in M.classes(cfg).values()}
    return out - {None}


@pytest.mark.parametrize("what", sorted(NEVER_RUN))
def test_the_models_produce_every_value_the_other_tests_never_run(what):
    want = NEVER_RUN[what][1]
    have = _produced(what, [(m[1], m[2]) for m in M.MODELS])
    assert want <= have, (what, sorted(want - have, key=str))
    others = _produced(what, M.OTHER_MODELS)
    assert not (want & others), (what, sorted(want & others, key=str))


def test_an_a_convolution_off_k_wino_between_k_wino_neighbours():
    """At level >= 1 under TZ-PA2: A_l of 80 / 112 / 160 columns runs TZ-PA1 chains while the gates of its level run k_wino."""
    found = set()
    for m in M.MODELS:
        cl = M.classes(M.config(m))
        for name, c in cl.items():
            if c["kind"] == "a" and c["level"] >= 1 and not c["wino_ok"] and cl["gates%d" % c["level"]]["wino_ok"]:
                found.add(c["ncb"])
    assert {5, 7, 10} <= found, found


def test_every_model_is_one_tz_model_load_and_prepare_accept():
    for mid, stack, rstack, hp, wp in M.MODELS:
        cfg = M.config((mid, stack, rstack))
        L = cfg.nb_layers
        assert 1 <= L <= 8 and cfg.stack_sizes[0] == 3 and all(s % 16 == 0 for s in cfg.stack_sizes[1:]), mid
        assert all(r % 16 == 0 or r <= 4 for r in cfg.R_stack_sizes), mid
        assert hp % 8 == 0 and wp % 8 == 0 and hp % (1 << (L - 1)) == 0 and wp % (1 << (L - 1)) == 0, mid
    hp, wp = M.BY_ID[M.DEFAULT_CONTRACT_MODEL][3:]
    assert hp * wp >= 256 * 256        # effective_contract: TZ-PA2 from here on


def test_the_family_rules_on_the_reference_model():
    """The restated rules give what tests/test_gpu_regimes.py asserts on (3, 48, 96, 192): five k_wino launches a step
    (gates of levels 1 to 3, A_1, A_2), levels 1 and 2 can split (seven launches), nothing on the general kernel."""
    cfg = M.config((None, (3, 48, 96, 192), None))
    assert M.wino_launches(cfg) == 5 and M.epart_can_split(cfg) == [1, 2]
    fam = M.families(cfg, 2)
    assert sorted(fam) == ["conv16b_level0", "conv_small_valu", "wino_pa2"], fam
    assert sorted(M.families(cfg, 1)) == ["conv16b_level0", "conv_small_valu", "lds"]


# ------------------------------------------------------------------------------------ the oracle against prednet_np
TOL = 2e-5      # the tolerance of tests/test_gpu_parity.py and tests/test_oracle_prednet.py: float32 summation order


def _deviation(mid):
    """max |C oracle - prednet_np| over the t = 0 prediction and the prediction of the first random frame, both contracts"""
    from oracle import prednet_np
    m = M.BY_ID[mid]
    cfg = M.config(m)
    f = M.frames(m[3], m[4])[0][0]
    ref = prednet_np.predict(M.weights(mid), cfg.stack_sizes, cfg.R_stack_sizes, np.stack([f, np.zeros_like(f)]))
    dev = 0.0
    for contract in (1, 2):
        got = M.oracle(mid, contract)
        assert all(np.isfinite(v).all() for v in got.values()), mid
        dev = max(dev, float(np.abs(got["t0"] - ref[0]).max()), float(np.abs(got["pred"][0] - ref[1]).max()))
    return dev


@pytest.mark.parametrize("mid", IDS)
def test_c_oracle_matches_numpy_restatement(mid):
    dev = _deviation(mid)
    print("%s: max |C oracle - prednet_np| = %.3g" % (mid, dev))
    assert dev <= TOL, dev


# ----------------------------------------------------------------------------------------------- TZ-PA1 against TZ-PA2
@pytest.mark.parametrize("mid", IDS)
def test_the_contracts_differ_exactly_where_a_convolution_is_wino_ok(mid):
    """The eligibility rule in a third place: the oracle's two outputs differ in bits exactly for the models where
    classes() reports a k_wino convolution; the constants (t = 0) are TZ-PA1 chains under both contracts."""
    cfg = M.config(M.BY_ID[mid])
    a, b = M.oracle(mid, 1), M.oracle(mid, 2)
    assert np.array_equal(a["t0"].view(np.uint32), b["t0"].view(np.uint32))
    differ = not np.array_equal(a["pred"].view(np.uint32), b["pred"].view(np.uint32))
    any_wino = any(c["wino_ok"] for c in M.classes(cfg).values())
    assert differ == any_wino, (mid, differ, any_wino)
    assert float(np.abs(a["pred"] - b["pred"]).max()) <= TOL
    # level by level, top-down: r of a level whose gates are not k_wino and whose inputs are the same bits is the same bits
    cl = M.classes(cfg)
    L = cfg.nb_layers
    e_same = [np.array_equal(a["e%d" % l].view(np.uint32), b["e%d" % l].view(np.uint32)) for l in range(L)]
    for l in range(1, L):      # e_l changes with the first k_wino A convolution below it, and not before
        assert e_same[l] == (not any(cl["a%d" % k]["wino_ok"] for k in range(l))), (mid, l, e_same)
    assert e_same[0]
    for l in range(L - 1, -1, -1):
        same = np.array_equal(a["r%d" % l].view(np.uint32), b["r%d" % l].view(np.uint32))
        changed_above = any(cl["gates%d" % k]["wino_ok"] for k in range(l, L)) or not all(e_same[l:])
        assert same == (not changed_above), (mid, l, same)


def test_there_is_a_model_with_no_k_wino_convolution_and_most_have_one():
    none = [m[0] for m in M.MODELS if not any(c["wino_ok"] for c in M.classes(M.config(m)).values())]
    assert none == ["M11"], none


# ------------------------------------------------------------------------------------------------------- DESIGN.md §3
def _table():
    print("| model | stack / R, frame | launch families TZ-PA1 | launch families TZ-PA2 | max abs(C oracle - numpy) |")
    print("|---|---|---|---|---|")
    for m in M.MODELS:
        cfg = M.config(m)
        fam = [", ".join("%s (%s)" % (k, " ".join(v)) for k, v in sorted(M.families(cfg, c).items())) for c in (1, 2)]
        print("| %s | %s / %s, %dx%d | %s | %s | %.2g |" % (m[0], "x".join(map(str, cfg.stack_sizes)), "x".join(map(str, cfg.R_stack_sizes)),
                                                         m[3], m[4], fam[0], fam[1], _deviation(m[0])))


if __name__ == "__main__":
    _table()
