"""k_l0_gates on pairs of pixels (-m gpu; tezip_amd/csrc/tz_l0_kernels.hip.h): a packed multiply-add is two pixels of one gate
column, the weight one half of a scalar register pair chosen by op_sel, and on a 32 x 32 tile where G0_0 is one row the start
values are scalar loads (ConvArgs::init_u, the consumer bit 8 of TEZIP_UNIFORM).  Every fmaf keeps its operands and its place
in its chain, so every comparison is of BIT PATTERNS, with the job, the references and the helpers of tests/test_gpu_l0valu.py:
  (a) the new kernel where it is taken, (b) TEZIP_L0VALU=0 (k_conv16b) on a fresh model in the same process,
  (c) tz_set_conv_impl(0) (k_conv3x3), (d) the C oracle
after one predictor step, after three chained steps and after a rollout of three-frame windows: the predictions, R1[0], E_1 and
every other tap that suite dumps.
Frame sizes: 32 x 32 is one gate tile, all border; 48 x 80 has partial tiles in both directions (and, for the uniform start
values, two whole tiles beside four partial ones); 64 x 64 is four whole tiles."""
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
import deadhalf_jobs as J  # noqa: E402
import test_gpu_l0valu as V  # noqa: E402

pytestmark = pytest.mark.gpu

WIDE = ((3, 32, 64, 128), None)   # R_1 of 32 channels: two 16-channel blocks, so the R_1 loop of the kernel runs twice
UNI_LINE = re.compile(r"\[tezip\] uniform constants, level 0 G0 \((\d+)x(\d+)\): .* one value: w (-?\d+),")
L0_UNIFORM_OFF = 7                # TEZIP_UNIFORM: every consumer but k_l0_gates' start values (bit 8)


def _gate_bias_model(seed):
    """Zero biases except on the level-0 i and o gate columns.  C0_0 = i * tanh(+0) is still +0 and so are R0_0 and Ahat0_0, so
    the gates still take k_l0_gates without the forget gate and without the positive half -- from a start row G0_0 that is not
    zero: the bias row, the same on the whole plane (fmaf(+0, w, b) = b under the padding as well)."""
    cfg, w = D.model(D.spec("zero", 16, 16, 1, seed=seed))
    names = [nm for nm, _ in cfg.weight_shapes()]
    rng = np.random.default_rng(seed)
    for nm in ("i0/bias", "o0/bias"):
        b = w[names.index(nm)]
        b[:] = rng.uniform(0.05, 0.4, b.shape).astype(np.float32) * np.float32(-1 if nm[0] == "o" else 1)
    return cfg, w


MODELS = {
    "zero": V.MODELS["zero"],
    "zero-3x32x64x128": lambda seed: D.model(D.spec("zero", 16, 16, 1, shape=WIDE, seed=seed)),
    "negzero": V.MODELS["negzero"],
    "gate-bias": _gate_bias_model,
}
SIZES = [(32, 32), (48, 80), (64, 64)]


def job(kind, hp, wp, batch, seed=123):
    return (kind, None, hp, wp, batch, seed, 2)   # (the tuple of test_gpu_l0valu.job)


def run(jb, impl=1, **env):
    """test_gpu_l0valu.run over the models of this file: the job in a context of its own, prepared with `env` set."""
    from tezip_amd import _lib
    cfg, w = MODELS[jb[0]](jb[5])
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    c = None
    try:
        c = _lib.Context(0)
        c.set_contract(jb[6])
        c.load_model(cfg, w)
        c.prepare(jb[2], jb[3], max_batch=jb[4])
        c.set_conv_impl(impl)
        return J._steps(c, cfg, jb)
    finally:
        if c is not None:
            c.close()
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@functools.lru_cache(maxsize=None)
def oracle(jb):
    """The C oracle's job (test_gpu_l0valu.oracle), computed once per job, shared, never written to."""
    from oracle import coracle
    from oracle import oracle as O
    cfg, w = MODELS[jb[0]](jb[5])
    hp, wp, batch = jb[2], jb[3], jb[4]
    net = coracle.CPredNet(w, cfg.stack_sizes, cfg.R_stack_sizes, hp, wp).set_contract(jb[6])
    x = D.as_float(D.frames_u8(batch, hp, wp))
    ref = {k: np.empty_like(x) for k in ("p1", "p2", "p3")}
    d1 = d3 = None
    for i in range(len(x)):
        ref["p1"][i], da = net.next(x[i], debug=True)
        ref["p2"][i] = net.next(ref["p1"][i])
        ref["p3"][i], db = net.next(ref["p2"][i], debug=True)
        if i == 0:
            d1, d3 = da, db
    for l in range(cfg.nb_layers):
        ref["e%d" % l], ref["r%d" % l], ref["ae%d" % l], ref["ar%d" % l] = d1["e"][l], d1["r"][l], d3["e"][l], d3["r"][l]

    class P:
        def c0(self, a, b):
            return net.c0()

        def next(self, f):
            return net.next(np.asarray(f, np.float32))

    u8 = D.frames_u8(batch * J.WIN, hp, wp, seed=7)
    ro = O.rollout(u8, 0, J.WIN, None, P())
    roll = np.zeros((len(u8), hp, wp, 3), np.float32)
    for start, preds in ro["groups"]:
        for i, p in enumerate(preds):
            roll[start + i] = p
    roll[ro["key"]] = 0
    ref["roll"], ref["key"] = roll, ro["key"]
    for v in ref.values():
        v.setflags(write=False)
    return ref


def check(jb, capfd, **env):
    """(a) = (b) = (c) = (d) in every bit of every prediction and tap, (a) prepared with `env`; returns (a), what the level-0
    log lines said and the ring of G0_0 that measure_uniform logged (None: not measured under this TEZIP_UNIFORM)."""
    cfg = MODELS[jb[0]](jb[5])[0]
    capfd.readouterr()
    new = run(jb, TEZIP_L0VALU_LOG=1, TEZIP_DEAD0_LOG=1, TEZIP_DEADHALF_LOG=1, TEZIP_UNIFORM_LOG=1, **env)
    err = capfd.readouterr().err
    rows, dead0, _ = V._log(err)
    ring = [int(m[3]) for m in map(UNI_LINE.search, err.splitlines()) if m and (int(m[1]), int(m[2])) == (jb[2], jb[3])]
    assert rows["gates"]["kernel"] == "k_l0_gates" and rows["gates"]["forget_out"] == "yes" and "9 of 12" in rows["gates"]["why"], rows
    assert rows["A"]["kernel"] == "k_conv16b" and dead0 == {"A": True, "gates": True}, (rows, dead0)
    old = run(jb, TEZIP_L0VALU=0, TEZIP_L0VALU_LOG=1)
    off = V._log(capfd.readouterr().err)[0]
    assert off["gates"]["kernel"] == "k_conv16b" and "TEZIP_L0VALU=0" in off["gates"]["why"], off
    J.same_bits(new, old, "against TEZIP_L0VALU=0", cfg)
    J.same_bits(new, run(jb, impl=0), "against tz_set_conv_impl(0)", cfg)
    J.same_bits(new, oracle(jb), "against the C oracle", cfg, rollout_taps=False)
    for k in ("e1", "r0", "ae1", "ar0", "qe1", "qr0"):   # E_1 and R1[0] by name (same_bits covered them)
        assert new[k].size > 0, k
    return new, rows, (ring[0] if ring else None)


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in V.ENV + ("TEZIP_UNIFORM_LOG",):
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("hp,wp", SIZES)
def test_zero_bias_reference_model(hp, wp, batch, capfd):
    """The bench's model, (3, 48, 96, 192): three blocks of R_1.  G0_0 is +0 on the whole plane, ring 0: every whole tile
    takes its start values from the row."""
    new, _, ring = check(job("zero", hp, wp, batch), capfd)
    assert ring == 0, ring
    assert (~new["key"]).sum() == batch * (J.WIN - 1)


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("hp,wp", SIZES)
def test_two_blocks_of_r1(hp, wp, batch, capfd):
    """A zero-bias (3, 32, 64, 128) model: the R_1 loop runs twice, the second block staged while the first is multiplied."""
    check(job("zero-3x32x64x128", hp, wp, batch, seed=77), capfd)


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("hp,wp", SIZES)
def test_the_sign_of_zero(hp, wp, batch, capfd):
    """test_gpu_l0valu.py::test_the_sign_of_zero's construction: chains that start from -0 and meet products of -0 until a pad
    term arrives.  A pad addition dropped or folded, per pixel of a pair, would leave a -0 where the other forms hold +0 -- as
    far as that reaches an output (that docstring)."""
    check(job("negzero", hp, wp, batch), capfd)


@pytest.mark.parametrize("uniform", ["on", "off"])
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("hp,wp", SIZES)
def test_a_start_row_that_is_not_zero(hp, wp, batch, uniform, capfd):
    """Non-zero biases on the level-0 i and o gate columns: still k_l0_gates without forget gate and positive half (read from the
    log line), from a uniform start row that is not zero.  With the kernel's uniform consumer on (scalar loads of the row on
    whole tiles, per-pixel loads on the partial ones) and off (TEZIP_UNIFORM=7: per-pixel loads everywhere), the same bits as
    all three references."""
    env = {} if uniform == "on" else {"TEZIP_UNIFORM": L0_UNIFORM_OFF}
    jb = job("gate-bias", hp, wp, batch, seed=31)
    cfg, w = MODELS["gate-bias"](jb[5])
    names = [nm for nm, _ in cfg.weight_shapes()]
    assert all((w[names.index(nm)] != 0).all() for nm in ("i0/bias", "o0/bias"))
    new, _, ring = check(jb, capfd, **env)
    assert ring == 0, ring                         # measured, not assumed: one row on the whole plane
    assert np.abs(new["r0"]).max() > 0
