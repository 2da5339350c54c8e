"""Level 0 on the vector ALU (-m gpu): k_l0_gates (tezip_amd/csrc/tz_l0_kernels.hip.h) against k_conv16b, k_conv3x3 and the C
oracle.  The new kernel walks the same fmaf chains as the matrix-core kernels -- pack_conv's slot order, pad terms included --
so every comparison is of BIT PATTERNS.  (A_0 keeps k_conv16b -- its vector-ALU form was not faster, EXPERIMENTS.md -- and the
log says so; E_1, which it writes from the new kernel's R1[0] one step on, is compared all the same.)

One job (tests/deadhalf_jobs.py: its steps, its names, its comparison) = three chained predictor steps from float frames
(tz_predict_next: k_err0 forms E_0 from float frames) with the taps of every level -- E_1 and R1[0] among them -- after the
first and after the third, then a rollout of three-frame windows from u8 key frames (k_err0 from u8; from its second step on a
window takes E_0 from the e0_out epilogue of k_conv_small) and the taps behind it.  Every case runs the job as
  (a) the new kernel where it is taken, (b) TEZIP_L0VALU=0 on a fresh model in the same process, (c) tz_set_conv_impl(0), (d) the C oracle
and reads what was chosen from the TEZIP_L0VALU_LOG=1 lines (with the TEZIP_DEAD0_LOG / TEZIP_DEADHALF_LOG lines beside them)."""
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

pytestmark = pytest.mark.gpu

ENV = J.ENV + ("TEZIP_L0VALU", "TEZIP_L0VALU_LOG")
L0_LINE = re.compile(r"\[tezip\] level 0 (A|gates): (k_l0_gates|k_conv16b)(?: \(vector ALU\))?"
                     r"(?:, forget-gate columns left out: (yes|no))?(?: \((.*)\))?$")
DEAD0_LINE = re.compile(r"\[tezip\] dead level 0, (A|gates): .* its k-step left out: (yes|no)")
HALF_LINE = re.compile(r"\[tezip\] dead half, level (\d): Ahat0 \+-0 over the whole plane: (yes|no)")


def _neg_zero_model(seed):
    """The zero-bias model with every level-0 bias -0 and every level-0 weight that multiplies a value that can be +0 -- R_0's own
    rows (r0_0 is +0 for this model, so G0_0 = fmaf(+0, w, -0) stays -0), the negative half of E_0 (+0 under a black pixel and
    outside the image) -- negative: those products are -0, and a chain that started from -0 sits at -0 when the first pad term
    arrives.  (The positive half is dead for this model and is left out.)"""
    cfg, w = D.model(D.spec("zero", 16, 16, 1, seed=seed))
    names = [nm for nm, _ in cfg.weight_shapes()]
    st0, r0 = cfg.stack_sizes[0], cfg.R_stack_sizes[0]
    for nm in ["a0/bias"] + ["%s0/bias" % g for g in "cfio"]:
        w[names.index(nm)][:] = np.float32(-0.0)
    k = w[names.index("a0/kernel")]
    k[:, :, st0:2 * st0, :] = -np.abs(k[:, :, st0:2 * st0, :]) - np.float32(1e-3)
    for g in "cfio":
        k = w[names.index("%s0/kernel" % g)]
        k[:, :, :r0, :] = -np.abs(k[:, :, :r0, :]) - np.float32(1e-3)
        k[:, :, r0 + st0:r0 + 2 * st0, :] = -np.abs(k[:, :, r0 + st0:r0 + 2 * st0, :]) - np.float32(1e-3)
    return cfg, w


def _inf_model(where, seed):
    """The zero-bias model with ONE +inf: 'forget' on a forget-gate weight of level 0 (on a row of R_1), 'e0' on a row of A_0
    that multiplies the dead positive half of E_0 (dead0_models: zero+inf)."""
    if where == "e0":
        return D.model(D.spec("zero+inf", 16, 16, 1, seed=seed))
    cfg, w = D.model(D.spec("zero", 16, 16, 1, seed=seed))
    names = [nm for nm, _ in cfg.weight_shapes()]
    w[names.index("f0/kernel")][1, 1, -1, 0] = np.inf
    return cfg, w


MODELS = {
    "zero": lambda seed: D.model(D.spec("zero", 16, 16, 1, seed=seed)),
    "bias": lambda seed: D.model(D.spec("bias", 16, 16, 1, seed=seed)),
    "zero-r0=1": lambda seed: D.model(D.spec("zero", 16, 16, 1, shape=D.R1, seed=seed)),
    "zero-3x16x32": lambda seed: D.model(D.spec("zero", 16, 16, 1, shape=D.SMALL, seed=seed)),
    "negzero": _neg_zero_model,
    "inf-forget": functools.partial(_inf_model, "forget"),
    "inf-e0": functools.partial(_inf_model, "e0"),
}


def job(kind, hp, wp, batch, contract=2, seed=123):
    return (kind, None, hp, wp, batch, seed, contract)   # (positions 2..4 as deadhalf_jobs reads them)


def run(jb, impl=1, **env):
    """The job in a context of its own, prepared with `env` set (the switches are read per prepare)."""
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
    """deadhalf_jobs.oracle for the models of this file and either contract: computed once per job, shared, never written to."""
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


def _log(stderr):
    rows, dead0, half = {}, {}, {}
    for ln in stderr.splitlines():
        m = L0_LINE.search(ln)
        if m:
            rows[m[1]] = dict(kernel=m[2], forget_out=m[3], why=m[4] or "")
        m = DEAD0_LINE.search(ln)
        if m:
            dead0[m[1]] = m[2] == "yes"
        m = HALF_LINE.search(ln)
        if m:
            half[int(m[1])] = m[2] == "yes"
    assert set(rows) == {"A", "gates"}, stderr[-2000:]
    return rows, dead0, half


def check(jb, capfd, with_oracle=True):
    """(a) = (b) = (c) [= (d)] in every bit of every prediction and tap; returns (a) and what the log lines said."""
    cfg = MODELS[jb[0]](jb[5])[0]
    capfd.readouterr()
    new = run(jb, TEZIP_L0VALU_LOG=1, TEZIP_DEAD0_LOG=1, TEZIP_DEADHALF_LOG=1)
    rows, dead0, half = _log(capfd.readouterr().err)
    old = run(jb, TEZIP_L0VALU=0, TEZIP_L0VALU_LOG=1)
    off = _log(capfd.readouterr().err)[0]
    assert off["A"]["kernel"] == off["gates"]["kernel"] == "k_conv16b" and "TEZIP_L0VALU=0" in off["gates"]["why"], off
    J.same_bits(new, old, "against TEZIP_L0VALU=0", cfg)
    gen = run(jb, impl=0)
    assert "level 0" not in capfd.readouterr().err            # nothing is printed unless asked
    J.same_bits(new, gen, "against tz_set_conv_impl(0)", cfg)
    if with_oracle:
        J.same_bits(new, oracle(jb), "against the C oracle", cfg, rollout_taps=False)
    for name, row in sorted(rows.items()):
        print("%s: %r  dead0 %r  dead half %r" % (name, row, dead0.get(name), half))
    # E_1 and R1[0] by name (same_bits covered them): the outputs of the two launches
    for k in ("e1", "r0", "ae1", "ar0", "qe1", "qr0"):
        assert new[k].size > 0, k
    return new, rows, dead0, half


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


VALU = {"A": "k_conv16b", "gates": "k_l0_gates"}


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("hp,wp", [(16, 16), (24, 40), (64, 64)])
def test_zero_bias_reference_model(hp, wp, batch, capfd):
    """The bench's model.  16 x 16: half a 32-pixel gate tile; 24 x 40: tiles cut by the border in both directions, odd block
    counts; 64 x 64: four gate tiles.  Everything that can be left out is: the positive half of E_0, the dead half of E_1's
    writer, the forget gate (9 of 12 columns); the log lines say so."""
    new, rows, dead0, half = check(job("zero", hp, wp, batch), capfd)
    assert {k: r["kernel"] for k, r in rows.items()} == VALU, rows
    assert rows["gates"]["forget_out"] == "yes" and "9 of 12" in rows["gates"]["why"], rows
    assert dead0 == {"A": True, "gates": True} and half[0] and half[1], (dead0, half)
    assert np.abs(new["r0"]).max() > 0 and np.abs(new["e1"]).max() > 0 and np.abs(new["p3"]).max() > 0
    assert (~new["key"]).sum() == batch * (J.WIN - 1)


def test_zero_bias_reference_model_under_the_first_contract(capfd):
    """Level 0 is TZ-PA1 under either contract; under TZ-PA1 the levels above run k_conv16 / k_convlat at this size."""
    _, rows, _, _ = check(job("zero", 24, 40, 3, contract=1), capfd)
    assert {k: r["kernel"] for k, r in rows.items()} == VALU, rows


@pytest.mark.parametrize("hp,wp,batch,seed", [(24, 40, 3, 123), (64, 64, 1, 31)])
def test_biased_model_nothing_dead(hp, wp, batch, seed, capfd):
    """bias_scale 0.1: both quads of E_0 are live and C0_0 is not zero.  With anything live k_conv16b measured faster than the
    12-column, two-quad form of the new kernel, so the gates keep it -- the log says why -- and TEZIP_L0VALU changes nothing."""
    new, rows, dead0, half = check(job("bias", hp, wp, batch, seed=seed), capfd)
    assert rows["A"]["kernel"] == rows["gates"]["kernel"] == "k_conv16b" and "positive half of E_0 is walked" in rows["gates"]["why"], rows
    assert dead0 == {"A": False, "gates": False} and not half[0] and not half[1], (dead0, half)
    c = new["e1"].shape[-1] // 2
    assert np.abs(new["e1"][..., :c]).max() > 0 and np.abs(new["e1"][..., c:]).max() > 0


@pytest.mark.parametrize("kind,hp,wp,batch,valu", [("zero", 24, 40, 1, True), ("zero-r0=1", 24, 40, 3, False), ("zero-r0=1", 16, 16, 1, False),
                                                   ("zero-3x16x32", 24, 40, 1, True), ("zero-3x16x32", 64, 64, 3, True)],
                         ids=["3x48x96x192-24x40x1", "r0=1-24x40x3", "r0=1-16x16x1", "3x16x32-24x40x1", "3x16x32-64x64x3"])
def test_other_model_shapes(kind, hp, wp, batch, valu, capfd):
    """The model shapes of test_gpu_dead0.py::test_other_model_shapes: an R_1 of one 16-channel block (3, 16, 32) takes the new
    kernel; one-channel gates (R_0 = 1) are not the reference shape and keep k_conv16b -- the log shows it."""
    _, rows, _, _ = check(job(kind, hp, wp, batch, seed=77), capfd)
    if valu:
        assert {k: r["kernel"] for k, r in rows.items()} == VALU, rows
    else:
        assert rows["A"]["kernel"] == rows["gates"]["kernel"] == "k_conv16b" and "not the reference shape" in rows["gates"]["why"], rows


def test_the_sign_of_zero(capfd):
    """Chains that start from -0 and meet products of -0 until a pad term arrives (_neg_zero_model).  Restated on the frames:
    under a black pixel whose whole 3 x 3 neighbourhood is black or outside the image every product of the E_0 part is -0.
    Measured while writing this: the sign of a level-0 chain's zero does not reach any output of this network -- relu takes it
    from A_0, the hard sigmoids from i, f and o, and c = f * c_prev + i * g is -0 only with f * c_prev = -0, which C0_0 (+0 or a
    value that keeps G0_0's g column away from zero) never gives -- so this case holds the kernel to the same bits as the other
    three forms, as the rest do; that the pad terms are in the instruction stream is read from the disassembly."""
    jb = job("negzero", 24, 40, 3)
    cfg, w = MODELS["negzero"](jb[5])
    names = [nm for nm, _ in cfg.weight_shapes()]
    assert all(np.signbit(w[names.index(nm)]).all() for nm in ["a0/bias"] + ["%s0/bias" % g for g in "cfio"])
    x = D.frames_u8(3, 24, 40).max(axis=-1)
    pad = np.pad(x, ((0, 0), (1, 1), (1, 1)))
    black = sum(pad[:, dy:dy + 24, dx:dx + 40].astype(np.int32) for dy in range(3) for dx in range(3)) == 0
    print("pixels whose E_0 products are all -0:", int(black.sum()))
    assert black.sum() >= 300
    new, rows, dead0, _ = check(jb, capfd)
    assert {k: r["kernel"] for k, r in rows.items()} == VALU and dead0 == {"A": True, "gates": True}, (rows, dead0)
    assert rows["gates"]["forget_out"] == "yes", rows


@pytest.mark.parametrize("kind", ["inf-forget", "inf-e0"])
def test_a_non_finite_weight_keeps_what_it_multiplies(kind, capfd):
    """One +inf on a forget-gate weight: the forget columns are needed (f may be NaN), and the gates keep k_conv16b with its four
    gates.  One +inf on a row of A_0 that multiplies the dead positive half: A_0 walks both k-steps (0 x inf is a NaN the chain
    must keep) while the gates, whose weights are finite, take the new kernel.  Compared with TEZIP_L0VALU=0 and k_conv3x3 (what
    the oracle's libm makes of a NaN is its business)."""
    _, rows, dead0, _ = check(job(kind, 24, 40, 1), capfd, with_oracle=False)
    if kind == "inf-forget":
        assert rows["gates"]["kernel"] == "k_conv16b" and "not finite" in rows["gates"]["why"], rows
        assert dead0 == {"A": True, "gates": True}, dead0
    else:
        assert {k: r["kernel"] for k, r in rows.items()} == VALU, rows
        assert rows["gates"]["forget_out"] == "yes" and dead0 == {"A": False, "gates": True}, (rows, dead0)
