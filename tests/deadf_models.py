"""Models and the restated rule for the dead-forget-gate tests (tests/test_deadf_oracle.py on the CPU, tests/test_gpu_deadf.py on
the GPU).  The LSTM update is c = f * c_prev + i * g (a multiplication, a multiplication, an addition); in this predictor c_prev is
the per-model constant C0_l, the cell state after the t = 0 pass.  Where every word of C0_l is +0 the forget gate reaches no
result (tz_prednet.hip measure_deadf).  Here: the models the tests run, C0_l in numpy float32 (oracle/prednet_np.py's step
from the zero state) and the numpy restatement of the t = 1 gates, for counting products i * g that are -0."""
import functools

import numpy as np

from tezip_amd.prednet import PredNetConfig

DEFAULT = ((3, 48, 96, 192), None)
M9 = ((3, 80, 128), None)               # tests/model_space.py M9: five and eight column blocks of gates
BORDER_W = np.float32(0.5)              # a power of two: w * v - w * v is exactly +0 in every evaluation order, fused or not


def spec(kind, hp, wp, batch, shape=DEFAULT, seed=123):
    """A job: `batch` windows and one frame more than fits a batch, so that the last call is a batch of one (whose taps the
    library holds)."""
    return (kind, shape, hp, wp, batch, 3 if batch == 1 else batch + 1, int(seed))


def overwrite_forget_gate(cfg, w, seed):
    """Every forget-gate kernel and bias replaced by other finite random values (in place)."""
    names = [nm for nm, _ in cfg.weight_shapes()]
    rng = np.random.default_rng(seed)
    for l in range(cfg.nb_layers):
        for part in ("kernel", "bias"):
            a = w[names.index("f%d/%s" % (l, part))]
            new = rng.uniform(-0.3, 0.3, a.shape).astype(np.float32)
            assert np.isfinite(new).all() and not np.array_equal(new, a)
            a[:] = new


def model(sp):
    """(config, weights, frames) of a job.  Kinds:
    zero       Keras' default initialisation: zero biases (the bench's model)
    bias       bias_scale 0.1
    zero_f / bias_f   the same with every forget-gate weight overwritten
    mixed      zero biases except the c-gate bias of level 1
    border     top level: c-gate bias 0.3 (r0 there is one non-zero value everywhere); the level below: zero biases, c-gate weights
               on the upsampled channels zero except tap (1, 0) = +w and (1, 2) = -w on one channel
    inf_f      zero biases, one +inf in the forget gate of level 2 (on a channel of E_2, which the t = 0 pass does not read)
    D19 / D13  tests/regimes.py (zero biases, every weight times a gain that takes the sums subnormal); the seed slot holds
               the gain's exponent in tenths: gain = 10 ** (-seed / 10), 0 = the regime's own"""
    kind, (stack, rstack), hp, wp, _, n, seed = sp
    cfg = PredNetConfig(stack_sizes=stack, R_stack_sizes=rstack)
    names = [nm for nm, _ in cfg.weight_shapes()]
    L, st, rs = cfg.nb_layers, cfg.stack_sizes, cfg.R_stack_sizes
    if kind in ("D19", "D13"):
        import regimes
        cfg, w = regimes.model(kind, stack, rstack, gain=None if seed == 0 else 10.0 ** (-seed / 10.0))
    elif kind in ("bias", "bias_f"):
        w = cfg.init_weights(seed=seed, bias_scale=0.1)
    else:
        w = cfg.init_weights(seed=seed)
    if kind in ("zero_f", "bias_f"):
        overwrite_forget_gate(cfg, w, seed + 7)
    if kind == "mixed":
        w[names.index("c1/bias")][:] = np.random.default_rng(seed + 1).uniform(0.05, 0.2, rs[1]).astype(np.float32)
    if kind == "border":
        top = L - 1
        w[names.index("c%d/bias" % top)][:] = np.float32(0.3)
        k = w[names.index("c%d/kernel" % (top - 1))]
        up0 = rs[top - 1] + 2 * st[top - 1]                          # first upsampled input channel
        k[:, :, up0:, :] = 0.0
        k[1, 0, up0 + 5, :] = BORDER_W
        k[1, 2, up0 + 5, :] = -BORDER_W
    if kind == "inf_f":
        w[names.index("f2/kernel")][1, 1, rs[2] + 5, 7] = np.inf
    frames = np.random.default_rng(hp * 31 + wp).integers(0, 256, (n, hp, wp, 3)).astype(np.float32) / np.float32(255)
    return cfg, w, frames


def _zero_state(cfg, hp, wp):
    L = cfg.nb_layers
    r = [np.zeros((hp >> l, wp >> l, cfg.R_stack_sizes[l]), np.float32) for l in range(L)]
    e = [np.zeros((hp >> l, wp >> l, 2 * cfg.stack_sizes[l]), np.float32) for l in range(L)]
    return r, [z.copy() for z in r], e


@functools.lru_cache(maxsize=None)
def c0_numpy(sp):
    """C0_l of every level in numpy float32: the cell state after the t = 0 step from the zero state (it does not depend on the
    frame: the top-down pass runs before the frame is looked at)."""
    from oracle import prednet_np as P
    cfg, w, _ = model(sp)
    hp, wp = sp[2], sp[3]
    r, c, e = _zero_state(cfg, hp, wp)
    _, _, c0, _ = P.step(P.split_weights(w, cfg.nb_layers), cfg.nb_layers, np.zeros((hp, wp, 3), np.float32), r, c, e)
    for a in c0:
        a.setflags(write=False)
    return c0


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def c0_is_plus_zero(sp):
    """{level: every word of C0_l is 0x00000000}, levels >= 1, by the rule of measure_deadf on the numpy arrays; a plane that is
    not all +0 must be so by a margin numpy's rounding (~1e-6) cannot cross."""
    out = {}
    for l, c in enumerate(c0_numpy(sp)):
        if l == 0:
            continue
        out[l] = bool((bits(c) == 0).all())
        if not out[l]:
            assert float(np.abs(c).max()) > 1e-4, (l, float(np.abs(c).max()))
    return out


def negative_zero_products(sp):
    """{level: number of elements whose product i * g of the t = 1 gates is -0}, restated in numpy float32 for the LAST frame of
    the job (every prediction is a two-step run from the zero state)."""
    from oracle import prednet_np as P
    cfg, w, frames = model(sp)
    L, hp, wp = cfg.nb_layers, sp[2], sp[3]
    sw = P.split_weights(w, L)
    r, c, e = _zero_state(cfg, hp, wp)
    _, r0, c0, e0 = P.step(sw, L, frames[-1], r, c, e)
    counts, r_up = {}, None
    for l in reversed(range(L)):
        x = np.concatenate([r0[l], e0[l]] + ([r_up] if l < L - 1 else []), axis=-1)
        i, f, o = (P.hard_sigmoid(P.conv_same(x, *sw[k][l])) for k in "ifo")
        g = np.tanh(P.conv_same(x, *sw["c"][l])).astype(np.float32)
        t2 = (i * g).astype(np.float32)
        counts[l] = int((bits(t2) == 0x80000000).sum())
        cl = (f * c0[l]).astype(np.float32) + t2
        r_up = P.upsample((o * np.tanh(cl).astype(np.float32)).astype(np.float32))
    return counts
