"""Models, frames and the restated rule for the level-0 dead-half tests (tests/test_dead0_oracle.py on the CPU,
tests/test_gpu_dead0.py on the GPU).  E_0 = [relu(Ahat0_0 - x), relu(x - Ahat0_0)] with x a frame (>= +0): where the per-model
constant Ahat0_0 is +-0 over the whole plane, the positive half is +0 at every pixel of every frame, and k_conv16b leaves out
the k-step that multiplies it (tz_prednet.hip measure_dead)."""
import functools

import numpy as np

from tezip_amd.prednet import PredNetConfig

DEFAULT = ((3, 48, 96, 192), None)      # A_0 at three column tiles, gates of R_0 = 3
R1 = ((3, 64, 32), (1, 16, 32))         # one gray channel of R_0 (stack_sizes[0] itself must be 3: tz_model_load); A_0 at four tiles
SMALL = ((3, 16, 32), None)             # A_0 at one column tile
BORDER_W = np.float32(0.5)              # a power of two: w * v - w * v is exactly +0 in every evaluation order, fused or not


def spec(kind, hp, wp, batch, shape=DEFAULT, seed=123):
    return (kind, shape, hp, wp, batch, int(seed))


def pos_rows(cfg):
    """[(weight name, first input channel, count)]: every kernel row that multiplies the positive half of e_0."""
    st0, r0 = cfg.stack_sizes[0], cfg.R_stack_sizes[0]
    rows = [("a0/kernel", 0, st0)] if cfg.nb_layers > 1 else []
    return rows + [("%s0/kernel" % g, r0, st0) for g in "cfio"]


def overwrite_pos(cfg, w, how, seed=5):
    """Every weight that multiplies the positive half of e_0 replaced (in place): 'random' finite values, 'huge' +-1e30,
    'negative' all negative; 'inf' puts ONE +inf there and leaves the rest."""
    names = [nm for nm, _ in cfg.weight_shapes()]
    rng = np.random.default_rng(seed)
    for nm, c0, n in pos_rows(cfg):
        k = w[names.index(nm)]
        part = k[:, :, c0:c0 + n, :]
        if how == "random":
            new = rng.uniform(-0.7, 0.7, part.shape)
        elif how == "huge":
            new = rng.choice([-1e30, 1e30], part.shape)
        elif how == "negative":
            new = -rng.uniform(0.01, 2.0, part.shape)
        elif how == "inf":
            if nm == pos_rows(cfg)[0][0]:
                part[1, 1, n - 1, 0] = np.inf
            continue
        else:
            raise ValueError(how)
        new = new.astype(np.float32)
        assert np.isfinite(new).all() and not np.array_equal(new, part)
        part[...] = new


def model(sp):
    """(config, weights) of a job.  Kinds:
    zero       Keras' default initialisation: zero biases (the bench's model): Ahat0_0 = +0 everywhere
    bias       bias_scale 0.1: Ahat0_0 is not zero
    border     zero biases except the c-gate bias of level 0 (r0_0 is then one positive value everywhere: the levels above give
               exactly 0), and an Ahat_0 kernel that is zero but for tap (1, 0) = +w and (1, 2) = -w on one channel: Ahat0_0 is
               +0 inside and on the left border (relu of -w v) and w v > 0 on the right border column, where the padding takes
               the -w tap away
    zero+HOW / border+HOW   the same with overwrite_pos(HOW)"""
    kind, (stack, rstack) = sp[0], sp[1]
    seed = sp[5]
    base, _, how = kind.partition("+")
    cfg = PredNetConfig(stack_sizes=stack, R_stack_sizes=rstack)
    names = [nm for nm, _ in cfg.weight_shapes()]
    w = cfg.init_weights(seed=seed, bias_scale=0.1 if base == "bias" else 0.0)
    if base == "border":
        w[names.index("c0/bias")][:] = np.float32(0.3)
        k = w[names.index("ahat0/kernel")]
        k[...] = 0.0
        k[1, 0, 0, :] = BORDER_W
        k[1, 2, 0, :] = -BORDER_W
    elif base not in ("zero", "bias"):
        raise ValueError(kind)
    if how:
        overwrite_pos(cfg, w, how)
    return cfg, w


def frames_u8(n, h, w, seed=0):
    """n frames of noise with runs of 0 and 255: black and white blocks and stripes, a black and a white stretch of the right
    border column; frame 1 all black (n >= 3) and frame 2 all white (n >= 4): the last frame is always one of the mixed ones."""
    rng = np.random.default_rng(1000 * h + w + seed)
    f = rng.integers(0, 256, (n, h, w, 3)).astype(np.uint8)
    f[:, : h // 4, : w // 2] = 0
    f[:, h // 2: h // 2 + 3, :] = 255
    f[:, :, w // 3: w // 3 + 2, 1] = 0
    f[:, h // 4: h // 2, -1] = 0
    f[:, h // 2: 3 * h // 4, -1] = 255
    f[:, -1, : w // 2] = 0
    if n >= 3:
        f[1] = 0
    if n >= 4:
        f[2] = 255
    return f


def as_float(frames):
    return frames.astype(np.float32) / np.float32(255)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def ahat0(sp):
    """Ahat0_0 of the C oracle (the prediction before any frame), read-only."""
    from oracle import coracle
    cfg, w = model(sp)
    a = coracle.CPredNet(w, cfg.stack_sizes, cfg.R_stack_sizes, sp[2], sp[3]).c0()
    a.setflags(write=False)
    return a


def positive_half_is_dead(sp):
    """The rule of measure_dead restated on the oracle's Ahat0_0: no magnitude bit anywhere on the plane, border included; a
    plane that is not dead must be so by a margin no rounding crosses."""
    a = ahat0(sp)
    dead = bool(((bits(a) & 0x7FFFFFFF) == 0).all())
    if not dead:
        assert float(np.abs(a).max()) > 1e-3, float(np.abs(a).max())
    return dead
