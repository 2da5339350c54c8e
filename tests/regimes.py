"""Value regimes the glorot-initialised models of the other tests never reach: weights scaled until the gates
saturate (S4, S16: the clamp of Ahat_0 at pixel_max, tanh's middle branch, both clips of the hard sigmoid) or until sums
go subnormal (D19, D13).  Shared by tests/test_regimes.py (CPU: the C oracle is right there and every case really is in
its regime) and tests/test_gpu_regimes.py (the HIP predictor against the C oracle, bit for bit): the models, the case
list, the frames, the oracle's results (computed once per case and contract, never written to) and the comparison."""
import functools

import numpy as np

from tezip_amd.prednet import PredNetConfig

SEED = 11
FULL_STACK = (3, 48, 96, 192)
TINY = np.finfo(np.float32).tiny

# name -> (bias_scale of init_weights, gain): every weight array, biases included, times np.float32(gain)
REGIMES = {"S4": (0.3, 4.0), "S16": (0.3, 16.0), "D19": (0.0, 1e-19), "D13": (0.0, 3e-13)}

# (stack_sizes, R_stack_sizes, hp, wp): the reference model at four frame sizes, then the shapes that select the other
# kernels (SHAPES of tests/test_gpu_parity.py)
SHAPES = [
    (FULL_STACK, None, 8, 8),         # one-pixel top level
    (FULL_STACK, None, 8, 40),        # one-tile strip
    (FULL_STACK, None, 24, 40),       # odd top level, ragged tiles
    (FULL_STACK, None, 72, 88),       # interior and ragged tiles
    ((3, 16), None, 24, 40),
    ((3, 32, 64), (3, 48, 32), 40, 56),
    ((3, 64, 16), (4, 16, 64), 32, 48),
    ((3, 48, 96, 192), (16, 48, 96, 192), 32, 32),
    ((3,), (3,), 16, 24),
]

# A shape whose regime needs another gain than REGIMES names to meet its condition (conditions() below), and why.
# The subnormal regimes are named after the depth at which the reference model's sums go subnormal: a signal loses a
# factor `gain` per convolution, so a model with fewer levels never gets that far down with D13's gain.
GAIN_OVERRIDE = {
    # two levels and one level: nothing is below 1e-26 at gain 3e-13.  3e-20 puts the prediction (gain^2 * O(0.1)) near
    # 1e-40, where a float32 has 6 to 9 significant bits left: the other end of the subnormal range from D19's 1e-39
    ("D13", (3, 16), (3, 16)): 3e-20,
    ("D13", (3,), (3,)): 3e-20,
}


def scaled(weights, gain):
    return [a * np.float32(gain) for a in weights]


def config(stack, rstack):
    return PredNetConfig(stack_sizes=stack, R_stack_sizes=rstack)


def gain_of(regime, stack, rstack):
    cfg = config(stack, rstack)
    return GAIN_OVERRIDE.get((regime, cfg.stack_sizes, cfg.R_stack_sizes), REGIMES[regime][1])


def model(regime, stack=FULL_STACK, rstack=None, gain=None):
    """(config, weights) of a named regime; `gain` replaces the regime's own (gain 1 = what the other tests use)."""
    cfg = config(stack, rstack)
    g = gain_of(regime, stack, rstack) if gain is None else gain
    return cfg, scaled(cfg.init_weights(seed=SEED, bias_scale=REGIMES[regime][0]), g)


CASES = [(regime,) + shape for regime in REGIMES for shape in SHAPES]
# the saturated model through every dispatch path: the reference shape at 72x88 and 40x56
DISPATCH_CASES = [("S16", FULL_STACK, None, 72, 88), ("S16", FULL_STACK, None, 40, 56)]


def case_id(case):
    regime, stack, rstack, hp, wp = case
    return "%s-%s%s-%dx%d" % (regime, "x".join(map(str, stack)), "" if rstack is None else "-R" + "x".join(map(str, rstack)), hp, wp)


def frames(hp, wp):
    """(3 random frames, [all-zero, all-255]) as float32 / 255: constant frames are where the interior-tile shortcuts and
    the clamp meet."""
    rng = np.random.default_rng(1000 * hp + wp)
    rand = rng.integers(0, 256, (3, hp, wp, 3)).astype(np.float32) / np.float32(255)
    const = np.stack([np.zeros((hp, wp, 3), np.float32), np.full((hp, wp, 3), 255, np.float32) / np.float32(255)])
    return rand, const


@functools.lru_cache(maxsize=None)
def oracle(case, contract, gain=None):
    """What the C oracle computes for a case under a contract: the t = 0 prediction (`t0`; `c0` is a tap), the predictions of the three random frames, the e / r /
    c taps of the last of them, the predictions of the two constant frames, and the first prediction fed back."""
    from oracle import coracle
    regime, stack, rstack, hp, wp = case
    cfg, w = model(regime, stack, rstack, gain)
    net = coracle.CPredNet(w, cfg.stack_sizes, cfg.R_stack_sizes, hp, wp).set_contract(contract)
    rand, const = frames(hp, wp)
    out = {"t0": net.c0(), "pred": np.empty_like(rand)}
    out["pred"][0], out["pred"][1] = net.next(rand[0]), net.next(rand[1])
    out["pred"][2], taps = net.next(rand[2], debug=True)
    out["const"] = np.stack([net.next(f) for f in const])
    out["again"] = net.next(out["pred"][0])
    for k in "erc":
        for l in range(cfg.nb_layers):
            out["%s%d" % (k, l)] = taps[k][l]
    for v in out.values():
        v.setflags(write=False)
    return out


def taps_of(ref, levels):
    return {k: [ref["%s%d" % (k, l)] for l in range(levels)] for k in "erc"}


def subnormals(x):
    a = np.abs(x)
    return int(((a > 0) & (a < TINY)).sum())


def regime_counts(pred, taps):
    """The counts of DESIGN.md §3's table from the oracle's prediction and its e / r / c taps (lists over the levels)."""
    L = len(taps["c"])
    sub = {"pred": subnormals(pred)}
    for k in "erc":
        for l in range(L):
            sub["%s%d" % (k, l)] = subnormals(taps[k][l])
    return {
        "n": int(pred.size),
        "zero": int((pred == 0.0).sum()),
        "one": int((pred == 1.0).sum()),
        "between": int(((pred > 0.0) & (pred < 1.0)).sum()),
        "max_pred": float(pred.max()),
        "tanh_mid": [int((np.abs(c) >= np.float32(0.625)).sum()) for c in taps["c"]],        # tanh(c) past the polynomial
        "gate_clipped": [int(((r == 0) & (c != 0)).sum()) for r, c in zip(taps["r"], taps["c"])],  # o clipped to 0
        "subnormal": sub,
        "finite": bool(np.isfinite(pred).all() and all(np.isfinite(a).all() for k in "erc" for a in taps[k])),
    }


def conditions(regime, levels, counts):
    """[(what, holds)]: what a case must reach for its comparison to test the regime at all.  Stated for the reference
    model's four levels and cut to the levels a smaller model has."""
    c, sub = counts, counts["subnormal"]
    out = [("finite", c["finite"])]
    if regime in ("S4", "S16"):
        out += [("a prediction == 1.0", c["one"] > 0), ("a prediction == 0.0", c["zero"] > 0),
                ("a prediction strictly between", c["between"] > 0)]
        # (a one-level model has no level >= 1: its only level carries the condition)
        first = 0 if regime == "S16" or levels == 1 else 1
        for l in range(first, levels):
            out += [("|c| >= 0.625 at level %d" % l, c["tanh_mid"][l] > 0),
                    ("r == 0 and c != 0 at level %d" % l, c["gate_clipped"][l] > 0)]
    else:
        want = {"D19": ["pred", "r1", "c1", "e2"], "D13": ["r2", "c2", "e3"]}[regime]
        have = [k for k in want if k == "pred" or int(k[1:]) < levels]
        if not have:                    # (D13 on a model of one or two levels: GAIN_OVERRIDE moves it to the prediction)
            have = ["pred"]
        out += [("a subnormal in %s" % k, sub[k] > 0) for k in have]
    return out


def assert_same_bits(got, ref, msg=""):
    """Equality of the float32 BIT PATTERNS: a flushed subnormal and a zero of the other sign both show."""
    got, ref = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(ref, np.float32)
    assert got.shape == ref.shape, "%s: shape %r against %r" % (msg, got.shape, ref.shape)
    g, r = got.view(np.uint32), ref.view(np.uint32)
    if not np.array_equal(g, r):
        bad = np.argwhere(g != r)
        i = tuple(bad[0])
        raise AssertionError("%s: %d of %d elements differ in their bits; first at %r: got %r (0x%08x), expected %r (0x%08x)"
                             % (msg, len(bad), g.size, i, float(got[i]), int(g[i]), float(ref[i]), int(r[i])))


# ------------------------------------------------------------------------------------------------------------ whole jobs
# (nt, h, w, warm_up, window, threshold, mode, bound): model S16 of the reference shape, so that the predictions reach 0
# and 1 and the deltas trunc(pred * 255) - orig the ends of their range
JOBS = [
    (9, 16, 24, 0, 4, None, "abs", (0.0,)),        # unpadded: the fused lossless kernel
    (9, 16, 24, 0, 4, None, "abs", (2.0,)),        # unpadded: the quantiser with the delta taken inside it
    (9, 21, 30, 1, 3, None, "pwrel", (0.05,)),     # padded
    (8, 64, 64, 0, None, "auto", "rel", (0.01,)),  # DWP
]


def job_id(job):
    nt, h, w, p, window, thr, mode, bound = job
    return "%dx%dx%d-p%d-%s-%s%g" % (nt, h, w, p, "w%d" % window if window else "dwp", mode, bound[0])


def job_frames(nt, h, w):
    """synth.translating_scene with every third frame replaced, alternately by all-255 and all-0, from frame 2 on: against
    a prediction that holds 0.0 and 1.0 these give deltas of -255 and +255.  (From frame 2 and white first because an
    all-zero frame must not be a key frame -- the reference's decoder takes such a frame for 'no key frame here',
    decompress.py:123-129 -- and frames 4 and 8 are key frames of the jobs above.)"""
    from tezip_amd import synth
    frames = synth.translating_scene(nt, h, w, seed=31)
    for k, t in enumerate(range(2, nt, 3)):
        frames[t] = 0 if k % 2 else 255
    return frames


class OraclePredictor:
    def __init__(self, net):
        self.net = net

    def c0(self, hp, wp):
        return self.net.c0()

    def next(self, frame):
        return self.net.next(np.asarray(frame, np.float32))


def job_predictor(job, contract):
    from oracle import coracle
    cfg, w = model("S16")
    hp, wp = (job[1] + 7) // 8 * 8, (job[2] + 7) // 8 * 8
    return OraclePredictor(coracle.CPredNet(w, cfg.stack_sizes, cfg.R_stack_sizes, hp, wp).set_contract(contract))


@functools.lru_cache(maxsize=None)
def job_oracle(job, contract):
    """The oracle's compression of a job: compress_oracle's dict plus `thr` (the DWP threshold in force), `raw` (the deltas
    before the quantiser) and `decoded` (what the oracle's decoder makes of the stream)."""
    from oracle import oracle as O
    nt, h, w, p, window, thr, mode, bound = job
    frames = job_frames(nt, h, w)
    pred = job_predictor(job, contract)
    if thr == "auto":
        # between the two middle MSEs of a one-window rollout: windows of mixed lengths, and no MSE ties with the threshold
        mse = np.sort(O.rollout(frames, p, None, 1e9, pred)["mse"])
        thr = float(mse[len(mse) // 2 - 1] + mse[len(mse) // 2]) / 2
    ref = O.compress_oracle(frames, p, window, thr, mode, list(bound), pred, True)
    ref["thr"] = thr
    ref["raw"] = np.concatenate([O.delta_group(np.stack(preds), frames[start: start + len(preds)])
                                 for start, preds in ref["rollout"]["groups"]])
    ref["decoded"] = O.decode_stream(ref["stream"], ref["key_frame"], pred)
    return ref
