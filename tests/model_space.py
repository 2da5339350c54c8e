"""Model shapes tz_model_load accepts and no other test runs.  Which kernel a convolution runs on, and under
TZ-PA2 which arithmetic it uses, is a function of the channel counts alone; the other network-level tests run channel counts
from {16, 32, 48, 64, 96, 192}, at most four levels, and an R <= 4 at level 0 only.  Shared by tests/test_model_space.py (CPU:
the models below produce every dispatch value the others never do, and the C oracle is right on them) and
tests/test_gpu_model_space.py (the HIP predictor against the C oracle, bit for bit): the models, a plain-Python restatement
of the dispatch rules (`classes`, `families`), the frames, the oracle's results (computed once per model and contract, never
written to) and the comparison."""
import functools

import numpy as np

import regimes as R
from tezip_amd.prednet import PredNetConfig

SEED, BIAS_SCALE = 13, 0.25      # biases: G0 / C0 / Ahat0 are not uniform, the tile shortcuts see their periods

# (id, stack_sizes, R_stack_sizes (None: the same), hp, wp)
MODELS = [
    ("M1", (3, 80), None, 16, 24),                # 80 columns: A_0 / Ahat_1 at NT 1 ncb 5, gates of 5 column blocks (a prime for the ipw search)
    ("M2", (3, 112, 128), (2, 80, 128), 24, 40),  # R_0 = 2; A_0 / Ahat_1 at NT 1 ncb 7; gates of 5 and 8 blocks; level 1 can split
    ("M3", (3, 144, 256), (1, 112, 256), 24, 40),  # R_0 = 1; A_0 at NT 3 ncb 3; A_1 at NT 4 ncb 4; gates of 7 and 16 blocks
    ("M4", (3,) + (16,) * 7, None, 128, 128),     # eight levels, one-pixel top: the constants repeat with periods 2 .. 128
    ("M5", (3, 16, 32, 16, 32, 16), (4, 16, 4, 16, 2, 16), 32, 64),  # six levels; R of 4 and 2 at levels 2 and 4, 16-multiples between
    ("M6", (3, 48, 96, 192, 384), None, 32, 48),  # five levels; A_3 = 384 columns (NT 4 ncb 6); top gates 24 blocks over 1152 channels
    ("M7", (3, 160, 240), (16, 160, 240), 24, 40),  # A_0 at NT 1 ncb 10; A_1 at NT 3 ncb 5; gates of 10 and 15 blocks
    ("M8", (3, 64, 128), (3, 4, 128), 24, 40),    # R_1 = 4: packed gates on the general kernel, Ahat_1 from 4 channels, level 0 upsamples 4 channels
    ("M9", (3, 80, 128), None, 72, 88),           # interior and ragged 16x16 tiles with ncb 5 / 8; A_1 = 128 columns (NT 4 ncb 2) on k_wino
    ("M10", (3, 80, 128), None, 256, 256),        # contract 0: the default must pick TZ-PA2 at this size (one step only: size)
    ("M11", (3, 16, 80), (3, 4, 4), 16, 24),      # no k_wino convolution at all (TZ-PA1 and TZ-PA2 are the same bits); A_1 at NT 1 ncb 5, level >= 1
    ("M12", (3, 16, 80, 16, 112, 16, 160), None, 64, 64),  # seven levels, one-pixel top; A_1 / A_3 / A_5 at NT 1 ncb 5 / 7 / 10 between k_wino gates
]
BY_ID = {m[0]: m for m in MODELS}
DEFAULT_CONTRACT_MODEL = "M10"

# the models some other -m gpu test runs: SHAPES of tests/regimes.py (= tests/test_gpu_parity.py, test_gpu_wino.py) and every
# literal stack_sizes= of a GPU test
OTHER_MODELS = [(s, r) for s, r, _, _ in R.SHAPES] + [
    ((3, 16, 32), None), ((3, 64, 64), (3, 16, 16)), ((3, 64), None), ((3, 48, 96, 192), (16, 48, 96, 192))]


def config(model):
    return PredNetConfig(stack_sizes=model[1], R_stack_sizes=model[2])


@functools.lru_cache(maxsize=None)
def weights(mid):
    w = config(BY_ID[mid]).init_weights(seed=SEED, bias_scale=BIAS_SCALE)
    for a in w:
        a.setflags(write=False)
    return w


# ------------------------------------------------------------------------------------------ the dispatch rules, restated
def plain_nt(cout):
    """Column tiles of an A / Ahat convolution (tz_prednet.hip plain_nt)."""
    return 4 if cout % 64 == 0 else 3 if cout % 48 == 0 else 1


def classes(cfg):
    """{name: quantities} for every convolution of a model (a_l, ahat_l, gates_l), from the channel counts alone:
    NT (16-column tiles per column block), ncb (column blocks), cpt (16-channel blocks per source), fullk (every source a
    multiple of 16 channels), packed (the four gates of R <= 4 channels in one 16-column tile), ups (an upsampled source),
    kdepth (input channels of the whole convolution, the constant r_{t-1} part of a gate convolution included) and wino_ok
    (TZ-PA2 evaluates it as Winograd chains: the rule of oracle/tz_oracle.c wino_gate_ok / wino_a_ok).  `srcs` are the
    per-frame sources in chain order."""
    st, rs, L = cfg.stack_sizes, cfg.R_stack_sizes, cfg.nb_layers
    out = {}

    def entry(level, kind, nt, ncols, srcs, packed, ups, kdepth, wino_ok):
        return dict(level=level, kind=kind, NT=nt, ncb=ncols // (16 * nt), ncols=ncols, srcs=tuple(srcs),
                    cpt=tuple((c + 15) // 16 for c in srcs), fullk=all(c % 16 == 0 for c in srcs), packed=packed, ups=ups,
                    kdepth=kdepth, wino_ok=bool(wino_ok))

    for l in range(L - 1):
        cout = st[l + 1]
        out["a%d" % l] = entry(l, "a", plain_nt(cout), (cout + 15) // 16 * 16, [2 * st[l]], False, False, 2 * st[l],
                               l >= 1 and (2 * st[l]) % 16 == 0 and (cout % 64 == 0 or cout % 48 == 0))
    for l in range(L):
        cout = st[l]
        out["ahat%d" % l] = entry(l, "ahat", plain_nt(cout), (cout + 15) // 16 * 16, [rs[l]], False, False, rs[l], False)
    for l in range(L):
        r = rs[l]
        assert r % 16 == 0 or r <= 4, "tz_model_load refuses R_stack_sizes[%d] = %d" % (l, r)
        packed = r % 16 != 0
        srcs = [2 * st[l]] + ([rs[l + 1]] if l < L - 1 else [])
        out["gates%d" % l] = entry(l, "gates", 1 if packed else 4, 16 if packed else 4 * r, srcs, packed, l < L - 1, r + sum(srcs),
                                   l >= 1 and (2 * st[l]) % 16 == 0 and r % 16 == 0 and (l == L - 1 or rs[l + 1] % 16 == 0))
    return out


FAMILIES = ("wino_pa2", "conv16_lds_dma", "conv16b_level0", "conv_small_valu", "conv3x3_general", "convlat_small_grid")


def family(cfg, name, c, contract):
    """The launch family of one per-frame convolution under the default switches, by the rules of launch_conv
    (tz_prednet.hip): 'lds' stands for conv16_lds_dma or convlat_small_grid -- which of the two is a fitted cost model's
    choice (lat_plan), not a rule of the channel counts; set_conv_impl(1, lat='never') makes it conv16_lds_dma."""
    st, rs, L = cfg.stack_sizes, cfg.R_stack_sizes, cfg.nb_layers
    l = c["level"]
    if c["kind"] == "ahat":                      # (only Ahat_0 runs per frame)
        return "conv_small_valu" if rs[0] == 3 and st[0] == 3 else "conv3x3_general"
    if l == 0:                                   # E_0 is stored 8 floats wide: the block-step kernel where it has the case
        if c["kind"] == "a":
            return "conv16b_level0"
        return "conv16b_level0" if c["packed"] and (L == 1 or rs[1] % 16 == 0) else "conv3x3_general"
    if contract == 2 and c["wino_ok"]:
        return "wino_pa2"
    if c["fullk"] and c["NT"] >= 3:
        return "lds"
    return "conv3x3_general"


def families(cfg, contract):
    """{family: [names of the per-frame convolutions that run on it]} for one predict_next under the default switches."""
    out = {}
    for name, c in classes(cfg).items():
        if c["kind"] == "ahat" and c["level"] > 0:
            continue
        out.setdefault(family(cfg, name, c, contract), []).append(name)
    return out


def epart_can_split(cfg):
    """Levels whose gate convolution can run as two k_wino launches (tz_prednet.hip epart_levels): between the bottom and
    the top level, k_wino gates, and an upsampled source of whole 16-channel blocks."""
    cl = classes(cfg)
    return [l for l in range(1, cfg.nb_layers - 1) if cl["gates%d" % l]["wino_ok"]]


def wino_launches(cfg):
    """k_wino launches of one fused predictor step under TZ-PA2."""
    return sum(c["wino_ok"] for c in classes(cfg).values())


# ----------------------------------------------------------------------------------------------------- frames and oracle
frames = R.frames
assert_same_bits = R.assert_same_bits


@functools.lru_cache(maxsize=None)
def oracle(mid, contract):
    """What the C oracle computes for a model under a contract (the layout of regimes.oracle): the t = 0 prediction, the
    predictions of the three random frames, the e / r / c taps of the last of them, the predictions of the two constant
    frames, the first prediction fed back.  The 256 x 256 model runs one step only (`pred` holds one frame)."""
    from oracle import coracle
    _, stack, rstack, hp, wp = BY_ID[mid]
    cfg = config(BY_ID[mid])
    net = coracle.CPredNet(weights(mid), cfg.stack_sizes, cfg.R_stack_sizes, hp, wp).set_contract(contract)
    rand, const = frames(hp, wp)
    out = {"t0": net.c0()}
    if mid == DEFAULT_CONTRACT_MODEL:
        pred, taps = net.next(rand[0], debug=True)
        out["pred"] = pred[None]
    else:
        out["pred"] = np.empty_like(rand)
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


# ------------------------------------------------------------------------------------------------------------ whole jobs
JOB_MODELS = ["M2", "M5", "M6", "M8"]


def job_geometry(mid):
    """(nt, h, w): cropped below the model's padded size so that padding is exercised wherever the level count leaves a
    size of the same padding (h and w round up to multiples of 8; a model of six levels needs multiples of 32)."""
    _, _, _, hp, wp = BY_ID[mid]
    return 9, hp - 3, wp - 4


def job_frames(mid):
    from tezip_amd import synth
    nt, h, w = job_geometry(mid)
    return synth.translating_scene(nt, h, w, seed=17)


class MemoPredictor(R.OraclePredictor):
    """The oracle's predictor step is a pure function of its input frame (one step from the t = 0 state): the jobs of a model
    and the decoder's replay of a job ask for the same steps again and again, so each is computed once."""

    def __init__(self, net):
        super().__init__(net)
        self.memo = {}

    def next(self, frame):
        f = np.ascontiguousarray(frame, np.float32)
        key = f.tobytes()
        if key not in self.memo:
            out = self.net.next(f)
            out.setflags(write=False)
            self.memo[key] = out
        return self.memo[key]


@functools.lru_cache(maxsize=None)
def job_predictor(mid, contract):
    from oracle import coracle
    _, _, _, hp, wp = BY_ID[mid]
    cfg = config(BY_ID[mid])
    return MemoPredictor(coracle.CPredNet(weights(mid), cfg.stack_sizes, cfg.R_stack_sizes, hp, wp).set_contract(contract))


@functools.lru_cache(maxsize=None)
def job_oracle(mid, contract, window, bound):
    """The oracle's compression of a job: SWP (window = 3) or DWP (window None: one threshold inside the MSE
    range of a one-window rollout, chosen so that windows of mixed lengths come out), mode abs."""
    from oracle import oracle as O
    frames_ = job_frames(mid)
    pred = job_predictor(mid, contract)
    thr = None
    if window is None:
        # midpoints between neighbouring MSEs of a one-window rollout (no MSE ties with the threshold), from the median
        # outwards: the first one that gives windows of mixed lengths
        mse = np.sort(O.rollout(frames_, 0, None, 1e9, pred)["mse"])
        mids = sorted(((mse[i] + mse[i + 1]) / 2 for i in range(len(mse) - 1)), key=lambda t: abs(t - np.median(mse)))
        thr = next(float(t) for t in mids if 1 < int(O.rollout(frames_, 0, None, float(t), pred)["key"].sum()) < len(frames_) - 1)
    ref = O.compress_oracle(frames_, 0, window, thr, "abs", [bound], pred, True)
    ref["thr"] = thr
    ref["decoded"] = O.decode_stream(ref["stream"], ref["key_frame"], pred)
    return ref
