"""The jobs of the closed-loop tests (definition TZ-CL1, tezip_amd/closedloop.py), shared by tests/test_closedloop.py (CPU: the
slow statement against first principles) and tests/test_gpu_closedloop.py (the library against the slow statement, bit for
bit): the model, the frames, the C oracle as the predictor and the statement's results, computed once per job and never
written to."""
import functools

import numpy as np

import regimes

STACK = (3, 16, 32)
# glorot weights times GAIN, as tests/regimes.py scales them: at gain 1 the predictions of this small model stay below 0.27 and
# feeding the abs 6 decoded frame instead of the original moves 9 % of the truncated predictions; at 2 they reach 0.66 and 25 %
# move (at 4 the gates saturate and fewer do), so a loop that fed the wrong frame cannot pass
GAIN = 2.0
SIZES = [(24, 40), (61, 90)]                 # unpadded, and padded to 64 x 96 (rows of 270 samples: no 16-byte multiple)
# (nt, warm_up, window): the issue's four, and (9, 0, 4) with (nt - 1 - p) % w == 0 -- the trigger on the last frame
TRIPLES = [(7, 0, 2), (7, 0, 3), (7, 1, 2), (8, 1, 3), (9, 0, 4)]
BOUNDS = [("abs", (0.0,), "greedy"), ("abs", (2.0,), "lattice"), ("abs", (6.0,), "lattice")]
LAYOUTS = ("flat", "channel", "plane")


def model():
    return regimes.model("S4", STACK, None, gain=GAIN)


def frames(nt, h, w):
    from tezip_amd import synth
    f = synth.translating_scene(nt, h, w, seed=5)
    f.setflags(write=False)
    return f


def predictor(h, w, contract=1):
    from oracle import coracle
    cfg, wts = model()
    hp, wp = (h + 7) // 8 * 8, (w + 7) // 8 * 8
    return regimes.OraclePredictor(coracle.CPredNet(wts, cfg.stack_sizes, cfg.R_stack_sizes, hp, wp).set_contract(contract))


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def statement(nt, h, w, p, win, mode, bound, quant, contract=1):
    """closedloop.encode of a job."""
    from tezip_amd import closedloop
    return _freeze(closedloop.encode(frames(nt, h, w), p, win, mode, list(bound), quant, predictor(h, w, contract)))


@functools.lru_cache(maxsize=None)
def open_loop(nt, h, w, p, win, contract=1):
    """oracle.rollout of the open-loop SWP job: dict(key, pred) with pred (nt, hp, wp, 3), slot 0 of every group holding C0."""
    from oracle import oracle as O
    ro = O.rollout(frames(nt, h, w), p, win, None, predictor(h, w, contract))
    pred = np.concatenate([np.stack(g) for _, g in ro["groups"]]).astype(np.float32)
    return _freeze(dict(key=ro["key"], pred=pred))
