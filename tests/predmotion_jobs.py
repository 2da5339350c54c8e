"""The jobs of the motion-compensated tile tests (definition TZ-PM1, tezip_amd/predmotion.py), shared by tests/test_predmotion.py
(CPU: the slow statement against first principles) and tests/test_gpu_predmotion.py (the library against the slow statement, bit
for bit): the model, C-oracle predictor, SIZES, BOUNDS and LAYOUTS of tests/closedloop_jobs.py, the scenes of
tests/predselect_jobs.py and one more, and the statement's results, computed once per job and never written to."""
import functools

import numpy as np

import closedloop_jobs as J
import predselect_jobs as PJ

SIZES = J.SIZES                                      # 24 x 40: every tile on a frame edge, unpadded, rows of 120 bytes (a 4-byte multiple);
#                                                      61 x 90: rows of 270 bytes, ragged edge tiles and 2 x 4 interior tiles
TRIPLES = PJ.TRIPLES                                 # (7, 0, 3), (8, 1, 3), (9, 0, 4)
BOUNDS = J.BOUNDS
LAYOUTS = J.LAYOUTS

# "translating" and "flicker" as in predselect_jobs (flicker: regions that jump between 0 and 255, where no displacement helps and
# where many vectors tie).  "shift7": a fixed random texture rolled by (+7, -7) pixels a frame, so frame t is frame t-1 read at
# (y - 7, x + 7): interior tiles match exactly at the extreme vector (-7, +7), and edge tiles cannot (the roll wraps, the clamp does not).
# "still": a fixed random texture with a little noise on top: the frame in front wins where it lies, at the vector (0, 0).
SCENES = PJ.SCENES + ("shift7", "still")


@functools.lru_cache(maxsize=None)
def frames(scene, nt, h, w):
    if scene in PJ.SCENES:
        return PJ.frames(scene, nt, h, w)
    rng = np.random.default_rng(77)
    tex = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if scene == "shift7":
        f = np.stack([np.roll(tex, (7 * t, -7 * t), axis=(0, 1)) for t in range(nt)])
    else:
        f = np.stack([tex // 2 + rng.integers(0, 4, tex.shape, dtype=np.uint8) for t in range(nt)])
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def statement(scene, nt, h, w, p, win, mode, bound, quant, contract=1):
    """predmotion.encode of a job."""
    from tezip_amd import predmotion
    return J._freeze(predmotion.encode(frames(scene, nt, h, w), p, win, mode, list(bound), quant, J.predictor(h, w, contract)))


@functools.lru_cache(maxsize=None)
def select_statement(scene, nt, h, w, p, win, mode, bound, quant, contract=1):
    """predselect.encode (TZ-PS1) of the same job."""
    from tezip_amd import predselect
    if scene in PJ.SCENES:
        return PJ.statement(scene, nt, h, w, p, win, mode, bound, quant, contract)
    return J._freeze(predselect.encode(frames(scene, nt, h, w), p, win, mode, list(bound), quant, J.predictor(h, w, contract)))


@functools.lru_cache(maxsize=None)
def closed_statement(scene, nt, h, w, p, win, mode, bound, quant, contract=1):
    """closedloop.encode (TZ-CL1) of the same job."""
    from tezip_amd import closedloop
    if scene in PJ.SCENES:
        return PJ.closed_statement(scene, nt, h, w, p, win, mode, bound, quant, contract)
    return J._freeze(closedloop.encode(frames(scene, nt, h, w), p, win, mode, list(bound), quant, J.predictor(h, w, contract)))
