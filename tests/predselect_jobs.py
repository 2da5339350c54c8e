"""The jobs of the per-tile selection tests (definition TZ-PS1, tezip_amd/predselect.py), shared by tests/test_predselect.py (CPU:
the slow statement against first principles) and tests/test_gpu_predselect.py (the library against the slow statement, bit for
bit): the model, frames and C-oracle predictor of tests/closedloop_jobs.py at its SIZES and BOUNDS, and the statement's results,
computed once per job and never written to."""
import functools

import closedloop_jobs as J

SIZES = J.SIZES                                      # 24 x 40: 1.5 x 2.5 tiles, unpadded; 61 x 90: pads to 64 x 96, rows of 270 bytes
TRIPLES = [(7, 0, 3), (8, 1, 3), (9, 0, 4)]          # of J.TRIPLES; the last puts the trigger on the last frame
BOUNDS = J.BOUNDS
LAYOUTS = J.LAYOUTS
assert set(TRIPLES) <= set(J.TRIPLES)


# With the random weights of closedloop_jobs the frame in front wins EVERY tile of its translating scene, so a library that ignored
# the costs could pass on it.  "flicker" is that scene with two regions, neither aligned to the tiles, that jump between 0 and 255
# from frame to frame: there the frame in front misses by 255 a sample and the network, whose output stays below 0.66, by less.
SCENES = ("translating", "flicker")


@functools.lru_cache(maxsize=None)
def frames(scene, nt, h, w):
    f = J.frames(nt, h, w)
    if scene == "flicker":
        f = f.copy()
        for t in range(nt):
            f[t, 5:30, 10:37] = 255 * (t % 2)
            f[t, h - 9:, :21] = 255 * ((t + 1) % 2)
        f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def statement(scene, nt, h, w, p, win, mode, bound, quant, contract=1):
    """predselect.encode of a job."""
    from tezip_amd import predselect
    return J._freeze(predselect.encode(frames(scene, nt, h, w), p, win, mode, list(bound), quant, J.predictor(h, w, contract)))


@functools.lru_cache(maxsize=None)
def closed_statement(scene, nt, h, w, p, win, mode, bound, quant, contract=1):
    """closedloop.encode (TZ-CL1, no selection) of the same job."""
    from tezip_amd import closedloop
    if scene == "translating":
        return J.statement(nt, h, w, p, win, mode, bound, quant, contract)
    return J._freeze(closedloop.encode(frames(scene, nt, h, w), p, win, mode, list(bound), quant, J.predictor(h, w, contract)))
