"""The jobs of the TZ-CLF1 tests (tezip_amd/closedframes.py), shared by tests/test_closedframes.py (CPU: the slow statement against
first principles) and tests/test_gpu_closedframes.py (the library against the slow statement, bit for bit): closedloop_jobs'
model, predictor and sizes, a stack whose frames differ enough for every frame to find a bound of its own, and the statement's
results, computed once per job and never written to.

A uniform stack gives every frame the same bound under random weights, which could not catch a frame taking another frame's E.
So frames t % 3 == 2 of closedloop_jobs.frames are shifted right by 4 bits (f >> 4), then frames t % 4 == 1 are replaced by 255 - (f >> 5)."""
import functools

import numpy as np

import closedloop_jobs as J

SIZES = J.SIZES
TRIPLES = [(7, 0, 3), (8, 1, 3), (9, 0, 4)]
TARGETS = (30.0, 36.0)
GIVEN = (0.0, 0.9, 6.5, 255.0, 300.0, 3.0, 12.0, 1.0, 40.5)   # one per frame, in this order (fixed frames count as 0)
# the statement's k at the non-fixed frames, worked out once with the C oracle as the predictor (the issue's figures): no result at
# 0 or 510, at least two distinct ones
EXPECTED_K = {
    (7, 61, 90, 0, 3, 30.0): [37, 65, 27, 39],
    (7, 61, 90, 0, 3, 36.0): [17, 11, 13, 17],
    (8, 24, 40, 1, 3, 30.0): [67, 27, 39, 27],
}


@functools.lru_cache(maxsize=None)
def frames(nt, h, w):
    f = np.array(J.frames(nt, h, w))
    for t in range(nt):
        if t % 3 == 2:
            f[t] = f[t] >> 4
    for t in range(nt):
        if t % 4 == 1:
            f[t] = 255 - (f[t] >> 5)
    f.setflags(write=False)
    return f


def given(nt):
    return list(GIVEN[:nt])


def limit_of(db, h, w):
    from tezip_amd import target
    return target.sse_limit(db, h * w * 3)


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def searched(nt, h, w, p, win, db, contract=1):
    """closedframes.encode of the search at `db` dB."""
    from tezip_amd import closedframes
    return _freeze(closedframes.encode(frames(nt, h, w), p, win, J.predictor(h, w, contract), limit=limit_of(db, h, w)))


@functools.lru_cache(maxsize=None)
def with_bounds(nt, h, w, p, win, bounds, contract=1):
    """closedframes.encode under the tuple `bounds`."""
    from tezip_amd import closedframes
    return _freeze(closedframes.encode(frames(nt, h, w), p, win, J.predictor(h, w, contract), bounds=list(bounds)))


def check_spread(want):
    """The property that makes a job worth comparing: at least two distinct k among the searched frames, none 0 or 510."""
    ks = [k for k, fixed in zip(want["k"], want["key"]) if not fixed]
    assert len(set(ks)) >= 2 and 0 not in ks and 510 not in ks, ks
    return ks
