"""The jobs of the TZ-CLM1 tests (tezip_amd/closedmap.py), shared by tests/test_closedmap.py (CPU: the slow statement against first
principles) and tests/test_gpu_closedmap.py (the library against the slow statement, bit for bit): closedloop_jobs' model (gain 2),
C-oracle predictor and SIZES, predselect_jobs' "flicker" scene for selection, the map, and the statement's results, computed once
per job and never written to.

The map is asymmetric, varies at pixel granularity across every lane and tile boundary and holds 0 and 255, so that a kernel that
indexes it wrongly, or takes one pixel's E for its neighbour's, cannot pass: check_map_matters asserts that the job under the map
rolled by one pixel decodes to other bytes at most samples, and check_mixed that a selection job's modes are neither none nor all,
before a comparison counts."""
import functools

import numpy as np

import closedloop_jobs as J
import predselect_jobs as S

SIZES = J.SIZES                                      # 24 x 40: unpadded, 1.5 x 2.5 tiles; 61 x 90: pads to 64 x 96, W % 4 != 0
ROWS_SIZE = (20, 32)                                 # pads to 24 x 32 with W % 16 == 0: the row-walking form of k_clm_step
TRIPLES = [(7, 0, 3), (8, 1, 3), (9, 0, 4)]
LAYOUTS = J.LAYOUTS
# tiles that take the frame in front on "flicker" under the map, per size and triple (worked out once with the C oracle)
PREV_TILES = {(24, 40): {(7, 0, 3): (3, 24), (8, 1, 3): (3, 24), (9, 0, 4): (9, 36)},
              (61, 90): {(7, 0, 3): (79, 96), (8, 1, 3): (78, 96), (9, 0, 4): (122, 144)}}


@functools.lru_cache(maxsize=None)
def the_map(h, w):
    y, x = np.mgrid[:h, :w]
    m = ((7 * y + 3 * x) % 11).astype(np.uint8)
    m[h // 4:h // 2, w // 4:w // 2] = 0
    m[:, w - 3] = 255
    m[h - 2, :] = 40
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def uniform(h, w, k):
    m = np.full((h, w), k, np.uint8)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def rolled(h, w):
    m = np.roll(the_map(h, w), 1, 1)
    m.setflags(write=False)
    return m


MAPS = {"map": the_map, "rolled": rolled, "zero": lambda h, w: uniform(h, w, 0), "six": lambda h, w: uniform(h, w, 6),
        "full": lambda h, w: uniform(h, w, 255)}


def frames(scene, nt, h, w):
    return S.frames(scene, nt, h, w)


@functools.lru_cache(maxsize=None)
def statement(scene, nt, h, w, p, win, which="map", select=False, contract=1):
    """closedmap.encode of a job under MAPS[which]."""
    from tezip_amd import closedmap
    return J._freeze(closedmap.encode(frames(scene, nt, h, w), p, win, MAPS[which](h, w), J.predictor(h, w, contract), select=select))


def check_map_matters(scene, nt, h, w, p, win, select=False, contract=1):
    """The share of decoded samples of non-key frames that differ between the job under the map and under the map rolled by one
    pixel: asserted to be most of them."""
    a, b = statement(scene, nt, h, w, p, win, "map", select, contract), statement(scene, nt, h, w, p, win, "rolled", select, contract)
    nk = ~a["key"]
    share = float((a["dec"][nk] != b["dec"][nk]).mean())
    assert share > 0.5, share
    return share


def check_mixed(want):
    """Neither none nor all of the tiles of the non-key frames take the frame in front."""
    m = want["modes"][~want["key"]]
    k = int(np.count_nonzero(m))
    assert 0 < k < m.size, (k, m.size)
    return k, int(m.size)
