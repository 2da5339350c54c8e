"""CPU checks of the range decode (`-u --frames A:B`): the restart rule of tz_range_restart (host only, like
tz_build_table) against a plain restatement of what include/tezip_hip.h documents, and the --frames parser."""
import numpy as np
import pytest

from tezip_amd import tezip


@pytest.fixture(scope="module")
def lib():
    from tezip_amd import build
    build.build()
    from tezip_amd import _lib
    _lib.load()
    return _lib


def _rule(mask, warm_up, first):
    """include/tezip_hip.h: the largest key frame k with warm_up < k <= first, else 0."""
    for k in range(first, warm_up, -1):
        if mask[k]:
            return k
    return 0


def _masks(rng):
    for _ in range(3000):
        nt = int(rng.integers(1, 24))
        w = int(rng.integers(0, 5))
        mask = rng.random(nt) < rng.uniform(0.05, 0.6)
        mask[: min(nt, w + 1)] = True                    # a decodable stack: frames 0..warm_up carry samples
        yield mask, w
    for nt in (2, 5, 9):                                 # keys exactly at warm_up, warm_up + 1 and the last frame
        for w in range(0, min(nt, 5)):
            for extra in ([w], [w + 1], [nt - 1], [w, w + 1, nt - 1]):
                mask = np.zeros(nt, bool)
                mask[: w + 1] = True
                mask[[e for e in extra if e < nt]] = True
                yield mask, w


def test_restart_rule_matches_its_statement(lib):
    rng = np.random.default_rng(7)
    n = 0
    for mask, w in _masks(rng):
        for first in range(len(mask)):
            r = lib.range_restart(mask, w, first)
            assert r == _rule(mask, w, first), (mask.astype(int).tolist(), w, first)
            assert 0 <= r <= first
            assert r == 0 or (mask[r] and r > w)
            n += 1
    assert n > 10000


def test_restart_rule_rejects_bad_arguments(lib):
    m = np.ones(4, bool)
    for w, first in ((0, 4), (0, -1), (-1, 0)):
        with pytest.raises(lib.TezipError):
            lib.range_restart(m, w, first)


@pytest.mark.parametrize("spec,want", [("3:7", (3, 7)), ("0:1", (0, 1)), (":5", (0, 5)), ("4:", (4, None)),
                                       (":", (0, None)), ("6", (6, 7)), ("0", (0, 1)), (" 2:3 ", (2, 3))])
def test_frames_spec_accepted(spec, want):
    assert tezip.parse_frames(spec) == want
    arg = tezip.build_parser().parse_args(["-u", "m", "c", "o", "--frames", spec])
    assert tezip.check_frames_flag(arg) == (want, None)


@pytest.mark.parametrize("spec", ["", "a", "1:2:3", "-1", "-2:4", "3:-1", "5:5", "7:3", "1.5", "x:3", "2:y"])
def test_frames_spec_refused(spec):
    with pytest.raises(ValueError):
        tezip.parse_frames(spec)
    arg = tezip.build_parser().parse_args(["-u", "m", "c", "o", "--frames=" + spec])
    frames, problem = tezip.check_frames_flag(arg)
    assert frames is None and problem


@pytest.mark.parametrize("mode", [["-c", "m", "d", "o", "-p", "0", "-w", "5", "-m", "abs", "-b", "0"], ["-l", "m", "d"]])
def test_frames_refused_without_uncompress(mode, capsys):
    arg = tezip.build_parser().parse_args(mode + ["--frames", "1:3"])
    frames, problem = tezip.check_frames_flag(arg)
    assert frames is None and "-u" in problem
    with pytest.raises(SystemExit) as e:
        tezip.main(arg)
    assert e.value.code == 2
    assert capsys.readouterr().out.startswith("ERROR:")


def test_no_frames_flag_changes_nothing():
    arg = tezip.build_parser().parse_args(["-u", "m", "c", "o"])
    assert arg.frames is None and tezip.check_frames_flag(arg) == (None, None)
