"""`-c --target-psnr` without a GPU (definition TZ-TPSNR-1, tezip_amd/target.py): the limit, the bisection and its guarantee,
the slow statement of k_bound_err, the command line's refusals and what reaches compress.run.  Integers throughout: no test
compares a float PSNR with the target."""
import re

import numpy as np
import pytest

from tezip_amd import target


def test_sse_limit():
    assert target.sse_limit(40, 1000) == 6502
    assert target.sse_limit(400, 10) == 0
    assert 7 * 65025 - 1 <= target.sse_limit(1e-9, 7) <= 7 * 65025   # (never above N * 255^2)
    assert target.sse_limit(10, 3) == 19507 and target.sse_limit(20.0, 100) == 65025
    assert target.sse_limit(40, 0) == 0
    for bad in (0, -3.0, float("nan"), float("inf"), float("-inf"), None, "x"):
        with pytest.raises(ValueError):
            target.sse_limit(bad, 10)


def _guarantee(probe, limit, k):
    assert (probe(k) if k else 0) <= limit
    assert k == target.K_MAX or probe(k + 1) > limit


def _counted(fn):
    calls = []

    def probe(k):
        calls.append(k)
        return fn(k)

    return probe, calls


@pytest.mark.parametrize("limit", [1, 24, 25, 26, 1000, 65024, 65025, 10 ** 9])
def test_search_monotone_probe_yields_the_largest_passing_k(limit):
    fn = lambda k: k * k   # noqa: E731
    probe, calls = _counted(fn)
    k, trace = target.search(probe, limit)
    assert k == max(c for c in range(target.K_MAX + 1) if fn(c) <= limit)
    assert len(calls) <= 9 and [t["k"] for t in trace] == calls
    assert all(t["sse"] == fn(t["k"]) and t["pass"] == (t["sse"] <= limit) and t["bound"] == t["k"] / 2 for t in trace)
    _guarantee(fn, limit, k)


@pytest.mark.parametrize("seed", range(6))
def test_search_non_monotone_probe_still_meets_the_guarantee(seed):
    rng = np.random.default_rng(seed)
    sse = np.cumsum(rng.integers(-40, 100, target.K_MAX + 1))   # rises on the whole, falls between neighbours often
    sse = np.abs(sse)
    sse[0] = 0
    fn = lambda k: int(sse[k])   # noqa: E731
    assert (np.diff(sse) < 0).any()
    for limit in (1, 50, max(1, int(sse[200])), int(sse.max()) // 2, int(sse.max())):
        probe, calls = _counted(fn)
        k, trace = target.search(probe, limit)
        assert len(calls) <= 9 and len(trace) == len(calls)
        _guarantee(fn, limit, k)


def test_search_edges():
    probe, calls = _counted(lambda k: pytest.fail("limit 0: no probe at all"))
    assert target.search(probe, 0) == (0, [])
    n = 1890
    probe, calls = _counted(lambda k: n * 65025)   # nothing can exceed N * 255^2
    k, trace = target.search(probe, n * 65025)
    assert k == 510 and len(calls) == 9 and all(t["pass"] for t in trace)
    k, trace = target.search(lambda k: 5, 4)   # every candidate fails: lossless
    assert k == 0 and len(trace) == 8 and not any(t["pass"] for t in trace)


def test_errors_of_clamps_on_both_sides():
    #            plain   q == d   low clamp   high clamp   clamp hides the error   clamp makes it 0
    orig = np.array([[100, 7, 2, 250, 0, 255]], np.uint8)
    d = np.array([[5, -3, -10, 20, -4, 9]], np.int16)          # xh = 105, 4, -8, 270, -4, 264
    q = np.array([[3, -3, 1, 2, -1, 4]], np.int16)             # xh - q = 102, 7, -9, 268, -3, 260 -> 102, 7, 0, 255, 0, 255
    #                                                            e = 2, 0, -2, 5, 0, 0
    assert target.errors_of(orig, d, q).tolist() == [[4 + 4 + 25, 5, 3]]
    # unclamped the errors would be d - q = 2, 0, -11, 18, -3, 5: the clamp matters
    assert int(((d - q).astype(np.int64) ** 2).sum()) == 4 + 121 + 324 + 9 + 25
    two = target.errors_of(np.stack([orig[0], orig[0]]), np.stack([d[0], d[0] * 0]), np.stack([q[0], q[0] * 0]))
    assert two.tolist() == [[33, 5, 3], [0, 0, 0]]
    assert target.errors_of(np.zeros((2, 0), np.uint8), np.zeros((2, 0), np.int16), np.zeros((2, 0), np.int16)).tolist() == [[0, 0, 0]] * 2
    # shaped stacks: the frame axis is the first
    o4 = np.arange(2 * 2 * 3 * 3, dtype=np.uint8).reshape(2, 2, 3, 3)
    assert target.errors_of(o4, np.full(o4.shape, 4, np.int16), np.full(o4.shape, 1, np.int16)).tolist() == [[9 * 18, 3, 18]] * 2


def test_errors_of_a_one_channel_payload():
    """the decoder of a one-channel payload writes channel 0's reconstruction to all three channels of the pixel"""
    orig = np.array([[[10, 10, 10], [250, 250, 250], [0, 0, 0]]], np.uint8)           # gray: three equal channels
    d = np.array([[[5, 9, -2], [20, 1, 3], [-4, 7, 7]]], np.int16)                     # the model's channels differ
    q = np.array([[[3, 9, -2], [2, 1, 3], [-1, 7, 7]]], np.int16)                      # channels 1, 2: q == d, no error of their own
    # channel 0: 10 + 5 - 3 = 12 (e 2), 250 + 20 - 2 = 268 -> 255 (e 5), 0 - 4 + 1 = -3 -> 0 (e 0); each in three channels
    assert target.errors_of(orig, d, q, channels=1).tolist() == [[3 * (4 + 25), 5, 6]]
    assert target.errors_of(orig, d, q).tolist() == [[4 + 25, 5, 2]]                   # the three-channel job is another job
    assert target.errors_of(orig.reshape(1, 9), d.reshape(1, 9), q.reshape(1, 9), channels=1).tolist() == [[87, 5, 6]]
    with pytest.raises(ValueError):
        target.errors_of(orig.reshape(1, 9)[:, :8], d.reshape(1, 9)[:, :8], q.reshape(1, 9)[:, :8], channels=1)
    with pytest.raises(ValueError):
        target.errors_of(orig, d, q, channels=2)


def test_document_and_line(tmp_path):
    fn = lambda k: 1000 * k   # noqa: E731
    limit = target.sse_limit(40, 988)   # 6424
    k, trace = target.search(fn, limit)
    doc = target.make(40, 988, limit, trace, k)
    assert k == 6 and doc["result"] == {"k": 6, "mode": "abs", "bound": 3.0, "sse": 6000} and doc["sse_limit"] == 6424
    assert doc["definition"] == "TZ-TPSNR-1" and doc["samples"] == 988 and doc["probes"] == len(trace) == len(doc["trace"])
    assert target.stdout_line(doc) == "target: PSNR >= 40 dB -> abs bound 3 (9 probes, sse 6000 <= 6424)"
    import json
    assert json.load(open(target.write(str(tmp_path), doc))) == doc
    assert (tmp_path / "bound_search.json").exists()
    lossless = target.make(400, 10, 0, [], 0)
    assert lossless["result"]["sse"] == 0 and "abs bound 0 (0 probes, sse 0 <= 0)" in target.stdout_line(lossless)


# ---- command line
JOB = ["-c", "m", "d", "o", "-p", "2", "-w", "3"]


def _args(extra):
    from tezip_amd import tezip
    return tezip, tezip.build_parser().parse_args(extra)


@pytest.mark.parametrize("argv,env,word", [
    (["-u", "m", "o", "d", "--target-psnr", "40"], {}, "-c"),
    (["-l", "m", "d", "--target-psnr", "40"], {}, "-c"),
    (["-c", "m", "d", "o", "-p", "2", "--sweep", "--target-psnr", "40"], {}, "--sweep"),
    (JOB + ["--target-psnr", "40"], {"WORLD_SIZE": "2"}, "sharded"),
    (JOB + ["--target-psnr", "40", "-m", "abs"], {}, "-m and -b"),
    (JOB + ["--target-psnr", "40", "-b", "2"], {}, "-m and -b"),
    (JOB + ["--target-psnr", "40", "-m", "rel", "-b", "0.1"], {}, "-m and -b"),
    (JOB + ["--target-psnr", "nan"], {}, "finite"),
    (JOB + ["--target-psnr", "inf"], {}, "finite"),
    (JOB + ["--target-psnr", "0"], {}, "above 0"),
    (JOB + ["--target-psnr", "-40"], {}, "above 0"),
])
def test_cli_refusals(monkeypatch, capsys, argv, env, word):
    from tezip_amd import compress
    tezip, arg = _args(argv)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setattr(tezip, "probe_gpu", lambda force: pytest.fail("refused before a GPU is touched"))
    monkeypatch.setattr(compress, "run", lambda *a, **kw: pytest.fail("compress.run must not be called"))
    assert word in tezip.check_target_flag(arg)
    with pytest.raises(SystemExit) as e:
        tezip.main(arg)
    assert e.value.code == 2
    assert re.search(r"^ERROR: .*target-psnr", capsys.readouterr().out, flags=re.M)


def test_flag_reaches_run_as_an_abs_job_without_a_bound(monkeypatch, capsys):
    from tezip_amd import compress
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    calls = []
    tezip, arg = _args(JOB + ["--target-psnr", "40"])
    monkeypatch.setattr(tezip, "probe_gpu", lambda force: True)
    monkeypatch.setattr(compress, "run", lambda *a, **kw: calls.append((a, kw)))
    tezip.main(arg)
    assert calls == [(("m", "d", "o", 2, 3, None, "abs", [], True, False, True),
                      dict(SHUFFLE=False, REPORT=False, CODER="zstd", KEY_CODER="zstd", DIGESTS=False, GRAY=False, SDELTA="flat",
                           SSIM=False, TARGET_PSNR=40.0))]
    assert capsys.readouterr().out.splitlines() == ["GPU MODE", "compress mode", "abs"]   # the mode, where the reference prints it
    # every other flag travels with it
    del calls[:]
    tezip.main(_args(["-c", "m", "d", "o", "-p", "0", "-t", "0.5", "-n", "-v", "--target-psnr", "33.5", "--coder", "huffd", "--key-coder",
                      "huffg", "--gray", "--sdelta", "channel", "--report", "--ssim", "--digests"])[1])
    assert calls == [(("m", "d", "o", 0, None, 0.5, "abs", [], True, True, False),
                      dict(SHUFFLE=False, REPORT=True, CODER="huffd", KEY_CODER="huffg", DIGESTS=True, GRAY=True, SDELTA="channel",
                           SSIM=True, TARGET_PSNR=33.5))]
    del calls[:]
    tezip.main(_args(JOB + ["--target-psnr", "40", "--shuffle"])[1])
    assert calls[0][1]["SHUFFLE"] is True
    # the reference's own checks still apply: no window, no job
    del calls[:]
    capsys.readouterr()
    tezip.main(_args(["-c", "m", "d", "o", "-p", "2", "--target-psnr", "40"])[1])
    assert calls == [] and "window size" in capsys.readouterr().out


def test_jobs_without_the_flag_call_run_as_before(monkeypatch, capsys):
    from tezip_amd import compress
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    calls = []
    tezip, arg = _args(JOB + ["-m", "abs", "-b", "2"])
    monkeypatch.setattr(tezip, "probe_gpu", lambda force: True)
    monkeypatch.setattr(compress, "run", lambda *a, **kw: calls.append((a, kw)))
    tezip.main(arg)
    tezip.main(_args(JOB + ["-m", "abs", "-b", "2", "--report"])[1])
    assert calls == [(("m", "d", "o", 2, 3, None, "abs", [2.0], True, False, True), dict(SHUFFLE=False)),
                     (("m", "d", "o", 2, 3, None, "abs", [2.0], True, False, True), dict(SHUFFLE=False, REPORT=True))]


@pytest.mark.parametrize("kw,word", [
    (dict(MODE="rel", BOUND=[], T=40), "-m and -b"),
    (dict(MODE="abs", BOUND=[2.0], T=40), "-m and -b"),
    (dict(MODE="abs", BOUND=[], T=float("nan")), "finite"),
    (dict(MODE="abs", BOUND=[], T=0), "above 0"),
    (dict(MODE="abs", BOUND=[], T=40, sharded=True), "sharded"),
])
def test_a_direct_caller_of_run_is_refused(monkeypatch, capsys, kw, word):
    from tezip_amd import compress
    monkeypatch.setattr(compress.tzdist, "active", lambda: (0, 2) if kw.get("sharded") else None)
    monkeypatch.setattr(compress, "make_context", lambda *a, **k: pytest.fail("refused before a GPU is touched"))
    with pytest.raises(SystemExit) as e:
        compress.run("m", "d", "o", 2, 3, None, kw["MODE"], kw["BOUND"], True, False, True, TARGET_PSNR=kw["T"])
    out = capsys.readouterr().out
    assert e.value.code == 2 and out.startswith("ERROR:") and word in out


def test_abi_names():
    import os
    from conftest import ROOT
    from tezip_amd import _lib
    text = open(os.path.join(ROOT, "include", "tezip_hip.h")).read()
    for name in ("tz_bound_probe", "tz_bound_err"):
        assert re.search(r"int\s+%s\s*\(" % name, text) and name in _lib.EXPORTS
