"""`-c --target-ratio` without a GPU (definition TZ-TRATIO-1, tezip_amd/ratetarget.py): the budget, the search and its guarantee
against a brute force, the size of a file from a probe's record against the formats' own encoders, the slow statement of the
two kernels and the bijection claim behind them, the command line's refusals and what reaches compress.run.  Integers
throughout."""
import re

import numpy as np
import pytest

from tezip_amd import ratetarget as rt


@pytest.fixture(scope="module")
def mods():
    from tezip_amd import build
    build.build()   # (tz_huff_lengths / tz_huffr_lengths are host functions of the library)
    from tezip_amd import huff, huffd, huffr
    return {"huff": huff, "huffr": huffr, "huffd": huffd}


# ------------------------------------------------------------------------------------------------------- the budget
def test_budget():
    assert rt.budget(1000, 8) == 125 and rt.budget(1000, 1) == 1000 and rt.budget(1000, 0.5) == 2000      # exact quotients
    assert rt.budget(1000, 3) == 333 and rt.budget(1000, 7) == 142 and rt.budget(10, 4) == 2               # inexact ones: the floor
    assert rt.budget(5 * 61 * 90 * 3, 8.0) == 10293 and rt.budget(82350, 2.5) == 32940
    assert rt.budget(1000, 1e9) == 0 and rt.budget(0, 8) == 0
    assert rt.budget(3, 1e-3) == 3000 or rt.budget(3, 1e-3) == 2999      # (float64: one rounding, made in this module alone)
    for bad in (0, -3.0, float("nan"), float("inf"), float("-inf"), None, "x"):
        with pytest.raises(ValueError):
            rt.budget(1000, bad)
        assert rt.check_target(bad)
    with pytest.raises(ValueError):
        rt.budget(-1, 8)
    assert rt.check_target(8) is None and rt.check_target("2.5") is None


# ------------------------------------------------------------------------------------------------------- the search
def _counted(fn):
    calls = []

    def probe(k):
        calls.append(k)
        return fn(k)

    return probe, calls


def _check(fn, fixed, limit):
    """the search over fn against the brute force over all 511 candidates; -> k"""
    probe, calls = _counted(fn)
    k, trace = rt.search(probe, fixed, limit)
    passing = [c for c in range(rt.K_MAX + 1) if fixed + fn(c) <= limit]
    assert len(calls) <= rt.MAX_PROBES == 11 and [t["k"] for t in trace] == calls and len(set(calls)) == len(calls)
    assert all(t["entropy_bytes"] == fn(t["k"]) and t["pass"] == (fixed + t["entropy_bytes"] <= limit) and t["bound"] == t["k"] / 2
               for t in trace)
    if rt.K_MAX not in passing and 0 not in passing:
        assert k is None and calls == [0, rt.K_MAX]
        return k
    assert k in passing and (k == 0 or k - 1 not in passing)          # the guarantee
    if 0 in passing:
        assert k == 0 and calls == [0]
    return k


@pytest.mark.parametrize("limit", [0, 999, 1000, 1001, 5000, 40000, 99999, 100000, 100999, 101000, 10 ** 7])
def test_search_monotone_curve_yields_the_smallest_passing_k(limit):
    fn = lambda k: 100000 - 190 * k   # noqa: E731  (falls with the bound)
    k = _check(fn, 1000, limit)
    passing = [c for c in range(rt.K_MAX + 1) if 1000 + fn(c) <= limit]
    assert k == (min(passing) if passing else None)


@pytest.mark.parametrize("seed", range(6))
def test_search_curve_with_bumps_still_meets_the_guarantee(seed):
    rng = np.random.default_rng(seed)
    size = 200000 - np.cumsum(rng.integers(-150, 500, rt.K_MAX + 1))   # falls on the whole, rises between neighbours often
    size = np.maximum(size, 100)
    assert (np.diff(size) > 0).any()
    fn = lambda k: int(size[k])   # noqa: E731
    some_not_smallest = False
    for limit in (int(size[300]) + 7, int(size[100]) + 7, int(size[17]) + 7, int(size.min()) + 7, int(size[510]) + 7, int(size[1]) + 7):
        k = _check(fn, 7, limit)
        if k:
            some_not_smallest |= k != min(c for c in range(rt.K_MAX + 1) if 7 + fn(c) <= limit)
    print("seed %d: a boundary that is not the smallest passing bound: %s" % (seed, some_not_smallest))


def test_search_one_bump():
    """a bump: candidates 40 .. 59 pass, 60 .. 99 fail again, 100 .. pass -- the result is a boundary, not the smallest bound"""
    fn = lambda k: 10 if 40 <= k < 60 or k >= 100 else 1000   # noqa: E731
    k = _check(fn, 0, 500)
    assert k in (40, 100)
    assert k == 100    # (this bisection's midpoints 255, 127, 63 see 63 fail: it ends at the upper boundary)


def test_search_edges():
    assert _check(lambda k: 5, 10, 15) == 0                      # all pass: lossless, one probe
    assert _check(lambda k: 5, 10, 14) is None                   # all fail: two probes
    probe, calls = _counted(lambda k: 0 if k >= 1 else 9)        # 0 fails, 1 passes: 510 halves eight times on the way down
    k, trace = rt.search(probe, 0, 5)
    assert k == 1 and len(calls) == 10
    probe, calls = _counted(lambda k: 0 if k >= 510 else 9)      # only the last candidate passes: the longest search, the cap
    k, trace = rt.search(probe, 0, 5)
    assert k == 510 and len(calls) == 11 == rt.MAX_PROBES
    assert max(len(rt.search(lambda c, e=edge: 0 if c >= e else 9, 0, 5)[1]) for edge in range(1, 511)) == 11


def test_document_and_lines(tmp_path):
    import json
    fn = lambda k: 100000 - 190 * k   # noqa: E731
    raw = 823500
    limit = rt.budget(raw, 8)        # 102937
    k, trace = rt.search(fn, 20000, limit)
    doc = rt.make(8, raw, limit, 20000, trace, k)
    assert k == 90 and doc["result"] == {"k": 90, "mode": "abs", "bound": 45.0, "entropy_bytes": 82900}
    assert doc["definition"] == "TZ-TRATIO-1" and doc["raw_bytes"] == raw and doc["budget_bytes"] == 102937 and doc["fixed_bytes"] == 20000
    assert doc["target_ratio"] == 8.0 and doc["probes"] == len(trace) == len(doc["trace"]) == 11
    assert rt.stdout_line(doc) == "target: ratio >= 8 -> abs bound 45 (11 probes, 20000 + 82900 bytes <= 102937)"
    assert json.load(open(rt.write(str(tmp_path), doc))) == doc and (tmp_path / "bound_search.json").exists()
    k, trace = rt.search(fn, 20000, 100)
    doc = rt.make(8000, raw, 100, 20000, trace, k)
    assert k is None and doc["result"] is None and doc["probes"] == 2
    assert rt.unreachable_line(doc) == "ERROR: --target-ratio 8000 cannot be met: at abs 255 the files take 23100 bytes (ratio 35.6494)"


# ------------------------------------------------------------------- the kernels' slow statement and the size of a file
NT, H, W = 5, 37, 31      # 17205 elements: no multiple of 8, 256 or 16384, and more than one chunk; 5735 pixels likewise


@pytest.fixture(scope="module")
def stacks():
    """{bound: quantised delta stack (nt, H, W, 3) int16} of synth frames with the previous frame as a stand-in predictor,
    through the oracle's quantiser"""
    from oracle import oracle as O
    from tezip_amd import synth
    frames = np.ascontiguousarray(synth.translating_scene(NT, 40, 40)[:, :H, :W]).astype(np.int64)
    d = np.zeros_like(frames)
    d[1:] = frames[:-1] - frames[1:]
    out = {}
    for bound in (0.0, 2.0):
        q = d.copy()
        for t in range(1, NT):
            for c in range(3):
                q[t, :, :, c] = O.error_bound(frames[t, :, :, c], d[t, :, :, c], "abs", [bound])
        out[bound] = q.astype(np.int16)
    assert (out[0.0] == d).all() and (out[2.0] != d).any()
    return out


LAYOUTS = {"flat": (3, 1), "gray": (1, 1), "channel": (3, 3)}


def _payload(q, layout, entropy):
    """the oracle's encode tail over the layout's elements -> (payload, table | None, shape5)"""
    from oracle import oracle as O
    from tezip_amd import sdelta
    channels, stride = LAYOUTS[layout]
    x = q[..., 0] if channels == 1 else q
    if stride == 3:
        payload, table = sdelta.payload_from_delta(x, entropy, 3)
        return payload, table, (4, NT, H, W, 3)
    sd = O.finding_difference_enc(np.ascontiguousarray(x).reshape(-1))
    if not entropy:
        return sd, None, (1, NT, H, W, channels)
    y = (1600 - sd.astype(np.int64)).astype(np.int16)
    table = O.build_table(y)
    return O.remap_enc(y, table), table, (1, NT, H, W, channels)


@pytest.mark.parametrize("entropy", [True, False], ids=["table", "no_table"])
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("bound", [0.0, 2.0], ids=["lossless", "abs2"])
def test_counts_bits_and_file_bytes_equal_the_coders(mods, stacks, bound, layout, entropy):
    huffd = mods["huffd"]
    q = stacks[bound]
    channels, stride = LAYOUTS[layout]
    payload, table, shape5 = _payload(q, layout, entropy)
    n = payload.size
    assert n == NT * H * W * channels and n % 8 and n % 256 and n % 16384
    # the symbols in front of the remap, and the bijection: remapped, they are the payload
    sym = rt.symbols_of(q, channels, stride, entropy)
    np.testing.assert_array_equal(rt.rank_of(table)(sym.astype(np.int64)), payload.astype(np.int64))
    counts, bad = rt.count_of(q, channels, stride, entropy)
    assert not bad and int(counts[0].sum()) == n and not counts[0, rt.BINS:].any()
    if entropy:
        np.testing.assert_array_equal(rt.table_of(counts), table)
    # the counts of the UNREMAPPED symbols, permuted by the table, are huffd's counts of the remapped payload
    counts3, base = rt.remapped_counts(counts, table)
    A = int(payload.max()) - int(payload.min()) + 1
    assert base == int(payload.min()) and counts3.shape == (3, A + 8)
    np.testing.assert_array_equal(counts3, huffd.token_counts(payload, base, A))
    assert counts3[1, A:].any() or counts3[2, A:].any()      # (there are repeats to tokenise)
    for coder in ("huff", "huffr", "huffd"):
        fmt = mods[coder]
        dist, lengths = rt.code_of(counts3, coder)
        lens = rt.lens_of(lengths, coder, dist, base, table)
        words, bits, bad = rt.bits_of(q, lens, dist, channels, stride, entropy)
        assert not bad
        if coder == "huffd":
            assert bits == huffd.cost_bits(counts3[huffd.DISTS.index(dist)], lengths)
        data = fmt.encode_file(payload, table, shape5, 1)
        p = fmt.parse(data)
        assert (p.stream_words, p.A, p.base, getattr(p, "dist", dist)) == (words, A, base, dist)
        record = {"n": n, "stream_words": words, "A": A, "table_len": -1 if table is None else len(table)}
        assert rt.file_bytes(record, coder) == len(data), coder
    # a code that lacks a symbol present, and a symbol outside the bins
    _, _, bad = rt.bits_of(q, np.zeros(rt.BINS + 8, np.uint8), 0, channels, stride, entropy)
    assert bad
    far = q.copy().reshape(-1)
    far[9] = 9000
    assert rt.count_of(far, channels, stride, entropy)[1]


def test_symbols_of_every_layout():
    q = np.array([5, 7, 9, 4, 7, 1, 4, 0, 1, -3, 2, 2], np.int16)
    assert rt.symbols_of(q, 3, 1, False).tolist() == [5, -2, -2, 5, -3, 6, -3, 4, -1, 4, -5, 0]
    assert rt.symbols_of(q, 3, 3, False).tolist() == [5, 7, 9, 1, 0, 8, 0, 7, 0, 7, -2, -1]
    assert rt.symbols_of(q, 1, 1, False).tolist() == [5, 1, 0, 7]
    assert rt.symbols_of(q, 1, 1, True).tolist() == [1595, 1599, 1600, 1593]
    assert rt.symbols_of(np.array([-32768, 32767], np.int16), 3, 1, False).tolist() == [-32768, 1]   # int16 wrap
    with pytest.raises(ValueError):
        rt.symbols_of(q[:11], 1, 1)
    with pytest.raises(ValueError):
        rt.symbols_of(q, 1, 3)


def test_count_of_and_bits_of_by_hand():
    """two runs: no match across the run start, stretches cut at the run's end, the raw bits of a token"""
    sym = np.r_[np.full(256, 3), np.full(5, 3), [4, 9, 9, 4, 9, 9]].astype(np.int16)      # 267 symbols
    q = -np.cumsum(np.r_[-sym[:1], sym[1:]].astype(np.int64)).astype(np.int16)            # flat, no offset: q[i-1] - q[i] = sym[i]
    np.testing.assert_array_equal(rt.symbols_of(q, 3, 1, False), sym)
    counts, bad = rt.count_of(q, 3, 1, False)
    b = rt.BIAS
    assert not bad and counts[0, b + 3] == 261 and counts[0, b + 4] == 2 and counts[0, b + 9] == 4
    # distance 1: run 0 is a literal 3 and a stretch of 255 (T_7); run 1 a literal 3, a stretch of 4 (T_2), 4, 9, a stretch of 1 (T_0), 4, 9, T_0
    assert counts[1, b + 3] == 2 and counts[1, b + 4] == 2 and counts[1, b + 9] == 2
    assert counts[1, rt.BINS:].tolist() == [2, 0, 1, 0, 0, 0, 0, 1]
    # distance 3: run 0 three literals and a stretch of 253 (T_7); run 1 three literals 3, a stretch of 2 (T_1), 4, 9, 9, a stretch of 3 (T_1)
    assert counts[2, b + 3] == 6 and counts[2, b + 4] == 1 and counts[2, b + 9] == 2
    assert counts[2, rt.BINS:].tolist() == [0, 2, 0, 0, 0, 0, 0, 1]
    lens = np.zeros(rt.BINS + 8, np.uint8)
    lens[[b + 3, b + 4, b + 9]] = [1, 2, 3]
    lens[rt.BINS:] = [4, 5, 6, 7, 8, 9, 10, 11]
    assert rt.bits_of(q, lens, 0, 3, 1, False) == ((261 + 4 + 12 + 31) // 32, 261 + 4 + 12, False)
    want1 = (1 + 11 + 7) + (1 + 6 + 2) + 2 + 3 + 4 + 2 + 3 + 4
    assert want1 == 46 and rt.bits_of(q, lens, 1, 3, 1, False) == (2, want1, False)
    want3 = (3 + 11 + 7) + 3 + (5 + 1) + 2 + 3 + 3 + (5 + 1)
    assert want3 == 44 and rt.bits_of(q, lens, 3, 3, 1, False) == (2, want3, False)
    lens[rt.BINS + 7] = 0
    assert rt.bits_of(q, lens, 3, 3, 1, False)[2] and not rt.bits_of(q, lens, 0, 3, 1, False)[2]   # a token without a code
    with pytest.raises(ValueError):
        rt.bits_of(q, lens, 2, 3, 1, False)
    # chunks are rounded up one by one: 16384 symbols of 1 bit and one more
    long = np.zeros(16385, np.int16)
    lens0 = np.zeros(rt.BINS + 8, np.uint8)
    lens0[b] = 1
    assert rt.bits_of(long, lens0, 0, 3, 1, False) == (512 + 1, 16385, False)


# ---- command line
JOB = ["-c", "m", "d", "o", "-p", "2", "-w", "3"]
OK = JOB + ["--coder", "huffd", "--target-ratio", "8"]


def _args(extra):
    from tezip_amd import tezip
    return tezip, tezip.build_parser().parse_args(extra)


@pytest.mark.parametrize("argv,env,word", [
    (["-u", "m", "o", "d", "--target-ratio", "8"], {}, "-c"),
    (["-l", "m", "d", "--target-ratio", "8"], {}, "-c"),
    (["-c", "m", "d", "o", "-p", "2", "--sweep", "--coder", "huffd", "--target-ratio", "8"], {}, "--sweep"),
    (OK, {"WORLD_SIZE": "2"}, "sharded"),
    (OK + ["-m", "abs"], {}, "-m, -b"),
    (OK + ["-b", "2"], {}, "-m, -b"),
    (OK + ["-m", "rel", "-b", "0.1"], {}, "-m, -b"),
    (OK + ["--target-psnr", "40"], {}, "--target-psnr"),
    (JOB + ["--target-ratio", "8"], {}, "add --coder huffd"),
    (JOB + ["--target-ratio", "8", "--coder", "zstd"], {}, "add --coder huffd"),
    (OK + ["--shuffle"], {}, "--shuffle"),
    (JOB + ["--target-ratio", "8", "--shuffle"], {}, "--shuffle"),
    (JOB + ["--coder", "huff", "--target-ratio", "nan"], {}, "finite"),
    (JOB + ["--coder", "huffr", "--target-ratio", "inf"], {}, "finite"),
    (JOB + ["--coder", "huffd", "--target-ratio", "0"], {}, "above 0"),
    (JOB + ["--coder", "huffd", "--target-ratio", "-8"], {}, "above 0"),
])
def test_cli_refusals(monkeypatch, capsys, argv, env, word):
    from tezip_amd import compress
    tezip, arg = _args(argv)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setattr(tezip, "probe_gpu", lambda force: pytest.fail("refused before a GPU is touched"))
    monkeypatch.setattr(compress, "run", lambda *a, **kw: pytest.fail("compress.run must not be called"))
    assert word in tezip.check_ratio_flag(arg)
    with pytest.raises(SystemExit) as e:
        tezip.main(arg)
    assert e.value.code == 2
    out = capsys.readouterr().out
    assert re.search(r"^ERROR: .*target-ratio", out, flags=re.M) and word in out


def test_flag_reaches_run_as_an_abs_job_without_a_bound(monkeypatch, capsys):
    from tezip_amd import compress
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    calls = []
    monkeypatch.setattr(compress, "run", lambda *a, **kw: calls.append((a, kw)))
    for coder in ("huff", "huffr", "huffd"):
        tezip, arg = _args(JOB + ["--coder", coder, "--target-ratio", "8"])
        monkeypatch.setattr(tezip, "probe_gpu", lambda force: True)
        assert tezip.check_ratio_flag(arg) is None
        tezip.main(arg)
        assert calls.pop() == (("m", "d", "o", 2, 3, None, "abs", [], True, False, True),
                               dict(SHUFFLE=False, REPORT=False, CODER=coder, KEY_CODER="zstd", DIGESTS=False, GRAY=False, SDELTA="flat",
                                    SSIM=False, TARGET_RATIO=8.0))
        assert capsys.readouterr().out.splitlines() == ["GPU MODE", "compress mode", "abs"]   # the mode, where the reference prints it
    # every other flag travels with it
    tezip.main(_args(["-c", "m", "d", "o", "-p", "0", "-t", "0.5", "-n", "-v", "--target-ratio", "2.5", "--coder", "huffr", "--key-coder",
                      "huffg", "--gray", "--sdelta", "channel", "--report", "--ssim", "--digests"])[1])
    assert calls.pop() == (("m", "d", "o", 0, None, 0.5, "abs", [], True, True, False),
                           dict(SHUFFLE=False, REPORT=True, CODER="huffr", KEY_CODER="huffg", DIGESTS=True, GRAY=True, SDELTA="channel",
                                SSIM=True, TARGET_RATIO=2.5))
    # the reference's own checks still apply: no window, no job
    capsys.readouterr()
    tezip.main(_args(["-c", "m", "d", "o", "-p", "2", "--coder", "huffd", "--target-ratio", "8"])[1])
    assert calls == [] and "window size" in capsys.readouterr().out


def test_jobs_without_the_flag_call_run_as_before(monkeypatch):
    from tezip_amd import compress
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    calls = []
    tezip, arg = _args(JOB + ["-m", "abs", "-b", "2", "--coder", "huffd"])
    monkeypatch.setattr(tezip, "probe_gpu", lambda force: True)
    monkeypatch.setattr(compress, "run", lambda *a, **kw: calls.append((a, kw)))
    assert tezip.check_ratio_flag(arg) is None
    tezip.main(arg)
    tezip.main(_args(JOB + ["--target-psnr", "40"])[1])
    assert calls == [(("m", "d", "o", 2, 3, None, "abs", [2.0], True, False, True), dict(SHUFFLE=False, REPORT=False, CODER="huffd")),
                     (("m", "d", "o", 2, 3, None, "abs", [], True, False, True),
                      dict(SHUFFLE=False, REPORT=False, CODER="zstd", KEY_CODER="zstd", DIGESTS=False, GRAY=False, SDELTA="flat", SSIM=False,
                           TARGET_PSNR=40.0))]


@pytest.mark.parametrize("kw,word", [
    (dict(MODE="rel"), "-m, -b"),
    (dict(BOUND=[2.0]), "-m, -b"),
    (dict(TARGET_PSNR=40), "--target-psnr"),
    (dict(R=float("nan")), "finite"),
    (dict(R=float("inf")), "finite"),
    (dict(R=0), "above 0"),
    (dict(R=-2), "above 0"),
    (dict(sharded=True), "sharded"),
    (dict(CODER="zstd"), "add --coder huffd"),
    (dict(SHUFFLE=True), "--shuffle"),
])
def test_a_direct_caller_of_run_is_refused(monkeypatch, capsys, kw, word):
    from tezip_amd import compress
    monkeypatch.setattr(compress.tzdist, "active", lambda: (0, 2) if kw.get("sharded") else None)
    monkeypatch.setattr(compress, "make_context", lambda *a, **k: pytest.fail("refused before a GPU is touched"))
    with pytest.raises(SystemExit) as e:
        compress.run("m", "d", "o", 2, 3, None, kw.get("MODE", "abs"), kw.get("BOUND", []), True, False, True,
                     SHUFFLE=kw.get("SHUFFLE", False), CODER=kw.get("CODER", "huffd"), TARGET_PSNR=kw.get("TARGET_PSNR"),
                     TARGET_RATIO=kw.get("R", 8))
    out = capsys.readouterr().out
    assert e.value.code == 2 and out.startswith("ERROR:") and "target-ratio" in out and word in out


def test_abi_names():
    import os
    from conftest import ROOT
    from tezip_amd import _lib
    text = open(os.path.join(ROOT, "include", "tezip_hip.h")).read()
    for name in ("tz_size_probe", "tz_size_count_buf", "tz_size_bits_buf"):
        assert re.search(r"int\s+%s\s*\(" % name, text) and name in _lib.EXPORTS
    assert _lib.SIZE_DTYPE.itemsize == 64 and (_lib.SIZE_BINS, _lib.SIZE_BIAS) == (rt.BINS, rt.BIAS)
    assert re.search(r"#define\s+TZ_SIZE_BINS\s+4096", text) and re.search(r"#define\s+TZ_SIZE_BIAS\s+1024", text)
