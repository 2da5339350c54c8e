"""`-c --sdelta auto` without a GPU (definition TZ-SDA1, tezip_amd/sdauto.py): the plane symbols of the slow statement against
sdelta.encode_plane, its counts, bits and file sizes against the files the slow coders write from a plane payload, the choice,
three stacks on which three different layouts win, the command line's refusals and what reaches compress.run.  Integers
throughout."""
import re

import numpy as np
import pytest

from tezip_amd import ratetarget as rt
from tezip_amd import sdauto, sdelta

CODERS = ("huff", "huffr", "huffd")


@pytest.fixture(scope="module")
def mods():
    from tezip_amd import build
    build.build()   # (tz_huff_lengths / tz_huffr_lengths are host functions of the library)
    from tezip_amd import huff, huffd, huffr
    return {"huff": huff, "huffr": huffr, "huffd": huffd}


# ------------------------------------------------------------------------------------------------- 1. the plane symbols
def test_plane_symbols_are_encode_plane():
    rng = np.random.default_rng(3)
    for shape in ((1, 1, 1), (3, 1, 7), (3, 5, 1), (2, 3, 5), (2, 21, 30)):
        q = rng.integers(-255, 256, shape + (3,)).astype(np.int16)
        for offset in (True, False):
            np.testing.assert_array_equal(sdauto.plane_symbols(q, 3, offset), sdelta.encode_plane(q, offset))
            np.testing.assert_array_equal(sdauto.plane_symbols(q, 1, offset), sdelta.encode_plane(q[..., :1], offset))
            # by the definition, element by element: neighbours outside the frame are 0, every frame on its own
            x = q.astype(np.int64)
            nt, h, w = shape
            want = np.empty_like(x)
            for f in range(nt):
                for y in range(h):
                    for c in range(w):
                        a = x[f, y, c - 1] if c else 0
                        b = x[f, y - 1, c] if y else 0
                        d = x[f, y - 1, c - 1] if c and y else 0
                        want[f, y, c] = (a + b - d - x[f, y, c] + 256) % 512 - 256
            np.testing.assert_array_equal(sdauto.plane_symbols(q, 3, offset), (1600 - want if offset else want).reshape(-1))
    # the example of sdelta.py's docstring: one channel of a 2 x 2 frame, whatever channels 1 and 2 hold
    q = np.zeros((1, 2, 2, 3), np.int16)
    q[0, :, :, 0] = [[255, -255], [-255, 255]]
    q[..., 1:] = 77
    assert sdauto.plane_symbols(q, 1, False).tolist() == [-255, -2, -2, 4]
    assert sdauto.plane_symbols(q, 1, True).tolist() == [1855, 1602, 1602, 1596]
    assert sdauto.plane_symbols(q, 3, True)[0::3].tolist() == [1855, 1602, 1602, 1596]
    with pytest.raises(ValueError):
        sdauto.plane_symbols(q.reshape(-1), 3)
    with pytest.raises(ValueError):
        sdauto.plane_symbols(q, 2)
    with pytest.raises(ValueError):
        sdauto.plane_symbols(q * 2, 3)     # 510: no quantised delta


# ------------------------------------------------------------------------- 2. the slow statement and the size of a file
NT, H, W = 5, 37, 31      # 17205 elements: no multiple of 8, 256 or 16384, and more than one chunk; 5735 pixels likewise


@pytest.fixture(scope="module")
def stacks():
    """{bound: quantised delta stack (nt, H, W, 3) int16} of synth frames with the previous frame as a stand-in predictor,
    through the oracle's quantiser (tests/test_ratetarget.py)"""
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
    return out


def _sized(mods, sym, payload, table, shape5, check_files=True):
    """{coder: E} of the slow statement over the symbols `sym`; check_files: every figure against the file the slow coder
    writes from (payload, table)"""
    huffd = mods["huffd"]
    n = payload.size
    np.testing.assert_array_equal(rt.rank_of(table)(sym.astype(np.int64)), payload.astype(np.int64))   # the bijection
    counts, bad = rt.count_of_symbols(sym)
    assert not bad and int(counts[0].sum()) == n
    if table is not None:
        np.testing.assert_array_equal(rt.table_of(counts), table)
    counts3, base = rt.remapped_counts(counts, table)
    A = int(payload.max()) - int(payload.min()) + 1
    assert base == int(payload.min()) and counts3.shape == (3, A + 8)
    np.testing.assert_array_equal(counts3, huffd.token_counts(payload, base, A))
    out = {}
    for coder in CODERS:
        fmt = mods[coder]
        dist, lengths = rt.code_of(counts3, coder)
        lens = rt.lens_of(lengths, coder, dist, base, table)
        words, bits, bad = rt.bits_of_symbols(sym, lens, dist)
        assert not bad
        if coder == "huffd":
            assert bits == huffd.cost_bits(counts3[huffd.DISTS.index(dist)], lengths)
        record = {"n": n, "stream_words": words, "A": A, "table_len": -1 if table is None else len(table)}
        out[coder] = rt.file_bytes(record, coder)
        if check_files:
            data = fmt.encode_file(payload, table, shape5, 1)
            p = fmt.parse(data)
            assert (p.stream_words, p.A, p.base, getattr(p, "dist", dist)) == (words, A, base, dist)
            assert out[coder] == len(data), coder
    return out


@pytest.mark.parametrize("entropy", [True, False], ids=["table", "no_table"])
@pytest.mark.parametrize("channels", [3, 1])
@pytest.mark.parametrize("bound", [0.0, 2.0], ids=["lossless", "abs2"])
def test_plane_counts_bits_and_file_bytes_equal_the_coders(mods, stacks, bound, channels, entropy):
    q = stacks[bound]
    payload, table = sdelta.payload_from_delta(q if channels == 3 else q[..., :1], entropy, plane=True)
    n = payload.size
    assert n == NT * H * W * channels and n % 8 and n % 256 and n % 16384
    sym = sdauto.plane_symbols(q, channels, entropy)
    _sized(mods, sym, payload, table, (sdelta.MARK_PLANE, NT, H, W, channels))
    counts, bad = sdauto.count_of_plane(q, channels, entropy)
    np.testing.assert_array_equal(counts, rt.count_of_symbols(sym)[0])
    lens = np.full(rt.BINS + 8, 3, np.uint8)
    assert sdauto.bits_of_plane(q, lens, 1, channels, entropy) == rt.bits_of_symbols(sym, lens, 1)
    # a code that lacks a symbol present
    assert sdauto.bits_of_plane(q, np.zeros(rt.BINS + 8, np.uint8), 0, channels, entropy)[2]
    # the helpers behind count_of / bits_of serve the other layouts as before
    np.testing.assert_array_equal(rt.count_of(q, 3, 3, entropy)[0], rt.count_of_symbols(rt.symbols_of(q, 3, 3, entropy))[0])
    assert rt.bits_of(q, lens, 3, 1, 1, entropy) == rt.bits_of_symbols(rt.symbols_of(q, 1, 1, entropy), lens, 3)


# -------------------------------------------------------------------------------------------------------- 3. the choice
def _rec(n, words=100, A=40, table_len=40):
    return {"n": n, "stream_words": words, "A": A, "table_len": table_len}


def test_choose():
    e = lambda r: rt.file_bytes(r, "huffd")   # noqa: E731
    big, mid, small = _rec(5000, 900), _rec(5000, 500), _rec(5000, 100)
    assert e(big) > e(mid) > e(small)
    for order, want in (((big, mid, small), "plane"), ((big, small, mid), "channel"), ((small, big, mid), "flat"),
                        ((mid, mid, big), "flat"), ((big, mid, mid), "channel"), ((small, small, small), "flat")):   # ties: the earlier
        mode, sizes = sdauto.choose(list(order), "huffd")
        assert mode == want and sizes == [e(r) for r in order]
    # whole files are compared, not stream words: a longer table outweighs a few words
    assert sdauto.choose([_rec(5000, 100, 40, 400), _rec(5000, 110, 40, 40), _rec(5000, 300)], "huff")[0] == "channel"
    # a layout that is no candidate (n == 0, or None) is skipped, whatever else its record holds
    none = _rec(0, 0, 0, 0)
    assert sdauto.choose([mid, none, big], "huffr") == ("flat", [rt.file_bytes(mid, "huffr"), None, rt.file_bytes(big, "huffr")])
    assert sdauto.choose([big, None, mid], "huffr")[0] == "plane"
    assert sdauto.choose([none, none, mid], "huff")[0] == "plane"
    with pytest.raises(ValueError):
        sdauto.choose([none, none, none], "huffd")
    with pytest.raises(ValueError):
        sdauto.choose([mid, mid], "huffd")
    with pytest.raises(KeyError):
        sdauto.choose([mid, mid, mid], "zstd")
    # a numpy record of the library's own type
    from tezip_amd import _lib
    recs = np.zeros(3, _lib.SIZE_DTYPE)
    for i, r in enumerate((big, none, small)):
        for k, v in r.items():
            recs[i][k] = v
    assert sdauto.choose(recs, "huffd") == ("plane", [e(big), None, e(small)])
    assert sdauto.stdout_line("plane", [123456, 120000, 99000]) == "sdelta: auto -> plane (bytes: flat 123456, channel 120000, plane 99000)"
    assert sdauto.stdout_line("flat", [2004, None, 2088]) == "sdelta: auto -> flat (bytes: flat 2004, channel -, plane 2088)"
    assert sdauto.CANDIDATES == ("flat", "channel", "plane") == sdelta.MODES and sdauto.DEFINITION == "TZ-SDA1"


# ------------------------------------------------------------------------------------------ 4. each layout wins somewhere
SHAPE = (3, 16, 32)


def _smooth(rng):
    """a smooth 2-D field: per channel a linear ramp along every row and every column (the row's slope grows with y), mod ~200,
    plus noise in {-1, 0, 1}.  The delta along the row is a level per row, the plane delta one level everywhere"""
    nt, h, w = SHAPE
    f, y, x = np.meshgrid(np.arange(nt), np.arange(h), np.arange(w), indexing="ij")
    q = np.stack([(x * y + 3 * x + 5 * y + 11 * f) % 199, (x * y + 7 * x + 2 * y + 5 * f) % 203,
                  (2 * x * y + 4 * x + 9 * y + 3 * f) % 197], -1) - 100
    return (q + rng.integers(-1, 2, q.shape)).astype(np.int16)


def _runs(rng):
    """independent per channel: runs of random length 2-11 at a level in [-60, 60], over the flattened frame"""
    nt, h, w = SHAPE
    q = np.empty((nt, h * w, 3), np.int64)
    for f in range(nt):
        for c in range(3):
            m = h * w // 2 + 1
            q[f, :, c] = np.repeat(rng.integers(-60, 61, m), rng.integers(2, 12, m))[:h * w]
    return q.reshape(nt, h, w, 3).astype(np.int16)


def _sparse_gray(rng):
    """1/12 of the pixels non-zero in [-200, 200], three equal channels"""
    nt, h, w = SHAPE
    g = np.where(rng.random((nt, h, w)) < 1 / 12.0, rng.integers(-200, 201, (nt, h, w)), 0)
    return np.repeat(g[..., None], 3, axis=-1).astype(np.int16)


def _separable(rng):
    """r[y] + c[x] plus noise in {-1, 0, 1} in channel 0 (the others equal: a gray job's stack)"""
    nt, h, w = SHAPE
    g = rng.integers(-90, 91, (nt, h, 1)) + rng.integers(-90, 91, (nt, 1, w)) + rng.integers(-1, 2, (nt, h, w))
    return np.repeat(g[..., None], 3, axis=-1).astype(np.int16)


def _sizes(mods, q, channels, entropy):
    """{coder: [E(flat), E(channel) or None, E(plane)]} by the slow statement"""
    nt, h, w = q.shape[:3]
    x = q if channels == 3 else q[..., :1]
    per = []
    for mode in sdauto.CANDIDATES:
        if mode == "channel" and channels == 1:
            per.append(None)
            continue
        if mode == "plane":
            payload, table = sdelta.payload_from_delta(x, entropy, plane=True)
            sym = sdauto.plane_symbols(q, channels, entropy)
        else:
            stride = 3 if mode == "channel" else 1
            payload, table = sdelta.payload_from_delta(x, entropy, stride)
            sym = rt.symbols_of(q, channels, stride, entropy)
        per.append(_sized(mods, sym, payload, table, None, check_files=False))
    return {coder: [None if p is None else p[coder] for p in per] for coder in CODERS}


@pytest.mark.parametrize("entropy", [True, False], ids=["table", "no_table"])
@pytest.mark.parametrize("stack,channels,winner", [(_smooth, 3, "plane"), (_runs, 3, "channel"), (_sparse_gray, 3, "flat"),
                                                   (_separable, 1, "plane")],
                         ids=["smooth", "runs", "sparse_gray", "separable_gray"])
@pytest.mark.parametrize("seed", [5, 7])
def test_each_layout_wins_somewhere(mods, seed, stack, channels, winner, entropy):
    q = stack(np.random.default_rng(seed))
    assert q.shape == SHAPE + (3,) and int(np.abs(q).max()) <= 255
    for coder, sizes in _sizes(mods, q, channels, entropy).items():
        print(stack.__name__, seed, coder, "table" if entropy else "no table", sizes)
        smallest = min(e for e in sizes if e is not None)
        assert [m for m, e in zip(sdauto.CANDIDATES, sizes) if e == smallest] == [winner], (coder, sizes)   # (and no tie)
        assert (sizes[1] is None) == (channels == 1)


# --------------------------------------------------------------------------------------------------------- 5. command line
JOB = ["-c", "m", "d", "o", "-p", "2", "-w", "3", "-m", "abs", "-b", "2"]
OK = JOB + ["--coder", "huffd", "--sdelta", "auto"]


def _args(extra):
    from tezip_amd import tezip
    return tezip, tezip.build_parser().parse_args(extra)


@pytest.mark.parametrize("argv,env,word", [
    (JOB + ["--sdelta", "auto"], {}, "add --coder huffd"),
    (JOB + ["--sdelta", "auto", "--coder", "zstd"], {}, "add --coder huffd"),
    (JOB + ["--sdelta", "auto", "--shuffle"], {}, "--shuffle"),
    (["-c", "m", "d", "o", "-p", "2", "-m", "abs", "-b", "2", "--sweep", "--coder", "huffd", "--sdelta", "auto"], {}, "--sweep"),
    (OK, {"WORLD_SIZE": "2"}, "WORLD_SIZE"),
    (["-c", "m", "d", "o", "-p", "2", "-w", "3", "--coder", "huffd", "--sdelta", "auto", "--target-ratio", "8"], {}, "--target-ratio"),
    (["-u", "m", "o", "d", "--sdelta", "auto"], {}, "-c"),
    (["-l", "m", "d", "--sdelta", "auto"], {}, "-c"),
])
def test_cli_refusals(monkeypatch, capsys, argv, env, word):
    from tezip_amd import compress
    tezip, arg = _args(argv)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setattr(tezip, "probe_gpu", lambda force: pytest.fail("refused before a GPU is touched"))
    monkeypatch.setattr(compress, "run", lambda *a, **kw: pytest.fail("compress.run must not be called"))
    problem = tezip.check_sdelta_flag(arg)
    assert problem and word in problem and "sdelta" in problem
    with pytest.raises(SystemExit) as e:
        tezip.main(arg)
    assert e.value.code == 2
    out = capsys.readouterr().out
    assert len(re.findall(r"^ERROR: ", out, flags=re.M)) == 1 and out.startswith("ERROR: ")


def test_plane_with_target_ratio_stays_refused():
    from tezip_amd import compress
    tezip, arg = _args(["-c", "m", "d", "o", "-p", "2", "-w", "3", "--coder", "huffd", "--sdelta", "plane", "--target-ratio", "8"])
    assert tezip.check_sdelta_flag(arg) == compress.PLANE_NO_RATIO


def test_flag_reaches_run(monkeypatch, capsys):
    from tezip_amd import compress
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    calls = []
    monkeypatch.setattr(compress, "run", lambda *a, **kw: calls.append((a, kw)))
    for coder in CODERS:
        tezip, arg = _args(JOB + ["--coder", coder, "--sdelta", "auto"])
        monkeypatch.setattr(tezip, "probe_gpu", lambda force: True)
        assert tezip.check_sdelta_flag(arg) is None
        tezip.main(arg)
        assert calls.pop() == (("m", "d", "o", 2, 3, None, "abs", [2.0], True, False, True),
                               dict(SHUFFLE=False, REPORT=False, CODER=coder, KEY_CODER="zstd", DIGESTS=False, GRAY=False, SSIM=False,
                                    SDELTA="auto"))
    # the searches and every other flag travel with it
    tezip.main(_args(["-c", "m", "d", "o", "-p", "0", "-t", "0.5", "-n", "--target-psnr", "40", "--per-frame", "--coder", "huffr",
                      "--key-coder", "huffg", "--gray", "--sdelta", "auto", "--report", "--ssim", "--digests"])[1])
    a, kw = calls.pop()
    assert a == ("m", "d", "o", 0, None, 0.5, "abs", [], True, False, False)
    assert kw["SDELTA"] == "auto" and kw["TARGET_PSNR"] == 40.0 and kw["PER_FRAME"] and kw["GRAY"] and kw["CODER"] == "huffr"
    tezip.main(_args(OK + ["--quant", "lattice"])[1])
    a, kw = calls.pop()
    assert kw["SDELTA"] == "auto" and kw["QUANT"] == "lattice"
    assert calls == []


def test_jobs_without_the_flag_call_run_as_before(monkeypatch):
    from tezip_amd import compress
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    calls = []
    tezip, arg = _args(JOB + ["--coder", "huffd"])
    monkeypatch.setattr(tezip, "probe_gpu", lambda force: True)
    monkeypatch.setattr(compress, "run", lambda *a, **kw: calls.append((a, kw)))
    assert tezip.check_sdelta_flag(arg) is None
    tezip.main(arg)
    tezip.main(_args(JOB + ["--coder", "huffd", "--sdelta", "plane"])[1])
    tezip.main(_args(JOB + ["--sdelta", "flat"])[1])
    assert calls == [(("m", "d", "o", 2, 3, None, "abs", [2.0], True, False, True), dict(SHUFFLE=False, REPORT=False, CODER="huffd")),
                     (("m", "d", "o", 2, 3, None, "abs", [2.0], True, False, True),
                      dict(SHUFFLE=False, REPORT=False, CODER="huffd", KEY_CODER="zstd", DIGESTS=False, GRAY=False, SSIM=False,
                           SDELTA="plane")),
                     (("m", "d", "o", 2, 3, None, "abs", [2.0], True, False, True), dict(SHUFFLE=False))]


@pytest.mark.parametrize("kw,word", [
    (dict(CODER="zstd"), "add --coder huffd"),
    (dict(SHUFFLE=True), "--shuffle"),
    (dict(sharded=True), "WORLD_SIZE"),
    (dict(BOUND=[], TARGET_RATIO=8), "--target-ratio"),
])
def test_a_direct_caller_of_run_is_refused(monkeypatch, capsys, kw, word):
    from tezip_amd import compress
    monkeypatch.setattr(compress.tzdist, "active", lambda: (0, 2) if kw.get("sharded") else None)
    monkeypatch.setattr(compress, "make_context", lambda *a, **k: pytest.fail("refused before a GPU is touched"))
    with pytest.raises(SystemExit) as e:
        compress.run("m", "d", "o", 2, 3, None, "abs", kw.get("BOUND", [2.0]), True, False, True, SHUFFLE=kw.get("SHUFFLE", False),
                     CODER=kw.get("CODER", "huffd"), TARGET_RATIO=kw.get("TARGET_RATIO"), SDELTA="auto")
    out = capsys.readouterr().out
    assert e.value.code == 2 and out.startswith("ERROR:") and len(out.splitlines()) == 1 and word in out
    assert compress.check_sdelta("auto") is None and "auto" in compress.check_sdelta("bogus")


def test_abi_names():
    import os
    from conftest import ROOT
    from tezip_amd import _lib
    text = open(os.path.join(ROOT, "include", "tezip_hip.h")).read()
    for name in ("tz_sdelta_probe", "tz_size_count_plane_buf", "tz_size_bits_plane_buf"):
        assert re.search(r"int\s+%s\s*\(" % name, text) and name in _lib.EXPORTS
    assert "TZ-SDA1" in text and "TZ-SDA1" in open(os.path.join(ROOT, "DESIGN.md")).read()
