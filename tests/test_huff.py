"""The opt-in Huffman coder of entropy.dat on the CPU: tz_huff_lengths (host-only C), the numpy encoder / decoder of
tezip_amd/huff.py (the specification the kernels are tested against in tests/test_gpu_huff.py), the container's
validation, and the command line's refusals.  No GPU."""
import glob
import heapq
import os
import struct
import subprocess
import sys
from functools import lru_cache

import numpy as np
import pytest

from conftest import GOLDEN, ROOT


@pytest.fixture(scope="module")
def huff():
    from tezip_amd import build
    build.build()
    from tezip_amd import huff as H
    return H


def golden_payloads():
    """(name, payload, table, shape5, warm_up) of every *_entropy array of tests/golden/ref_runs*.npz."""
    from tezip_amd import decompress
    out = []
    for f in sorted(glob.glob(os.path.join(GOLDEN, "ref_runs*.npz"))):
        z = np.load(f)
        for k in z.files:
            if k.endswith("_entropy"):
                pay, tab, shape, p = decompress.parse_stream(np.ascontiguousarray(z[k]).tobytes())
                out.append((os.path.basename(f) + ":" + k, np.array(pay), None if tab is None else np.array(tab), shape, p))
    assert len(out) >= 20
    return out


def synthetic_payloads(H):
    """n = 1, R +- 1, one chunk +- 1, a one-symbol stream, a signed (-n style) stream."""
    rng = np.random.default_rng(7)
    chunk = H.RUN * H.CHUNK_RUNS
    out = []
    for n in (1, H.RUN - 1, H.RUN, H.RUN + 1, chunk - 1, chunk, chunk + 1, 3 * chunk + 5 * H.RUN + 17):
        out.append(("ranks_n%d" % n, np.minimum(rng.geometric(0.2, n) - 1, 1020).astype(np.int16)))
    out.append(("one_symbol", np.full(2 * chunk + 3, 5, np.int16)))
    out.append(("signed", np.clip(np.rint(rng.normal(0, 30, 40000)), -510, 510).astype(np.int16)))
    out.append(("all_2111", np.concatenate([np.arange(2111), rng.integers(0, 2111, 30000)]).astype(np.int16)))
    return out


def filling_payloads(H):
    """(name, payload, lengths) under GIVEN codes, none of them code_lengths' choice -- huff_tables accepts any code with
    Kraft sum <= 1.  all12: 2111 symbols of 12 bits (Kraft 2111/4096), so every full run is R * L = 3072 bits and every full
    chunk 6144 words, the whole LDS image of the kernels; all1: two symbols of one bit, every run exactly 8 words (no lane
    shares a word with its neighbour) and a last run of one bit; incomplete: three symbols of 2 bits, a quarter of the decode
    table reached by no code."""
    rng = np.random.default_rng(13)
    chunk = H.RUN * H.CHUNK_RUNS
    out = [("all12_n%d" % (2 * chunk + 300), np.concatenate([np.arange(2111), rng.integers(0, 2111, 2 * chunk + 300 - 2111)]).astype(np.int16),
            np.full(2111, 12, np.uint8))]
    pay = rng.integers(0, 2, chunk + 256 + 1).astype(np.int16)
    pay[0] = 0
    out.append(("all1_n%d" % pay.size, pay, np.array([1, 1], np.uint8)))
    pay = rng.integers(0, 3, chunk + 777).astype(np.int16)
    pay[0] = 0
    out.append(("incomplete_222_n%d" % pay.size, pay, np.array([2, 2, 2], np.uint8)))
    return out


def assert_fills_the_image(H, name, n, chunk_off, run_bits):
    """The index of an all-12 stream: every full run is R * L bits, the first chunk takes all 6144 words."""
    full = n // H.RUN
    assert full >= 2 * H.CHUNK_RUNS and (np.asarray(run_bits[:full], np.int64) == H.RUN * H.MAX_LEN).all(), name
    assert int(chunk_off[1]) - int(chunk_off[0]) == H.RUN * H.CHUNK_RUNS * H.MAX_LEN // 32 == 6144, name
    assert int(chunk_off[2]) - int(chunk_off[1]) == 6144, name


def _cost(counts, lengths):
    return int(np.sum(np.asarray(counts, np.int64) * np.asarray(lengths, np.int64)))


def _huffman_cost(counts):
    """Total cost and depth of an unlimited Huffman code (heap; ties do not change the cost)."""
    h = [(int(c), 0) for c in counts if c]
    heapq.heapify(h)
    total = 0
    while len(h) > 1:
        a, da = heapq.heappop(h)
        b, db = heapq.heappop(h)
        total += a + b
        heapq.heappush(h, (a + b, max(da, db) + 1))
    return total, h[0][1]


def _limited_optimum(counts, L):
    """Optimal cost of a prefix code with lengths <= L, by exhaustive dynamic programming over complete code shapes: the
    symbols in descending count take lengths in ascending order; state = (next symbol, depth, open nodes at this depth)."""
    w = sorted((int(c) for c in counts if c), reverse=True)
    m = len(w)
    inf = float("inf")

    @lru_cache(maxsize=None)
    def f(i, depth, open_nodes):
        if i == m:
            return 0
        if open_nodes == 0:
            return inf
        best = inf
        if depth >= 1:                               # a leaf here
            best = w[i] * depth + f(i + 1, depth, open_nodes - 1)
        if depth < L:                                # one level down: every open node splits (more than m - i are of no use)
            best = min(best, f(i, depth + 1, min(2 * open_nodes, m - i)))
        return best

    return f(0, 0, 1)


def _check_code(H, counts, lengths):
    counts = np.asarray(counts)
    assert lengths.dtype == np.uint8 and lengths.size == counts.size
    assert ((lengths == 0) == (counts == 0)).all()
    assert int(lengths.max()) <= 12
    present = int((counts > 0).sum())
    if present >= 2:
        assert H.kraft_sum(lengths) == 1 << 12
    order = np.argsort(-counts.astype(np.float64), kind="stable")
    ln = lengths[order][: present].astype(int)
    assert (np.diff(ln) >= 0).all(), "a rarer symbol got a shorter code"


def test_lengths_basic_properties(huff):
    rng = np.random.default_rng(0)
    for trial in range(20):
        A = int(rng.integers(2, 2112))
        counts = (rng.geometric(rng.uniform(0.001, 0.2), A) * (rng.random(A) < rng.uniform(0.2, 1.0))).astype(np.uint64)
        counts[int(rng.integers(0, A))] += 1
        counts[int(rng.integers(0, A))] += 5
        ln = huff.code_lengths(counts)
        _check_code(huff, counts, ln)
        assert (huff.code_lengths(counts.copy()) == ln).all()          # deterministic
        cost, depth = _huffman_cost(counts)
        if depth <= 12:                                                # the limit does not bind: Huffman's own cost
            assert _cost(counts, ln) == cost
        else:
            assert _cost(counts, ln) >= cost


def test_lengths_equal_counts_and_ties(huff):
    counts = np.full(2111, 3, np.uint64)                               # all 2111 present, all equal
    ln = huff.code_lengths(counts)
    _check_code(huff, counts, ln)
    assert set(ln.tolist()) == {11, 12} and _cost(counts, ln) == _huffman_cost(counts)[0]
    counts = np.array([5, 5, 5, 5, 5], np.uint64)
    ln = huff.code_lengths(counts)
    assert sorted(ln.tolist()) == [2, 2, 2, 3, 3]
    assert ln.tolist() == [2, 2, 2, 3, 3]                              # ties: the larger symbol takes the longer code


def test_lengths_limit_binds_fibonacci(huff):
    fib = [1, 1]
    while len(fib) < 24:
        fib.append(fib[-1] + fib[-2])
    counts = np.zeros(40, np.uint64)
    counts[3:3 + len(fib)] = fib                                       # unlimited Huffman would need 23 bits
    assert _huffman_cost(counts)[1] > 12
    ln = huff.code_lengths(counts)
    _check_code(huff, counts, ln)
    assert int(ln.max()) == 12
    assert _cost(counts, ln) == _limited_optimum(counts, 12)
    for L in (5, 6, 8):                                                # other limits: the same optimum
        ln = huff.code_lengths(counts, L)
        assert int(ln.max()) <= L and _cost(counts, ln) == _limited_optimum(counts, L)
    rng = np.random.default_rng(3)
    for _ in range(10):
        c = np.sort(rng.integers(1, 10 ** rng.integers(1, 9), 14)).astype(np.uint64)
        for L in (4, 5, 7):
            assert _cost(c, huff.code_lengths(c, L)) == _limited_optimum(c, L)


def test_lengths_edge_cases(huff):
    one = np.zeros(17, np.uint64)
    one[9] = 1234
    assert huff.code_lengths(one).tolist() == [0] * 9 + [1] + [0] * 7
    with pytest.raises(ValueError):
        huff.code_lengths(np.zeros(5, np.uint64))                      # nothing present
    with pytest.raises(ValueError):
        huff.code_lengths(np.ones(2112, np.uint64))                    # A > TZ_NBINS
    with pytest.raises(ValueError):
        huff.code_lengths(np.ones(9, np.uint64), 3)                    # 9 symbols need more than 3 bits
    full = np.ones(2111, np.uint64)
    full[:5] = [10 ** 9, 10 ** 8, 10 ** 7, 10 ** 6, 10 ** 5]
    _check_code(huff, full, huff.code_lengths(full))


def test_tables_are_consistent(huff):
    counts = np.array([50, 0, 20, 7, 7, 1, 1, 0, 3], np.uint64)
    ln = huff.code_lengths(counts)
    enc, dec = huff.encode_table(ln), huff.decode_table(ln)
    for s in np.nonzero(ln)[0]:
        code, l = int(enc[s]) & 0xFFF, int(enc[s]) >> 12
        assert l == ln[s]
        hits = dec[code + (np.arange(1 << (12 - l)) << l)]
        assert (hits == (s | (l << 12))).all()
    assert (dec >> 12 >= 1).all() and ((dec & 0xFFF) < counts.size).all()
    one = huff.decode_table(np.array([0, 0, 1], np.uint8))              # half of the table is reached by no code
    assert (one == (2 | (1 << 12))).all()


def test_numpy_pair_is_the_identity(huff):
    for name, pay, tab, shape, p in golden_payloads():
        data = huff.encode_file(pay, tab, shape, p)
        assert huff.is_huff(data[:4]) and data[:4] != b"\x28\xb5\x2f\xfd"
        dec, parsed = huff.decode_file(data, key_len=pay.size)
        assert dec.dtype == np.int16 and (dec == pay).all(), name
        assert parsed.shape == tuple(shape) and parsed.warm_up == p and parsed.n == pay.size, name
        assert (parsed.table is None) == (tab is None) and (tab is None or (parsed.table == tab).all()), name
    for name, pay in synthetic_payloads(huff):
        base = int(pay.min())
        ln = huff.code_lengths(np.bincount(pay.astype(np.int64) - base))
        co, rb, words = huff.encode_body(pay, ln, base)
        nruns, nchunks = huff.geometry(pay.size)
        assert co.size == nchunks and rb.size == nruns and (np.diff(co.astype(np.int64)) >= 0).all(), name
        assert int(rb.astype(np.int64).sum()) == int(ln[pay.astype(np.int64) - base].astype(np.int64).sum()), name
        assert (huff.decode_body(co, rb, words, pay.size, ln, base) == pay).all(), name
        assert len(huff.pack_body(co, rb, words)) == huff.body_bytes(pay.size, words.size), name


def test_numpy_pair_is_the_identity_under_given_codes(huff):
    """So far the pair was the identity under optimal codes only; the kernels are held to it under any valid code."""
    for name, pay, ln in filling_payloads(huff):
        huff.check_lengths(ln)
        assert huff.kraft_sum(ln) < 1 << 12 or ln.size == 2, name
        co, rb, words = huff.encode_body(pay, ln, 0)
        nruns, nchunks = huff.geometry(pay.size)
        assert co.size == nchunks and rb.size == nruns and words.size == (int(ln[0]) * pay.size + 31) // 32, name
        assert (huff.decode_body(co, rb, words, pay.size, ln, 0) == pay).all(), name
        if name.startswith("all12"):
            assert_fills_the_image(huff, name, pay.size, co, rb)
        if name.startswith("all1_"):
            assert (rb[:-1] == 256).all() and rb[-1] == 1 and co.tolist() == [0, 64 * 8], name
    tab = huff.decode_table(np.array([2, 2, 2], np.uint8))
    assert (tab[3::4] == (0 | (1 << 12))).all()                         # the unreachable quarter still advances a decoder


def _file(huff, n=3 * 8 * 8 * 3, table=True, seed=0):
    rng = np.random.default_rng(seed)
    pay = np.minimum(rng.geometric(0.3, n) - 1, 30).astype(np.int16)
    tab = (np.arange(31) + 1600).astype(np.int16) if table else None
    return bytearray(huff.encode_file(pay, tab, (1, 3, 8, 8, 3), 0, base=0 if table else None)), pay


def _offsets(huff, data):
    f = huff.HEADER.unpack(bytes(data[:48]))
    A, nchunks, trailer_len, n = f[5], f[8], f[10], f[3]
    o_len = 48 + ((trailer_len * 2 + 3) & ~3)
    o_idx = o_len + ((A + 3) & ~3)
    return dict(lengths=o_len, index=o_idx, runs=o_idx + nchunks * 4, A=A, n=n)


def test_container_validation_names_the_field(huff, monkeypatch):
    from tezip_amd import _lib
    good, pay = _file(huff)
    assert (huff.decode_file(bytes(good))[0] == pay).all()
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("validation must not call the library"))
    o = _offsets(huff, good)

    def bad(mutate, match):
        d = bytearray(good)
        d = mutate(d) or d
        with pytest.raises(ValueError, match=match):
            huff.parse(bytes(d))

    bad(lambda d: d[:-5], "file size")                                  # truncated
    bad(lambda d: d[:20], "header")
    bad(lambda d: d.__setitem__(slice(4, 6), struct.pack("<H", 2)), "version")
    bad(lambda d: d.__setitem__(slice(20, 24), struct.pack("<I", 2112)), "A = 2112")
    bad(lambda d: d.__setitem__(o["lengths"], 13), "code lengths hold 13")
    bad(lambda d: d.__setitem__(slice(o["lengths"], o["lengths"] + 3), b"\x01\x01\x01"), "Kraft")
    bad(lambda d: d.__setitem__(slice(o["index"], o["index"] + 4), struct.pack("<I", 1 << 20)), "chunk offset")
    bad(lambda d: d.__setitem__(slice(o["runs"], o["runs"] + 2), struct.pack("<H", 3073)), "run length")
    bad(lambda d: d.__setitem__(slice(o["runs"], o["runs"] + 2), struct.pack("<H", 3000)), "run lengths of chunk 0")
    bad(lambda d: d.__setitem__(slice(8, 16), struct.pack("<Q", o["n"] - 1)), "n = %d" % (o["n"] - 1))
    bad(lambda d: d.__setitem__(slice(0, 4), b"TZH2"), "magic")
    bad(lambda d: d.__setitem__(slice(24, 28), struct.pack("<I", 128)), "R = 128")
    with pytest.raises(ValueError, match="key_frame.dat"):
        huff.parse(bytes(good), key_len=o["n"] + 1)


def test_second_chunk_offset_past_the_end(huff):
    rng = np.random.default_rng(2)
    nt, h, w = 4, 40, 40                                                # 19200 elements: two chunks
    pay = np.minimum(rng.geometric(0.3, nt * h * w * 3) - 1, 30).astype(np.int16)
    data = bytearray(huff.encode_file(pay, None, (1, nt, h, w, 3), 1))
    o = _offsets(huff, data)
    words = huff.parse(bytes(data)).stream_words
    d = bytearray(data)
    d[o["index"] + 4: o["index"] + 8] = struct.pack("<I", words + 1)
    with pytest.raises(ValueError, match="chunk offset"):
        huff.parse(bytes(d))
    d = bytearray(data)
    d[o["index"] + 4: o["index"] + 8] = struct.pack("<I", 1)           # chunk 0 would have one word for all its runs
    with pytest.raises(ValueError, match="run lengths of chunk 0"):
        huff.parse(bytes(d))


def _cli(args, env=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([sys.executable, "-m", "tezip_amd.tezip"] + args, cwd=ROOT, capture_output=True, text=True, timeout=120,
                          env=e)


@pytest.mark.parametrize("extra,env,word", [
    (["--shuffle"], None, "--shuffle"),
    (["--sweep", "4", "8"], None, "--sweep"),
    ([], {"WORLD_SIZE": "2"}, "sharded"),
])
def test_cli_refuses_coder_combinations(huff, tmp_path, extra, env, word):
    out = tmp_path / "out"
    args = ["-c", str(tmp_path / "model"), str(tmp_path / "data"), str(out), "-p", "0", "-m", "abs", "-b", "2", "--coder", "huff"]
    if "--sweep" not in extra:
        args += ["-w", "4"]
    r = _cli(args + extra, env)
    assert r.returncode == 2, r.stdout + r.stderr
    assert "ERROR:" in r.stdout and word in r.stdout
    assert "GPU MODE" not in r.stdout and "CPU MODE" not in r.stdout   # refused before a GPU is touched
    assert not out.exists()


def test_cli_refuses_coder_with_uncompress(huff, tmp_path):
    out = tmp_path / "dec"
    r = _cli(["-u", str(tmp_path / "model"), str(tmp_path / "comp"), str(out), "--coder", "huff"])
    assert r.returncode == 2 and "ERROR:" in r.stdout and "-c" in r.stdout, r.stdout + r.stderr
    assert not out.exists()


def test_run_refuses_for_a_direct_caller(huff, tmp_path, monkeypatch, capsys):
    from tezip_amd import compress
    out = tmp_path / "out"
    with pytest.raises(SystemExit) as e:
        compress.run("m", "d", str(out), 0, 4, None, "abs", [2.0], True, False, True, SHUFFLE=True, CODER="huff")
    assert e.value.code == 2 and "--shuffle" in capsys.readouterr().out
    with pytest.raises(SystemExit) as e:
        compress._run_sharded("m", "d", str(out), 0, 4, None, "abs", [2.0], False, True, 0, False, "huff")
    assert e.value.code == 2 and "sharded" in capsys.readouterr().out
    with pytest.raises(SystemExit) as e:
        compress.run("m", "d", str(out), 0, 4, None, "abs", [2.0], True, False, True, CODER="lz")
    assert e.value.code == 2
    assert not out.exists()
