"""The opt-in Huffman coder with repeat tokens (`--coder huffr`, format TZR1) on the CPU: the tokeniser, the numpy encoder /
decoder of tezip_amd/huffr.py (the specification the kernels are tested against in tests/test_gpu_huffr.py), the decoding
rules for arbitrary bits, the container's validation, and the command line's refusals.  No GPU."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import fake_predictor
from conftest import ROOT
from oracle import oracle as O
from test_huff import golden_payloads, synthetic_payloads


@pytest.fixture(scope="module")
def mods():
    from tezip_amd import build
    build.build()
    from tezip_amd import huff, huffr
    return huff, huffr


def _code(R, pay):
    """(lengths over A + 8 symbols, base) of a payload, from its own token counts."""
    base = int(pay.min())
    return R.code_lengths(R.token_counts(pay, base, int(pay.max()) - base + 1)), base


def _oracle_payload(frames, window, bound):
    from tezip_amd import decompress
    enc = O.compress_oracle(frames, 0, window, None, "abs", [float(bound)], O.FnPredictor(fake_predictor.c0_image, fake_predictor.g_next), True)
    pay, tab, shape, p = decompress.parse_stream(np.ascontiguousarray(enc["stream"]).tobytes())
    return np.array(pay), np.array(tab), shape, p


def _roundtrip(R, name, pay):
    ln, base = _code(R, pay)
    co, rb, words = R.encode_body(pay, ln, base)
    nruns, nchunks = R.geometry(pay.size)
    assert co.size == nchunks and rb.size == nruns and (np.diff(co.astype(np.int64)) >= 0).all(), name
    assert int(rb.astype(np.int64).max()) <= R.RUN * R.MAX_LEN, name
    dec = R.decode_body(co, rb, words, pay.size, ln, base)
    assert dec.dtype == np.int16 and (dec == pay).all(), name
    assert len(R.pack_body(co, rb, words)) == R.body_bytes(pay.size, words.size), name
    return words.size


def test_numpy_pair_is_the_identity(mods):
    from tezip_amd import synth
    huff, R = mods
    for name, pay, tab, shape, p in golden_payloads():
        data = R.encode_file(pay, tab, shape, p, base=None if tab is None else 0)
        assert R.is_huffr(data[:4]) and not huff.is_huff(data[:4]) and data[:4] != b"\x28\xb5\x2f\xfd"
        dec, parsed = R.decode_file(data, key_len=pay.size)
        assert dec.dtype == np.int16 and (dec == pay).all(), name
        assert parsed.shape == tuple(shape) and parsed.warm_up == p and parsed.n == pay.size, name
        assert (parsed.table is None) == (tab is None) and (tab is None or (parsed.table == tab).all()), name
    for name, pay in synthetic_payloads(huff):
        _roundtrip(R, name, pay)
    frames = synth.moving_blobs(5, 40, 56, seed=3)
    for bound in (0, 2):
        pay, tab, shape, p = _oracle_payload(frames, 3, bound)
        _roundtrip(R, "oracle abs %d" % bound, pay)
        data = R.encode_file(pay, tab, shape, p, base=0)
        assert (R.decode_file(data, key_len=pay.size)[0] == pay).all()


def filling_payloads(R):
    """(name, payload, lengths) under a GIVEN code of 2111 + 8 lengths of 12 (Kraft 2119/4096): on a payload without any match
    every full run is R * L = 3072 bits and every full chunk 6144 words, the whole LDS image of the kernels; on pixel runs the
    tokens and their raw bits are coded under it too."""
    rng = np.random.default_rng(11)
    chunk = R.RUN * R.CHUNK_RUNS
    ln = np.full(2111 + R.NTOK, 12, np.uint8)
    out = [("all12_no_match", (np.arange(2 * chunk + 300) % 2111).astype(np.int16), ln)]           # s[j] != s[j - 3] everywhere
    runs = np.repeat(rng.integers(0, 50, (4000, 3)), rng.geometric(0.05, 4000), 0).reshape(-1).astype(np.int16)
    runs[:3] = 0
    out.append(("all12_pixel_runs_n%d" % (runs.size - 5), runs[: runs.size - 5], ln))
    return out


def test_numpy_pair_is_the_identity_under_a_given_code(mods):
    from test_huff import assert_fills_the_image
    huff, R = mods
    for name, pay, ln in filling_payloads(R):
        R.check_lengths(ln)
        assert int(pay.min()) == 0
        co, rb, words = R.encode_body(pay, ln, 0)
        nruns, nchunks = R.geometry(pay.size)
        assert co.size == nchunks and rb.size == nruns and int(rb.astype(np.int64).max()) <= R.RUN * R.MAX_LEN, name
        assert (R.decode_body(co, rb, words, pay.size, ln, 0) == pay).all(), name
        if name == "all12_no_match":
            assert int(R.token_counts(pay, 0, 2111)[2111:].sum()) == 0
            assert_fills_the_image(R, name, pay.size, co, rb)
        else:
            assert int(R.token_counts(pay, 0, 2111)[2111:].sum()) > 1000 and pay.size > 2 * R.RUN * R.CHUNK_RUNS, name


def test_vector_tokeniser_is_the_loop(mods):
    """tokenise (what encode_body uses) against tokenise_run, the plain loop over one run."""
    huff, R = mods
    rng = np.random.default_rng(1)
    pays = [p for _, p in synthetic_payloads(huff)[:8]]
    pays.append(np.repeat(rng.integers(0, 9, (300, 1)), 3, 1).repeat(rng.integers(1, 9, 300), 0).reshape(-1).astype(np.int16))   # period-3 runs
    for pay in pays:
        sym = pay.astype(np.int64) - int(pay.min())
        A = int(sym.max()) + 1
        tok, extra, nextra = R.tokenise(sym, A)
        for r0 in range(0, sym.size, R.RUN):
            want = R.tokenise_run(sym[r0: r0 + R.RUN].tolist())
            got = [("L", int(tok[i])) if tok[i] < A else ("T", int(tok[i]) - A, int(extra[i]))
                   for i in range(r0, min(r0 + R.RUN, sym.size)) if tok[i] >= 0]
            assert got == want
            assert all(nextra[i] == max(int(tok[i]) - A, 0) for i in range(r0, min(r0 + R.RUN, sym.size)) if tok[i] >= 0)


def test_tokeniser_properties_on_hand_made_runs(mods):
    _, R = mods
    T = R.tokenise_run
    assert T([5, 5, 5]) == [("L", 5)] * 3                              # nothing in front of j = 3 can match
    assert T([5, 5, 5, 5]) == [("L", 5)] * 3 + [("T", 0, 0)]
    assert T([7] * 256) == [("L", 7)] * 3 + [("T", 7, 253 - 128)]       # m = 253: T_7 and 7 raw bits holding 125
    assert T([1, 2, 3] * 85 + [1]) == [("L", 1), ("L", 2), ("L", 3), ("T", 7, 253 - 128)]
    assert T([1, 2, 3, 1, 2, 3, 9, 2, 3, 9]) == [("L", 1), ("L", 2), ("L", 3), ("T", 1, 1), ("L", 9), ("T", 1, 1)]
    assert T([4, 0, 0, 4, 1, 0, 4, 1]) == [("L", 4), ("L", 0), ("L", 0), ("T", 0, 0), ("L", 1), ("T", 1, 1)]
    for m in range(1, 254):                                             # every stretch length: k = floor(log2 m), m - 2^k behind it
        run = [1, 2, 3] + [(1, 2, 3)[j % 3] for j in range(m)] + [100 + j for j in range(253 - m)]
        toks = T(run)
        k = m.bit_length() - 1
        assert toks[3] == ("T", k, m - (1 << k)) and len(toks) == 4 + 253 - m
    # two runs and a short third one, all one period-3 pattern: history stops at every run boundary, so each run codes as
    # 3 literals and one token, and the last run of 3 + 20 elements too
    pay = np.array([1, 2, 3] * 200, np.int16)[: 2 * 256 + 23]
    sym = pay.astype(np.int64) - 1
    tok, extra, nextra = R.tokenise(sym, 3)
    coded = np.nonzero(tok >= 0)[0]
    assert coded.tolist() == [0, 1, 2, 3, 256, 257, 258, 259, 512, 513, 514, 515]
    assert tok[3] == 3 + 7 and extra[3] == 125 and nextra[3] == 7 and tok[259] == 3 + 7
    assert tok[515] == 3 + 4 and extra[515] == 20 - 16 and nextra[515] == 4
    assert (tok[coded[[0, 1, 2]]] == sym[:3]).all() and (tok[[256, 257, 258]] == sym[256:259]).all()
    counts = R.token_counts(pay, 1, 3)
    assert counts.tolist() == [3, 3, 3, 0, 0, 0, 0, 1, 0, 0, 2]
    ln, base = _code(R, pay)
    co, rb, words = R.encode_body(pay, ln, base)
    assert rb.size == 3 and (R.decode_body(co, rb, words, pay.size, ln, base) == pay).all()


def test_constant_payload_is_a_quarter_of_tzh1(mods):
    """Derived bound: TZH1 spends at least one bit per element, n bits; a run of a constant payload is 3 literals and one
    token with at most 7 raw bits, 3 * 12 + 12 + 7 = 55 bits per 256 elements at most."""
    huff, R = mods
    for n in (256, 5000, 3 * 16384 + 77):
        pay = np.full(n, 1600, np.int16)
        lh = huff.code_lengths(np.bincount(pay.astype(np.int64) - 1600))
        h_bits = int(huff.encode_body(pay, lh, 1600)[1].astype(np.int64).sum())
        ln, base = _code(R, pay)
        co, rb, words = R.encode_body(pay, ln, base)
        r_bits = int(rb.astype(np.int64).sum())
        assert h_bits >= n
        assert (rb.astype(np.int64) <= 55).all() and r_bits <= 55 * len(rb)
        assert 4 * r_bits < h_bits and (n < 5000 or 4 * words.size < huff.encode_body(pay, lh, 1600)[2].size)
        assert (R.decode_body(co, rb, words, n, ln, base) == pay).all()


def test_tzr1_file_is_smaller_on_a_bounded_oracle_job(mods, capsys):
    from tezip_amd import synth
    huff, R = mods
    pay, tab, shape, p = _oracle_payload(synth.turbulence(6, 96, 96), 5, 2)
    h = huff.encode_file(pay, tab, shape, p, base=0)
    r = R.encode_file(pay, tab, shape, p, base=0)
    with capsys.disabled():
        print("\nturbulence(6, 96, 96) w5 abs 2: TZH1 %d bytes (%.3f bits/element), TZR1 %d bytes (%.3f)"
              % (len(h), 8 * len(h) / pay.size, len(r), 8 * len(r) / pay.size))
    assert (R.decode_file(r, key_len=pay.size)[0] == pay).all()
    assert len(r) < len(h)
    with capsys.disabled():                                              # recorded only: small payloads without stretches may grow
        for name, pay, tab, shape, p in golden_payloads():
            base = None if tab is None else 0
            print("%-64s TZH1 %6d  TZR1 %6d bytes" % (name, len(huff.encode_file(pay, tab, shape, p, base=base)),
                                                      len(R.encode_file(pay, tab, shape, p, base=base))))


# ---------------------------------------------------------------------------------- decoding rules for arbitrary bits
def _bits_to_words(bits):
    """[(value, nbits), ...] appended from the least significant end -> uint32 words."""
    acc, nb = 0, 0
    for v, l in bits:
        acc |= v << nb
        nb += l
    return np.array([(acc >> (32 * i)) & 0xFFFFFFFF for i in range((nb + 31) // 32 or 1)], np.uint32), nb


def test_decoder_rules_for_tokens_out_of_place(mods):
    huff, R = mods
    # 4 literals (values 10..13) and all eight tokens, 4 bits each: a complete code over 12 of the 16 codes
    ln = np.array([4] * 4 + [4] * 8, np.uint8)
    codes = huff.canonical_codes(ln)
    lit = lambda s: (int(codes[s]), 4)
    tok = lambda k, extra: [(int(codes[4 + k]), 4), (extra, k)]
    # a token at j = 0: three elements copy the imaginary history (base), then elements 3.. copy elements 0..
    words, nb = _bits_to_words(tok(2, 1) + [lit(2), lit(3)])             # m = 5, then literals 12, 13
    out = R.decode_body([0], [nb], words, 7, ln, 10)
    assert out.tolist() == [10, 10, 10, 10, 10, 12, 13]
    # a token at j = 1 copies base twice, then out[0]
    words, nb = _bits_to_words([lit(3)] + tok(2, 0) + [lit(1)])          # 13, m = 4, 11
    assert R.decode_body([0], [nb], words, 6, ln, 10).tolist() == [13, 10, 10, 13, 10, 11]
    # an over-long stretch is clamped to its run: m = 255 at j = 3 of a run of 256, and the next run starts afresh
    first = [lit(1), lit(2), lit(3)] + tok(7, 127)
    w0, nb0 = _bits_to_words(first)
    second = [lit(0)] * 5
    w1, nb1 = _bits_to_words([(0, nb0)] + second)
    words = np.zeros(max(w0.size, w1.size), np.uint32)
    words[: w0.size] |= w0
    words[: w1.size] |= w1
    out = R.decode_body([0], [nb0, nb1 - nb0], words, 256 + 5, ln, 10)
    assert out[:256].tolist() == [11, 12, 13] * 85 + [11] and out[256:].tolist() == [10] * 5
    # ... and to a short last run
    out = R.decode_body([0], [nb0], w0, 40, ln, 10)
    assert out.tolist() == ([11, 12, 13] * 14)[:40]


def test_scrambled_stream_words_decode_without_an_exception(mods):
    huff, R = mods
    rng = np.random.default_rng(4)
    for name, pay in synthetic_payloads(huff)[3:10]:
        ln, base = _code(R, pay)
        co, rb, words = R.encode_body(pay, ln, base)
        A = ln.size - R.NTOK
        for scramble in (rng.integers(0, 1 << 32, words.size, dtype=np.uint64).astype(np.uint32), ~words, np.zeros_like(words),
                         np.full_like(words, 0xFFFFFFFF)):
            out = R.decode_body(co, rb, scramble, pay.size, ln, base)
            assert out.size == pay.size and out.min() >= base and out.max() < base + A, name
        rb2 = rng.integers(0, R.RUN * R.MAX_LEN + 1, rb.size).astype(np.uint16)      # any admissible index
        assert R.decode_body(co, rb2, words, pay.size, ln, base).size == pay.size


# ------------------------------------------------------------------------------------------------- container
def _file(R, n=3 * 8 * 8 * 3, table=True, seed=0):
    rng = np.random.default_rng(seed)
    pay = np.repeat(np.minimum(rng.geometric(0.3, n // 6) - 1, 30), 6)[:n].astype(np.int16)
    tab = (np.arange(31) + 1600).astype(np.int16) if table else None
    return bytearray(R.encode_file(pay, tab, (1, 3, 8, 8, 3), 0, base=0 if table else None)), pay


def _offsets(R, data):
    f = R.HEADER.unpack(bytes(data[:48]))
    A, nchunks, trailer_len, n = f[5], f[8], f[10], f[3]
    o_len = 48 + ((trailer_len * 2 + 3) & ~3)
    o_idx = o_len + ((A + 8 + 3) & ~3)
    return dict(lengths=o_len, index=o_idx, runs=o_idx + nchunks * 4, A=A, n=n)


def test_container_validation_names_the_field(mods, monkeypatch):
    from tezip_amd import _lib
    huff, R = mods
    good, pay = _file(R)
    assert (R.decode_file(bytes(good))[0] == pay).all()
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("validation must not call the library"))
    o = _offsets(R, good)
    parsed = R.parse(bytes(good))
    assert parsed.lengths.size == o["A"] + 8 and parsed.A == o["A"] and parsed.body.size == R.body_bytes(o["n"], parsed.stream_words)

    def bad(mutate, match, parse=R.parse):
        d = bytearray(good)
        d = mutate(d) or d
        with pytest.raises(ValueError, match=match):
            parse(bytes(d))

    bad(lambda d: d[:-5], "file size")                                  # truncated
    bad(lambda d: d[:20], "header")
    bad(lambda d: d.__setitem__(slice(0, 4), b"TZH1"), "magic")
    bad(lambda d: d, "magic", parse=huff.parse)                         # and TZH1's parser refuses a TZR1 file
    bad(lambda d: d.__setitem__(slice(4, 6), struct.pack("<H", 2)), "version")
    bad(lambda d: d.__setitem__(slice(20, 24), struct.pack("<I", 2112)), "A = 2112")
    bad(lambda d: d.__setitem__(slice(20, 24), struct.pack("<I", o["A"] - 4)), "file size")    # A + 8 lengths: the sections move
    bad(lambda d: d.__setitem__(o["lengths"] + o["A"] + 7, 13), "code lengths hold 13")         # the last token's length
    bad(lambda d: d.__setitem__(slice(o["lengths"] + o["A"], o["lengths"] + o["A"] + 3), b"\x01\x01\x01"), "Kraft")
    bad(lambda d: d.__setitem__(slice(o["lengths"], o["lengths"] + o["A"]), bytes(o["A"])), "no literal")
    bad(lambda d: d.__setitem__(slice(o["index"], o["index"] + 4), struct.pack("<I", 1 << 20)), "chunk offset")
    bad(lambda d: d.__setitem__(slice(o["runs"], o["runs"] + 2), struct.pack("<H", 3073)), "run length")
    bad(lambda d: d.__setitem__(slice(o["runs"], o["runs"] + 2), struct.pack("<H", 3000)), "run lengths of chunk 0")
    bad(lambda d: d.__setitem__(slice(8, 16), struct.pack("<Q", o["n"] - 1)), "n = %d" % (o["n"] - 1))
    bad(lambda d: d.__setitem__(slice(24, 28), struct.pack("<I", 128)), "R = 128")
    with pytest.raises(ValueError, match="key_frame.dat"):
        R.parse(bytes(good), key_len=o["n"] + 1)


def test_lengths_over_more_than_tz_nbins_symbols(mods):
    """All 2111 literals and tokens present: tz_huffr_lengths takes A + 8 counts (tz_huff_lengths stops at TZ_NBINS) and gives
    what tz_huff_lengths gives where both apply."""
    huff, R = mods
    rng = np.random.default_rng(8)
    counts = rng.integers(1, 1000, 2111 + 8).astype(np.uint64)
    ln = R.code_lengths(counts)
    assert ln.size == 2119 and ln.min() >= 1 and ln.max() <= 12 and huff.kraft_sum(ln) == 1 << 12
    small = rng.integers(0, 50, 300).astype(np.uint64)
    assert (R.code_lengths(small) == huff.code_lengths(small)).all()
    with pytest.raises(ValueError):
        R.code_lengths(np.ones(2120, np.uint64))
    with pytest.raises(ValueError):
        huff.code_lengths(counts)


# ------------------------------------------------------------------------------------------------------ CLI
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
def test_cli_refuses_coder_combinations(mods, tmp_path, extra, env, word):
    out = tmp_path / "out"
    args = ["-c", str(tmp_path / "model"), str(tmp_path / "data"), str(out), "-p", "0", "-m", "abs", "-b", "2", "--coder", "huffr"]
    if "--sweep" not in extra:
        args += ["-w", "4"]
    r = _cli(args + extra, env)
    assert r.returncode == 2, r.stdout + r.stderr
    assert "ERROR:" in r.stdout and word in r.stdout and "huffr" in r.stdout
    assert "GPU MODE" not in r.stdout and "CPU MODE" not in r.stdout   # refused before a GPU is touched
    assert not out.exists()


def test_cli_refuses_coder_with_uncompress(mods, tmp_path):
    out = tmp_path / "dec"
    r = _cli(["-u", str(tmp_path / "model"), str(tmp_path / "comp"), str(out), "--coder", "huffr"])
    assert r.returncode == 2 and "ERROR:" in r.stdout and "-c" in r.stdout, r.stdout + r.stderr
    assert not out.exists()


def test_run_refuses_for_a_direct_caller(mods, tmp_path, capsys):
    from tezip_amd import compress
    assert "huffr" in compress.CODERS
    out = tmp_path / "out"
    with pytest.raises(SystemExit) as e:
        compress.run("m", "d", str(out), 0, 4, None, "abs", [2.0], True, False, True, SHUFFLE=True, CODER="huffr")
    assert e.value.code == 2 and "--shuffle" in capsys.readouterr().out
    with pytest.raises(SystemExit) as e:
        compress._run_sharded("m", "d", str(out), 0, 4, None, "abs", [2.0], False, True, 0, False, "huffr")
    assert e.value.code == 2 and "sharded" in capsys.readouterr().out
    assert not out.exists()
