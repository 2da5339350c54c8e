"""The opt-in Huffman coder that picks its match distance (`--coder huffd`, format TZR2) on the CPU: the numpy encoder / decoder
of tezip_amd/huffd.py at every distance (the specification the kernels are tested against in tests/test_gpu_huffd.py), the
rule that chooses the distance, the size guarantee against TZH1 and TZR1, the container's validation, the decoding rules for
arbitrary bits, and the command line's refusals.  No GPU."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_huff import golden_payloads

SIZES = (1, 2, 3, 4, 255, 256, 257, 16383, 16385)


@pytest.fixture(scope="module")
def mods():
    from tezip_amd import build
    build.build()
    from tezip_amd import huff, huffd, huffr
    return huff, huffr, huffd


def _shape(n):
    """A stack shape of n one-channel elements whose sides fit the trailer's int16."""
    w = max(d for d in range(1, min(n, 32767) + 1) if n % d == 0)
    assert n // w <= 32767
    return (1, 1, n // w, w, 1)


def _mixed(n, seed):
    """Values that repeat at distance 1 and at distance 3, and some that do neither: every distance has tokens to code."""
    rng = np.random.default_rng(seed)
    px = np.repeat(rng.integers(-9, 40, (n // 3 + 2, 1)), 3, 1)                     # gray pixels: distance 1
    px[rng.random(px.shape[0]) < 0.5, 1] += 50                                      # ... or colour: distance 3 only
    pay = np.repeat(px, rng.integers(1, 4, px.shape[0]), 0).reshape(-1)
    return pay[:n].astype(np.int16)


def constructed_payloads():
    """name -> (payload, the D the rule must choose): the four cases of the choice rule, and a second tie."""
    rng = np.random.default_rng(21)
    out = {}
    out["equal_runs"] = (np.repeat(rng.integers(0, 200, 3000), rng.integers(2, 30, 3000)).astype(np.int16)[:40001], 1)
    triple = np.array([5, -3, 17], np.int16)
    out["repeating_triple"] = (np.tile(triple, 14000)[:40001], 3)
    out["iid_2111"] = (np.concatenate([np.arange(2111), rng.integers(0, 2111, 60000)]).astype(np.int16), 0)
    # a tie of all three: no element equals the one in front or the one three back, the three histograms are the same
    out["tie_no_match"] = ((np.arange(3 * 16384 + 77) % 7).astype(np.int16), 0)
    # a tie of 1 and 3 below "none": blocks p q r p p u v w of eight distinct-looking values.  At distance 1 the second of the
    # two p's is a stretch of one, at distance 3 the first of them, so both histograms hold 7 literals + T_0 per block
    blocks = (np.arange(32 * 40)[:, None] * 7 + np.array([0, 1, 2, 0, 0, 3, 4, 5])[None, :]) % 2100
    out["tie_1_and_3"] = (blocks.reshape(-1).astype(np.int16), 1)
    return out


def test_coder_is_registered_and_parses(mods):
    from tezip_amd import compress, tezip
    assert "huffd" in compress.CODERS
    arg = tezip.build_parser().parse_args(["-c", "m", "d", "o", "--coder", "huffd"])
    assert arg.coder == "huffd"
    assert compress.check_coder("huffd") is None
    assert "--shuffle" in compress.check_coder("huffd", shuffle=True) and "sharded" in compress.check_coder("huffd", sharded=True)


@pytest.mark.parametrize("dist", [0, 1, 3])
def test_round_trip_at_every_forced_distance(mods, dist):
    huff, huffr, D = mods
    for n in SIZES:
        pay = _mixed(n, n)
        shape = _shape(n)
        data = D.encode_file(pay, None, shape, 0, dist=dist)
        assert D.is_huffd(data[:4]) and not huff.is_huff(data[:4]) and not huffr.is_huffr(data[:4])
        assert struct.unpack("<I", data[44:48])[0] == dist
        dec, p = D.decode_file(data)
        assert dec.dtype == np.int16 and (dec == pay).all(), (dist, n)
        assert p.dist == dist and p.n == n and p.shape == shape and p.lengths.size == p.A + 8, (dist, n)
        assert p.run_bits.size == 0 or int(p.run_bits.astype(np.int64).max()) <= D.RUN * D.MAX_LEN
        if dist == 0:
            assert not p.lengths[-8:].any()


def test_distance_3_is_tzr1_and_distance_0_is_tzh1(mods):
    huff, huffr, D = mods
    for n in SIZES + (3 * 16384 + 77,):
        pay = _mixed(n, 100 + n)
        base = int(pay.min())
        A = int(pay.max()) - base + 1
        counts3 = D.token_counts(pay, base, A)
        assert (counts3[2] == huffr.token_counts(pay, base, A)).all()
        assert (counts3[0][:A] == np.bincount(pay.astype(np.int64) - base, minlength=A)).all() and not counts3[0][A:].any()
        ln3 = D.lengths_of(counts3[2], 3)
        assert (ln3 == huffr.code_lengths(counts3[2])).all()
        for got, want in zip(D.encode_body(pay, ln3, base, 3), huffr.encode_body(pay, ln3, base)):
            assert got.dtype == want.dtype and got.size == want.size and (got == want).all(), n
        ln0 = D.lengths_of(counts3[0], 0)
        assert (ln0[:A] == huff.code_lengths(counts3[0][:A])).all() and not ln0[A:].any()
        for got, want in zip(D.encode_body(pay, ln0, base, 0), huff.encode_body(pay, ln0[:A], base)):
            assert got.dtype == want.dtype and got.size == want.size and (got == want).all(), n
        # the files differ from TZR1 / TZH1 in the magic, D and -- TZH1 -- the eight token lengths only
        f3, r1 = D.encode_file(pay, None, _shape(n), 0, dist=3), huffr.encode_file(pay, None, _shape(n), 0)
        assert f3[4:44] == r1[4:44] and f3[48:] == r1[48:]


def test_distance_1_tokens_on_hand_made_runs(mods):
    huff, huffr, D = mods
    A = 4
    sym = np.array([2, 2, 2, 2, 1, 1, 3, 2, 2], np.int64)
    tok, extra, nextra = D.tokenise(sym, A, 1)
    assert tok.tolist() == [2, A + 1, -1, -1, 1, A + 0, 3, 2, A + 0]           # 2 T_1(+1) 1 T_0 3 2 T_0
    assert extra.tolist() == [0, 1, 0, 0, 0, 0, 0, 0, 0] and nextra.tolist() == [0, 1, 0, 0, 0, 0, 0, 0, 0]
    run = np.zeros(2 * D.RUN, np.int64)                                        # a stretch is cut at the run's end: 255 + 255
    tok, extra, nextra = D.tokenise(run, 1, 1)
    assert tok[0] == 0 and tok[1] == 1 + 7 and extra[1] == 255 - 128 and (tok[2:D.RUN] == -1).all()
    assert tok[D.RUN] == 0 and tok[D.RUN + 1] == 1 + 7 and int((tok >= 0).sum()) == 4
    assert D.tokenise(sym, A, 0)[0].tolist() == sym.tolist()
    with pytest.raises(ValueError):
        D.tokenise(sym, A, 2)


def test_choice_rule_on_constructed_payloads(mods):
    huff, huffr, D = mods
    for name, (pay, want) in constructed_payloads().items():
        base = int(pay.min())
        counts3 = D.token_counts(pay, base, int(pay.max()) - base + 1)
        dist, lengths, costs = D.choose(counts3)
        print("%s: D = %d, costs %r" % (name, dist, costs))
        assert dist == want, (name, dist, costs)
        assert all(isinstance(c, int) for c in costs) and costs[D.DISTS.index(dist)] == min(costs), name
        assert (lengths == D.lengths_of(counts3[D.DISTS.index(dist)], dist)).all(), name
        if name == "tie_no_match":
            assert costs[0] == costs[1] == costs[2], costs
        if name == "tie_1_and_3":
            assert costs[1] == costs[2] < costs[0], costs
        # cost_D is the stream's size in bits before the chunks are padded to words
        for i, d in enumerate(D.DISTS):
            co, rb, words = D.encode_body(pay, D.lengths_of(counts3[i], d), base, d)
            assert int(rb.astype(np.int64).sum()) == costs[i], (name, d)
        data = D.encode_file(pay, None, _shape(pay.size), 0)
        dec, p = D.decode_file(data)
        assert p.dist == want and (dec == pay).all(), name


def _guarantee(mods, name, pay, tab, shape, p):
    huff, huffr, D = mods
    base = None if tab is None else 0
    d = D.encode_file(pay, tab, shape, p, base=base)
    h = huff.encode_file(pay, tab, shape, p, base=base)
    r = huffr.encode_file(pay, tab, shape, p, base=base)
    nchunks = D.geometry(pay.size)[1]
    assert len(d) <= min(len(h), len(r)) + 4 * nchunks + 12, (name, len(d), len(h), len(r), nchunks)
    assert (D.decode_file(d)[0] == pay).all(), name
    return len(d), len(h), len(r)


def test_size_guarantee_against_tzh1_and_tzr1(mods):
    for name, (pay, _) in constructed_payloads().items():
        _guarantee(mods, name, pay, None, _shape(pay.size), 0)
    for name, pay, tab, shape, p in golden_payloads():
        _guarantee(mods, name, pay, tab, shape, p)


def _file(D, dist=1, n=5000):
    pay = _mixed(n, 3)
    return pay, bytearray(D.encode_file(pay, None, _shape(n), 0, dist=dist))


def test_parser_refusals(mods):
    huff, huffr, D = mods
    pay, good = _file(D, 1)
    assert D.parse(bytes(good)).dist == 1
    bad = bytearray(good)
    bad[44:48] = struct.pack("<I", 2)
    with pytest.raises(ValueError, match="match distance"):
        D.parse(bytes(bad))
    bad[44:48] = struct.pack("<I", 4)
    with pytest.raises(ValueError, match="match distance"):
        D.parse(bytes(bad))
    # D = 0 over a code that gives a repeat token a length
    bad = bytearray(good)
    bad[44:48] = struct.pack("<I", 0)
    assert D.parse(bytes(good)).lengths[-8:].any()
    with pytest.raises(ValueError, match="repeat token"):
        D.parse(bytes(bad))
    _, zero = _file(D, 0)
    p0 = D.parse(bytes(zero))
    assert p0.table is None
    o_len = 48 + 16                                                           # header | 7 trailer values, padded to 16 bytes
    assert bytes(zero[o_len: o_len + p0.A + 8]) == bytes(p0.lengths)
    zero[o_len + p0.A + 2] = 3
    with pytest.raises(ValueError, match="repeat token"):
        D.parse(bytes(zero))
    # each parser knows its own magic only
    for other in (huff, huffr):
        with pytest.raises(ValueError, match="magic"):
            other.parse(bytes(good))
    n = pay.size
    for other in (huff, huffr):
        with pytest.raises(ValueError, match="magic"):
            D.parse(other.encode_file(pay, None, _shape(n), 0))
    with pytest.raises(ValueError):
        D.parse(bytes(good[:40]))
    with pytest.raises(ValueError):
        D.parse(bytes(good[:-4]))


@pytest.mark.parametrize("dist", [0, 1, 3])
def test_random_bodies_decode_to_n_elements(mods, dist):
    huff, huffr, D = mods
    rng = np.random.default_rng(dist)
    for n in (1, 3, 257, 16385, 40001):
        pay, data = _file(D, dist, n)
        p = D.parse(bytes(data))
        words = rng.integers(0, 1 << 32, p.words.size, dtype=np.uint64).astype(np.uint32)
        out = D.decode_body(p.chunk_off, p.run_bits, words, n, p.lengths, p.base, dist)
        assert out.size == n and out.dtype == np.int16
        assert int(out.min()) >= p.base and int(out.max()) < p.base + p.A      # a literal, or a copy of one or of `base`
        ones = np.full(p.words.size, 0xFFFFFFFF, np.uint32)                    # the longest stretches: clamped to the run
        assert D.decode_body(p.chunk_off, p.run_bits, ones, n, p.lengths, p.base, dist).size == n


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
    args = ["-c", str(tmp_path / "model"), str(tmp_path / "data"), str(out), "-p", "0", "-m", "abs", "-b", "2", "--coder", "huffd"]
    if "--sweep" not in extra:
        args += ["-w", "4"]
    r = _cli(args + extra, env)
    assert r.returncode == 2, r.stdout + r.stderr
    assert "ERROR:" in r.stdout and word in r.stdout and "huffd" in r.stdout
    assert "GPU MODE" not in r.stdout and "CPU MODE" not in r.stdout   # refused before a GPU is touched
    assert not out.exists()


@pytest.mark.parametrize("mode", ["-u", "-l"])
def test_cli_refuses_coder_with_uncompress_and_learn(mods, tmp_path, mode):
    out = tmp_path / "dec"
    args = [mode, str(tmp_path / "model"), str(tmp_path / "comp")] + ([str(out)] if mode == "-u" else [])
    r = _cli(args + ["--coder", "huffd"])
    assert r.returncode == 2 and "ERROR:" in r.stdout and "-c" in r.stdout, r.stdout + r.stderr
    assert not out.exists()


def test_run_refuses_for_a_direct_caller(mods, tmp_path, capsys):
    from tezip_amd import compress
    out = tmp_path / "out"
    with pytest.raises(SystemExit) as e:
        compress.run("m", "d", str(out), 0, 4, None, "abs", [2.0], True, False, True, SHUFFLE=True, CODER="huffd")
    assert e.value.code == 2 and "--shuffle" in capsys.readouterr().out
    with pytest.raises(SystemExit) as e:
        compress._run_sharded("m", "d", str(out), 0, 4, None, "abs", [2.0], False, True, 0, False, "huffd")
    assert e.value.code == 2 and "sharded" in capsys.readouterr().out
    assert not out.exists()
