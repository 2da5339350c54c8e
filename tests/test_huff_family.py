"""The five coded formats that share one Huffman stream (TZH1 `huff`, TZR1 `huffr`, TZR2 `huffd`, TZK1 `keycoder`, TZK2
`keycoderg`) against what the commit before their common code wrote and refused: the SHA-256 of every `encode_file` and the
text of every `parse` refusal were recorded there (tests/golden/huff_family_parent.json, written by
tests/golden/make_huff_family.py) and are recomputed here.  The `huffd` entries were recorded at the commit before huffd.py was
put on huffr.py's tokeniser and decode loop, while it still held its own.  No GPU."""
import hashlib
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

FIXTURE = os.path.join(GOLDEN, "huff_family_parent.json")
SIZES = (1, 255, 256, 257, 16383, 16384, 16385, 3 * 16384 + 5)   # around a run (256) and a chunk (64 runs)


@pytest.fixture(scope="module")
def mods():
    from tezip_amd import build
    build.build()
    from tezip_amd import huff, huffd, huffr, keycoder, keycoderg
    return {"huff": huff, "huffr": huffr, "huffd": huffd, "keycoder": keycoder, "keycoderg": keycoderg}


@pytest.fixture(scope="module")
def parent():
    with open(FIXTURE) as f:
        return json.load(f)


def payload(n, repeats, seed=0):
    """int16[n].  repeats: period-3 stretches broken by a few literals, and none of those in the last 40 elements of a
    run, so a stretch is cut by every run's end.  Otherwise v[i] != v[i - 3] everywhere: no repeat at all."""
    rng = np.random.default_rng(1000 * seed + n)
    i = np.arange(n)
    if not repeats:
        return ((i // 3) % 2 * 5 + rng.integers(0, 5, n) - 4).astype(np.int16)   # differs from v[i - 3] by 1..9
    v = np.array([3, -2, 7])[i % 3]
    spike = (rng.random(n) < 0.03) & (i % 256 < 216)
    return np.where(spike, rng.integers(-9, 10, n), v).astype(np.int16)


def payload_shape(n):
    return (1, 1, 1, max(n // 3, 1), 3)   # the trailer's shape: the payload's own where 3 divides n


def payload_cases():
    for n in SIZES:
        for repeats in (True, False):
            yield "n%d_%s" % (n, "rep" if repeats else "norep"), payload(n, repeats)


def stretches(n):
    """int16[n]: distance-1 stretches of 2^k - 1 and 2^k matches (the `stretches` family of tests/test_gpu_huffd.py)."""
    m = [v for k in range(8) for v in ((1 << k) - 1, 1 << k)]
    groups = np.repeat(np.arange(len(m)) % 5 + 3 * (np.arange(len(m)) % 2), np.array(m) + 1)
    return np.tile(groups, n // groups.size + 1)[:n].astype(np.int16)


def huffd_cases():
    yield from payload_cases()
    yield "n16385_stretches", stretches(16385)


HUFFD_DISTS = (None, 0, 1, 3)   # None: the distance the format's rule chooses
NCASES = {"huff": 16, "huffr": 16, "huffd": 17 * len(HUFFD_DISTS), "keycoder": 12, "keycoderg": 12}


def key_stack(nt, H, W, ngray, seed=0):
    """uint8 (nt, H, W, 3): smooth colour frames with noise, the first `ngray` of them with three equal channels."""
    rng = np.random.default_rng(seed + 7 * nt + 31 * H + ngray)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    out = np.zeros((nt, H, W, 3), np.uint8)
    for t in range(nt):
        f = np.stack([100 + 9 * xx + 3 * t, 60 + 5 * yy, 30 + 2 * xx * yy], -1) + rng.integers(0, 4, (H, W, 3))
        out[t] = f & 255
        if t < ngray:
            out[t] = out[t][:, :, :1]
    return out


def key_cases():
    for nt in (2, 3):
        for H, W in ((5, 7), (16, 16)):
            for label, ngray in (("none", 0), ("one", 1), ("all", nt)):
                yield "nt%d_%dx%d_gray_%s" % (nt, H, W, label), key_stack(nt, H, W, ngray)


def _sections(M, data):
    """(chunk_off, run_bits, words, n, lengths, base) of a TZH1 / TZR1 file, by its header alone."""
    magic, version, L, n, base, A, run, cr, nchunks, sw, tlen, _ = M.HEADER.unpack(data[:48])
    nl = A + (M.NTOK if hasattr(M, "NTOK") else 0)
    o_len = 48 + ((tlen * 2 + 3) & ~3)
    o_idx = o_len + ((nl + 3) & ~3)
    nruns = (n + run - 1) // run
    o_runs = o_idx + nchunks * 4
    o_bits = o_runs + ((nruns * 2 + 3) & ~3)
    buf = np.frombuffer(data, np.uint8)
    return (buf[o_idx:o_runs].view("<u4"), buf[o_runs:o_runs + nruns * 2].view("<u2"), buf[o_bits:].view("<u4"), n, buf[o_len:o_len + nl], base)


def digests(mods):
    """{module: {case: sha256 of encode_file}}; every case is decoded again on the way."""
    out = {k: {} for k in mods}
    for name, pay in payload_cases():
        for k in ("huff", "huffr"):
            M = mods[k]
            data = M.encode_file(pay, None, payload_shape(pay.size), 0)
            if pay.size % 3 == 0:
                dec, p = M.decode_file(data, key_len=pay.size)
                assert p.n == pay.size and type(p) is M.Parsed
            else:   # no (1, nt, H, W, 3) stack has n elements: parse refuses the trailer last of all, the body decodes
                with pytest.raises(ValueError, match=r"entropy.dat \(%s\): element count n = %d, the trailer's shape says %d" % (k, pay.size, max(pay.size // 3, 1) * 3)):
                    M.decode_file(data)
                dec = M.decode_body(*_sections(M, data))
            assert dec.dtype == np.int16 and (dec == pay).all(), (k, name)
            out[k][name] = hashlib.sha256(data).hexdigest()
    chosen = set()
    for name, pay in huffd_cases():
        M = mods["huffd"]
        for dist in HUFFD_DISTS:
            data = M.encode_file(pay, None, payload_shape(pay.size), 0, dist=dist)
            D = M.HEADER.unpack(data[:48])[11]
            if dist is None:
                chosen.add(D)
            else:
                assert D == dist
            if pay.size % 3 == 0:
                dec, p = M.decode_file(data, key_len=pay.size)
                assert p.n == pay.size and type(p) is M.Parsed and p.dist == D
            else:
                with pytest.raises(ValueError, match=r"entropy.dat \(huffd\): element count n = %d, the trailer's shape says %d" % (pay.size, max(pay.size // 3, 1) * 3)):
                    M.decode_file(data)
                dec = M.decode_body(*_sections(M, data), D)
            assert dec.dtype == np.int16 and (dec == pay).all(), ("huffd", name, dist)
            out["huffd"]["%s_d%s" % (name, "chosen" if dist is None else dist)] = hashlib.sha256(data).hexdigest()
    assert chosen == {0, 1, 3}                               # the rule picks every distance somewhere in the cases
    for name, stack in key_cases():
        for k in ("keycoder", "keycoderg"):
            M = mods[k]
            data = M.encode_file(stack, np.arange(stack.shape[0]), stack.shape[0])
            assert (M.decode_file(data) == stack).all(), (k, name)
            out[k][name] = hashlib.sha256(data).hexdigest()
    return out


def _refusal(M, data):
    try:
        M.parse(bytes(data))
    except ValueError as e:
        return str(e)
    return None


def _with_field(M, data, i, value):
    f = list(M.HEADER.unpack(data[:48]))
    f[i] = value
    return M.HEADER.pack(*f) + data[48:]


def _with_words(data, offset, dtype, values):
    b = bytearray(data)
    raw = np.asarray(values, dtype).tobytes()
    b[offset:offset + len(raw)] = raw
    return bytes(b)


def corruptions(M, data, key):
    """(name, corrupted file) of one good three-chunk file: one header or index field at a time."""
    p = M.parse(data)
    f = M.HEADER.unpack(data[:48])
    if not key:   # magic, version, L, n, base, A, R, chunk_runs, nchunks, stream_words, trailer_len
        fields = [("magic", 0, b"TZXX"), ("version", 1, 2), ("L", 2, 11), ("n_zero", 3, 0), ("n_more", 3, f[3] + 16384), ("base", 4, -32769),
                  ("A_zero", 5, 0), ("A_large", 5, 2112), ("A_plus4", 5, f[5] + 4), ("R", 6, 128), ("chunk_runs", 7, 32), ("nchunks", 8, f[8] + 1),
                  ("stream_words", 9, f[9] + 1), ("trailer_len_small", 10, 6), ("trailer_len_large", 10, 2119), ("trailer_len_plus2", 10, f[10] + 2)]
    else:         # magic, version, L, nt, H, W, C, nkeys, R, chunk_runs, nchunks, stream_words
        fields = [("magic", 0, b"TZXX"), ("version", 1, 2), ("L", 2, 11), ("nt_zero", 3, 0), ("H_zero", 4, 0), ("H_more", 4, f[4] + 64), ("W_large", 5, 32768),
                  ("C", 6, 4), ("nkeys_zero", 7, 0), ("nkeys_more", 7, f[3] + 1), ("R", 8, 128), ("chunk_runs", 9, 32), ("nchunks", 10, f[10] + 1),
                  ("stream_words", 11, f[11] + 1)]
    for name, i, v in fields:
        yield name, _with_field(M, data, i, v)
    yield "length_minus1", data[:-1]
    yield "length_plus1", data + b"\0"
    yield "header_cut", data[:47]
    o_co = len(data) - p.body.size
    o_rb = o_co + p.nchunks * 4
    co = p.chunk_off.astype(np.int64)
    assert p.nchunks == 3 and co[1] < co[2]
    yield "first_offset", _with_words(data, o_co, "<u4", [1])
    yield "descending_offset", _with_words(data, o_co + 4, "<u4", [co[2] + 1])
    yield "offset_past_stream", _with_words(data, o_co + 8, "<u4", [p.stream_words + 1])
    yield "oversized_run", _with_words(data, o_rb, "<u2", [256 * 12 + 1])
    yield "chunk_overflow", _with_words(data, o_rb + 2, "<u2", [256 * 12])
    yield "last_chunk_overflow", _with_words(data, o_rb + 2 * (p.nruns - 1), "<u2", [256 * 12])
    if key:
        yield "key_index_descending", _with_words(data, 48 + 4, "<u4", [0])
        yield "key_index_past_nt", _with_words(data, 48 + 4 * (p.nkeys - 1), "<u4", [p.nt])
        o_pred = 48 + 4 * p.nkeys
        yield "pred_4", _with_words(data, o_pred + p.nkeys - 1, np.uint8, [4])
        yield "pred_8", _with_words(data, o_pred + p.nkeys - 1, np.uint8, [8])
        yield "length_13", _with_words(data, o_pred + 4, np.uint8, [13])
    else:
        o_len = o_co - ((p.lengths.size + 3) & ~3)
        yield "length_13", _with_words(data, o_len, np.uint8, [13])
        yield "lengths_all_1", _with_words(data, o_len, np.uint8, [1] * p.lengths.size)
        yield "warm_up", _with_words(data, 48 + 2 * (f[10] - 1), "<i2", [5])


def good_files(mods):
    """One valid file per format, each of three chunks."""
    pay = payload(33000, True, seed=1)                       # 129 runs
    out = {k: mods[k].encode_file(pay, None, (1, 1, 100, 110, 3), 0) for k in ("huff", "huffr", "huffd")}
    out["keycoder"] = mods["keycoder"].encode_file(key_stack(3, 64, 64, 1, seed=1), np.arange(3), 3)    # 64 * 64 * 9 symbols
    out["keycoderg"] = mods["keycoderg"].encode_file(key_stack(3, 64, 80, 1, seed=1), np.arange(3), 3)  # 64 * 80 * 7 symbols
    return out


def refusals(mods):
    """{module: {corruption: text of parse's ValueError, or None where parse accepts the file}}"""
    out = {}
    for k, data in good_files(mods).items():
        out[k] = {name: _refusal(mods[k], bad) for name, bad in corruptions(mods[k], data, k.startswith("key"))}
    M, data = mods["huffd"], good_files(mods)["huffd"]       # the D field, the header's last u32
    assert M.HEADER.unpack(data[:48])[11] == 3 and M.parse(data).lengths[-M.NTOK:].any()
    at0 = M.encode_file(payload(33000, True, seed=1), None, (1, 1, 100, 110, 3), 0, dist=0)
    out["huffd"]["dist_2"] = _refusal(M, _with_field(M, data, 11, 2))
    out["huffd"]["dist_0_with_token_length"] = _refusal(M, _with_field(M, data, 11, 0))
    out["huffd"]["dist_3_coded_at_0"] = _refusal(M, _with_field(M, at0, 11, 3))   # may parse: the index still checks
    return out


def test_coded_bytes_are_the_parents(mods, parent):
    got = digests(mods)
    for k in got:
        assert set(got[k]) == set(parent["digests"][k]) and len(got[k]) == NCASES[k]
        for name in got[k]:
            assert got[k][name] == parent["digests"][k][name], (k, name)


def test_parser_refusals_are_the_parents(mods, parent):
    got = refusals(mods)
    for k in got:
        assert set(got[k]) == set(parent["refusals"][k])
        for name in got[k]:
            assert got[k][name] == parent["refusals"][k][name], (k, name)
        # every corruption above is refused, but for a TZR2 file coded at D = 0 that names D = 3, where the parent says so
        assert {n for n, v in got[k].items() if v is None} <= ({"dist_3_coded_at_0"} if k == "huffd" else set()), k
