"""The opt-in coder of key_frame.dat that stores a gray key frame once (`--key-coder huffg`, format TZK2) on the CPU: the gray
flag, the numpy residuals and their inverses, the container and its validation (tezip_amd/keycoderg.py, the specification the
kernels are tested against in tests/test_gpu_keycoderg.py), its relation to TZK1, and the command line's refusals.  The built
library is needed for tz_huff_lengths only.  No GPU."""
import struct

import numpy as np
import pytest

SHAPES = [(1, 1), (1, 7), (5, 1), (5, 7), (61, 90)]


@pytest.fixture(scope="module")
def kg():
    from tezip_amd import build
    build.build()
    from tezip_amd import keycoderg
    return keycoderg


@pytest.fixture(scope="module")
def kc(kg):
    from tezip_amd import keycoder
    return keycoder


def gray_stack(k, h, w, seed):
    """k smooth-ish gray frames as RGB."""
    rng = np.random.default_rng(seed)
    g = (np.cumsum(rng.integers(-3, 4, (k, h, w)), axis=2) + np.cumsum(rng.integers(-2, 3, (k, h, 1)), axis=1) + 90) & 255
    return np.repeat(g.astype(np.uint8)[..., None], 3, axis=-1)


def colour_stack(k, h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (k, h, w, 3), dtype=np.uint8)


def one_sample_cases(h, w):
    """(name, flat pixel, channel): the three positions at which one sample makes a frame non-gray."""
    return [("channel 1 of pixel 0", 0, 1), ("channel 2 of the last pixel", h * w - 1, 2), ("a pixel in the middle", (h * w) // 2, 0)]


@pytest.mark.parametrize("h,w", SHAPES)
def test_gray_flag_is_exact(kg, h, w):
    g = gray_stack(2, h, w, h * 100 + w)
    assert kg.gray_flags(g).tolist() == [True, True]
    for name, px, ch in one_sample_cases(h, w):
        x = g.copy()
        x[1].reshape(h * w, 3)[px, ch] ^= 1
        assert kg.gray_flags(x).tolist() == [True, False], name
    assert not kg.gray_flags(colour_stack(2, h, w, 1)).any() or h * w == 1


@pytest.mark.parametrize("h,w", SHAPES)
def test_unresidual_inverts_residual(kg, kc, h, w):
    g = gray_stack(1, h, w, h + w)[0]
    c = colour_stack(1, h, w, h + w)[0]
    for p in range(4):
        r = kg.residual(g, p | kg.GRAY)
        assert r.dtype == np.int16 and r.shape == (h * w,) and r.min() >= 0 and r.max() <= 255
        assert (r == kc.residual(g, p)[0::3]).all() and (r == kc.residual(g, p)[2::3]).all()
        assert (kg.unresidual(r, p | kg.GRAY, h, w) == g).all(), "gray, predictor %d at %dx%d" % (p, h, w)
        assert (kg.residual(c, p) == kc.residual(c, p)).all()
        assert (kg.unresidual(kg.residual(c, p), p, h, w) == c).all()
    for bad in (8, -1):
        with pytest.raises(ValueError, match="pred byte"):
            kg.residual(g, bad)
        with pytest.raises(ValueError, match="pred byte"):
            kg.unresidual(np.zeros(h * w, np.int16), bad, h, w)


def mixed_stack(h, w, seed):
    """Six frames; the key frames 0, 2, 5 are gray, colour, gray-but-for-one-sample."""
    x = gray_stack(6, h, w, seed)
    x[2] = colour_stack(1, h, w, seed)[0]
    x[5, h // 2, w // 2, 1] ^= 0x40
    return x, [0, 2, 3, 5]


@pytest.mark.parametrize("h,w", SHAPES)
def test_files_round_trip(kg, h, w):
    for name, x, idx in (("all gray", gray_stack(5, h, w, 7), [0, 3, 4]), ("no gray", colour_stack(4, h, w, 8), [1, 2]),
                         ("mixed",) + mixed_stack(h, w, 9)):
        d = kg.encode_file(x, idx, x.shape[0])
        p = kg.parse(d)
        want = np.zeros_like(x)
        want[idx] = x[idx]
        assert (kg.decode_file(d) == want).all(), name
        flags = kg.gray_flags(x[idx])
        assert (p.gray == flags).all() and (p.pred & 3 == p.pred - 4 * flags).all()
        assert p.n == int(np.where(flags, h * w, h * w * 3).sum()) and p.offsets[0] == 0
        assert (kg.encode_file(x[idx], idx, x.shape[0]) == d), "the key frames alone give the same file"


def test_mixed_file_has_unequal_offsets(kg):
    x, idx = mixed_stack(5, 7, 3)
    p = kg.parse(kg.encode_file(x, idx, 6))
    assert p.gray.tolist() == [True, False, True, False]
    assert p.offsets.tolist() == [0, 35, 35 + 105, 35 + 105 + 35] and p.n == 35 + 105 + 35 + 105


def test_gray_predictor_comes_from_the_one_channel_counts(kg, kc):
    x = gray_stack(3, 21, 30, 5)
    c3 = kc.predictor_counts(x)
    c1 = kg.gray_counts(c3, [True, True, True])
    assert (c1 * 3 == c3).all()
    one = np.stack([[np.bincount(kc.residual(f, p)[0::3], minlength=256) for p in range(4)] for f in x])
    assert (c1 == one).all(), "a third of the three-channel counts is the count of channel 0"
    p = kg.parse(kg.encode_file(x, [0, 1, 2], 3))
    assert (p.pred == (kc.choose_predictors(c1) | 4)).all()
    with pytest.raises(ValueError, match="multiples of 3"):
        kg.gray_counts(kc.predictor_counts(colour_stack(1, 5, 7, 1)), [True])


def _header(d):
    return list(struct.unpack("<4sHH10I", bytes(d[:48])))


def _with_header(d, **kw):
    names = ["magic", "version", "L", "nt", "H", "W", "C", "nkeys", "R", "chunk_runs", "nchunks", "stream_words", "zero"]
    h = _header(d)
    for k, v in kw.items():
        h[names.index(k)] = v
    return struct.pack("<4sHH10I", *h) + bytes(d[48:])


def test_parse_refusals(kg, kc):
    x, idx = mixed_stack(61, 90, 4)
    d = kg.encode_file(x, idx, 6)
    p = kg.parse(d)
    o_pred = 48 + 4 * len(idx)
    for bad in (8, 12, 255):
        e = bytearray(d)
        e[o_pred + 1] = bad
        with pytest.raises(ValueError, match="pred byte"):
            kg.parse(bytes(e))
    # a pred byte whose GRAY bit is flipped changes n: the file no longer describes its own index
    # (n changes by 2 * 5490 symbols: 3 chunks still with fewer runs, or 4 chunks)
    e = bytearray(d)
    e[o_pred + 1] |= 4
    with pytest.raises(ValueError, match="file size"):
        kg.parse(bytes(e))
    e = bytearray(d)
    e[o_pred] &= 3
    with pytest.raises(ValueError, match="nchunks"):
        kg.parse(bytes(e))
    with pytest.raises(ValueError, match="nchunks"):
        kg.parse(_with_header(d, nchunks=p.nchunks + 1))
    with pytest.raises(ValueError, match="nchunks"):
        kg.parse(_with_header(d, H=20))       # (a wrong n through the shape: 1 chunk instead of 3)
    with pytest.raises(ValueError, match="file size"):
        kg.parse(_with_header(d, H=60))       # (3 chunks still, fewer runs)
    with pytest.raises(ValueError, match="file size"):
        kg.parse(d[:-4])
    with pytest.raises(ValueError, match="file size"):
        kg.parse(_with_header(d, stream_words=p.stream_words + 1))
    with pytest.raises(ValueError, match="magic"):
        kg.parse(_with_header(d, magic=b"TZK1"))
    with pytest.raises(ValueError, match="magic"):
        kg.parse(kc.encode_file(x, idx, 6))
    with pytest.raises(ValueError, match="magic"):
        kc.parse(d)
    with pytest.raises(ValueError, match="C = "):
        kg.parse(_with_header(d, C=1))
    with pytest.raises(ValueError, match="version"):
        kg.parse(_with_header(d, version=2))
    with pytest.raises(ValueError, match="shorter"):
        kg.parse(d[:40])
    with pytest.raises(ValueError, match="shorter"):
        kg.parse(d[:60])
    with pytest.raises(ValueError, match="ascending"):
        e = bytearray(d)
        e[48:52], e[52:56] = e[52:56], e[48:52]
        kg.parse(bytes(e))
    assert kg.is_keycoded(d[:4]) and not kc.is_keycoded(d[:4]) and not kg.is_keycoded(b"TZK1")


def test_corrupt_body_decodes_to_wrong_samples_only(kg):
    rng = np.random.default_rng(5)
    x, idx = mixed_stack(21, 30, 6)
    d = bytearray(kg.encode_file(x, idx, 6))
    p = kg.parse(bytes(d))
    for off in rng.integers(len(d) - p.stream_words * 4, len(d), 40):
        d[off] ^= 0xFF
    out = kg.decode_file(bytes(d))
    assert out.shape == x.shape and out.dtype == np.uint8
    for k, i in enumerate(idx):
        if p.gray[k]:
            assert (out[i, ..., 0] == out[i, ..., 1]).all() and (out[i, ..., 1] == out[i, ..., 2]).all()


def test_all_gray_file_is_a_third_of_tzk1(kg, kc):
    """A gray stack's TZK2 body holds a third of TZK1's symbols under the same code lengths.  The two layouts share the
    304 + 4 k + pad4(k) bytes in front of the index (k key frames); the index has 4 bytes per chunk of 16384 symbols and 2 per
    run of 256; the bit stream is padded to a word per chunk.  So len(TZK2) - len(TZK1) / 3 is two thirds of the front plus
    rounding of a few bytes per chunk: far inside the 512 bytes of slack for the handful of key frames used here."""
    from tezip_amd import synth
    for x, idx in ((synth.moving_blobs(12, 64, 64), [0, 4, 8]), (synth.detector(1, 256, 256), [0]), (gray_stack(4, 61, 90, 2), [0, 1, 2, 3])):
        a, b = kg.encode_file(x, idx, x.shape[0]), kc.encode_file(x, idx, x.shape[0])
        pa, pb = kg.parse(a), kc.parse(b)
        print("TZK2 %d bytes, TZK1 %d bytes, slack used %.1f" % (len(a), len(b), len(a) - len(b) / 3))
        assert pa.gray.all() and pa.n * 3 == pb.n
        assert (pa.pred & 3 == pb.pred).all() and (pa.lengths == pb.lengths).all()
        assert len(a) <= len(b) / 3 + 512


def test_file_without_a_gray_frame_is_tzk1_but_for_the_magic(kg, kc):
    from tezip_amd import synth
    for x, idx in ((synth.translating_scene(12, 61, 90), [0, 5, 9]), (colour_stack(3, 5, 7, 3), [1])):
        a, b = kg.encode_file(x, idx, x.shape[0]), kc.encode_file(x, idx, x.shape[0])
        assert a[:4] == b"TZK2" and b[:4] == b"TZK1" and a[4:] == b[4:]


def _args(extra):
    from tezip_amd import tezip
    return tezip, tezip.build_parser().parse_args(extra)


@pytest.mark.parametrize("argv,env,word", [
    (["-u", "m", "c", "d", "--key-coder", "huffg"], {}, "-c"),
    (["-l", "m", "d", "--key-coder", "huffg"], {}, "-c"),
    (["-c", "m", "d", "o", "-p", "0", "-m", "abs", "-b", "2", "--sweep", "4", "8", "--key-coder", "huffg"], {}, "--sweep"),
    (["-c", "m", "d", "o", "-p", "0", "-w", "4", "-m", "abs", "-b", "2", "--key-coder", "huffg"], {"WORLD_SIZE": "2"}, "sharded"),
])
def test_cli_refuses_key_coder_combinations(kg, monkeypatch, capsys, argv, env, word):
    tezip, arg = _args(argv)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setattr(tezip, "probe_gpu", lambda force: pytest.fail("refused before a GPU is touched"))
    assert word in tezip.check_key_coder_flag(arg)
    with pytest.raises(SystemExit) as e:
        tezip.main(arg)
    out = capsys.readouterr().out
    assert e.value.code == 2 and out.startswith("ERROR:") and word in out and len(out.strip().splitlines()) == 1


def test_flag_is_accepted_where_it_is_valid(kg, monkeypatch):
    from tezip_amd import compress
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    base = ["-c", "m", "d", "o", "-p", "0", "-w", "4", "-m", "abs", "-b", "2"]
    for extra in (["--key-coder", "huffg"], ["--key-coder", "huffg", "--shuffle"], ["--key-coder", "huffg", "--coder", "huffr"],
                  ["--key-coder", "huffg", "--coder", "huff", "--report", "--digests"]):
        tezip, arg = _args(base + extra)
        assert tezip.check_key_coder_flag(arg) is None and tezip.check_coder_flag(arg) is None, extra
    assert compress.check_key_coder("huffg", sharded=True) and compress.check_key_coder("huffg") is None


def test_sharded_uncompress_refuses_a_tzk2_file(kg, tmp_path, monkeypatch, capsys):
    from tezip_amd import decompress, synth, weights
    from tezip_amd.prednet import PredNetConfig
    cfg = PredNetConfig(stack_sizes=(3, 16, 32))
    mdir, comp, out = str(tmp_path / "model"), tmp_path / "comp", tmp_path / "dec"
    weights.save_model(mdir, cfg, cfg.init_weights(seed=1), 24, 32)
    comp.mkdir()
    stack = synth.moving_blobs(4, 32, 40, seed=1)
    (comp / "key_frame.dat").write_bytes(kg.encode_file(stack, [0, 2], 4))
    (comp / "filename.txt").write_text("1\n" + "".join("f%d.png\n" % i for i in range(4)))
    monkeypatch.setattr(decompress.tzdist, "active", lambda: (1, 2))
    with pytest.raises(SystemExit) as e:
        decompress.run(mdir, str(comp), str(out), True, False)
    assert e.value.code == 2 and "sharded" in capsys.readouterr().out
