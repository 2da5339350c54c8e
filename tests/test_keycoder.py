"""The opt-in coder of key_frame.dat (`--key-coder huff`, format TZK1) on the CPU: the numpy residuals and their inverses, the
choice of predictors, the container and its validation (tezip_amd/keycoder.py, the specification the kernels are tested
against in tests/test_gpu_keycoder.py), and the command line's refusals.  The built library is needed for
tz_huff_lengths only.  No GPU."""
import struct

import numpy as np
import pytest

SHAPES = [(1, 1), (1, 7), (5, 1), (21, 30), (61, 90)]


@pytest.fixture(scope="module")
def kc():
    from tezip_amd import build
    build.build()
    from tezip_amd import keycoder
    return keycoder


@pytest.fixture(scope="module")
def turbulence_frame():
    from tezip_amd import synth
    return synth.turbulence(nt=2)[0]


@pytest.mark.parametrize("h,w", SHAPES)
def test_unresidual_inverts_residual(kc, h, w):
    rng = np.random.default_rng(h * 100 + w)
    wrap = np.zeros((h, w, 3), np.uint8)
    wrap.reshape(-1)[::2] = 255                                           # 0 / 255 alternating: every difference wraps
    for f in (rng.integers(0, 256, (h, w, 3), dtype=np.uint8), wrap):
        for p in range(4):
            r = kc.residual(f, p)
            assert r.dtype == np.int16 and r.shape == (h * w * 3,) and r.min() >= 0 and r.max() <= 255
            assert (kc.unresidual(r, p, h, w) == f).all(), "predictor %d at %dx%d" % (p, h, w)
        assert (kc.residual(f, 0) == f.reshape(-1)).all()


def test_residual_is_the_formula_of_the_format(kc):
    """Sample by sample, as the format states it: a, b, c of the same channel, zero outside the frame."""
    rng = np.random.default_rng(3)
    h, w = 4, 5
    f = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    for p in range(4):
        want = np.zeros((h, w, 3), np.int64)
        for y in range(h):
            for x in range(w):
                for ch in range(3):
                    a = int(f[y, x - 1, ch]) if x else 0
                    b = int(f[y - 1, x, ch]) if y else 0
                    c = int(f[y - 1, x - 1, ch]) if x and y else 0
                    want[y, x, ch] = (int(f[y, x, ch]) - (0, a, b, a + b - c)[p]) % 256
        assert (kc.residual(f, p) == want.reshape(-1)).all(), p
    for bad in (4, -1):
        with pytest.raises(ValueError, match="predictor id"):
            kc.residual(f, bad)
        with pytest.raises(ValueError, match="predictor id"):
            kc.unresidual(np.zeros(h * w * 3, np.int16), bad, h, w)


@pytest.mark.parametrize("nt,idx", [(1, [0]), (9, [0, 1, 4, 8]), (3, [0, 1, 2])])
def test_file_round_trip(kc, nt, idx):
    from tezip_amd import synth
    h, w = 21, 30
    stack = synth.translating_scene(nt, h, w, seed=2)
    data = kc.encode_file(stack, idx, nt)
    assert kc.is_keycoded(data[:64]) and not kc.is_keycoded(b"\x28\xb5\x2f\xfd")
    p = kc.parse(data)
    assert (p.nt, p.H, p.W, p.nkeys, p.n) == (nt, h, w, len(idx), len(idx) * h * w * 3)
    assert p.idx.tolist() == idx and p.pred.size == len(idx) and p.lengths.size == 256 and len(data) % 4 == 0
    want = np.zeros_like(stack)
    want[idx] = stack[idx]
    assert (kc.decode_file(data) == want).all()
    assert kc.encode_file(stack[idx], idx, nt) == data                   # the key frames alone give the same file
    with pytest.raises(ValueError, match="ascending"):
        kc.encode_file(stack, idx[::-1] + [0], nt)


def test_choose_predictors(kc, turbulence_frame):
    from tezip_amd import synth
    det = synth.detector(nt=1)[0]
    counts = kc.predictor_counts(np.stack([turbulence_frame]))
    assert counts.shape == (1, 4, 256) and (counts.sum(axis=2) == turbulence_frame.size).all()
    assert kc.choose_predictors(counts).tolist() == [3]                  # smooth: the Lorenzo predictor
    assert kc.choose_predictors(kc.predictor_counts(np.stack([det]))).tolist() == [0]   # sparse: no predictor helps
    tie = np.zeros((2, 4, 256), np.int64)
    tie[0, :, 7] = 100                                                   # every predictor costs 0: the lowest id
    tie[1, 0, :2] = 50
    tie[1, 1, :2] = 50
    tie[1, 2, :2] = (99, 1)                                              # cheaper than 0 and 1, equal to 3
    tie[1, 3, :2] = (1, 99)
    assert kc.choose_predictors(tie).tolist() == [0, 2]
    assert (kc.chosen_counts(tie, [0, 2]) == tie[0, 0] + tie[1, 2]).all()


def test_smooth_frame_is_under_half_of_zstd(kc, turbulence_frame):
    from tezip_amd import zstd
    data = kc.encode_file(np.stack([turbulence_frame]), [0], 1)
    z = len(zstd.compress_array(turbulence_frame, 9))
    print("TZK1 %d bytes, zstd-9 %d bytes, ratio %.3f" % (len(data), z, len(data) / z))
    assert len(data) < 0.5 * z
    assert (kc.decode_file(data)[0] == turbulence_frame).all()


def _offsets(kc, p):
    o_pred = 48 + p.nkeys * 4
    o_len = o_pred + ((p.nkeys + 3) & ~3)
    o_idx = o_len + 256
    return dict(keys=48, pred=o_pred, lengths=o_len, index=o_idx, runs=o_idx + p.nchunks * 4)


def test_container_validation_names_the_field(kc, monkeypatch):
    from tezip_amd import _lib
    rng = np.random.default_rng(4)
    nt, h, w, idx = 6, 61, 90, [0, 2, 5]                                 # 49410 symbols: four chunks
    stack = np.minimum(rng.geometric(0.3, (nt, h, w, 3)), 40).astype(np.uint8)
    good = kc.encode_file(stack, idx, nt)
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("validation must not call the library"))
    p = kc.parse(good)
    o = _offsets(kc, p)
    assert p.nchunks == 4

    def bad(mutate, match):
        d = bytearray(good)
        d = mutate(d) or d
        with pytest.raises(ValueError, match=match):
            kc.parse(bytes(d))

    def put(off, fmt, v):
        return lambda d: d.__setitem__(slice(off, off + struct.calcsize(fmt)), struct.pack(fmt, v))

    bad(lambda d: d[:20], "header")
    bad(lambda d: d[:-4], "file size")                                   # truncated
    bad(lambda d: d + b"\0\0\0\0", "file size")
    bad(put(0, "<4s", b"TZK2"), "magic")
    bad(put(4, "<H", 2), "version")
    bad(put(6, "<H", 11), "L = 11")
    bad(put(8, "<I", 0), "nt = 0")
    bad(put(8, "<I", 2), "nkeys = 3")                                    # fewer frames than keys
    bad(put(8, "<I", 5), "key indices")                                  # the last index is 5: out of range
    bad(put(12, "<I", h + 1), "file size|nchunks")                       # H does not fit the file
    bad(put(20, "<I", 4), "C = 4")
    bad(put(24, "<I", 0), "nkeys = 0")
    bad(put(28, "<I", 128), "R = 128")
    bad(put(32, "<I", 32), "chunk of 32 runs")
    bad(put(36, "<I", 3), "nchunks = 3")
    bad(put(40, "<I", p.stream_words + 1), "file size")
    bad(put(o["keys"] + 4, "<I", 0), "key indices")                      # 0, 0, 5: not strictly ascending
    bad(put(o["keys"] + 4, "<I", 7), "key indices")                      # 0, 7, 5
    bad(put(o["pred"] + 1, "<B", 4), "predictor id 4")
    bad(put(o["lengths"], "<B", 13), "code lengths hold 13")
    bad(lambda d: d.__setitem__(slice(o["lengths"], o["lengths"] + 3), b"\x01\x01\x01"), "Kraft")
    bad(lambda d: d.__setitem__(slice(o["lengths"], o["lengths"] + 256), bytes(256)), "no symbol")
    bad(put(o["index"], "<I", 1), "chunk offset")                        # the first offset is not 0
    bad(put(o["index"] + 4, "<I", 1 << 20), "chunk offset")              # past the stream's end
    bad(put(o["index"] + 8, "<I", 1), "chunk offset|run lengths of chunk 1")   # descending
    bad(put(o["index"] + 4, "<I", 1), "run lengths of chunk 0")          # chunk 0 would have one word for all its runs
    bad(put(o["runs"], "<H", 3073), "run length")
    bad(put(o["runs"], "<H", 3000), "run lengths of chunk 0")
    for match in ("key_frame.dat",):                                     # every message names the file
        bad(put(o["lengths"], "<B", 13), match)


def test_numpy_decoder_survives_a_corrupt_body(kc):
    """The clamps of the decoder are exercised here, on the numpy statement: flipped bits in the bit stream give wrong
    samples of the right shape, never an exception (no GPU test feeds a kernel such a body)."""
    rng = np.random.default_rng(8)
    stack = np.minimum(rng.geometric(0.2, (2, 21, 30, 3)), 60).astype(np.uint8)
    d = bytearray(kc.encode_file(stack, [0, 1], 2))
    p = kc.parse(bytes(d))
    for off in rng.integers(len(d) - p.stream_words * 4, len(d), 40):
        d[off] ^= 0xFF
    out = kc.decode_file(bytes(d))
    assert out.shape == stack.shape and out.dtype == np.uint8


def _args(extra):
    from tezip_amd import tezip
    return tezip, tezip.build_parser().parse_args(extra)


@pytest.mark.parametrize("argv,env,word", [
    (["-u", "m", "c", "d", "--key-coder", "huff"], {}, "-c"),
    (["-l", "m", "d", "--key-coder", "huff"], {}, "-c"),
    (["-c", "m", "d", "o", "-p", "0", "-m", "abs", "-b", "2", "--sweep", "4", "8", "--key-coder", "huff"], {}, "--sweep"),
    (["-c", "m", "d", "o", "-p", "0", "-w", "4", "-m", "abs", "-b", "2", "--key-coder", "huff"], {"WORLD_SIZE": "2"}, "sharded"),
])
def test_cli_refuses_key_coder_combinations(kc, monkeypatch, capsys, argv, env, word):
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


def test_flag_is_accepted_where_it_is_valid(kc, monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    base = ["-c", "m", "d", "o", "-p", "0", "-w", "4", "-m", "abs", "-b", "2"]
    for extra in (["--key-coder", "huff"], ["--key-coder", "huff", "--shuffle"], ["--key-coder", "huff", "--coder", "huffr"],
                  ["--key-coder", "huff", "--coder", "huff", "--report"], ["--key-coder", "zstd"], []):
        tezip, arg = _args(base + extra)
        assert tezip.check_key_coder_flag(arg) is None and tezip.check_coder_flag(arg) is None, extra
    tezip, arg = _args(["-u", "m", "c", "d", "--key-coder", "zstd"])    # the default value is no request
    assert tezip.check_key_coder_flag(arg) is None
    with pytest.raises(SystemExit):
        _args(base + ["--key-coder", "lz"])


def test_run_refuses_for_a_direct_caller(kc, tmp_path, monkeypatch, capsys):
    from tezip_amd import compress
    out = tmp_path / "out"
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit) as e:
        compress.run("m", "d", str(out), 0, 4, None, "abs", [2.0], True, False, True, KEY_CODER="lz")
    assert e.value.code == 2 and "--key-coder" in capsys.readouterr().out
    assert compress.check_key_coder("huff", sharded=True) and compress.check_key_coder("huff") is None
    assert not out.exists()


def test_sharded_uncompress_refuses_a_tzk1_file(kc, tmp_path, monkeypatch, capsys):
    from tezip_amd import decompress, synth, weights
    from tezip_amd.prednet import PredNetConfig
    cfg = PredNetConfig(stack_sizes=(3, 16, 32))
    mdir, comp, out = str(tmp_path / "model"), tmp_path / "comp", tmp_path / "dec"
    weights.save_model(mdir, cfg, cfg.init_weights(seed=1), 24, 32)
    comp.mkdir()
    stack = synth.translating_scene(4, 21, 30, seed=1)
    (comp / "key_frame.dat").write_bytes(kc.encode_file(stack, [0, 2], 4))
    (comp / "filename.txt").write_text("1\n" + "".join("f%d.png\n" % i for i in range(4)))
    monkeypatch.setattr(decompress.tzdist, "active", lambda: (1, 2))
    with pytest.raises(SystemExit) as e:
        decompress.run(mdir, str(comp), str(out), True, False)
    assert e.value.code == 2 and "sharded" in capsys.readouterr().out
    assert not any(out.iterdir())
