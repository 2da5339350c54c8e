"""The 2-D spatial delta of the payload on the CPU (`-c --sdelta plane`, definition TZ-SD2, tezip_amd/sdelta.py): the numpy
statement of the format on the literal example, its round trips at the edge shapes, the wrap, frame independence, the trailer
checks of `-u`, the Huffman files, the sidecar key, the refusals of the command line, and the size on smooth colour data."""
import json

import numpy as np
import pytest

EXTREMES = np.array([-255, -254, 0, 254, 255], np.int16)


@pytest.fixture(scope="module")
def sd():
    from tezip_amd import sdelta
    return sdelta


def _extreme_stack(shape, seed):
    return np.random.default_rng(seed).choice(EXTREMES, size=shape).astype(np.int16)


def test_the_literal_example(sd):
    q = np.array([[255, -255], [-255, 255]], np.int16).reshape(1, 2, 2, 1)
    assert sd.encode_plane(q, False).tolist() == [-255, -2, -2, 4]
    assert sd.encode_plane(q, True).tolist() == [1855, 1602, 1602, 1596]
    assert sd.decode_plane(sd.encode_plane(q, True), q.shape, True).tolist() == q.reshape(-1).tolist()
    assert (sd.MARK_PLANE, sd.MARK_PLANE_SHUFFLE) == (8, 9) and "plane" in sd.MODES
    assert sd.mark(False, plane=True) == 8 and sd.mark(True, plane=True) == 9


def test_the_definition_element_by_element(sd):
    q = _extreme_stack((2, 3, 4, 3), 1)
    y = sd.encode_plane(q, False).reshape(q.shape)
    g = lambda f, r, x, c: int(q[f, r, x, c]) if r >= 0 and x >= 0 else 0
    for f, r, x, c in np.ndindex(*q.shape):
        v = g(f, r, x - 1, c) + g(f, r - 1, x, c) - g(f, r - 1, x - 1, c) - g(f, r, x, c)
        assert int(y[f, r, x, c]) == (v + 256) % 512 - 256, (f, r, x, c)


@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (1, 1, 1, 3), (1, 1, 9, 3), (3, 9, 1, 1), (1, 1, 9, 1), (3, 9, 1, 3), (1, 3, 5, 3),
                                   (3, 7, 11, 3), (3, 7, 11, 1), (1, 16, 24, 1)])
@pytest.mark.parametrize("offset", [False, True])
def test_round_trip(sd, shape, offset):
    for q in (_extreme_stack(shape, sum(shape)), np.random.default_rng(2).integers(-255, 256, shape).astype(np.int16)):
        y = sd.encode_plane(q, offset)
        assert y.dtype == np.int16 and y.shape == (q.size,)
        np.testing.assert_array_equal(sd.decode_plane(y, shape, offset), q.reshape(-1))
    # the inverse in int16 arithmetic: cumulative sums mod 2^16, as the kernels take them
    s = (-sd.encode_plane(q, False).astype(np.int64)).astype(np.int16).reshape(shape)
    with np.errstate(over="ignore"):
        S = np.cumsum(np.cumsum(s, axis=1, dtype=np.int16), axis=2, dtype=np.int16)
    np.testing.assert_array_equal(sd.wrap9(S).astype(np.int16), q)


def test_symbols_stay_in_the_alphabet_and_the_wrap_is_exercised(sd):
    q = _extreme_stack((3, 16, 24, 3), 7)
    y = sd.encode_plane(q, True)
    assert y.min() >= 1345 and y.max() <= 1856
    p = np.zeros(q.shape, np.int64)
    p[:, :, 1:] += q[:, :, :-1]
    p[:, 1:, :] += q[:, :-1, :]
    p[:, 1:, 1:] -= q[:, :-1, :-1]
    raw = p - q
    wrapped = (raw < -256) | (raw > 255)
    assert wrapped.mean() > 0.25, wrapped.mean()
    np.testing.assert_array_equal(sd.decode_plane(y, q.shape, True), q.reshape(-1))
    with pytest.raises(ValueError):
        sd.encode_plane(np.full((1, 2, 2, 1), 256, np.int16), True)


def test_frames_are_coded_on_their_own(sd):
    q = _extreme_stack((2, 5, 6, 3), 9)
    y = sd.encode_plane(q, True).reshape(q.shape)
    q2 = q.copy()
    q2[0] = _extreme_stack(q[0].shape, 10)
    y2 = sd.encode_plane(q2, True).reshape(q.shape)
    assert (y2[0] != y[0]).any()
    np.testing.assert_array_equal(y2[1], y[1])
    np.testing.assert_array_equal(sd.encode_plane(q[1:], True), y[1].reshape(-1))       # a frame's symbols are its own stack's
    np.testing.assert_array_equal(sd.decode_plane(y[1], (1,) + q.shape[1:], True), q[1].reshape(-1))


def test_payload_layout_arguments(sd):
    q = np.random.default_rng(4).integers(-40, 41, (3, 9, 11, 3)).astype(np.int16)
    payload, table = sd.payload_from_delta(q, True, plane=True)
    y = sd.encode_plane(q, True)
    np.testing.assert_array_equal(np.asarray(table)[payload], y)
    assert table.tolist() == sd.build_table(y).tolist()
    np.testing.assert_array_equal(sd.delta_from_payload(payload, table, plane_shape=q.shape), q.reshape(-1))
    raw, none = sd.payload_from_delta(q, False, plane=True)
    assert none is None
    np.testing.assert_array_equal(raw, sd.encode_plane(q, False))
    np.testing.assert_array_equal(sd.delta_from_payload(raw, None, plane_shape=q.shape), q.reshape(-1))
    # on one channel plane is NOT the flat delta
    q1 = q[..., :1]
    assert (sd.encode_plane(q1, True) != sd.encode(q1, 1, True)).any()


def test_check_stream_accepts_the_plane_marks(sd):
    from tezip_amd import compress, decompress
    nt, h, w = 2, 4, 5
    n1 = nt * h * w
    decompress.check_stream((8, nt, h, w, 3), 0, n1 * 3, n1 * 3)
    decompress.check_stream((8, nt, h, w, 1), 1, n1, n1 * 3)           # a --gray plane stream is marked
    decompress.check_stream((9, nt, h, w, 3), 0, n1 * 3, n1 * 3)
    decompress.check_stream((9, nt, h, w, 1), 0, n1, n1 * 3)
    for one in (3, 6, 7, 10):
        with pytest.raises(ValueError, match="shape"):
            decompress.check_stream((one, nt, h, w, 3), 0, n1 * 3, n1 * 3)
    for one in (4, 5):
        with pytest.raises(ValueError, match="shape"):
            decompress.check_stream((one, nt, h, w, 1), 0, n1, n1 * 3)
    assert [sd.is_plane(v) for v in (1, 2, 4, 5, 8, 9)] == [False, False, False, False, True, True]
    assert [sd.is_strided(v) for v in (1, 2, 3, 4, 5, 8, 9)] == [False, False, False, True, True, False, False]
    assert [sd.is_shuffled(v) for v in (1, 2, 4, 5, 8, 9)] == [False, True, False, True, False, True]
    p, t, shape, warm = decompress.parse_stream(
        compress.build_stream(np.arange(n1, dtype=np.int16), np.array([1600, 1601], np.int16), (8, nt, h, w, 1), 1).tobytes())
    assert shape == (8, nt, h, w, 1) and warm == 1
    decompress.check_stream(shape, warm, p.size, n1 * 3)


@pytest.mark.parametrize("fmt_name", ["huff", "huffr", "huffd"])
@pytest.mark.parametrize("channels", [3, 1])
def test_coded_files_carry_the_mark_verbatim(sd, fmt_name, channels):
    import importlib
    fmt = importlib.import_module("tezip_amd." + fmt_name)
    nt, h, w = 3, 9, 11
    q = np.random.default_rng(5).integers(-30, 31, (nt, h, w, channels)).astype(np.int16)
    payload, table = sd.payload_from_delta(q, True, plane=True)
    data = fmt.encode_file(payload, table, (8, nt, h, w, channels), 0)
    got, p = fmt.decode_file(data, nt * h * w * 3)
    assert tuple(p.shape) == (8, nt, h, w, channels)
    np.testing.assert_array_equal(got, payload)
    np.testing.assert_array_equal(sd.delta_from_payload(got, p.table, plane_shape=q.shape), q.reshape(-1))
    for one in (9, 7, 6, 3):           # byte planes are never Huffman-coded
        with pytest.raises(ValueError, match="shape"):
            fmt.parse(fmt.encode_file(payload, table, (one, nt, h, w, channels), 0), nt * h * w * 3)


def test_sidecar_key(tmp_path, monkeypatch):
    from tezip_amd import _lib, decompress, sidecar

    class Lib:
        @staticmethod
        def tz_version():
            return 101

    monkeypatch.setattr(_lib, "load", lambda: Lib)
    wts = [np.zeros(3, np.float32)]
    plain, plane = tmp_path / "plain", tmp_path / "plane"
    plain.mkdir()
    plane.mkdir()
    assert "sdelta" not in sidecar.write(str(plain), 2, wts, 64, 64, (12, 64, 64, 0))
    assert sidecar.write(str(plane), 2, wts, 64, 64, (12, 64, 64, 0), sdelta="plane")["sdelta"] == "plane"
    assert json.loads((plane / sidecar.NAME).read_text())["sdelta"] == "plane"
    assert sidecar.sdelta_of(sidecar.read(str(plane))) == "plane"
    # the trailer is authoritative: a sidecar that says otherwise is an error, no sidecar is no opinion
    assert decompress.check_sdelta(str(plane), 8) == 2 and decompress.check_sdelta(str(plane), 9) == 2
    assert decompress.check_sdelta(str(tmp_path), 8) == 2
    for one in (1, 2, 4, 5):
        with pytest.raises(ValueError, match="spatial delta"):
            decompress.check_sdelta(str(plane), one)
    with pytest.raises(ValueError, match="spatial delta"):
        decompress.check_sdelta(str(plain), 8)

    class Ctx:
        calls = []

        def set_delta_plane(self, on):
            self.calls.append(("plane", on))

        def set_delta_stride(self, mode):
            self.calls.append(("stride", mode))

    for mode in (0, 1, 2):
        decompress.set_sdelta(Ctx(), mode)
    assert Ctx.calls == [("stride", 0), ("stride", 1), ("plane", 1)]


def _args(extra):
    from tezip_amd import tezip
    return tezip, tezip.build_parser().parse_args(extra)


COMPRESS = ["-c", "m", "d", "o", "-p", "0", "-w", "4", "-m", "abs", "-b", "2"]


@pytest.mark.parametrize("argv,env,word", [
    (["-u", "m", "c", "d", "--sdelta", "plane"], {}, "-c"),
    (["-l", "m", "d", "--sdelta", "plane"], {}, "-c"),
    (["-c", "m", "d", "o", "-p", "0", "-m", "abs", "-b", "2", "--sweep", "4", "8", "--sdelta", "plane"], {}, "--sweep"),
    (COMPRESS + ["--sdelta", "plane"], {"WORLD_SIZE": "2"}, "sharded"),
    (COMPRESS[:8] + ["--sdelta", "plane", "--target-ratio", "4", "--coder", "huffd"], {}, "size probe"),
])
def test_cli_refusals(monkeypatch, capsys, argv, env, word):
    tezip, arg = _args(argv)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setattr(tezip, "probe_gpu", lambda force: pytest.fail("refused before a GPU is touched"))
    assert word in tezip.check_sdelta_flag(arg)
    with pytest.raises(SystemExit) as e:
        tezip.main(arg)
    out = capsys.readouterr().out
    assert e.value.code == 2 and out.startswith("ERROR:") and word in out and len(out.strip().splitlines()) == 1


def test_flag_is_accepted_where_it_is_valid_and_reaches_run(monkeypatch, capsys):
    from tezip_amd import compress
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit):
        _args(COMPRESS + ["--sdelta", "row"])
    capsys.readouterr()
    checks = ("check_sdelta_flag", "check_gray_flag", "check_coder_flag", "check_key_coder_flag", "check_report_flag",
              "check_digests_flag", "check_ssim_flag", "check_quant_flag", "check_target_flag")
    for extra in (["--sdelta", "plane"], ["--sdelta", "plane", "--shuffle"], ["--sdelta", "plane", "-n"],
                  ["--sdelta", "plane", "--quant", "lattice"], ["--sdelta", "plane", "-t", "0.01"],
                  ["--sdelta", "plane", "--gray", "--coder", "huffd", "--key-coder", "huffg", "--report", "--ssim", "--digests"],
                  ["--sdelta", "plane", "--coder", "huff"], ["--sdelta", "plane", "--coder", "huffr", "--key-coder", "huff"]):
        tezip, arg = _args(COMPRESS + extra)
        for name in checks:
            assert getattr(tezip, name)(arg) is None, (extra, name)
    for extra in (["--target-psnr", "40"], ["--target-psnr", "40", "--per-frame"], ["--frame-bounds", "b.json"]):
        tezip, arg = _args(COMPRESS[:8] + ["--sdelta", "plane"] + extra)
        for name in checks:
            assert getattr(tezip, name)(arg) is None, (extra, name)
    assert compress.check_sdelta("plane", sharded=True) and compress.check_sdelta("plane") is None
    assert "row" in compress.check_sdelta("row") and "plane" in compress.check_sdelta("row")
    seen = {}
    monkeypatch.setattr(tezip, "probe_gpu", lambda force: True)
    monkeypatch.setattr(compress, "run", lambda *a, **kw: seen.update(kw))
    tezip.main(_args(COMPRESS + ["--sdelta", "plane", "--coder", "huffd", "--digests", "--gray"])[1])
    assert seen["SDELTA"] == "plane" and seen["CODER"] == "huffd" and seen["DIGESTS"] is True and seen["GRAY"] is True
    seen.clear()
    tezip.main(_args(COMPRESS + ["--sdelta", "plane", "--quant", "lattice"])[1])
    assert seen["SDELTA"] == "plane" and seen["QUANT"] == "lattice"
    seen.clear()
    tezip.main(_args(COMPRESS[:8] + ["--sdelta", "plane", "--target-psnr", "40", "--per-frame"])[1])
    assert seen["SDELTA"] == "plane" and seen["PER_FRAME"] is True


def test_a_direct_caller_of_run_is_refused(monkeypatch, capsys):
    from tezip_amd import compress
    monkeypatch.setattr(compress.tzdist, "active", lambda: (0, 2))
    with pytest.raises(SystemExit) as e:
        compress.run("m", "d", "o", 0, 4, None, "abs", [2.0], True, False, True, SDELTA="plane")
    assert e.value.code == 2 and "sharded" in capsys.readouterr().out
    monkeypatch.setattr(compress.tzdist, "active", lambda: None)
    with pytest.raises(SystemExit) as e:
        compress.run("m", "d", "o", 0, 4, None, "abs", [], True, False, True, SDELTA="plane", TARGET_RATIO=4.0, CODER="huffd")
    out = capsys.readouterr().out
    assert e.value.code == 2 and "size probe" in out and "--target-ratio" in out


def test_a_sharded_decoder_refuses_a_plane_stream(tmp_path, monkeypatch, capsys):
    from tezip_amd import compress, decompress, zstd
    nt, h, w = 2, 8, 8
    n = nt * h * w * 3
    (tmp_path / "filename.txt").write_text("1\n" + "".join("f%d.png\n" % i for i in range(nt)))
    (tmp_path / "key_frame.dat").write_bytes(zstd.compress_array(np.zeros(n, np.uint8), 9))
    stream = compress.build_stream(np.zeros(n, np.int16), np.array([1600], np.int16), (8, nt, h, w, 3), 0)
    (tmp_path / "entropy.dat").write_bytes(zstd.compress_array(stream, 9))
    monkeypatch.setattr(decompress.tzdist, "active", lambda: (0, 2))
    monkeypatch.setattr(decompress, "open_model", lambda d: (None, [np.zeros(1, np.float32)], None))
    monkeypatch.setattr(decompress, "make_context", lambda *a, **k: pytest.fail("refused before a GPU is touched"))
    with pytest.raises(SystemExit) as e:
        decompress.run("m", str(tmp_path), str(tmp_path / "out"), True, False)
    assert e.value.code == 2 and "--sdelta plane" in capsys.readouterr().out


def test_the_context_has_the_new_calls():
    from tezip_amd import _lib
    assert hasattr(_lib.Context, "set_delta_plane") and hasattr(_lib.Context, "spatial_delta_plane")
    assert hasattr(_lib.Context, "spatial_undelta_plane") and hasattr(_lib.Context, "get_delta_plane")


def test_plane_is_smaller_on_smooth_colour_data(sd):
    """synth.turbulence(7, 128, 128) under the previous-frame predictor, lossless: the order-0 cost of the plane symbols is
    below 0.85 x that of the channel-stride symbols (measured: 142 541 against 179 356 bytes, 0.795)."""
    from tezip_amd import lattice, synth
    _, d, _ = lattice.previous_frame_deltas(synth.turbulence(7, 128, 128), 0)
    q = d[1:]
    channel = lattice.order0_bytes(sd.encode(q, 3, True))
    plane = lattice.order0_bytes(sd.encode_plane(q, True))
    print("order-0 bytes: channel %d, plane %d, ratio %.3f" % (channel, plane, plane / channel))
    assert plane < 0.85 * channel
    np.testing.assert_array_equal(sd.decode_plane(sd.encode_plane(q, True), q.shape, True), q.reshape(-1))
