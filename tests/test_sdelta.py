"""The spatial delta at the channel stride on the CPU (`-c --sdelta channel`, tezip_amd/sdelta.py): the numpy statement of the
format round-trips and is the oracle's finding_difference at stride 1, the trailer checks of `-u`, the sidecar key, the
refusals of the command line, and the golden payloads re-encoded at stride 3."""
import glob
import json
import os

import numpy as np
import pytest

from oracle import oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def sd():
    from tezip_amd import sdelta
    return sdelta


def _full_range(n, seed):
    x = np.random.default_rng(seed).integers(-32768, 32768, n, dtype=np.int16)
    x[:2] = [32767, -32768][:min(n, 2)]                    # differences that wrap
    return x


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 3001])
@pytest.mark.parametrize("stride", [1, 3])
def test_round_trip_on_full_range_int16(sd, n, stride):
    x = _full_range(n, n)
    carry = np.array([32767, -32768, 12345], np.int16)[:stride]
    for c in (None, carry):
        for offset in (False, True):
            y = sd.encode(x, stride, offset, c)
            assert y.dtype == np.int16 and y.shape == (n,)
            np.testing.assert_array_equal(sd.decode(y, stride, offset, c), x)
    # the definition, element by element, with Python integers
    y = sd.encode(x, stride, False)
    for i in range(n):
        want = int(x[i]) if i < stride else int(x[i - stride]) - int(x[i])
        assert int(y[i]) == (want + 32768) % 65536 - 32768, i
    yc = sd.encode(x, stride, True, carry)
    for i in range(min(n, stride)):
        assert int(yc[i]) == (1600 - (int(carry[i]) - int(x[i])) + 32768) % 65536 - 32768
    if n > stride:                                           # a decoder that starts behind a prefix
        n0 = (n - 1) // stride * stride
        c0 = sd.carry_of(x, n0, stride)
        np.testing.assert_array_equal(sd.decode(y[n0:], stride, False, c0), x[n0:])
        np.testing.assert_array_equal(sd.encode(x[n0:], stride, False, c0), y[n0:])


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 3001])
def test_stride_one_is_the_oracles_finding_difference(sd, n):
    x = _full_range(n, 100 + n)
    np.testing.assert_array_equal(sd.encode(x, 1, False), O.finding_difference_enc(x))
    np.testing.assert_array_equal(sd.decode(x, 1, False), O.finding_difference_dec(x))
    np.testing.assert_array_equal(sd.decode(O.finding_difference_enc(x), 1, False), x)


def test_payload_is_the_oracle_with_the_strided_delta(sd):
    """Offset, table and remap are the reference's (the oracle's remap and table on the strided symbols)."""
    rng = np.random.default_rng(3)
    delta = rng.integers(-40, 41, (3, 9, 11, 3)).astype(np.int16)
    payload, table = sd.payload_from_delta(delta, True)
    y = (1600 - sd.encode(delta, 3, False).astype(np.int64)).astype(np.int16)
    assert y.min() >= 1600 - 510 and y.max() <= 1600 + 510
    counts = np.bincount(y.astype(np.int64))
    order = sorted(np.nonzero(counts)[0], key=lambda s: (-counts[s], s))
    assert table.tolist() == order
    np.testing.assert_array_equal(np.asarray(table)[payload], y)
    np.testing.assert_array_equal(sd.delta_from_payload(payload, table), delta.reshape(-1))
    raw, none = sd.payload_from_delta(delta, False)
    assert none is None
    np.testing.assert_array_equal(sd.delta_from_payload(raw, None), delta.reshape(-1))


def test_check_stream_accepts_the_marks_with_three_channels_only(sd):
    from tezip_amd import compress, decompress
    nt, h, w = 2, 4, 5
    n1 = nt * h * w
    assert (sd.MARK, sd.MARK_SHUFFLE) == (4, 5) and sd.mark(False) == 4 and sd.mark(True) == 5
    decompress.check_stream((4, nt, h, w, 3), 0, n1 * 3, n1 * 3)
    decompress.check_stream((5, nt, h, w, 3), 1, n1 * 3, n1 * 3)
    decompress.check_stream((1, nt, h, w, 3), 0, n1 * 3, n1 * 3)                    # the reference's, as ever
    decompress.check_stream((compress.SHUFFLE_MARK, nt, h, w, 3), 0, n1 * 3, n1 * 3)
    with pytest.raises(ValueError, match="shape"):
        decompress.check_stream((3, nt, h, w, 3), 0, n1 * 3, n1 * 3)
    for one in (4, 5):
        with pytest.raises(ValueError, match="shape"):
            decompress.check_stream((one, nt, h, w, 1), 0, n1, n1 * 3)             # one channel has stride 1: never marked
    with pytest.raises(ValueError, match="shape"):
        decompress.check_stream((6, nt, h, w, 3), 0, n1 * 3, n1 * 3)
    assert [sd.is_strided(v) for v in (1, 2, 3, 4, 5)] == [False, False, False, True, True]
    assert [sd.is_shuffled(v) for v in (1, 2, 4, 5)] == [False, True, False, True]
    payload = np.arange(n1 * 3, dtype=np.int16)
    table = np.array([1600, 1601], np.int16)
    p, t, shape, warm = decompress.parse_stream(compress.build_stream(payload, table, (4, nt, h, w, 3), 1).tobytes())
    assert shape == (4, nt, h, w, 3) and warm == 1
    decompress.check_stream(shape, warm, p.size, n1 * 3)


@pytest.mark.parametrize("fmt_name", ["huff", "huffr", "huffd"])
def test_coded_files_carry_the_mark_verbatim(sd, fmt_name):
    import importlib
    fmt = importlib.import_module("tezip_amd." + fmt_name)
    nt, h, w = 3, 9, 11
    delta = np.random.default_rng(5).integers(-30, 31, (nt, h, w, 3)).astype(np.int16)
    payload, table = sd.payload_from_delta(delta, True)
    data = fmt.encode_file(payload, table, (4, nt, h, w, 3), 0)
    got, p = fmt.decode_file(data, nt * h * w * 3)
    assert tuple(p.shape) == (4, nt, h, w, 3)
    np.testing.assert_array_equal(got, payload)
    for shape in ((3, nt, h, w, 3), (5, nt, h, w, 3), (2, nt, h, w, 3)):           # byte planes are never Huffman-coded
        with pytest.raises(ValueError, match="shape"):
            fmt.parse(fmt.encode_file(payload, table, shape, 0), nt * h * w * 3)
    with pytest.raises(ValueError, match="shape"):
        fmt.parse(fmt.encode_file(payload[: nt * h * w], table, (4, nt, h, w, 1), 0), nt * h * w * 3)


def test_sidecar_key(tmp_path, monkeypatch):
    from tezip_amd import _lib, decompress, sidecar

    class Lib:
        @staticmethod
        def tz_version():
            return 101

    monkeypatch.setattr(_lib, "load", lambda: Lib)
    wts = [np.zeros(3, np.float32)]
    plain, chan = tmp_path / "plain", tmp_path / "chan"
    plain.mkdir()
    chan.mkdir()
    assert "sdelta" not in sidecar.write(str(plain), 2, wts, 64, 64, (12, 64, 64, 0))
    assert "sdelta" not in sidecar.write(str(plain), 2, wts, 64, 64, (12, 64, 64, 0), sdelta="flat")
    assert sidecar.write(str(chan), 2, wts, 64, 64, (12, 64, 64, 0), sdelta="channel")["sdelta"] == "channel"
    assert "sdelta" not in json.loads((plain / sidecar.NAME).read_text())
    assert json.loads((chan / sidecar.NAME).read_text())["sdelta"] == "channel"
    assert sidecar.sdelta_of(None) is None
    assert sidecar.sdelta_of(sidecar.read(str(plain))) == "flat" and sidecar.sdelta_of(sidecar.read(str(chan))) == "channel"
    assert sidecar.stack_of(sidecar.read(str(chan))) == (12, 64, 64, 0)             # what the early rollout starts from
    # the trailer is authoritative: a sidecar that says otherwise is an error, no sidecar is no opinion
    assert decompress.check_sdelta(str(chan), 4) == 1 and decompress.check_sdelta(str(chan), 5) == 1
    assert decompress.check_sdelta(str(plain), 1) == 0 and decompress.check_sdelta(str(plain), 2) == 0
    assert decompress.check_sdelta(str(tmp_path), 4) == 1 and decompress.check_sdelta(str(tmp_path), 1) == 0
    with pytest.raises(ValueError, match="spatial delta"):
        decompress.check_sdelta(str(chan), 1)
    with pytest.raises(ValueError, match="spatial delta"):
        decompress.check_sdelta(str(plain), 4)
    for bad in ("flat", "row", 3):
        doc = json.loads((chan / sidecar.NAME).read_text())
        doc["sdelta"] = bad
        (chan / sidecar.NAME).write_text(json.dumps(doc))
        with pytest.raises(ValueError, match="sdelta"):
            decompress.check_sdelta(str(chan), 4)


def _args(extra):
    from tezip_amd import tezip
    return tezip, tezip.build_parser().parse_args(extra)


COMPRESS = ["-c", "m", "d", "o", "-p", "0", "-w", "4", "-m", "abs", "-b", "2"]


@pytest.mark.parametrize("argv,env,word", [
    (["-u", "m", "c", "d", "--sdelta", "channel"], {}, "-c"),
    (["-u", "m", "c", "d", "--sdelta", "flat"], {}, "-c"),
    (["-l", "m", "d", "--sdelta", "channel"], {}, "-c"),
    (["-l", "m", "d", "--sdelta", "flat"], {}, "-c"),
    (["-c", "m", "d", "o", "-p", "0", "-m", "abs", "-b", "2", "--sweep", "4", "8", "--sdelta", "channel"], {}, "--sweep"),
    (COMPRESS + ["--sdelta", "channel"], {"WORLD_SIZE": "2"}, "sharded"),
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
    for extra in (["--sdelta", "channel"], ["--sdelta", "flat"], ["--sdelta", "channel", "--shuffle"], ["--sdelta", "channel", "-n"],
                  ["--sdelta", "channel", "--gray", "--coder", "huffd", "--key-coder", "huffg", "--report", "--ssim", "--digests"],
                  ["--sdelta", "flat", "--sweep", "4", "8"]):
        tezip, arg = _args((COMPRESS[:6] + COMPRESS[8:] if "--sweep" in extra else COMPRESS) + extra)
        for check in (tezip.check_sdelta_flag, tezip.check_gray_flag, tezip.check_coder_flag, tezip.check_key_coder_flag,
                      tezip.check_report_flag, tezip.check_digests_flag, tezip.check_ssim_flag):
            assert check(arg) is None, extra
    assert compress.check_sdelta("channel", sharded=True) and compress.check_sdelta("channel") is None
    assert compress.check_sdelta("flat", sharded=True) is None and "row" in compress.check_sdelta("row")
    seen = {}
    monkeypatch.setattr(tezip, "probe_gpu", lambda force: True)
    monkeypatch.setattr(compress, "run", lambda *a, **kw: seen.update(kw))
    tezip.main(_args(COMPRESS + ["--sdelta", "channel", "--coder", "huffd", "--digests", "--gray"])[1])
    assert seen["SDELTA"] == "channel" and seen["CODER"] == "huffd" and seen["DIGESTS"] is True and seen["GRAY"] is True
    for argv in (COMPRESS, COMPRESS + ["--sdelta", "flat"]):
        seen.clear()
        tezip.main(_args(argv)[1])
        assert "SDELTA" not in seen     # flat is the call it was without the flag


def test_a_direct_caller_of_run_is_refused(monkeypatch, capsys):
    from tezip_amd import compress
    monkeypatch.setattr(compress.tzdist, "active", lambda: (0, 2))
    with pytest.raises(SystemExit) as e:
        compress.run("m", "d", "o", 0, 4, None, "abs", [2.0], True, False, True, SDELTA="channel")
    assert e.value.code == 2 and "sharded" in capsys.readouterr().out
    monkeypatch.setattr(compress.tzdist, "active", lambda: None)
    with pytest.raises(SystemExit) as e:
        compress.run("m", "d", "o", 0, 4, None, "abs", [2.0], True, False, True, SDELTA="row")
    assert e.value.code == 2 and "--sdelta" in capsys.readouterr().out


def test_a_sharded_decoder_refuses_a_channel_stride_stream(tmp_path, monkeypatch, capsys):
    from tezip_amd import compress, decompress, zstd
    nt, h, w = 2, 8, 8
    n = nt * h * w * 3
    (tmp_path / "filename.txt").write_text("1\n" + "".join("f%d.png\n" % i for i in range(nt)))
    (tmp_path / "key_frame.dat").write_bytes(zstd.compress_array(np.zeros(n, np.uint8), 9))
    stream = compress.build_stream(np.zeros(n, np.int16), np.array([1600], np.int16), (4, nt, h, w, 3), 0)
    (tmp_path / "entropy.dat").write_bytes(zstd.compress_array(stream, 9))
    monkeypatch.setattr(decompress.tzdist, "active", lambda: (0, 2))
    monkeypatch.setattr(decompress, "open_model", lambda d: (None, [np.zeros(1, np.float32)], None))
    monkeypatch.setattr(decompress, "make_context", lambda *a, **k: pytest.fail("refused before a GPU is touched"))
    with pytest.raises(SystemExit) as e:
        decompress.run("m", str(tmp_path), str(tmp_path / "out"), True, False)
    assert e.value.code == 2 and "--sdelta channel" in capsys.readouterr().out


def _golden_delta_stacks():
    """(name, flat payload, table, shape5, warm_up, delta stack) of every *_entropy array of tests/golden/ref_runs*.npz: the
    reference's own streams, undone with the oracle's operators."""
    from tezip_amd import decompress
    out = []
    for f in sorted(glob.glob(os.path.join(GOLDEN, "ref_runs*.npz"))):
        z = np.load(f)
        for k in z.files:
            if k.endswith("_entropy"):
                pay, tab, shape, p = decompress.parse_stream(np.ascontiguousarray(z[k]).tobytes())
                pay = np.array(pay)
                sym = pay if tab is None else (1600 - np.asarray(tab, np.int64)[pay.astype(np.int64)]).astype(np.int16)
                out.append((os.path.basename(f) + ":" + k, pay, None if tab is None else np.array(tab), shape, p,
                            O.finding_difference_dec(sym)))
    assert len(out) >= 20
    return out


def test_golden_payloads_re_encode_at_stride_three(sd):
    """The delta stacks of the reference's runs, coded at the channel stride, decode back to the same stacks from a whole
    file of each coder.  Sizes are recorded, not asserted: 25 k elements from a fake predictor."""
    from tezip_amd import compress, decompress, huffd, zstd
    total = {"flat zstd": 0, "channel zstd": 0, "flat huffd": 0, "channel huffd": 0}
    for name, pay, tab, shape, warm, delta in _golden_delta_stacks():
        one, nt, h, w, c = shape
        assert (one, c) == (1, 3) and delta.size == nt * h * w * 3
        flat_again, flat_table = sd.payload_from_delta(delta, tab is not None, stride=1)
        np.testing.assert_array_equal(flat_again, pay, name)                   # stride 1 IS the reference's payload
        if tab is not None:
            np.testing.assert_array_equal(flat_table, tab, name)
        p3, t3 = sd.payload_from_delta(delta, tab is not None)
        stream = compress.build_stream(p3, t3, (sd.MARK, nt, h, w, 3), warm)
        z3 = zstd.compress_array(stream, 9)
        got, t, shape3, warm3 = decompress.parse_stream(zstd.decompress(z3))
        decompress.check_stream(shape3, warm3, got.size, nt * h * w * 3)
        assert sd.is_strided(shape3[0]) and warm3 == warm
        np.testing.assert_array_equal(sd.delta_from_payload(got, t), delta.reshape(-1), name)
        z1 = zstd.compress_array(compress.build_stream(pay, tab, shape, warm), 9)
        sizes = [len(z1), len(z3)]
        if tab is not None:                                                    # the Huffman coders code ranks
            h3 = huffd.encode_file(p3, t3, (sd.MARK, nt, h, w, 3), warm)
            got, p = huffd.decode_file(h3, nt * h * w * 3)
            np.testing.assert_array_equal(sd.delta_from_payload(got, p.table), delta.reshape(-1), name)
            h1 = huffd.encode_file(pay, tab, shape, warm)
            sizes += [len(h1), len(h3), huffd.parse(h1).dist, huffd.parse(h3).dist]
            total["flat huffd"] += len(h1)
            total["channel huffd"] += len(h3)
            print("%-58s zstd-9 %6d -> %6d  huffd %6d (D=%d) -> %6d (D=%d)" % (name, sizes[0], sizes[1], sizes[2], sizes[4], sizes[3], sizes[5]))
        else:
            print("%-58s zstd-9 %6d -> %6d" % (name, sizes[0], sizes[1]))
        total["flat zstd"] += len(z1)
        total["channel zstd"] += len(z3)
    print("totals (bytes, flat -> channel): zstd-9 %d -> %d, huffd %d -> %d"
          % (total["flat zstd"], total["channel zstd"], total["flat huffd"], total["channel huffd"]))
