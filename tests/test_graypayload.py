"""The one-channel payload of a gray job (`-c --gray`, tezip_amd/graypayload.py) without a GPU: the slow statement of the
format against the oracle's operators applied to channel 0, the trailer checks of `-u`, the sidecar key and the refusals of
the flag."""
import json

import numpy as np
import pytest


@pytest.fixture(scope="module")
def gp():
    from tezip_amd import graypayload
    return graypayload


def gray_delta_stack(nt, h, w, seed, other_channels=False):
    """A quantised delta stack as a gray job has it: three equal channels, values of a prediction residual.
    other_channels: channels 1 and 2 hold something else, which must not matter."""
    rng = np.random.default_rng(seed)
    d0 = np.clip(np.rint(rng.normal(0, 6, (nt, h, w))), -255, 255).astype(np.int16)
    d0[rng.random((nt, h, w)) < 0.01] = 255
    d0[rng.random((nt, h, w)) < 0.01] = -255
    d = np.repeat(d0[..., None], 3, axis=-1)
    if other_channels:
        d[..., 1:] = rng.integers(-255, 256, (nt, h, w, 2), dtype=np.int16)
    return d


@pytest.mark.parametrize("other", [False, True])
@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 5, 7), (4, 61, 45)])
def test_payload_is_the_oracle_on_channel_0(gp, shape, other):
    from oracle import oracle
    d = gray_delta_stack(*shape, seed=3, other_channels=other)
    sd = oracle.finding_difference_enc(np.ascontiguousarray(d[..., 0]).reshape(-1))
    y = (1600 - sd).astype(np.int16)
    table = oracle.build_table(y)
    payload, got_table = gp.payload_from_delta(d, True)
    assert payload.dtype == np.int16 and payload.size == d.size // 3
    np.testing.assert_array_equal(got_table, table)
    np.testing.assert_array_equal(payload, oracle.remap_enc(y, table))
    raw, none = gp.payload_from_delta(d, False)
    assert none is None
    np.testing.assert_array_equal(raw, sd)
    # and back: the oracle's decoder operators give channel 0 again
    np.testing.assert_array_equal(oracle.finding_difference_dec(1600 - oracle.remap_dec(payload, table)).reshape(shape), d[..., 0])


def test_table_breaks_ties_by_ascending_symbol(gp):
    y = np.array([1601, 1599, 1600, 1600, 1599, 1601, 1700], np.int16)
    assert gp.build_table(y).tolist() == [1599, 1600, 1601, 1700]
    assert gp.remap(y, gp.build_table(y)).tolist() == [2, 0, 1, 1, 0, 2, 3]


def test_spatial_delta_wraps_and_takes_a_carry(gp):
    x = np.array([-32768, 32767, 5], np.int16)
    assert gp.spatial_delta(x).tolist() == [-32768, 1, 32762]
    assert gp.spatial_delta(x, carry=7).tolist() == [-32761, 1, 32762]


def test_reconstruct_replicates_and_clamps(gp):
    base = np.array([[[0, 10], [250, 255]]])
    delta = np.array([[[5, -3], [-10, 300]]], np.int16)
    out = gp.reconstruct(base, delta)
    assert out.shape == (1, 2, 2, 3) and out.dtype == np.uint8 and out.flags["C_CONTIGUOUS"]
    assert out[..., 0].tolist() == [[[0, 13], [255, 0]]]
    assert gp.is_gray(out)


def test_is_gray(gp):
    f = np.repeat(np.arange(24, dtype=np.uint8).reshape(2, 3, 4, 1), 3, axis=-1)
    assert gp.is_gray(f) and gp.is_gray(f[0])
    for c in (1, 2):
        g = f.copy()
        g[1, 2, 3, c] ^= 1   # one sample of the last pixel of the last frame
        assert not gp.is_gray(g)
    with pytest.raises(ValueError):
        gp.is_gray(np.zeros((2, 3, 4), np.uint8))


def test_check_stream_accepts_one_channel_and_nothing_else():
    from tezip_amd import compress, decompress
    nt, h, w = 2, 4, 5
    n1 = nt * h * w
    decompress.check_stream((1, nt, h, w, 1), 0, n1, n1 * 3)                        # the new format
    decompress.check_stream((compress.SHUFFLE_MARK, nt, h, w, 1), 1, n1, n1 * 3)    # ... byte-shuffled
    decompress.check_stream((1, nt, h, w, 3), 0, n1 * 3, n1 * 3)                    # the reference's, as ever
    with pytest.raises(ValueError, match="shape"):
        decompress.check_stream((1, nt, h, w, 2), 0, n1 * 2, n1 * 3)
    with pytest.raises(ValueError, match="shape"):
        decompress.check_stream((1, nt, h, w, 0), 0, 0, n1 * 3)
    with pytest.raises(ValueError, match="payload holds"):
        decompress.check_stream((1, nt, h, w, 1), 0, n1 * 3, n1 * 3)               # three channels under C == 1
    with pytest.raises(ValueError, match="payload holds"):
        decompress.check_stream((1, nt, h, w, 3), 0, n1, n1 * 3)                   # one channel under C == 3
    with pytest.raises(ValueError, match="key_frame.dat"):
        decompress.check_stream((1, nt, h, w, 1), 0, n1, n1)                       # key_frame.dat keeps three channels
    # the stream compress writes for such a job parses back to the same pieces
    payload = np.arange(n1, dtype=np.int16)
    table = np.array([1600, 1601], np.int16)
    p, t, shape, warm = decompress.parse_stream(compress.build_stream(payload, table, (1, nt, h, w, 1), 1).tobytes())
    assert shape == (1, nt, h, w, 1) and warm == 1 and t.tolist() == [1600, 1601]
    np.testing.assert_array_equal(p, payload)
    decompress.check_stream(shape, warm, p.size, n1 * 3)


@pytest.mark.parametrize("fmt_name", ["huff", "huffr"])
def test_coded_files_carry_a_one_channel_trailer(gp, fmt_name):
    import importlib
    fmt = importlib.import_module("tezip_amd." + fmt_name)
    nt, h, w = 3, 9, 11
    payload, table = gp.payload_from_delta(gray_delta_stack(nt, h, w, seed=5), True)
    data = fmt.encode_file(payload, table, (1, nt, h, w, 1), 0)
    got, p = fmt.decode_file(data, nt * h * w * 3)
    assert p.shape == (1, nt, h, w, 1) and p.n == nt * h * w
    np.testing.assert_array_equal(got, payload)
    with pytest.raises(ValueError, match="key_frame.dat"):
        fmt.parse(data, nt * h * w)
    with pytest.raises(ValueError, match="shape"):
        fmt.parse(fmt.encode_file(payload, table, (1, nt, h, w, 2), 0), nt * h * w * 3)


def test_sidecar_records_one_channel_only(tmp_path, monkeypatch):
    from tezip_amd import _lib, decompress, sidecar

    class Lib:
        @staticmethod
        def tz_version():
            return 101

    monkeypatch.setattr(_lib, "load", lambda: Lib)
    wts = [np.zeros(3, np.float32)]
    plain, gray = tmp_path / "plain", tmp_path / "gray"
    plain.mkdir()
    gray.mkdir()
    assert "payload_channels" not in sidecar.write(str(plain), 2, wts, 64, 64, (12, 64, 64, 0))
    assert sidecar.write(str(gray), 2, wts, 64, 64, (12, 64, 64, 0), payload_channels=1)["payload_channels"] == 1
    assert "payload_channels" not in json.loads((plain / sidecar.NAME).read_text())
    assert json.loads((gray / sidecar.NAME).read_text())["payload_channels"] == 1
    assert sidecar.channels_of(None) is None
    assert sidecar.channels_of(sidecar.read(str(plain))) == 3 and sidecar.channels_of(sidecar.read(str(gray))) == 1
    # the trailer is authoritative: a sidecar that says otherwise is an error, no sidecar is no opinion
    decompress.check_channels(str(gray), 1)
    decompress.check_channels(str(plain), 3)
    decompress.check_channels(str(tmp_path), 1)
    with pytest.raises(ValueError, match="channel"):
        decompress.check_channels(str(gray), 3)
    with pytest.raises(ValueError, match="channel"):
        decompress.check_channels(str(plain), 1)
    doc = json.loads((gray / sidecar.NAME).read_text())
    doc["payload_channels"] = 2
    (gray / sidecar.NAME).write_text(json.dumps(doc))
    with pytest.raises(ValueError, match="payload_channels"):
        decompress.check_channels(str(gray), 1)


def _args(extra):
    from tezip_amd import tezip
    return tezip, tezip.build_parser().parse_args(extra)


@pytest.mark.parametrize("argv,env,word", [
    (["-u", "m", "c", "d", "--gray"], {}, "-c"),
    (["-l", "m", "d", "--gray"], {}, "-c"),
    (["-c", "m", "d", "o", "-p", "0", "-m", "abs", "-b", "2", "--sweep", "4", "8", "--gray"], {}, "--sweep"),
    (["-c", "m", "d", "o", "-p", "0", "-w", "4", "-m", "abs", "-b", "2", "--gray"], {"WORLD_SIZE": "2"}, "sharded"),
])
def test_cli_refuses_gray_combinations(monkeypatch, capsys, argv, env, word):
    tezip, arg = _args(argv)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setattr(tezip, "probe_gpu", lambda force: pytest.fail("refused before a GPU is touched"))
    assert word in tezip.check_gray_flag(arg)
    with pytest.raises(SystemExit) as e:
        tezip.main(arg)
    out = capsys.readouterr().out
    assert e.value.code == 2 and out.startswith("ERROR:") and word in out and len(out.strip().splitlines()) == 1


def test_flag_is_accepted_where_it_is_valid_and_reaches_run(monkeypatch):
    from tezip_amd import compress
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    base = ["-c", "m", "d", "o", "-p", "0", "-w", "4", "-m", "abs", "-b", "2"]
    for extra in (["--gray"], ["--gray", "--shuffle"], ["--gray", "--coder", "huffr"], ["-t", "0.01", "--gray"],
                  ["--gray", "--coder", "huff", "--key-coder", "huffg", "--report", "--digests"]):
        tezip, arg = _args((base[:6] + base[8:] if "-t" in extra else base) + extra)
        for check in (tezip.check_gray_flag, tezip.check_coder_flag, tezip.check_key_coder_flag, tezip.check_report_flag,
                      tezip.check_digests_flag):
            assert check(arg) is None, extra
    assert compress.check_gray(True, sharded=True) and compress.check_gray(True) is None and compress.check_gray(False, True) is None
    seen = {}
    monkeypatch.setattr(tezip, "probe_gpu", lambda force: True)
    monkeypatch.setattr(compress, "run", lambda *a, **kw: seen.update(kw))
    tezip.main(_args(base + ["--gray", "--coder", "huff", "--digests"])[1])
    assert seen["GRAY"] is True and seen["CODER"] == "huff" and seen["DIGESTS"] is True and seen["KEY_CODER"] == "zstd"
    seen.clear()
    tezip.main(_args(base)[1])
    assert "GRAY" not in seen     # without the flag the call is the one it was


def test_a_direct_caller_of_run_is_refused_when_sharded(monkeypatch, capsys):
    from tezip_amd import compress
    monkeypatch.setattr(compress.tzdist, "active", lambda: (0, 2))
    with pytest.raises(SystemExit) as e:
        compress.run("m", "d", "o", 0, 4, None, "abs", [2.0], True, False, True, GRAY=True)
    assert e.value.code == 2 and "sharded" in capsys.readouterr().out
