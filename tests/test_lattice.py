"""The lattice quantiser TZ-QL1 on the CPU (tezip_amd/lattice.py, `-c --quant lattice`): the properties of the definition over
seeded random slabs, a stream made from a lattice delta stack read by the oracle's restatement of the reference decoder, the
size claim of the README against the reference's greedy quantiser, and the command line's refusals."""
import numpy as np
import pytest

from oracle import oracle as O
from tezip_amd import lattice

MODE_CASES = [("abs", [0.5]), ("abs", [0.999]), ("abs", [1.0]), ("abs", [2.0]), ("abs", [-2.5]), ("abs", [6.0]), ("abs", [127.0]),
              ("abs", [254.9]), ("abs", [255.0]), ("abs", [300.0]), ("abs", [float("inf")]),
              ("rel", [0.0039]), ("rel", [0.01]), ("rel", [0.3]), ("rel", [2.0]),
              ("absrel", [3.0, 0.05]), ("absrel", [40.0, 0.02]), ("absrel", [0.5, 1.0]),
              ("pwrel", [0.003]), ("pwrel", [0.05]), ("pwrel", [1.5])]


def _slab(seed, shape=(23, 31)):
    rng = np.random.default_rng(seed)
    orig = rng.integers(0, 256, shape)
    if seed % 3 == 0:
        orig = np.clip(orig, 40, 90)               # a narrow range: rel tolerances below and around 1
    diff = rng.integers(-255, 256, shape)
    diff.reshape(-1)[:6] = [-255, 255, 0, -1, 1, 254]
    return orig.astype(np.uint8), diff.astype(np.int16)


@pytest.mark.parametrize("mode,value", MODE_CASES)
def test_properties_of_quantise(mode, value):
    for seed in range(6):
        orig, diff = _slab(seed)
        e = lattice.tolerance(orig, mode, value)
        q = lattice.quantise(orig, diff, mode, value)
        assert q.shape == diff.shape and q.dtype == np.int64
        E = np.minimum(255, np.floor(np.broadcast_to(np.asarray(e, np.float64), diff.shape))).astype(np.int64)
        assert (np.abs(q - diff) <= E).all() and (E <= np.broadcast_to(e, diff.shape)).all()          # |q - d| <= floor(e) <= e
        assert (np.abs(q) <= 255).all()
        np.testing.assert_array_equal(q[E == 0], diff[E == 0])                                       # e < 1: the identity
        assert not q[E == 255].any()                                                                 # E = 255: all zero
        s = 2 * E + 1
        assert ((q % s == 0) | (np.abs(q) == 255)).all()                                             # lattice points, or the clamp
        np.testing.assert_array_equal(lattice.quantise(orig, -diff, mode, value), -q)               # odd in d
    if mode == "abs" and abs(value[0]) >= 255:
        assert not lattice.quantise(*_slab(1), mode, value).any()
    if mode == "abs" and abs(value[0]) < 1:
        np.testing.assert_array_equal(lattice.quantise(*_slab(1), mode, value), _slab(1)[1])


def test_the_tolerance_is_the_greedy_quantisers():
    orig, _ = _slab(3)
    rng = float(int(orig.max()) - int(orig.min()))
    assert lattice.tolerance(orig, "abs", [-2.5]) == 2.5
    assert lattice.tolerance(orig, "rel", [0.1]) == rng * 0.1
    assert lattice.tolerance(orig, "absrel", [3.0, 0.1]) == min(3.0, rng * 0.1)
    assert lattice.tolerance(orig, "absrel", [300.0, 0.1]) == rng * 0.1
    np.testing.assert_array_equal(lattice.tolerance(orig, "pwrel", [0.1]), orig.astype(np.float64) * 0.1)
    for mode, value in (("rel", [-0.1]), ("pwrel", [-0.1]), ("absrel", [1.0, -0.1]), ("abs", [float("nan")]), ("absrel", [1.0, float("nan")]),
                        ("huh", [1.0])):
        with pytest.raises(ValueError):
            lattice.quantise(orig, orig.astype(np.int16), mode, value)


def test_stack_helper_skip_mask_and_frame_bounds():
    rng = np.random.default_rng(5)
    orig = rng.integers(0, 256, (6, 9, 14, 3)).astype(np.uint8)
    diff = rng.integers(-255, 256, orig.shape).astype(np.int16)
    skip = np.array([1, 0, 0, 1, 0, 0], np.uint8)
    for mode, value in (("abs", [3.0]), ("rel", [0.02]), ("pwrel", [0.04])):
        got = lattice.quantise_stack(orig, diff, mode, value, skip)
        assert got.dtype == np.int16
        for f in range(6):
            for c in range(3):
                want = diff[f, :, :, c] if skip[f] else lattice.quantise(orig[f, :, :, c], diff[f, :, :, c], mode, value)
                np.testing.assert_array_equal(got[f, :, :, c], want)
        assert (got != diff).any()
    bounds = [9.0, 0.0, 2.5, 7.0, 0.999, 255.0]
    got = lattice.quantise_stack(orig, diff, "abs", [99.0], skip, bounds=bounds)
    for f, b in enumerate(bounds):
        want = diff[f] if skip[f] else lattice.quantise_stack(orig[f:f + 1], diff[f:f + 1], "abs", [b])[0]
        np.testing.assert_array_equal(got[f], want)
        assert np.abs(got[f].astype(int) - diff[f]).max() <= (0 if skip[f] else int(b))
    np.testing.assert_array_equal(got[1], diff[1])
    np.testing.assert_array_equal(got[4], diff[4])
    assert not got[5].any()
    for bad in ([1.0] * 5, [1.0] * 5 + [-1.0], [1.0] * 5 + [float("nan")]):
        with pytest.raises(ValueError):
            lattice.quantise_stack(orig, diff, "abs", [0.0], skip, bounds=bad)


# ------------------------------------------------------------------------------------------- the reference decoder reads it
class _Fake:
    def c0(self, hp, wp):
        import fake_predictor
        return fake_predictor.c0_image(hp, wp)

    def next(self, frame):
        import fake_predictor
        return fake_predictor.g_next(frame)


def _lattice_stream(frames, ro, p, mode, bound, entropy):
    """oracle.encode_stream with lattice.quantise in error_bound's place, from the oracle's own pieces"""
    nt, h, w, _ = frames.shape
    parts = []
    for g, (start, preds) in enumerate(ro["groups"]):
        k = len(preds)
        orig = frames[start: start + k]
        d = O.delta_group(np.stack(preds), orig)
        if not (p != 0 and g == 0):
            for j in range(1, k):
                for c in range(3):
                    d[j, :, :, c] = lattice.quantise(orig[j, :, :, c], d[j, :, :, c], mode, bound)
        parts.append(d)
    dm = np.concatenate(parts, axis=0).astype(np.int16)
    sd = O.finding_difference_enc(dm).reshape(-1)
    assert np.abs(sd.astype(int)).max() <= 510
    if not entropy:
        return O.build_stream(sd, None, nt, h, w, p), dm
    y = (O.OFFSET - sd.astype(np.int64)).astype(np.int16)
    table = O.build_table(y)
    assert len(table) <= 1021
    return O.build_stream(O.remap_enc(y, table), table, nt, h, w, p), dm


@pytest.mark.parametrize("p,window,mode,bound", [(0, 3, "abs", [2.0]), (1, 4, "abs", [6.0]), (2, 3, "rel", [0.02]), (0, 4, "pwrel", [0.05]),
                                                 (0, 3, "abs", [0.5])])
def test_the_reference_decoder_reads_a_lattice_stream(p, window, mode, bound):
    from tezip_amd import synth
    frames = synth.translating_scene(8, 21, 30)
    ro = O.rollout(frames, p, window, None, _Fake())
    for entropy in (True, False):
        stream, dm = _lattice_stream(frames, ro, p, mode, bound, entropy)
        dec = O.decode_stream(stream, O.key_frame_stream(frames, ro["key"]), _Fake())
        err = np.abs(dec.astype(int) - frames.astype(int))
        for f in range(len(frames)):
            for c in range(3):
                e = lattice.tolerance(frames[f, :, :, c], mode, bound)
                E = np.minimum(255, np.floor(np.broadcast_to(np.asarray(e, np.float64), err[f, :, :, c].shape)))
                assert (err[f, :, :, c] <= E).all(), (f, c)
        assert (err[ro["key"]] == 0).all()
        if mode == "abs" and abs(bound[0]) < 1:
            assert not err.any()
            np.testing.assert_array_equal(dm, O.encode_stream(frames, ro, p, "abs", [0.0], entropy)["delta"])
        else:
            assert err.any()                       # the job is lossy: the case shows something


# -------------------------------------------------------------------------------------------------------- the size claim
def _rows(name):
    from tezip_amd import synth
    frames = {"turbulence": lambda: synth.turbulence(7, 128, 128), "translating_scene": lambda: synth.translating_scene(7, 64, 80),
              "detector": lambda: synth.detector(4, 128, 128)}[name]()
    return {(b, q): (flat0, chan0) for b, q, _, flat0, _, chan0, _ in lattice.table_rows(frames, O.error_bound)}


@pytest.mark.parametrize("name", ["turbulence", "translating_scene"])
def test_lattice_payload_is_at_most_three_quarters_of_the_greedy_one(name):
    rows = _rows(name)
    for b in (2.0, 6.0):
        for layout in (0, 1):                      # flat, channel stride
            g, lat = rows[b, "greedy"][layout], rows[b, "lattice"][layout]
            print(name, "abs", b, ("flat", "channel")[layout], "greedy", g, "lattice", lat, "ratio %.3f" % (lat / g))
            assert lat <= 0.75 * g


def test_sparse_frames_at_a_loose_bound_are_larger_under_the_lattice():
    """the README's warning: detector frames at abs 6"""
    rows = _rows("detector")
    for layout in (0, 1):
        g, lat = rows[6.0, "greedy"][layout], rows[6.0, "lattice"][layout]
        print("detector abs 6", ("flat", "channel")[layout], "greedy", g, "lattice", lat, "ratio %.3f" % (lat / g))
        assert lat > g


# ---------------------------------------------------------------------------------------------------------------- the CLI
JOB = ["-c", "m", "d", "o", "-p", "0", "-w", "4"]


def _args(extra):
    from tezip_amd import tezip
    return tezip, tezip.build_parser().parse_args(extra)


@pytest.mark.parametrize("argv,env,word", [
    (["-u", "m", "c", "d", "--quant", "lattice"], {}, "-c"),
    (["-u", "m", "c", "d", "--quant", "greedy"], {}, "-c"),
    (["-l", "m", "d", "--quant", "lattice"], {}, "-c"),
    (["-l", "m", "d", "--quant", "greedy"], {}, "-c"),
    (["-c", "m", "d", "o", "-p", "0", "-m", "abs", "-b", "2", "--sweep", "4", "8", "--quant", "lattice"], {}, "--sweep"),
    (JOB + ["-m", "abs", "-b", "2", "--quant", "lattice"], {"WORLD_SIZE": "2"}, "sharded"),
])
def test_cli_refusals(monkeypatch, capsys, argv, env, word):
    from tezip_amd import compress
    tezip, arg = _args(argv)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setattr(tezip, "probe_gpu", lambda force: pytest.fail("refused before a GPU is touched"))
    monkeypatch.setattr(compress, "run", lambda *a, **kw: pytest.fail("compress.run must not be called"))
    with pytest.raises(SystemExit) as e:
        tezip.main(arg)
    out = capsys.readouterr().out
    assert e.value.code == 2 and out.startswith("ERROR:") and word in out and "--quant" in out and len(out.strip().splitlines()) == 1, out


def test_an_unknown_quantiser_is_a_usage_error(capsys):
    with pytest.raises(SystemExit) as e:
        _args(JOB + ["-m", "abs", "-b", "2", "--quant", "nearest"])
    assert e.value.code == 2


ACCEPTED = [
    ["-m", "abs", "-b", "2"], ["-m", "rel", "-b", "0.01", "-n"], ["-m", "absrel", "-b", "2", "0.01", "--shuffle"], ["-m", "pwrel", "-b", "0.1", "-v"],
    ["-m", "abs", "-b", "2", "--report"], ["-m", "abs", "-b", "2", "--report", "--ssim"], ["-m", "abs", "-b", "2", "--digests"],
    ["-m", "abs", "-b", "2", "--coder", "huff"], ["-m", "abs", "-b", "2", "--coder", "huffr"], ["-m", "abs", "-b", "2", "--coder", "huffd"],
    ["-m", "abs", "-b", "2", "--key-coder", "huff"], ["-m", "abs", "-b", "2", "--key-coder", "huffg"], ["-m", "abs", "-b", "2", "--gray"],
    ["-m", "abs", "-b", "2", "--sdelta", "channel"], ["--target-psnr", "40"], ["--target-psnr", "40", "--per-frame"],
    ["--target-ratio", "4", "--coder", "huffd"],
]


@pytest.mark.parametrize("flags", ACCEPTED, ids=lambda f: " ".join(f))
def test_quant_is_accepted_wherever_c_is(monkeypatch, flags):
    """--quant greedy is the job without the flag, call for call; --quant lattice is the same job with QUANT="lattice" """
    from tezip_amd import compress
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    calls = []
    monkeypatch.setattr(compress, "run", lambda *a, **kw: calls.append((a, kw)))
    for job in (JOB, ["-c", "m", "d", "o", "-p", "1", "-t", "0.01"]):
        calls.clear()
        for extra in ([], ["--quant", "greedy"], ["--quant", "lattice"]):
            tezip, arg = _args(job + flags + extra)
            monkeypatch.setattr(tezip, "probe_gpu", lambda force: True)
            tezip.main(arg)
        plain, greedy, lat = calls
        assert greedy == plain and "QUANT" not in plain[1]
        assert lat[0] == plain[0] and lat[1]["QUANT"] == "lattice"
        defaults = dict(SHUFFLE=False, REPORT=False, CODER="zstd", KEY_CODER="zstd", DIGESTS=False, GRAY=False, SDELTA="flat", SSIM=False,
                        TARGET_PSNR=None, TARGET_RATIO=None, PER_FRAME=False, FRAME_BOUNDS=None)
        assert dict(defaults, **plain[1]) == {k: v for k, v in lat[1].items() if k != "QUANT"}


def test_frame_bounds_file_travels_with_the_flag(monkeypatch, tmp_path):
    from tezip_amd import compress
    path = tmp_path / "b.json"
    path.write_text("[0, 1, 2, 3]")
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    calls = []
    monkeypatch.setattr(compress, "run", lambda *a, **kw: calls.append((a, kw)))
    tezip, arg = _args(JOB + ["-m", "abs", "--frame-bounds", str(path), "--quant", "lattice"])
    monkeypatch.setattr(tezip, "probe_gpu", lambda force: True)
    tezip.main(arg)
    (a, kw), = calls
    assert a[6:8] == ("abs", []) and kw["FRAME_BOUNDS"] == str(path) and kw["QUANT"] == "lattice"


def test_a_direct_caller_of_run_is_refused(monkeypatch, capsys, tmp_path):
    from tezip_amd import compress
    monkeypatch.setattr(compress, "make_context", lambda *a, **k: pytest.fail("refused before a GPU is touched"))
    run = lambda **kw: compress.run("m", str(tmp_path), str(tmp_path / "o"), 0, 4, None, "abs", [2.0], True, False, True, **kw)  # noqa: E731
    with pytest.raises(SystemExit) as e:
        run(QUANT="nearest")
    out = capsys.readouterr().out
    assert e.value.code == 2 and out.startswith("ERROR:") and "--quant" in out and len(out.strip().splitlines()) == 1
    monkeypatch.setattr(compress.tzdist, "active", lambda: (0, 2))
    with pytest.raises(SystemExit) as e:
        run(QUANT="lattice")
    out = capsys.readouterr().out
    assert e.value.code == 2 and "sharded" in out and "--quant" in out


def test_sidecar_records_the_quantiser(tmp_path):
    import json
    from tezip_amd import sidecar
    wts = [np.zeros(3, np.float32)]
    doc = sidecar.write(str(tmp_path), 1, wts, 8, 8, (4, 8, 8, 0), quant="lattice")
    assert doc["quant"] == "lattice" and json.load(open(tmp_path / sidecar.NAME))["quant"] == "lattice"
    assert sidecar.resolve(sidecar.read(str(tmp_path)), wts) == 1          # -u reads the file as any other
    assert "quant" not in sidecar.write(str(tmp_path), 1, wts, 8, 8, (4, 8, 8, 0))
