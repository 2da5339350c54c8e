"""The spatial delta at the channel stride (`-c --sdelta channel`, tz_set_delta_stride(1)) on the GPU: k_sdelta_s3, k_scan3p and
k_undelta_carry_s3 give the numpy statement (tezip_amd/sdelta.py) bit for bit, tz_encode under mode 1 gives the payload and
table that statement makes of the mode-0 encode's own delta stack, the decoder restores the frames mode 0 restores from its
own payload, and the command line round-trips to the images of the flat job."""
import contextlib
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NBINS = 2111
# The sizes of the issue, then the boundaries of the kernels as built.  k_scan3p: a wave-tile is 1024 elements, a block owns
# four (4096), a launch has at most 4096 blocks, so a wave owns ONE tile up to 16 777 216 elements.  k_sdelta_s3: groups of 8,
# 8192 elements per histogram block, the grid wraps beyond 4 194 304.  k_undelta_carry_s3: groups of 24, 6144 per block.
SIZES = [1, 2, 3, 4, 7, 8, 47, 48, 49, 3073, 12289, 1048581, 5000003,
         1023, 1024, 1025, 4095, 4096, 4097, 8191, 8193, 6143, 6145]
N_TWO_TILES = 16777216 + 1029      # 16 386 wave-tiles on 4096 blocks of four waves: every wave owns two tiles


@pytest.fixture(scope="module")
def ctx():
    from tezip_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def sd():
    from tezip_amd import sdelta
    return sdelta


def pad8(v):
    return (v + 7) // 8 * 8


def _counts(y):
    inside = y[(y >= 0) & (y < NBINS)].astype(np.int64)      # what the library counts (as tz_spatial_delta)
    return np.bincount(inside, minlength=NBINS).astype(np.uint64)


def _stack(n, seed):
    """Full-range int16 with a stretch of encoder-like values, so that the histogram's central bins, its far bins and the
    symbols outside it all occur."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-32768, 32768, n, dtype=np.int16)
    if n > 64:
        x[n // 3: n // 3 + n // 4] = rng.integers(-12, 13, n // 4)
    return x


CARRY = np.array([-77, 30000, -32768], np.int16)


def _check_seams(ctx, sd, n, combos, seed):
    x = _stack(n, seed)
    hold = np.empty(n + 1, np.int16)            # the same elements from a host buffer at an odd element offset
    out = np.empty(n + 1, np.int16)
    for carry, offset in combos:
        what = "n %d carry %r offset %d" % (n, carry is not None, offset)
        want = sd.encode(x, 3, offset, carry)
        hist = np.full(NBINS, 3, np.uint64)                      # the counts are ADDED
        got = ctx.spatial_delta_stride(x, 3, offset, carry=carry, hist=hist)
        np.testing.assert_array_equal(got, want, what)
        np.testing.assert_array_equal(hist - np.uint64(3), _counts(want), "histogram, " + what)
        hold[1:] = x
        np.testing.assert_array_equal(ctx.spatial_delta_stride(hold[1:], 3, offset, carry=carry, out=out[1:]), want, what)
        if offset:
            continue            # the inverse seam has no offset: once per carry
        # full-range deltas (`x` itself, read as a delta stream) and what the encoder made of x
        np.testing.assert_array_equal(ctx.spatial_undelta_stride(x, 3, carry=carry), sd.decode(x, 3, False, carry), "undelta, " + what)
        np.testing.assert_array_equal(ctx.spatial_undelta_stride(want, 3, carry=carry), x, "round trip, " + what)
        hold[1:] = want
        np.testing.assert_array_equal(ctx.spatial_undelta_stride(hold[1:], 3, carry=carry, out=out[1:]), x, "odd offset, " + what)


ALL = [(None, 0), (None, 1), (CARRY, 0), (CARRY, 1)]


@pytest.mark.parametrize("n", SIZES)
def test_seams_are_the_numpy_functions(ctx, sd, n):
    _check_seams(ctx, sd, n, ALL, n)


def test_seams_when_a_wave_owns_two_tiles(ctx, sd):
    """The only launch shape in which k_scan3p's run of a wave has a second tile (and k_undelta_carry_s3's grid wraps)."""
    n = N_TWO_TILES
    x = _stack(n, 1)
    for carry in (None, CARRY):
        s = sd.encode(x, 3, False, carry)
        np.testing.assert_array_equal(ctx.spatial_delta_stride(x, 3, 0, carry=carry), s)
        np.testing.assert_array_equal(ctx.spatial_undelta_stride(s, 3, carry=carry), x)
    n0 = n // 3 * 3
    np.testing.assert_array_equal(ctx.undelta_carry_stride(sd.encode(x, 3, False), n0, 3), x[n0 - 3: n0])


@pytest.mark.parametrize("n", [1, 2, 3, 4, 7, 8, 49, 4097, 12289])
def test_stride_one_gives_the_flat_seams_bytes(ctx, sd, n):
    from oracle import oracle as O
    x = _stack(n, 50 + n)
    for carry in (None, np.array([-5], np.int16)):
        c = None if carry is None else int(carry[0])
        for offset in (0, 1):
            flat = ctx.spatial_delta(x, offset, carry=c)
            np.testing.assert_array_equal(ctx.spatial_delta_stride(x, 1, offset, carry=carry), flat)
            np.testing.assert_array_equal(flat, sd.encode(x, 1, offset, carry))
        s = ctx.spatial_delta(x, 0, carry=c)
        np.testing.assert_array_equal(ctx.spatial_undelta_stride(s, 1, carry=carry), ctx.spatial_undelta(s, carry=c))
        np.testing.assert_array_equal(ctx.spatial_undelta_stride(s, 1, carry=carry), x)
    np.testing.assert_array_equal(ctx.spatial_delta_stride(x, 1, 0), O.finding_difference_enc(x))
    if n > 1:
        s = sd.encode(x, 1, False)
        assert int(ctx.undelta_carry_stride(s, n - 1, 1)[0]) == ctx.undelta_carry(s, n - 1) == int(x[n - 2])


@pytest.mark.parametrize("n", [49, 4099, 12289])
def test_seams_on_device_buffers_off_alignment(ctx, sd, n):
    """Device buffers that start off the 16-byte grid take the element-by-element path of both kernels; guard elements stay."""
    import torch
    x = _stack(n, 9)
    want = sd.encode(x, 3, True, CARRY)
    plain = sd.encode(x, 3, False, CARRY)
    for s_in, s_out in [(0, 0), (1, 1), (3, 3), (0, 5), (8, 8), (1, 0)]:
        src = torch.zeros(n + 64, dtype=torch.int16, device="cuda")
        src[s_in: s_in + n].copy_(torch.from_numpy(x))
        out = torch.full((n + 64,), 0x5A5A, dtype=torch.int16, device="cuda")
        hist = torch.zeros(NBINS, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        ctx.spatial_delta_stride(src[s_in: s_in + n], 3, 1, carry=CARRY, hist=hist, out=out[s_out: s_out + n])
        ctx.synchronize()
        o = out.cpu().numpy()
        assert (o[s_out: s_out + n] == want).all(), (s_in, s_out)
        assert (o[:s_out] == 0x5A5A).all() and (o[s_out + n:] == 0x5A5A).all(), "guard elements written at %r" % ((s_in, s_out),)
        np.testing.assert_array_equal(hist.cpu().numpy().astype(np.uint64), _counts(want))
        src[s_in: s_in + n].copy_(torch.from_numpy(plain))
        out.fill_(0x5A5A)
        torch.cuda.synchronize()
        ctx.spatial_undelta_stride(src[s_in: s_in + n], 3, carry=CARRY, out=out[s_out: s_out + n])
        ctx.synchronize()
        o = out.cpu().numpy()
        assert (o[s_out: s_out + n] == x).all(), (s_in, s_out)
        assert (o[:s_out] == 0x5A5A).all() and (o[s_out + n:] == 0x5A5A).all(), "guard elements written at %r" % ((s_in, s_out),)
        n0 = n // 3 * 3
        src[s_in: s_in + n].copy_(torch.from_numpy(sd.encode(x, 3, False)))
        torch.cuda.synchronize()
        np.testing.assert_array_equal(ctx.undelta_carry_stride(src[s_in: s_in + n], n0, 3), x[n0 - 3: n0])


@pytest.mark.parametrize("n", [3, 6, 24, 27, 48, 3072, 12288, 1048581 // 3 * 3, 5000001])
def test_undelta_carry_stride_with_and_without_a_table(ctx, sd, n):
    rng = np.random.default_rng(n)
    x = _stack(n + 5, n)
    s = sd.encode(x, 3, False)
    for n0 in sorted({3, n // 2 // 3 * 3 or 3, n}):
        np.testing.assert_array_equal(ctx.undelta_carry_stride(s, n0, 3), x[n0 - 3: n0], "raw symbols, n0 %d" % n0)
    d = rng.integers(-255, 256, n + 5).astype(np.int16)            # a delta stack as the encoder has it: a table applies
    payload, table = sd.payload_from_delta(d, True)
    for n0 in sorted({3, n // 2 // 3 * 3 or 3, n}):
        np.testing.assert_array_equal(ctx.undelta_carry_stride(payload, n0, 3, table), d[n0 - 3: n0], "ranks, n0 %d" % n0)
    hold = np.empty(payload.size + 1, np.int16)
    hold[1:] = payload
    np.testing.assert_array_equal(ctx.undelta_carry_stride(hold[1:], n, 3, table), d[n - 3: n])


def test_seam_refusals(ctx):
    from tezip_amd import _lib
    x = np.zeros(12, np.int16)
    for call in (lambda: ctx.spatial_delta_stride(x, 2, 0), lambda: ctx.spatial_undelta_stride(x, 0),
                 lambda: ctx.undelta_carry_stride(x, 6, 2), lambda: ctx.undelta_carry_stride(x, 4, 3),
                 lambda: ctx.undelta_carry_stride(x, 0, 3)):
        with pytest.raises(_lib.TezipError) as e:
            call()
        assert e.value.status == -1


# ------------------------------------------------------------------------------------------- encode / decode on a rollout
WINDOW = 2
VARIANTS = [("abs", [0.0], True), ("rel", [1e-3], True), ("abs", [2.0], True), ("abs", [2.0], False)]
IDS = ["lossless", "rel1e-3", "abs2", "abs2-n"]


def _model():
    from tezip_amd.prednet import PredNetConfig
    cfg = PredNetConfig(stack_sizes=(3, 16, 32))
    return cfg, cfg.init_weights(seed=4, bias_scale=0.2)


@pytest.fixture(scope="module", params=[(3, 21, 30), (5, 40, 56)], ids=["3x21x30", "5x40x56"])
def rolled(request):
    """A context with the encoder rollout of a colour job, the job, and per variant what mode 0 makes of it."""
    from tezip_amd import _lib, synth
    nt, h, w = request.param
    cfg, wts = _model()
    frames = np.ascontiguousarray(synth.translating_scene(nt, h, w, seed=3))
    c = _lib.Context(0)
    c.load_model(cfg, wts)
    c.prepare(pad8(h), pad8(w), 4)
    key = c.rollout(frames, 0, WINDOW)[0]
    flat = []
    for mode, bound, entropy in VARIANTS:
        payload, table, delta = c.encode(mode, bound, entropy, want_delta=True)
        flat.append((payload.copy(), None if table is None else table.copy(), delta.copy()))
    yield c, frames, key, flat
    c.close()


@pytest.mark.parametrize("v", range(len(VARIANTS)), ids=IDS)
def test_encode_under_the_channel_stride(rolled, sd, v):
    from tezip_amd import _lib
    ctx, frames, key, flat = rolled
    mode, bound, entropy = VARIANTS[v]
    payload0, table0, delta = flat[v]
    n = frames.size
    want_payload, want_table = sd.payload_from_delta(delta, entropy)
    ctx.set_delta_stride(1)
    try:
        assert ctx.get_delta_stride() == 1
        payload, table, delta1 = ctx.encode(mode, bound, entropy, want_delta=True)
        np.testing.assert_array_equal(delta1, delta, "the delta stack does not depend on the stride")
        np.testing.assert_array_equal(payload, want_payload)
        if entropy:
            assert len(table) == len(want_table)
            np.testing.assert_array_equal(table, want_table)
        else:
            assert table is None
        np.testing.assert_array_equal(ctx.encode(mode, bound, entropy)[0], want_payload)     # without the tap
        ctx.encode(mode, bound, entropy, payload="resident")
        np.testing.assert_array_equal(np.concatenate([ctx.payload_get(0, 5), ctx.payload_get(5, n - 5)]), want_payload)
        q1 = ctx.encode_quality("resident", table)
        d1 = ctx.encode_digests(payload, table)
        if n % 8 == 0:
            planes, t2, _ = ctx.encode(mode, bound, entropy, shuffle=True)
            np.testing.assert_array_equal(ctx.byte_unshuffle(planes.view(np.uint8)), want_payload)
            if entropy:
                np.testing.assert_array_equal(t2, want_table)
            assert ctx.encode_quality(planes, t2, shuffle=True).tolist() == q1.tolist()
        else:                                       # 3 x 21 x 30 x 3 elements: the shuffle bit is refused as under mode 0
            with pytest.raises(_lib.TezipError) as e:
                ctx.encode(mode, bound, entropy, shuffle=True)
            assert e.value.status == -1
        ctx.set_delta_stride(0)
        assert ctx.get_delta_stride() == 0
        with pytest.raises(_lib.TezipError):       # the change dropped the resident payload
            ctx.encode_quality("resident", table0)
        assert ctx.encode_quality(payload0, table0).tolist() == q1.tolist(), "the quality of the job does not depend on the stride"
        d0 = ctx.encode_digests(payload0, table0)
        np.testing.assert_array_equal(d0[0], d1[0])
        np.testing.assert_array_equal(d0[1], d1[1])
        np.testing.assert_array_equal(ctx.encode(mode, bound, entropy)[0], payload0)          # mode 0 is what it was
    finally:
        ctx.set_delta_stride(0)


def test_decode_and_ranges(rolled, sd):
    from tezip_amd import _lib
    enc, frames, key, flat = rolled
    nt, h, w = frames.shape[:3]
    fe = h * w * 3
    cfg, wts = _model()
    strided = []
    enc.set_delta_stride(1)
    try:
        for mode, bound, entropy in VARIANTS:
            payload, table, _ = enc.encode(mode, bound, entropy)
            strided.append((payload.copy(), None if table is None else table.copy()))
    finally:
        enc.set_delta_stride(0)
    key_stack = np.where(key[:, None, None, None], frames, 0).astype(np.uint8)
    ctx = _lib.Context(0)
    try:
        ctx.load_model(cfg, wts)
        ctx.prepare(pad8(h), pad8(w), 4)
        ctx.rollout_decode(key_stack, 0)
        wholes = []
        for (p0, t0, delta), (p1, t1) in zip(flat, strided):
            ctx.set_delta_stride(0)
            want = ctx.decode(p0, t0).copy()
            ctx.set_delta_stride(1)
            np.testing.assert_array_equal(ctx.decode(p1, t1), want)
            wholes.append(want)
        np.testing.assert_array_equal(wholes[0], frames)                       # lossless
        assert int(np.abs(wholes[2].astype(int) - frames.astype(int)).max()) <= 2
        for first, count in ((0, 1), (1, 2), (4, 1)):
            if first + count > nt:
                continue                                                       # (4, 1) needs the five-frame job
            ctx.rollout_decode_range(key_stack, 0, first, count)
            for (p0, t0, delta), (p1, t1), whole in zip(flat, strided, wholes):
                np.testing.assert_array_equal(ctx.decode_range(p1, t1, first, count), whole[first: first + count])
                if first:
                    n0 = first * fe
                    np.testing.assert_array_equal(ctx.undelta_carry_stride(p1, n0, 3, t1), delta.reshape(-1)[n0 - 3: n0])
                    np.testing.assert_array_equal(sd.delta_from_payload(p1, t1)[n0 - 3: n0], delta.reshape(-1)[n0 - 3: n0])
    finally:
        ctx.close()


def test_unsupported_entry_points_and_invalid_mode(rolled):
    from tezip_amd import _lib
    ctx, frames, key, flat = rolled
    with pytest.raises(_lib.TezipError) as e:
        ctx.set_delta_stride(2)
    assert e.value.status == -1 and ctx.get_delta_stride() == 0
    ctx.set_delta_stride(1)
    try:
        for call, name in ((lambda: ctx.encode_begin("abs", [2.0], True), "tz_encode_begin"),
                           (lambda: ctx.encode_finish(None, None), "tz_encode_finish"),
                           (lambda: ctx.encode_delta("abs", [2.0]), "tz_encode_delta"),
                           (lambda: ctx.decode_delta(np.zeros(frames.shape, np.int16)), "tz_decode_delta"),
                           (lambda: ctx.undelta_carry(flat[0][0], 3, flat[0][1]), "tz_undelta_carry")):
            with pytest.raises(_lib.TezipError) as e:
                call()
            assert e.value.status == -6 and name in str(e.value) and "tz_set_delta_stride" in str(e.value), name
    finally:
        ctx.set_delta_stride(0)
    ctx.encode_delta("abs", [2.0])                                             # mode 0: served as ever


# ------------------------------------------------------------------------------------------------------------ the CLI
def _read(d, n):
    with open(os.path.join(d, n), "rb") as f:
        return f.read()


def _tezip(args):
    """tezip.py's main in this process -> (exit status, stdout)."""
    from tezip_amd import tezip
    buf = io.StringIO()
    code = 0
    with contextlib.redirect_stdout(buf):
        try:
            tezip.main(tezip.build_parser().parse_args([str(a) for a in args]))
        except SystemExit as e:
            code = 0 if e.code is None else e.code
    return code, buf.getvalue()


NT = 12
LOSSY = ["-p", "0", "-w", "4", "-m", "abs", "-b", "2"]


@pytest.fixture(scope="module")
def jobs(tmp_path_factory):
    from PIL import Image
    from tezip_amd import _lib, synth, weights
    tmp = tmp_path_factory.mktemp("sdelta")
    cfg, wts = _model()
    out = {}
    for name, frames in (("colour", synth.translating_scene(NT, 61, 90)), ("gray", synth.moving_blobs(NT, 64, 64))):
        mdir, ddir = str(tmp / (name + "_model")), tmp / (name + "_data")
        weights.save_model(mdir, cfg, wts, _lib.pad8(frames.shape[1]), _lib.pad8(frames.shape[2]))
        ddir.mkdir()
        names = ["f_%03d.png" % t for t in range(NT)]
        for t, f in enumerate(frames):
            Image.fromarray(f).save(ddir / names[t])
        out[name] = (mdir, str(ddir), names)
    os.environ.pop("WORLD_SIZE", None)
    return tmp, out


def _trailer(path):
    from tezip_amd import decompress, zstd
    data = _read(path, "entropy.dat")
    fmt = decompress.coded_format(data[:4])
    if fmt is not None:
        p = fmt.parse(np.frombuffer(data, np.uint8))
        return tuple(int(v) for v in p.shape)
    return tuple(int(v) for v in decompress.parse_stream(zstd.decompress(data))[2])


@pytest.mark.parametrize("coder", ["zstd", "huffd"])
def test_cli_round_trip(jobs, monkeypatch, coder):
    tmp, sets = jobs
    mdir, ddir, names = sets["colour"]
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("TEZIP_NO_STREAMING", raising=False)
    d = {k: str(tmp / ("%s_%s" % (k, coder))) for k in ("plain_c", "flat_c", "flat_u", "chan_c", "chan_u", "part", "slow", "poison")}
    common = LOSSY + ["--coder", coder, "--report", "--digests"]
    code, text = _tezip(["-c", mdir, ddir, d["plain_c"]] + common)
    assert code == 0 and "sdelta" not in text, text
    code, text = _tezip(["-c", mdir, ddir, d["flat_c"]] + common + ["--sdelta", "flat"])
    assert code == 0 and "sdelta" not in text, text
    for n in ("entropy.dat", "key_frame.dat", "filename.txt", "tezip_amd.json", "frame_digests.json"):
        assert _read(d["flat_c"], n) == _read(d["plain_c"], n), "--sdelta flat changes %s" % n
    assert _trailer(d["flat_c"]) == (1, NT, 61, 90, 3)
    code, text = _tezip(["-u", mdir, d["flat_c"], d["flat_u"], "--verify", "require"])
    assert code == 0, text

    code, text = _tezip(["-c", mdir, ddir, d["chan_c"]] + common + ["--sdelta", "channel"])
    assert code == 0 and "sdelta: channel (stride 3)" in text, text
    assert _trailer(d["chan_c"]) == (4, NT, 61, 90, 3)
    assert json.loads(_read(d["chan_c"], "tezip_amd.json"))["sdelta"] == "channel"
    assert "sdelta" not in json.loads(_read(d["flat_c"], "tezip_amd.json"))
    for n in ("key_frame.dat", "filename.txt", "frame_digests.json"):
        assert _read(d["chan_c"], n) == _read(d["flat_c"], n), n
    qf, qc = (json.loads(_read(d[k], "quality.json")) for k in ("flat_c", "chan_c"))
    assert qc["max_abs_err"] == qf["max_abs_err"] <= 2 and qc["psnr_db"] == qf["psnr_db"]
    assert [f["max_abs_err"] for f in qc["per_frame"]] == [f["max_abs_err"] for f in qf["per_frame"]]
    print("%s: entropy.dat %d bytes flat, %d bytes channel" % (coder, len(_read(d["flat_c"], "entropy.dat")), len(_read(d["chan_c"], "entropy.dat"))))
    code, text = _tezip(["-u", mdir, d["chan_c"], d["chan_u"], "--verify", "require"])
    assert code == 0 and "verified: %d frames" % NT in text, text
    assert sorted(os.listdir(d["chan_u"])) == names
    for nm in names:
        assert _read(d["chan_u"], nm) == _read(d["flat_u"], nm), nm
    code, text = _tezip(["-u", mdir, d["chan_c"], d["part"], "--frames", "5:9"])
    assert code == 0, text
    assert sorted(os.listdir(d["part"])) == names[5:9]
    for nm in names[5:9]:
        assert _read(d["part"], nm) == _read(d["flat_u"], nm), nm
    monkeypatch.setenv("TEZIP_NO_STREAMING", "1")                      # the whole-array path of -u
    code, text = _tezip(["-u", mdir, d["chan_c"], d["slow"], "--verify", "require"])
    assert code == 0 and "verified: %d frames" % NT in text, text
    for nm in names:
        assert _read(d["slow"], nm) == _read(d["flat_u"], nm), nm
    monkeypatch.delenv("TEZIP_NO_STREAMING")
    # TEZIP_POISON is read once per process: a fresh child writes the same entropy.dat from poisoned buffers
    env = dict(os.environ, TEZIP_POISON="0xA5")
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m", "tezip_amd.tezip", "-c", mdir, ddir, d["poison"]] + common
                       + ["--sdelta", "channel"], cwd=ROOT, capture_output=True, text=True, env=env, timeout=330)
    assert r.returncode == 0, r.stdout + r.stderr
    assert _read(d["poison"], "entropy.dat") == _read(d["chan_c"], "entropy.dat")


def test_cli_shuffle_and_sidecar_contradiction(jobs, monkeypatch):
    tmp, sets = jobs
    mdir, ddir, names = sets["colour"]
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("TEZIP_NO_STREAMING", raising=False)
    # 61 x 90 frames hold no multiple of 8 elements: the byte planes need the 64 x 64 job's shape, in colour
    from PIL import Image
    from tezip_amd import _lib, synth, weights
    cfg, wts = _model()
    m2, d2 = str(tmp / "sq_model"), tmp / "sq_data"
    weights.save_model(m2, cfg, wts, 64, 64)
    d2.mkdir()
    for t, f in enumerate(synth.translating_scene(NT, 64, 64)):
        Image.fromarray(f).save(d2 / names[t])
    c_flat, c_chan, u_flat, u_chan = (str(tmp / k) for k in ("shf_c", "shc_c", "shf_u", "shc_u"))
    assert _tezip(["-c", m2, d2, c_flat] + LOSSY + ["--shuffle"])[0] == 0
    code, text = _tezip(["-c", m2, d2, c_chan] + LOSSY + ["--shuffle", "--sdelta", "channel"])
    assert code == 0 and "sdelta: channel (stride 3)" in text, text
    assert _trailer(c_chan) == (5, NT, 64, 64, 3) and _trailer(c_flat) == (2, NT, 64, 64, 3)
    assert _tezip(["-u", m2, c_flat, u_flat])[0] == 0
    assert _tezip(["-u", m2, c_chan, u_chan])[0] == 0
    for nm in names:
        assert _read(u_chan, nm) == _read(u_flat, nm), nm
    # a sidecar that contradicts the trailer belongs to another stream
    doc = json.loads(_read(c_chan, "tezip_amd.json"))
    del doc["sdelta"]
    with open(os.path.join(c_chan, "tezip_amd.json"), "w") as f:
        json.dump(doc, f)
    with pytest.raises(ValueError, match="spatial delta"):
        _tezip(["-u", m2, c_chan, str(tmp / "never")])


def test_cli_gray_job_writes_the_files_of_gray_alone(jobs, monkeypatch):
    tmp, sets = jobs
    mdir, ddir, names = sets["gray"]
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    both, alone = str(tmp / "gray_both"), str(tmp / "gray_alone")
    code, text = _tezip(["-c", mdir, ddir, both] + LOSSY + ["--gray", "--sdelta", "channel"])
    assert code == 0 and "sdelta: channel equals flat on a one-channel payload" in text and "gray: yes" in text, text
    code, text = _tezip(["-c", mdir, ddir, alone] + LOSSY + ["--gray"])
    assert code == 0 and "sdelta" not in text, text
    assert sorted(os.listdir(both)) == sorted(os.listdir(alone))
    for n in os.listdir(alone):
        assert _read(both, n) == _read(alone, n), n
    assert _trailer(both) == (1, NT, 64, 64, 1)
