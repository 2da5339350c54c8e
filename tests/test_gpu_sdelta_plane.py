"""The 2-D spatial delta of the payload (`-c --sdelta plane`, tz_set_delta_plane(1), definition TZ-SD2) on the GPU:
k_sdelta_plane, k_unplane_cols and k_unplane_rows give the numpy statement (tezip_amd/sdelta.py encode_plane / decode_plane) bit
for bit, histogram included; tz_encode under plane gives the payload and table that statement makes of the flat encode's own
delta stack; the decoder restores the frames the flat job restores; a range decode takes no carry; and the command line
round-trips to the images of the flat job."""
import contextlib
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import devmem

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NBINS = 2111
# the kernels' own boundaries (tezip_amd/csrc/tz_codec.hip)
UNPLANE_ROW_TILE = 512     # elements of a wave-tile of k_unplane_rows (64 lanes x 8)
UNPLANE_BAND_ROWS = 32     # k_unplane_cols walks a frame as one band up to this many rows, else as up to four of >= this many
# (H, W): the sizes of the issue; then a row of exactly one wave-tile of pass two with one channel, one element more (with one
# channel, and 171 x 3 = 513 with three), an H one row past a band boundary of pass one, and frames of three and of four bands
FRAMES = [(1, 1), (1, 9), (9, 1), (3, 5), (7, 11), (16, 24),
          (2, UNPLANE_ROW_TILE), (2, UNPLANE_ROW_TILE + 1), (2, (UNPLANE_ROW_TILE + 1) // 3), (UNPLANE_BAND_ROWS + 1, 5),
          (2 * UNPLANE_BAND_ROWS + 6, 4), (4 * UNPLANE_BAND_ROWS + 2, 4)]
EXTREMES = np.array([-255, -254, 0, 254, 255], np.int16)


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
    inside = y[(y >= 0) & (y < NBINS)].astype(np.int64)
    return np.bincount(inside, minlength=NBINS).astype(np.uint64)


def _stacks(shape, seed):
    """The extreme-value stack (45 % of its symbols wrap) and an encoder-like one (small deltas around 0 with a few far ones,
    so that the histogram's central bins and its far bins both occur)."""
    rng = np.random.default_rng(seed)
    small = rng.integers(-6, 7, shape).astype(np.int16)
    far = rng.random(shape) < 0.05
    small[far] = rng.integers(-255, 256, int(far.sum()))
    return [rng.choice(EXTREMES, size=shape).astype(np.int16), small]


@pytest.mark.parametrize("frame", FRAMES, ids=["%dx%d" % f for f in FRAMES])
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("nt", [1, 3])
def test_seams_are_the_numpy_functions(ctx, sd, frame, channels, nt):
    shape = (nt,) + frame + (channels,)
    for k, q in enumerate(_stacks(shape, sum(shape))):
        what = "%r stack %d" % (shape, k)
        for offset in (0, 1):
            want = sd.encode_plane(q, offset)
            hist = np.full(NBINS, 3, np.uint64)                      # the counts are ADDED
            got = ctx.spatial_delta_plane(q, shape, offset, hist=hist)
            np.testing.assert_array_equal(got, want, what)
            np.testing.assert_array_equal(hist - np.uint64(3), _counts(want), "histogram, " + what)
            np.testing.assert_array_equal(ctx.spatial_delta_plane(q, shape, offset), want, what)        # without the histogram
        raw = sd.encode_plane(q, False)
        np.testing.assert_array_equal(ctx.spatial_undelta_plane(raw, shape), q.reshape(-1), "undelta, " + what)
        payload, table = sd.payload_from_delta(q, True, plane=True)
        np.testing.assert_array_equal(ctx.spatial_undelta_plane(payload, shape, table), q.reshape(-1), "undelta through the LUT, " + what)


@pytest.mark.parametrize("frame", [(3, 5), (16, 24), (UNPLANE_BAND_ROWS + 1, 8), (2, UNPLANE_ROW_TILE)], ids=lambda f: "%dx%d" % f)
@pytest.mark.parametrize("channels", [1, 3])
def test_seams_on_device_buffers_one_element_off_the_grid(ctx, sd, frame, channels):
    """Device buffers that start one element behind a 16-byte boundary take the element-by-element routes; guard bytes stay."""
    import torch
    shape = (3,) + frame + (channels,)
    q = _stacks(shape, 5)[0]
    want = sd.encode_plane(q, True)
    payload, table = sd.payload_from_delta(q, True, plane=True)
    for off_in, off_out in ((2, 2), (0, 2), (2, 0), (0, 0)):
        what = "%r offsets %d / %d" % (shape, off_in, off_out)
        src, src_ok = devmem.view(q.reshape(-1), off_in)
        out, out_ok = devmem.view(devmem.fill(q.size, np.int16), off_out)
        hist = torch.zeros(NBINS, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        ctx.spatial_delta_plane(src, shape, 1, hist=hist, out=out)
        ctx.synchronize()
        np.testing.assert_array_equal(devmem.host(out), want, what)
        np.testing.assert_array_equal(hist.cpu().numpy().astype(np.uint64), _counts(want), what)
        assert src_ok() and out_ok(), "guard bytes written, " + what
        src, src_ok = devmem.view(payload, off_in)
        out, out_ok = devmem.view(devmem.fill(q.size, np.int16), off_out)
        ctx.spatial_undelta_plane(src, shape, table, out=out)
        ctx.synchronize()
        np.testing.assert_array_equal(devmem.host(out), q.reshape(-1), "undelta, " + what)
        assert src_ok() and out_ok(), "guard bytes written by the inverse, " + what


def test_seam_and_setter_refusals(ctx):
    from tezip_amd import _lib
    x = np.zeros(24, np.int16)
    for call in (lambda: ctx.spatial_delta_plane(x, (1, 2, 6, 2), 0), lambda: ctx.spatial_undelta_plane(x, (1, 0, 4, 3)),
                 lambda: ctx.spatial_delta_plane(x, (1, 2, 0, 3), 0), lambda: ctx.set_delta_plane(2), lambda: ctx.set_delta_plane(-1)):
        with pytest.raises(_lib.TezipError) as e:
            call()
        assert e.value.status == -1
    assert ctx.get_delta_plane() == 0
    # one spatial delta per payload: each setter refuses while the other is in force, and names both calls
    ctx.set_delta_stride(1)
    try:
        with pytest.raises(_lib.TezipError) as e:
            ctx.set_delta_plane(1)
        assert e.value.status == -1 and "tz_set_delta_plane" in str(e.value) and "tz_set_delta_stride" in str(e.value)
        assert ctx.get_delta_plane() == 0
    finally:
        ctx.set_delta_stride(0)
    ctx.set_delta_plane(1)
    try:
        assert ctx.get_delta_plane() == 1
        with pytest.raises(_lib.TezipError) as e:
            ctx.set_delta_stride(1)
        assert e.value.status == -1 and "tz_set_delta_plane" in str(e.value) and "tz_set_delta_stride" in str(e.value)
        with pytest.raises(_lib.TezipError) as e:
            ctx.set_delta_stride(2)                     # as ever
        assert e.value.status == -1
        ctx.set_delta_stride(0)
        assert ctx.get_delta_stride() == 0
    finally:
        ctx.set_delta_plane(0)
    assert ctx.get_delta_plane() == 0


# ------------------------------------------------------------------------------------------- encode / decode on a rollout
WINDOW = 2
VARIANTS = [("greedy", [0.0]), ("greedy", [2.0]), ("lattice", [2.0])]
IDS = ["lossless", "abs2-greedy", "abs2-lattice"]


def _model():
    from tezip_amd.prednet import PredNetConfig
    cfg = PredNetConfig(stack_sizes=(3, 16, 32))
    return cfg, cfg.init_weights(seed=4, bias_scale=0.2)


def _frames(nt, h, w, gray):
    from tezip_amd import synth
    f = np.ascontiguousarray(synth.translating_scene(nt, h, w, seed=3))
    return np.ascontiguousarray(np.repeat(f[..., :1], 3, axis=-1)) if gray else f


JOBS = [(5, 24, 40, False), (5, 61, 90, False), (5, 24, 40, True), (5, 61, 90, True)]


@pytest.fixture(scope="module", params=JOBS, ids=["%dx%dx%d%s" % (j[0], j[1], j[2], "-gray" if j[3] else "") for j in JOBS])
def rolled(request):
    """A context with the encoder rollout of a job (unpadded 24 x 40, padded 61 x 90; colour, or all gray for the one-channel
    payload), and per variant what the flat layout makes of it: payload, table, the three-channel delta stack, quality and
    digest records."""
    from tezip_amd import _lib
    nt, h, w, gray = request.param
    cfg, wts = _model()
    frames = _frames(nt, h, w, gray)
    c = _lib.Context(0)
    c.load_model(cfg, wts)
    c.prepare(pad8(h), pad8(w), 4)
    key = c.rollout(frames, 0, WINDOW)[0]
    flat = []
    for quant, bound in VARIANTS:
        c.set_quantiser(quant)
        _, _, delta = c.encode("abs", bound, True, want_delta=True)
        c.set_payload_channels(1 if gray else 3)
        payload, table, _ = c.encode("abs", bound, True)
        flat.append((payload.copy(), table.copy(), delta.copy(), c.encode_quality(payload, table).copy(), c.encode_digests(payload, table)))
        c.set_payload_channels(3)
    c.set_quantiser("greedy")
    yield c, frames, key, flat, gray
    c.close()


@pytest.mark.parametrize("v", range(len(VARIANTS)), ids=IDS)
def test_encode_under_plane(rolled, sd, v):
    from tezip_amd import _lib
    ctx, frames, key, flat, gray = rolled
    quant, bound = VARIANTS[v]
    payload0, table0, delta, q0, d0 = flat[v]
    channels = 1 if gray else 3
    n = frames.size // 3 * channels
    stack = delta[..., :channels]
    want_payload, want_table = sd.payload_from_delta(stack, True, plane=True)
    want_raw, _ = sd.payload_from_delta(stack, False, plane=True)
    ctx.set_quantiser(quant)
    ctx.set_payload_channels(channels)
    ctx.set_delta_plane(1)
    try:
        assert ctx.get_delta_plane() == 1
        if gray:
            payload, table, _ = ctx.encode("abs", bound, True)
        else:
            payload, table, delta1 = ctx.encode("abs", bound, True, want_delta=True)
            np.testing.assert_array_equal(delta1, delta, "the delta stack does not depend on the spatial delta")
            np.testing.assert_array_equal(ctx.encode("abs", bound, True)[0], want_payload)     # without the tap
            np.testing.assert_array_equal(ctx.encode_delta("abs", bound).reshape(delta.shape), delta)
        np.testing.assert_array_equal(payload, want_payload)
        np.testing.assert_array_equal(table, want_table)
        raw, none, _ = ctx.encode("abs", bound, False)
        assert none is None
        np.testing.assert_array_equal(raw, want_raw)
        ctx.encode("abs", bound, True, payload="resident")
        np.testing.assert_array_equal(np.concatenate([ctx.payload_get(0, 5), ctx.payload_get(5, n - 5)]), want_payload)
        q1 = ctx.encode_quality("resident", table)
        assert q1.tolist() == q0.tolist(), "the quality of the job does not depend on the spatial delta"
        d1 = ctx.encode_digests(payload, table)
        np.testing.assert_array_equal(d1[0], d0[0])
        np.testing.assert_array_equal(d1[1], d0[1])
        assert ctx.bound_probe("abs", bound).tolist() == q0.tolist()
        s1 = ctx.encode_ssim(payload, table)
        ctx.set_delta_plane(0)
        assert ctx.encode_ssim(payload0, table0).tolist() == s1.tolist()
        ctx.set_delta_plane(1)
        if n % 8 == 0:
            planes, t2, _ = ctx.encode("abs", bound, True, shuffle=True)
            np.testing.assert_array_equal(ctx.byte_unshuffle(planes.view(np.uint8)), want_payload)
            np.testing.assert_array_equal(t2, want_table)
            assert ctx.encode_quality(planes, t2, shuffle=True).tolist() == q0.tolist()
        else:                                       # the shuffle bit is refused as without plane
            with pytest.raises(_lib.TezipError) as e:
                ctx.encode("abs", bound, True, shuffle=True)
            assert e.value.status == -1
        if not gray and v == 1:                     # frame bounds: frame f as `abs bounds[f]`
            bounds = [0.0, 2.0, 0.0, 3.0, 1.0]
            ctx.set_frame_bounds(bounds)
            try:
                pb, tb, db = ctx.encode("abs", [0.0], True, want_delta=True)
                wp, wt = sd.payload_from_delta(db, True, plane=True)
                np.testing.assert_array_equal(pb, wp)
                np.testing.assert_array_equal(tb, wt)
                assert (db != delta).any()
            finally:
                ctx.set_frame_bounds(None)
        ctx.encode("abs", bound, True, payload="resident")
        ctx.set_delta_plane(0)
        with pytest.raises(_lib.TezipError):       # the change dropped the resident payload
            ctx.encode_quality("resident", table0)
        np.testing.assert_array_equal(ctx.encode("abs", bound, True)[0], payload0)             # plane off: what it was
    finally:
        ctx.set_delta_plane(0)
        ctx.set_payload_channels(3)
        ctx.set_quantiser("greedy")


def test_decode_and_ranges(rolled, sd, monkeypatch):
    from tezip_amd import _lib
    enc, frames, key, flat, gray = rolled
    nt, h, w = frames.shape[:3]
    channels = 1 if gray else 3
    cfg, wts = _model()
    plane = []
    enc.set_payload_channels(channels)
    enc.set_delta_plane(1)
    try:
        for quant, bound in VARIANTS:
            enc.set_quantiser(quant)
            payload, table, _ = enc.encode("abs", bound, True)
            plane.append((payload.copy(), table.copy()))
    finally:
        enc.set_delta_plane(0)
        enc.set_payload_channels(3)
        enc.set_quantiser("greedy")
    key_stack = np.where(key[:, None, None, None], frames, 0).astype(np.uint8)
    ctx = _lib.Context(0)
    try:
        ctx.load_model(cfg, wts)
        ctx.prepare(pad8(h), pad8(w), 4)
        ctx.set_payload_channels(channels)
        ctx.rollout_decode(key_stack, 0)
        wholes = []
        for (p0, t0, _, _, _), (p1, t1) in zip(flat, plane):
            ctx.set_delta_plane(0)
            want = ctx.decode(p0, t0).copy()
            ctx.set_delta_plane(1)
            np.testing.assert_array_equal(ctx.decode(p1, t1), want)
            wholes.append(want)
        np.testing.assert_array_equal(wholes[0], frames)                       # lossless
        # pass two reconstructs itself on unpadded frames whose rows are whole 16-byte groups (24 x 40), and leaves the delta
        # stack to the reconstruct kernel on padded ones (61 x 90) and under TEZIP_DECODE_UNFUSED=1: the same frames either way
        fused = (h, w) == (pad8(h), pad8(w)) and (w * channels) % 8 == 0
        ctx.prof_enable(True)
        ctx.prof_reset()
        np.testing.assert_array_equal(ctx.decode(plane[1][0], plane[1][1]), wholes[1])
        prof = ctx.prof_get()
        assert (int(prof["undelta_scan"][1]), int(prof["reconstruct"][1])) == ((1, 0) if fused else (1, 1))
        ctx.prof_enable(False)
        monkeypatch.setenv("TEZIP_DECODE_UNFUSED", "1")                        # read when a context is made
        unfused = _lib.Context(0)
        try:
            unfused.load_model(cfg, wts)
            unfused.prepare(pad8(h), pad8(w), 4)
            unfused.set_payload_channels(channels)
            unfused.set_delta_plane(1)
            unfused.rollout_decode(key_stack, 0)
            for (p1, t1), whole in zip(plane, wholes):
                np.testing.assert_array_equal(unfused.decode(p1, t1), whole)
        finally:
            unfused.close()
        monkeypatch.delenv("TEZIP_DECODE_UNFUSED")
        assert int(np.abs(wholes[1].astype(int) - frames.astype(int)).max()) <= 2
        assert int(np.abs(wholes[2].astype(int) - frames.astype(int)).max()) <= 2
        pe = h * w * channels
        for first, count in ((0, 1), (1, 2), (4, 1)):
            ctx.rollout_decode_range(key_stack, 0, first, count)
            for (p1, t1), whole in zip(plane, wholes):
                np.testing.assert_array_equal(ctx.decode_range(p1, t1, first, count), whole[first: first + count])
                # no carry and no read of the payload prefix: whatever lies in front of the range, the frames are the same
                junk = p1.copy()
                junk[: first * pe] = 0
                np.testing.assert_array_equal(ctx.decode_range(junk, t1, first, count), whole[first: first + count])
    finally:
        ctx.close()


def test_unsupported_entry_points(rolled):
    from tezip_amd import _lib
    ctx, frames, key, flat, gray = rolled
    ctx.set_delta_plane(1)
    try:
        for call, name in ((lambda: ctx.encode_begin("abs", [2.0], True), "tz_encode_begin"),
                           (lambda: ctx.encode_finish(None, None), "tz_encode_finish"),
                           (lambda: ctx.decode_delta(np.zeros(frames.shape, np.int16)), "tz_decode_delta"),
                           (lambda: ctx.undelta_carry(flat[0][0], 3, flat[0][1]), "tz_undelta_carry"),
                           (lambda: ctx.undelta_carry_stride(flat[0][0], 3, 3, flat[0][1]), "tz_undelta_carry_stride"),
                           (lambda: ctx.size_probe("abs", [2.0]), "tz_size_probe")):
            with pytest.raises(_lib.TezipError) as e:
                call()
            assert e.value.status == -6 and name in str(e.value) and "tz_set_delta_plane" in str(e.value), name
    finally:
        ctx.set_delta_plane(0)
    ctx.size_probe("abs", [2.0])                                               # plane off: served as ever
    ctx.undelta_carry(flat[0][0], 3, flat[0][1])


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


NT = 8
JOB = ["-p", "0", "-w", "4"]
LOSSLESS = JOB + ["-m", "abs", "-b", "0"]
LATTICE = JOB + ["-m", "abs", "-b", "2", "--quant", "lattice"]
LINE = "sdelta: plane (TZ-SD2)"


@pytest.fixture(scope="module")
def jobs(tmp_path_factory):
    from PIL import Image
    from tezip_amd import _lib, synth, weights
    tmp = tmp_path_factory.mktemp("plane")
    cfg, wts = _model()
    out = {}
    for name, frames in (("colour", synth.translating_scene(NT, 64, 64)), ("gray", synth.moving_blobs(NT, 64, 64))):
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


def _same_images(a, b, names):
    assert sorted(os.listdir(a)) == sorted(names)
    for nm in names:
        assert _read(a, nm) == _read(b, nm), nm


@pytest.mark.parametrize("bound", [LOSSLESS, LATTICE], ids=["lossless", "lattice-abs2"])
def test_cli_round_trip(jobs, monkeypatch, bound):
    tmp, sets = jobs
    mdir, ddir, names = sets["colour"]
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("TEZIP_NO_STREAMING", raising=False)
    tag = "ll" if bound is LOSSLESS else "lat"
    d = {k: str(tmp / ("%s_%s" % (k, tag))) for k in ("flat_c", "flat_u", "plane_c", "plane_u", "part", "slow", "poison")}
    common = bound + ["--report", "--ssim", "--digests"]
    code, text = _tezip(["-c", mdir, ddir, d["flat_c"]] + common)
    assert code == 0 and "sdelta" not in text, text
    assert _tezip(["-u", mdir, d["flat_c"], d["flat_u"], "--verify", "require"])[0] == 0
    code, text = _tezip(["-c", mdir, ddir, d["plane_c"]] + common + ["--sdelta", "plane"])
    assert code == 0 and LINE in text, text
    assert _trailer(d["plane_c"]) == (8, NT, 64, 64, 3) and _trailer(d["flat_c"]) == (1, NT, 64, 64, 3)
    assert json.loads(_read(d["plane_c"], "tezip_amd.json"))["sdelta"] == "plane"
    for n in ("key_frame.dat", "filename.txt", "frame_digests.json"):
        assert _read(d["plane_c"], n) == _read(d["flat_c"], n), n
    qf, qp = (json.loads(_read(d[k], "quality.json")) for k in ("flat_c", "plane_c"))
    assert qp["max_abs_err"] == qf["max_abs_err"] <= 2 and qp["psnr_db"] == qf["psnr_db"]
    print("%s: entropy.dat %d bytes flat, %d bytes plane" % (tag, len(_read(d["flat_c"], "entropy.dat")), len(_read(d["plane_c"], "entropy.dat"))))
    code, text = _tezip(["-u", mdir, d["plane_c"], d["plane_u"], "--verify", "require"])
    assert code == 0 and "verified: %d frames" % NT in text, text
    _same_images(d["plane_u"], d["flat_u"], names)
    code, text = _tezip(["-u", mdir, d["plane_c"], d["part"], "--frames", "2:4"])
    assert code == 0, text
    _same_images(d["part"], d["flat_u"], names[2:4])
    monkeypatch.setenv("TEZIP_NO_STREAMING", "1")                      # the whole-array path of -u
    code, text = _tezip(["-u", mdir, d["plane_c"], d["slow"], "--verify", "require"])
    assert code == 0 and "verified: %d frames" % NT in text, text
    _same_images(d["slow"], d["flat_u"], names)
    monkeypatch.delenv("TEZIP_NO_STREAMING")
    if bound is LATTICE:
        # TEZIP_POISON is read once per process: a fresh child writes the same entropy.dat from poisoned buffers
        env = dict(os.environ, TEZIP_POISON="0xA5")
        r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m", "tezip_amd.tezip", "-c", mdir, ddir, d["poison"]] + common
                           + ["--sdelta", "plane"], cwd=ROOT, capture_output=True, text=True, env=env, timeout=330)
        assert r.returncode == 0, r.stdout + r.stderr
        assert _read(d["poison"], "entropy.dat") == _read(d["plane_c"], "entropy.dat")


@pytest.mark.parametrize("coder", ["huff", "huffr", "huffd"])
def test_cli_coders_round_trip(jobs, monkeypatch, coder):
    tmp, sets = jobs
    mdir, ddir, names = sets["colour"]
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("TEZIP_NO_STREAMING", raising=False)
    flat_u = str(tmp / "coder_flat_u")
    if not os.path.isdir(flat_u):
        assert _tezip(["-c", mdir, ddir, str(tmp / "coder_flat_c")] + LATTICE)[0] == 0
        assert _tezip(["-u", mdir, str(tmp / "coder_flat_c"), flat_u])[0] == 0
    c_dir, u_dir = str(tmp / ("c_" + coder)), str(tmp / ("u_" + coder))
    code, text = _tezip(["-c", mdir, ddir, c_dir] + LATTICE + ["--sdelta", "plane", "--coder", coder, "--key-coder", "huff"])
    assert code == 0 and LINE in text, text
    assert _trailer(c_dir) == (8, NT, 64, 64, 3)
    assert _tezip(["-u", mdir, c_dir, u_dir])[0] == 0
    _same_images(u_dir, flat_u, names)


def test_cli_shuffle_and_sidecar_contradiction(jobs, monkeypatch):
    tmp, sets = jobs
    mdir, ddir, names = sets["colour"]
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("TEZIP_NO_STREAMING", raising=False)
    c_flat, c_plane, u_flat, u_plane = (str(tmp / k) for k in ("shf_c", "shp_c", "shf_u", "shp_u"))
    assert _tezip(["-c", mdir, ddir, c_flat] + LATTICE + ["--shuffle"])[0] == 0
    code, text = _tezip(["-c", mdir, ddir, c_plane] + LATTICE + ["--shuffle", "--sdelta", "plane"])
    assert code == 0 and LINE in text, text
    assert _trailer(c_plane) == (9, NT, 64, 64, 3) and _trailer(c_flat) == (2, NT, 64, 64, 3)
    assert _tezip(["-u", mdir, c_flat, u_flat])[0] == 0
    assert _tezip(["-u", mdir, c_plane, u_plane])[0] == 0
    _same_images(u_plane, u_flat, names)
    # a sidecar that contradicts the trailer belongs to another stream
    doc = json.loads(_read(c_plane, "tezip_amd.json"))
    doc["sdelta"] = "channel"
    with open(os.path.join(c_plane, "tezip_amd.json"), "w") as f:
        json.dump(doc, f)
    with pytest.raises(ValueError, match="spatial delta"):
        _tezip(["-u", mdir, c_plane, str(tmp / "never")])


def test_cli_gray_job_marks_its_one_channel_stream(jobs, monkeypatch):
    tmp, sets = jobs
    mdir, ddir, names = sets["gray"]
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("TEZIP_NO_STREAMING", raising=False)
    c_gray, c_plane, u_gray, u_plane = (str(tmp / k) for k in ("g_c", "gp_c", "g_u", "gp_u"))
    assert _tezip(["-c", mdir, ddir, c_gray] + LOSSLESS + ["--gray"])[0] == 0
    code, text = _tezip(["-c", mdir, ddir, c_plane] + LOSSLESS + ["--gray", "--sdelta", "plane"])
    assert code == 0 and LINE in text and "gray: yes" in text, text
    assert _trailer(c_plane) == (8, NT, 64, 64, 1) and _trailer(c_gray) == (1, NT, 64, 64, 1)
    assert _read(c_plane, "key_frame.dat") == _read(c_gray, "key_frame.dat")
    assert _tezip(["-u", mdir, c_gray, u_gray])[0] == 0
    assert _tezip(["-u", mdir, c_plane, u_plane])[0] == 0
    _same_images(u_plane, u_gray, names)
