"""The one-channel payload of a gray job (`-c --gray`, tz_set_payload_channels(1)) on the GPU: k_sdelta_gray and k_recon_gray*
give the numpy statement (tezip_amd/graypayload.py) bit for bit, tz_encode under one channel gives the payload and table
that statement makes of the three-channel encode's own delta stack (a path the parity tests pin to the oracle), the decoder
restores channel 0 of what the three-channel decoder restores in all three channels, and the command line round-trips."""
import contextlib
import io
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NBINS = 2111
SIZES = [(1, 1), (5, 7), (61, 45), (64, 64), (3, 300)]   # 35 pixels: no whole group of 8; 2745: odd, off every boundary;
NF = 3                                                    # 4096: flat path, whole groups; 3 x 300: several workgroups of columns


@pytest.fixture(scope="module")
def ctx():
    from tezip_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def gp():
    from tezip_amd import graypayload
    return graypayload


def pad8(v):
    return (v + 7) // 8 * 8


# ------------------------------------------------------------------------------------------------------ k_sdelta_gray
def _delta_stacks(h, w, seed):
    """Two (NF, h, w, 3) int16 stacks in [-255, 255]: one with three equal channels, one whose channels 1 and 2 hold other
    values, which must not matter."""
    rng = np.random.default_rng(seed)
    d0 = rng.integers(-255, 256, (NF, h, w), dtype=np.int16)
    d0.reshape(-1)[[0, -1]] = [255, -255]
    eq = np.repeat(d0[..., None], 3, axis=-1)
    other = eq.copy()
    other[..., 1:] = rng.integers(-255, 256, (NF, h, w, 2), dtype=np.int16)
    return eq, other


def _want_sdelta(gp, d3, carry, offset):
    sd = gp.spatial_delta(np.ascontiguousarray(d3[..., 0]), carry)
    y = (1600 - sd.astype(np.int64)).astype(np.int16) if offset else sd
    inside = y[(y >= 0) & (y < NBINS)].astype(np.int64)      # what the library counts (as tz_spatial_delta)
    return y, np.bincount(inside, minlength=NBINS).astype(np.uint64)


@pytest.mark.parametrize("h,w", SIZES)
def test_spatial_delta_gray_is_the_numpy_function(ctx, gp, h, w):
    for d3 in _delta_stacks(h, w, 100 * h + w):
        for carry in (None, -77):
            for offset in (0, 1):
                want, counts = _want_sdelta(gp, d3, carry, offset)
                got = ctx.spatial_delta_gray(d3, offset, carry=carry)
                assert got.size == NF * h * w
                np.testing.assert_array_equal(got, want, "carry %r offset %d" % (carry, offset))
                hist = np.full(NBINS, 3, np.uint64)             # the counts are ADDED
                got = ctx.spatial_delta_gray(d3, offset, carry=carry, hist=hist)
                np.testing.assert_array_equal(got, want)
                np.testing.assert_array_equal(hist - np.uint64(3), counts, "histogram, carry %r offset %d" % (carry, offset))
                if offset:
                    assert int(counts.sum()) == want.size


def test_spatial_delta_gray_far_symbols_and_wrap(ctx, gp):
    """Values outside the encoder's range: the int16 wrap-around of finding_difference, symbols far from the centre of the
    histogram and outside its bins."""
    rng = np.random.default_rng(8)
    d3 = rng.integers(-32768, 32768, (2, 33, 41, 3), dtype=np.int16)
    d3[0, :8] = rng.integers(-300, 301, (8, 41, 3))
    for offset in (0, 1):
        want, counts = _want_sdelta(gp, d3, None, offset)
        hist = np.zeros(NBINS, np.uint64)
        np.testing.assert_array_equal(ctx.spatial_delta_gray(d3, offset, hist=hist), want)
        np.testing.assert_array_equal(hist, counts)


# (input shift, output shift) in int16 elements: every shift of the issue on both buffers, and two pairs at which a scalar
# head of 1 resp. 5 pixels brings BOTH buffers onto a 16-byte boundary, so that head, vector groups and tail all run
SHIFTS = [(0, 0), (1, 1), (2, 2), (3, 3), (5, 5), (5, 7), (1, 3)]


@pytest.mark.parametrize("h,w", [(61, 45), (64, 64)])
def test_spatial_delta_gray_device_buffers_off_alignment(ctx, gp, h, w):
    import torch
    d3 = _delta_stacks(h, w, 5)[1]
    n1, n3 = NF * h * w, NF * h * w * 3
    for hist_on in (False, True):
        want, counts = _want_sdelta(gp, d3, 9, 1)
        for s_in, s_out in SHIFTS:
            src = torch.zeros(n3 + 64, dtype=torch.int16, device="cuda")
            src[s_in: s_in + n3].copy_(torch.from_numpy(d3.reshape(-1)))
            out = torch.full((n1 + 64,), 0x5A5A, dtype=torch.int16, device="cuda")
            hist = torch.zeros(NBINS, dtype=torch.int64, device="cuda") if hist_on else None
            torch.cuda.synchronize()
            ctx.spatial_delta_gray(src[s_in: s_in + n3], 1, carry=9, hist=hist, out=out[s_out: s_out + n1])
            ctx.synchronize()
            o = out.cpu().numpy()
            assert (o[s_out: s_out + n1] == want).all(), (s_in, s_out)
            assert (o[:s_out] == 0x5A5A).all() and (o[s_out + n1:] == 0x5A5A).all(), "guard elements written at %r" % ((s_in, s_out),)
            if hist_on:
                np.testing.assert_array_equal(hist.cpu().numpy().astype(np.uint64), counts)


# ----------------------------------------------------------------------------------------------------- k_recon_gray*
def _recon_case(h, w, seed):
    rng = np.random.default_rng(seed)
    hp, wp = pad8(h), pad8(w)
    pred = rng.random((NF, hp, wp, 3), dtype=np.float32)
    pred.reshape(-1)[rng.integers(0, pred.size, 16)] = 1.0
    key = rng.integers(0, 256, (NF, h, w, 3), dtype=np.uint8)         # channels 1 and 2 of the key stack are never read
    d = rng.integers(-255, 256, (NF, h, w), dtype=np.int16)
    flat = d.reshape(-1)
    flat[::7] = 300                                                     # below 0 whatever the base
    flat[3::11] = -300                                                  # above 255 whatever the base
    return pred, key, d


def _want_recon(gp, pred, key, mask, d):
    h, w = d.shape[1:]
    base_pred = (pred[:, :h, :w, 0] * np.float32(255.0)).astype(np.int64)   # trunc(f32(pred * 255)), as k_recon
    base = np.where(np.asarray(mask, bool)[:, None, None], key[..., 0].astype(np.int64), base_pred)
    return gp.reconstruct(base, d)


@pytest.mark.parametrize("h,w", SIZES)
def test_reconstruct_gray_is_the_numpy_function(ctx, gp, h, w):
    pred, key, d = _recon_case(h, w, 7 * h + w)
    for mask in ([1, 0, 0], [0, 1, 0], [1, 1, 1]):
        want = _want_recon(gp, pred, key, mask, d)
        assert want.min() == 0 and (want.max() == 255 or h * w < 4), "the deltas drive the clamp at both ends"
        got = ctx.reconstruct_gray(pred, key, mask, d)
        assert got.shape == (NF, h, w, 3)
        np.testing.assert_array_equal(got, want, "mask %r" % (mask,))
        assert (got[..., 0] == got[..., 1]).all() and (got[..., 1] == got[..., 2]).all()


@pytest.mark.parametrize("h,w", [(61, 45), (64, 64)])      # the general form (61 x 45 inside 64 x 48) and the flat form
def test_reconstruct_gray_device_buffers_off_alignment(ctx, gp, h, w):
    import torch
    pred, key, d = _recon_case(h, w, 31)
    mask = [0, 1, 0]
    want = _want_recon(gp, pred, key, mask, d).reshape(-1)
    n1, n3 = d.size, d.size * 3
    for s in (0, 1, 2, 3, 5):
        t_pred = torch.zeros(pred.size + 16, dtype=torch.float32, device="cuda")
        t_pred[s: s + pred.size].copy_(torch.from_numpy(pred.reshape(-1)))
        t_key = torch.zeros(n3 + 16, dtype=torch.uint8, device="cuda")
        t_key[s: s + n3].copy_(torch.from_numpy(key.reshape(-1)))
        t_d = torch.zeros(n1 + 16, dtype=torch.int16, device="cuda")
        t_d[s: s + n1].copy_(torch.from_numpy(d.reshape(-1)))
        out = torch.full((n3 + 64,), 0x5A, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ctx.reconstruct_gray(t_pred[s: s + pred.size], t_key[s: s + n3], mask, t_d[s: s + n1].view(NF, h, w), out=out[s: s + n3])
        ctx.synchronize()
        o = out.cpu().numpy()
        assert (o[s: s + n3] == want).all(), s
        assert (o[:s] == 0x5A).all() and (o[s + n3:] == 0x5A).all(), "guard bytes written at shift %d" % s


# ------------------------------------------------------------------------------------------- encode / decode on a rollout
NT, WINDOW = 12, 4
BOUNDS = [("abs", [0.0]), ("abs", [2.0]), ("rel", [0.01]), ("pwrel", [0.01])]


def _model():
    from tezip_amd.prednet import PredNetConfig
    cfg = PredNetConfig(stack_sizes=(3, 16, 32))
    return cfg, cfg.init_weights(seed=4, bias_scale=0.2)


def _job_frames(crop):
    from tezip_amd import synth
    frames = synth.moving_blobs(NT, 64, 64)
    return np.ascontiguousarray(frames[:, :61, :45]) if crop else frames


def _recon_mask(key, warm_up):
    """The frames the decoder reconstructs from their key bytes (decompress.py:138-186): frame 0 and every key frame from
    the warm_up-th on."""
    r = np.zeros(len(key), bool)
    k = 0
    for i, is_key in enumerate(key):
        if is_key:
            r[i] = k >= warm_up
            k += 1
    r[0] = True
    return r


@pytest.mark.parametrize("warm_up", [0, 1])
@pytest.mark.parametrize("crop", [False, True], ids=["64x64", "61x45"])
def test_encode_and_decode_on_a_rollout(gp, crop, warm_up, monkeypatch):
    from tezip_amd import _lib
    cfg, wts = _model()
    frames = _job_frames(crop)
    nt, h, w = frames.shape[:3]
    assert gp.is_gray(frames)
    n1 = nt * h * w

    def context():
        c = _lib.Context(0)
        c.load_model(cfg, wts)
        c.prepare(pad8(h), pad8(w), 4)
        return c

    ctx = context()
    try:
        key = ctx.rollout(frames, warm_up, WINDOW)[0]
        assert all(frames[i].any() for i in np.nonzero(key)[0]), "key discovery needs a non-zero sample in every key frame"
        pred = ctx.get_predictions()
        base_pred = (pred[:, :h, :w, 0] * np.float32(255.0)).astype(np.int64)
        base0 = np.where(_recon_mask(key, warm_up)[:, None, None], frames[..., 0].astype(np.int64), base_pred)
        runs = []
        for mode, bound in BOUNDS:
            assert ctx.get_payload_channels() == 3
            _, _, delta3 = ctx.encode(mode, bound, True, want_delta=True)   # (the predictions, and so the deltas, differ per channel)
            ctx.set_payload_channels(1)
            assert ctx.get_payload_channels() == 1
            for entropy in (True, False):
                payload, table, _ = ctx.encode(mode, bound, entropy)
                want_payload, want_table = gp.payload_from_delta(delta3, entropy)
                assert payload.size == n1
                np.testing.assert_array_equal(payload, want_payload, "%s %r entropy %r" % (mode, bound, entropy))
                if entropy:
                    np.testing.assert_array_equal(table, want_table)
                else:
                    assert table is None
            payload, table, _ = ctx.encode(mode, bound, True)
            # the resident form is the same payload, in pieces
            ctx.encode(mode, bound, True, payload="resident")
            np.testing.assert_array_equal(np.concatenate([ctx.payload_get(0, 5), ctx.payload_get(5, n1 - 5)]), payload)
            q = ctx.encode_quality("resident", table)
            q2 = ctx.encode_quality(payload, table)
            assert q.tolist() == q2.tolist()
            dec_dig = ctx.encode_digests(payload, table)[0]
            want = gp.reconstruct(base0, delta3[..., 0])
            np.testing.assert_array_equal(dec_dig, ctx.frame_digests(want))
            if n1 % 8 == 0:                               # the shuffle bit: the byte planes of the same payload
                planes, t2, _ = ctx.encode(mode, bound, True, shuffle=True)
                np.testing.assert_array_equal(ctx.byte_unshuffle(planes.view(np.uint8)), payload)
                assert ctx.encode_quality(planes, t2, shuffle=True).tolist() == q.tolist()
            if mode == "abs":
                assert int(q["max_abs"].max()) <= int(bound[0]), "abs %r: max_abs per frame %r" % (bound, q["max_abs"].tolist())
                runs.append((bound, payload, table, want))
            ctx.set_payload_channels(3)
        # ---- the decoder
        key_stack = np.where(key[:, None, None, None], frames, 0).astype(np.uint8)
        ctx.set_payload_channels(1)
        ctx.rollout_decode(key_stack, warm_up)
        wholes = []
        for bound, payload, table, want in runs:
            got = ctx.decode(payload, table)
            assert got.shape == (nt, h, w, 3)
            np.testing.assert_array_equal(got, want, "decode at abs %r" % (bound,))
            assert gp.is_gray(got)
            if bound[0] == 0:
                np.testing.assert_array_equal(got, frames)
            else:
                assert int(np.abs(got.astype(int) - frames.astype(int)).max()) <= 2
            wholes.append(got.copy())
            with pytest.raises(ValueError):
                ctx.decode(np.zeros(n1 * 3, np.int16), table)
        for first, count in ((5, 4), (11, 1)):          # [5, 9) crosses a window boundary
            ctx.rollout_decode_range(key_stack, warm_up, first, count)
            for (bound, payload, table, want), whole in zip(runs, wholes):
                assert ctx.undelta_carry(payload, first * h * w, table) == _decoded_element(payload, table, first * h * w - 1)
                np.testing.assert_array_equal(ctx.decode_range(payload, table, first, count), whole[first: first + count])
    finally:
        ctx.close()
    monkeypatch.setenv("TEZIP_DECODE_UNFUSED", "1")
    c2 = context()
    try:
        c2.set_payload_channels(1)
        c2.rollout_decode(key_stack, warm_up)
        for (bound, payload, table, want), whole in zip(runs, wholes):
            np.testing.assert_array_equal(c2.decode(payload, table), whole)
    finally:
        c2.close()


def _decoded_element(payload, table, i):
    """Element i of the delta stream the payload decodes to: the inverse remap, 1600 - x, and the inverse of
    finding_difference (x[i] = s[0] - sum(s[1..i]) mod 2^16)."""
    sym = np.asarray(table, np.int64)[np.asarray(payload, np.int64)]
    s = 1600 - sym
    v = int(s[0]) - int(s[1: i + 1].sum())
    return (v + 32768) % 65536 - 32768


def test_refusals(gp):
    from tezip_amd import _lib
    cfg, wts = _model()
    frames = _job_frames(False).copy()
    ctx = _lib.Context(0)
    try:
        ctx.load_model(cfg, wts)
        ctx.prepare(64, 64, 4)
        with pytest.raises(_lib.TezipError) as e:
            ctx.set_payload_channels(2)
        assert e.value.status == -1 and ctx.get_payload_channels() == 3
        ctx.rollout(frames, 0, WINDOW)
        ctx.set_payload_channels(1)
        ctx.encode("abs", [2.0], True)                                   # gray: served
        with pytest.raises(_lib.TezipError) as e:
            ctx.encode("abs", [2.0], True, want_delta=True)
        assert e.value.status == -1 and "delta_out" in str(e.value)
        for call, name in ((lambda: ctx.encode_begin("abs", [2.0], True), "tz_encode_begin"),
                           (lambda: ctx.encode_finish(None, None), "tz_encode_finish"),
                           (lambda: ctx.encode_delta("abs", [2.0]), "tz_encode_delta"),
                           (lambda: ctx.decode_delta(np.zeros(frames.shape, np.int16)), "tz_decode_delta")):
            with pytest.raises(_lib.TezipError) as e:
                call()
            assert e.value.status == -6 and name in str(e.value), name
        frames[NT - 1, 63, 63, 2] ^= 1                                   # one colour sample, last pixel of the last frame
        assert not gp.is_gray(frames)
        ctx.rollout(frames, 0, WINDOW)
        with pytest.raises(_lib.TezipError) as e:
            ctx.encode("abs", [2.0], True)
        assert e.value.status == -1 and "frame %d " % (NT - 1) in str(e.value)
        ctx.set_payload_channels(3)
        payload, _, _ = ctx.encode("abs", [2.0], True)                   # three channels: served as ever
        assert payload.size == frames.size
    finally:
        ctx.close()


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


BASE = ["-p", "0", "-w", "4", "-m", "abs", "-b", "0"]


@pytest.fixture(scope="module")
def jobs(tmp_path_factory):
    """Image directory and model of the gray job (64 x 64) and of the colour job (61 x 90), and what a plain lossless
    `-c` / `-u` of the gray job writes."""
    from PIL import Image
    from tezip_amd import _lib, synth, weights
    tmp = tmp_path_factory.mktemp("gray")
    cfg, wts = _model()
    out = {}
    for name, frames in (("gray", synth.moving_blobs(NT, 64, 64)), ("colour", synth.translating_scene(NT, 61, 90))):
        mdir, ddir = str(tmp / (name + "_model")), tmp / (name + "_data")
        weights.save_model(mdir, cfg, wts, _lib.pad8(frames.shape[1]), _lib.pad8(frames.shape[2]))
        ddir.mkdir()
        names = ["f_%03d.png" % t for t in range(NT)]
        for t, f in enumerate(frames):
            Image.fromarray(f).save(ddir / names[t])
        out[name] = (mdir, str(ddir), names, frames)
    os.environ.pop("WORLD_SIZE", None)
    mdir, ddir, names, frames = out["gray"]
    plain_c, plain_u = str(tmp / "plain_c"), str(tmp / "plain_u")
    code, text = _tezip(["-c", mdir, ddir, plain_c] + BASE)
    assert code == 0 and "gray:" not in text, text
    code, text = _tezip(["-u", mdir, plain_c, plain_u])
    assert code == 0, text
    return tmp, out, plain_c, plain_u


def _trailer(path):
    """(shape5, warm_up, payload elements) of an entropy.dat of any coder."""
    from tezip_amd import decompress, zstd
    data = _read(path, "entropy.dat")
    fmt = decompress.coded_format(data[:4])
    if fmt is not None:
        p = fmt.parse(np.frombuffer(data, np.uint8))
        return p.shape, p.warm_up, p.n
    payload, _, shape, warm_up = decompress.parse_stream(zstd.decompress(data))
    return shape, warm_up, payload.size


@pytest.mark.parametrize("extra", [["--coder", "zstd"], ["--coder", "huff"], ["--coder", "huffr"], ["--key-coder", "huffg"], ["--shuffle"]],
                         ids=["zstd", "huff", "huffr", "huffg", "shuffle"])
def test_cli_round_trip_of_a_gray_job(jobs, monkeypatch, extra):
    tmp, sets, plain_c, plain_u = jobs
    mdir, ddir, names, frames = sets["gray"]
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("TEZIP_NO_STREAMING", raising=False)
    tag = extra[-1].strip("-")
    comp, whole, part, slow = (str(tmp / ("%s_%s" % (k, tag))) for k in ("c", "u", "r", "s"))
    code, text = _tezip(["-c", mdir, ddir, comp] + BASE + ["--gray", "--digests"] + extra)
    assert code == 0 and "gray: yes, payload stores 1 of 3 channels" in text, text
    shape, warm_up, n = _trailer(comp)
    assert tuple(shape[1:]) == (NT, 64, 64, 1) and warm_up == 0 and n == NT * 64 * 64
    assert shape[0] == (2 if extra == ["--shuffle"] else 1)
    assert json.loads(_read(comp, "tezip_amd.json"))["payload_channels"] == 1
    assert _read(comp, "filename.txt") == _read(plain_c, "filename.txt")
    if "--key-coder" not in extra:
        assert _read(comp, "key_frame.dat") == _read(plain_c, "key_frame.dat")
    print("%s: entropy.dat %d bytes with --gray, %d bytes three-channel zstd" % (tag, len(_read(comp, "entropy.dat")), len(_read(plain_c, "entropy.dat"))))
    code, text = _tezip(["-u", mdir, comp, whole, "--verify", "require"])
    assert code == 0 and "verified: %d frames" % NT in text, text
    assert sorted(os.listdir(whole)) == names
    for nm in names:
        assert _read(whole, nm) == _read(plain_u, nm), nm
    code, text = _tezip(["-u", mdir, comp, part, "--frames", "5:9", "--verify", "require"])
    assert code == 0, text
    assert sorted(os.listdir(part)) == names[5:9]
    for nm in names[5:9]:
        assert _read(part, nm) == _read(whole, nm), nm
    monkeypatch.setenv("TEZIP_NO_STREAMING", "1")                      # the whole-array path of -u
    code, text = _tezip(["-u", mdir, comp, slow, "--verify", "require"])
    assert code == 0 and "verified: %d frames" % NT in text, text
    for nm in names:
        assert _read(slow, nm) == _read(plain_u, nm), nm


def test_cli_lossy_gray_job_keeps_its_bound_and_decodes_gray(jobs, monkeypatch):
    from PIL import Image
    tmp, sets, _, _ = jobs
    mdir, ddir, names, frames = sets["gray"]
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("TEZIP_NO_STREAMING", raising=False)
    comp, three, out, out3 = (str(tmp / k) for k in ("lossy_c", "lossy_c3", "lossy_u", "lossy_u3"))
    # (the three-channel job quantises each channel's own deltas: its images need not be gray; channel 0 is the same chain)
    lossy = ["-p", "0", "-w", "4", "-m", "abs", "-b", "2"]
    code, text = _tezip(["-c", mdir, ddir, comp] + lossy + ["--gray", "--report"])
    assert code == 0 and "gray: yes" in text, text
    assert json.loads(_read(comp, "quality.json"))["max_abs_err"] <= 2
    code, text = _tezip(["-c", mdir, ddir, three] + lossy)
    assert code == 0, text
    for src, dst in ((comp, out), (three, out3)):
        code, text = _tezip(["-u", mdir, src, dst])
        assert code == 0, text
    for t, nm in enumerate(names):
        got = np.asarray(Image.open(os.path.join(out, nm)))
        assert (got[..., 0] == got[..., 1]).all() and (got[..., 1] == got[..., 2]).all(), nm
        assert int(np.abs(got.astype(int) - frames[t].astype(int)).max()) <= 2, nm
        got3 = np.asarray(Image.open(os.path.join(out3, nm)))
        assert (got[..., 0] == got3[..., 0]).all(), "channel 0 is what the three-channel job decodes to: %s" % nm


def test_cli_colour_job_writes_what_it_writes_without_the_flag(jobs, monkeypatch):
    tmp, sets, _, _ = jobs
    mdir, ddir, names, frames = sets["colour"]
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with_flag, without = str(tmp / "colour_gray"), str(tmp / "colour_plain")
    code, text = _tezip(["-c", mdir, ddir, with_flag] + BASE + ["--gray"])
    assert code == 0 and "gray: no (frame 0 f_000.png has colour), payload keeps three channels" in text, text
    code, text = _tezip(["-c", mdir, ddir, without] + BASE)
    assert code == 0 and "gray:" not in text, text
    assert sorted(os.listdir(with_flag)) == sorted(os.listdir(without))
    for n in ("entropy.dat", "key_frame.dat", "filename.txt", "tezip_amd.json"):
        assert _read(with_flag, n) == _read(without, n), n
    assert "payload_channels" not in json.loads(_read(with_flag, "tezip_amd.json"))
    assert _trailer(with_flag)[0][4] == 3
