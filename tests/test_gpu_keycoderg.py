"""The key-frame coder that stores a gray key frame once (`--key-coder huffg`, format TZK2) on the GPU: k_key_gray gives the
numpy flag exactly, k_keyg_resid / k_keyg_unresid_* the numpy residuals and their inverses bit for bit, compress.run the
bytes of keycoderg.encode_file, and `-c --key-coder huffg --digests` then `-u --verify require` the images of a
`--key-coder zstd` job (tezip_amd/keycoderg.py is the specification).  No test feeds a kernel a corrupted body: the
container's validation and the decoder's low-byte rule are tested on the CPU (tests/test_keycoderg.py)."""
import contextlib
import io
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from tezip_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def gray_stack(k, h, w, seed):
    rng = np.random.default_rng(seed)
    g = (np.cumsum(rng.integers(-3, 4, (k, h, w)), axis=2) + np.cumsum(rng.integers(-2, 3, (k, h, 1)), axis=1) + 90) & 255
    return np.repeat(g.astype(np.uint8)[..., None], 3, axis=-1)


def colour_stack(k, h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (k, h, w, 3), dtype=np.uint8)


def _resident(ctx, stack):
    ctx.frames_begin(*stack.shape[:3])
    ctx.frames_put(0, stack)


# ------------------------------------------------------------------------------------------------------------ k_key_gray
@pytest.mark.parametrize("h,w", [(61, 90), (5, 7), (1, 1), (64, 64)])
def test_gray_flag_on_one_sample_cases(ctx, h, w):
    """Frame bytes 16 470 and 105 are no multiple of 16 or 48; the stack holds three frames of which 1 and 2 are the key
    frames, so both start off a 16-byte boundary (and at different phases of the 48-byte groups)."""
    from tezip_amd import keycoderg
    g = gray_stack(3, h, w, h * 100 + w)
    g[0] = colour_stack(1, h, w, 1)[0]                                  # (not a key frame: must not matter)
    keys = [1, 2]
    _resident(ctx, g)
    assert ctx.keys_gray(keys).tolist() == [True, True]
    assert ctx.keys_gray([0, 1, 2]).tolist() == keycoderg.gray_flags(g).tolist()
    cases = [("channel 1 of pixel 0", 0, 1), ("channel 2 of the last pixel", h * w - 1, 2), ("a pixel in the middle", (h * w) // 2, 0)]
    for frame in (1, 2):
        for name, px, ch in cases:
            x = g.copy()
            x[frame].reshape(h * w, 3)[px, ch] ^= 0x80
            _resident(ctx, x)
            want = keycoderg.gray_flags(x[keys])
            assert want.tolist() == [frame != 1, frame != 2]
            assert ctx.keys_gray(keys).tolist() == want.tolist(), "%s of key frame %d at %dx%d" % (name, frame, h, w)


def test_gray_flag_at_every_sample_of_a_small_frame(ctx):
    """5 x 7: each of the 105 samples of the second key frame changed alone -- every position relative to the 16-byte head,
    the 48-byte groups and the tail -- and a change that keeps two of the three channels equal."""
    h, w = 5, 7
    g = gray_stack(3, h, w, 11)
    for i in range(h * w * 3):
        x = g.copy()
        x[2].reshape(-1)[i] += 1
        _resident(ctx, x)
        assert ctx.keys_gray([0, 2]).tolist() == [True, False], "sample %d" % i
    x = g.copy()
    x[2, 4, 6, :2] += 1                                                  # channels 0 and 1 equal, channel 2 differs
    _resident(ctx, x)
    assert ctx.keys_gray([1, 2]).tolist() == [True, False]


# --------------------------------------------------------------------------------------- k_keyg_resid / k_keyg_unresid_*
@pytest.mark.parametrize("h,w", [(5, 7), (64, 64), (1, 1), (61, 90), (3, 300)])
def test_unresidual_buf_is_the_numpy_function(ctx, h, w):
    """Each of the 8 pred bytes alone, and stacks that mix them so that the frames' offsets differ.  3 x 300 has more than
    one workgroup of columns and a row of more than four 64-column steps; the symbols' high bytes must not count."""
    from tezip_amd import keycoderg
    rng = np.random.default_rng(h * 31 + w)
    for preds in [[p] for p in range(8)] + [[7, 3, 5], [0, 4, 6, 2], [6, 7, 1]]:
        n = int(keycoderg.frame_symbols([p & 4 for p in preds], h, w).sum())
        sym = rng.integers(0, 256, n).astype(np.int16)
        sym[::5] |= np.int16(0x4100)
        off, _ = keycoderg.offsets([p & 4 for p in preds], h, w)
        cnt = keycoderg.frame_symbols([p & 4 for p in preds], h, w)
        want = np.stack([keycoderg.unresidual(sym[int(o): int(o) + int(c)], p, h, w) for o, c, p in zip(off, cnt, preds)])
        got = ctx.keysg_unresidual_buf(sym, preds, h, w)
        assert got.shape == want.shape and (got == want).all(), "inverse %r at %dx%d" % (preds, h, w)


@pytest.mark.parametrize("h,w", [(5, 7), (64, 64), (1, 1), (61, 90)])
def test_residual_buf_is_the_numpy_function(ctx, h, w):
    from tezip_amd import keycoderg
    frames = gray_stack(4, h, w, h + 3 * w)
    frames[1] = colour_stack(1, h, w, 2)[0]
    frames[3] = colour_stack(1, h, w, 3)[0]
    for preds in ([4, 0, 5, 1], [7, 3, 6, 2], [5, 1, 7, 3], [6, 2, 4, 0]):
        want = keycoderg.symbols(frames, preds)
        got = ctx.keysg_residual_buf(frames, preds)
        assert got.dtype == np.int16 and got.shape == want.shape and (got == want).all(), "residuals %r at %dx%d" % (preds, h, w)
        assert (ctx.keysg_unresidual_buf(got, preds, h, w) == frames).all(), "round trip %r at %dx%d" % (preds, h, w)


def test_device_buffers_off_alignment(ctx):
    """The replicated store goes out as aligned dwords: every alignment of the frames' address, nothing written outside."""
    import torch
    from tezip_amd import keycoderg
    h, w, preds = 5, 71, [7, 1, 5]
    frames = gray_stack(3, h, w, 9)
    frames[1] = colour_stack(1, h, w, 9)[0]
    sym_np = keycoderg.symbols(frames, preds)
    n = frames.size
    for shift in (0, 1, 2, 3, 5):
        sym = torch.zeros(sym_np.size + 16, dtype=torch.int16, device="cuda")
        sym[1: 1 + sym_np.size].copy_(torch.from_numpy(sym_np))
        out = torch.full((n + 64,), 0x5A, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ctx.keysg_unresidual_buf(sym[1: 1 + sym_np.size], preds, h, w, out=out[shift: shift + n])
        torch.cuda.synchronize()
        o = out.cpu().numpy()
        assert (o[shift: shift + n] == frames.reshape(-1)).all(), shift
        assert (o[:shift] == 0x5A).all() and (o[shift + n:] == 0x5A).all(), shift


def _file_from_context(ctx, stack, keys):
    """compress.run's steps on a resident stack -> the TZK2 file."""
    from tezip_amd import huff, keycoderg
    nt, h, w = stack.shape[:3]
    gray = ctx.keys_gray(keys)
    counts = keycoderg.gray_counts(ctx.keys_counts(keys), gray)
    predg = keycoderg.pred_bytes(counts, gray)
    lengths = huff.code_lengths(keycoderg.chosen_counts(counts, predg))
    nbytes = ctx.keysg_encode(keys, predg, lengths)
    body = np.concatenate([ctx.keysg_get(0, 100), ctx.keysg_get(100, nbytes - 100)])
    n = keycoderg.offsets(gray, h, w)[1]
    return keycoderg.pack_front(nt, h, w, keys, predg, lengths, huff.geometry(n)[1], (nbytes - huff.body_bytes(n, 0)) // 4) + body.tobytes()


def test_resident_forms_match_numpy_and_refuse_the_other_format(ctx):
    from tezip_amd import _lib, keycoder, keycoderg
    stack = gray_stack(7, 21, 30, 3)
    stack[4] = colour_stack(1, 21, 30, 4)[0]
    stack[6, 20, 29, 2] ^= 1
    keys = [0, 1, 4, 6]
    _resident(ctx, stack)
    data = _file_from_context(ctx, stack, keys)
    assert data == keycoderg.encode_file(stack, keys, 7), "the GPU file differs from the numpy encoder's"
    p = keycoderg.parse(data)
    assert p.gray.tolist() == [True, True, False, False]
    want = np.zeros_like(stack)
    want[keys] = stack[keys]
    b = np.ascontiguousarray(p.body)
    for cuts in ([b.size], [7, b.size // 2 + 1, b.size]):
        ctx.keysg_begin(b.size, p.nt, p.H, p.W, p.idx, p.pred, p.lengths)
        lo = 0
        for hi in cuts:
            ctx.keysg_put(lo, b[lo:hi])
            lo = hi
        ctx.keysg_decode()
        assert (ctx.frames_get(0, 7) == want).all(), "decoded stack, pieces %r" % (cuts,)

    def refused(status, call):
        with pytest.raises(_lib.TezipError) as e:
            call()
        assert e.value.status == status

    # a body staged for one format is refused by the other's put and decode, and stays usable by its own
    ctx.keysg_begin(b.size, p.nt, p.H, p.W, p.idx, p.pred, p.lengths)
    refused(-1, lambda: ctx.keys_put(0, b))
    refused(-4, ctx.keys_decode)
    ctx.keysg_put(0, b)
    refused(-4, ctx.keys_decode)
    ctx.keysg_decode()
    assert (ctx.frames_get(0, 7) == want).all()
    p1 = keycoder.parse(keycoder.encode_file(stack, keys, 7))
    b1 = np.ascontiguousarray(p1.body)
    ctx.keys_begin(b1.size, p1.nt, p1.H, p1.W, p1.idx, p1.pred, p1.lengths)
    refused(-1, lambda: ctx.keysg_put(0, b1))
    refused(-4, ctx.keysg_decode)
    ctx.keys_put(0, b1)
    refused(-4, ctx.keysg_decode)
    ctx.keys_decode()
    assert (ctx.frames_get(0, 7) == want).all()
    refused(-1, lambda: ctx.keysg_begin(b.size, p.nt, p.H, p.W, p.idx, [8, 0, 0, 0], p.lengths))    # a pred byte above 7
    refused(-1, lambda: ctx.keysg_begin(b.size, p.nt, p.H, p.W, [0, 4, 1, 6], p.pred, p.lengths))   # indices not ascending
    _resident(ctx, stack)
    refused(-1, lambda: ctx.keysg_encode(keys, [0, 1, 9, 2], p.lengths))
    refused(-1, lambda: ctx.keys_gray([3, 3]))


# ------------------------------------------------------------------------------------------- compress.run / decompress.run
NT = 12


def _job_frames(name):
    from tezip_amd import synth
    if name == "gray":
        return synth.moving_blobs(NT, 64, 64)
    if name == "colour":
        return synth.translating_scene(NT, 61, 90)
    frames = synth.moving_blobs(NT, 64, 64)
    frames[4, 40, 23, 1] += 1                                            # frame 4 is a key frame of -p 0 -w 4; one sample
    return frames


@pytest.fixture(scope="module")
def jobs(tmp_path_factory):
    """The three jobs of the format: all key frames gray, none gray, mixed -- image directory and model of each."""
    from PIL import Image
    from tezip_amd import _lib, weights
    from tezip_amd.prednet import PredNetConfig
    tmp = tmp_path_factory.mktemp("keycoderg")
    cfg = PredNetConfig(stack_sizes=(3, 16, 32))
    wts = cfg.init_weights(seed=4, bias_scale=0.2)
    out = {}
    for name in ("gray", "colour", "mixed"):
        frames = _job_frames(name)
        mdir, ddir = str(tmp / (name + "_model")), tmp / (name + "_data")
        weights.save_model(mdir, cfg, wts, _lib.pad8(frames.shape[1]), _lib.pad8(frames.shape[2]))
        ddir.mkdir()
        names = ["f_%03d.png" % t for t in range(NT)]
        for t, f in enumerate(frames):
            Image.fromarray(f).save(ddir / names[t])
        out[name] = (mdir, str(ddir), names, frames)
    return tmp, out


def _read(d, n):
    with open(os.path.join(d, n), "rb") as f:
        return f.read()


WANT_GRAY = {"gray": [True, True, True], "colour": [False, False, False], "mixed": [True, False, True]}


@pytest.mark.parametrize("name", ["gray", "colour", "mixed"])
def test_compress_run_writes_the_numpy_encoders_file(jobs, monkeypatch, name):
    from tezip_amd import compress, keycoderg
    tmp, sets = jobs
    mdir, ddir, names, frames = sets[name]
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    out = str(tmp / ("run_" + name))
    compress.run(mdir, ddir, out, 0, 4, None, "abs", [2.0], True, False, True, KEY_CODER="huffg")
    kk = _read(out, "key_frame.dat")
    p = keycoderg.parse(kk)
    assert p.idx.tolist() == [0, 4, 8] and p.gray.tolist() == WANT_GRAY[name]
    assert kk == keycoderg.encode_file(frames, p.idx, NT), "byte for byte the numpy encoder's file"


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


@pytest.mark.parametrize("name", ["gray", "colour", "mixed"])
def test_cli_round_trip(jobs, monkeypatch, name):
    from tezip_amd import keycoder, keycoderg
    tmp, sets = jobs
    mdir, ddir, names, frames = sets[name]
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("TEZIP_NO_STREAMING", raising=False)
    cz, ck, cg, uz, ug, ur = (str(tmp / ("%s_%s" % (k, name))) for k in ("cz", "ck", "cg", "uz", "ug", "ur"))
    base = ["-p", "0", "-w", "4", "-m", "abs", "-b", "2"]
    for out, extra in ((cz, ["--key-coder", "zstd"]), (ck, ["--key-coder", "huff"]), (cg, ["--key-coder", "huffg", "--digests"])):
        code, text = _tezip(["-c", mdir, ddir, out] + base + extra)
        assert code == 0, text
    for n in ("entropy.dat", "filename.txt", "tezip_amd.json"):
        assert _read(cz, n) == _read(cg, n), n
    kg, kk = _read(cg, "key_frame.dat"), _read(ck, "key_frame.dat")
    assert kg[:4] == b"TZK2" and kg == keycoderg.encode_file(frames, [0, 4, 8], NT)
    assert kk[:4] == b"TZK1" and kk == keycoder.encode_file(frames, [0, 4, 8], NT), "--key-coder huff writes what it wrote"
    print("%s: TZK2 %d bytes, TZK1 %d bytes, zstd-9 %d bytes" % (name, len(kg), len(kk), len(_read(cz, "key_frame.dat"))))
    code, text = _tezip(["-u", mdir, cz, uz])
    assert code == 0, text
    code, text = _tezip(["-u", mdir, cg, ug, "--verify", "require"])
    assert code == 0, text
    assert sorted(os.listdir(ug)) == names
    for n in names:
        assert _read(ug, n) == _read(uz, n), n
    code, text = _tezip(["-u", mdir, cg, ur, "--frames", "5:7", "--verify", "require"])
    assert code == 0, text
    assert sorted(os.listdir(ur)) == names[5:7]
    for n in names[5:7]:
        assert _read(ur, n) == _read(uz, n), n
