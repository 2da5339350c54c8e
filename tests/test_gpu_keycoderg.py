"""The key-frame coder that stores a gray key frame once (`--key-coder huffg`, format TZK2) on the GPU: k_key_gray gives the
numpy flag exactly, k_key_resid / k_key_unresid_* the numpy residuals and their inverses bit for bit, compress.run the
bytes of keycoderg.encode_file, and `-c --key-coder huffg --digests` then `-u --verify require` the images of a
`--key-coder zstd` job (tezip_amd/keycoderg.py is the specification).  TZK1 = TZK2 with no GRAY bit: pred bytes 0..3 through
the TZK2 entry points give what the TZK1 entry points give, and both coders' scope counts, digests and refusal texts are those
of the commit before they shared one residual path (tests/golden/key_coder_parent.json).  No test feeds a kernel a corrupted body: the
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


# ------------------------------------------------------------------- k_key_resid / k_key_unresid_* under pred bytes 0..7
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


def mixed_stack():
    """7 x 21 x 30: gray frames, a colour frame (4) and a frame one bit off gray (6); the key frames are 0, 1, 4 and 6."""
    stack = gray_stack(7, 21, 30, 3)
    stack[4] = colour_stack(1, 21, 30, 4)[0]
    stack[6, 20, 29, 2] ^= 1
    return stack, [0, 1, 4, 6]


def test_resident_forms_match_numpy_and_refuse_the_other_format(ctx):
    from tezip_amd import _lib, keycoder, keycoderg
    stack, keys = mixed_stack()
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


# ------------------------------------------------------------------------------------------ TZK1 = TZK2 with no GRAY bit
@pytest.mark.parametrize("h,w", [(1, 1), (5, 7), (3, 300), (61, 90), (64, 64)])
def test_without_a_gray_bit_it_is_the_tzk1_coder(ctx, h, w):
    """Pred bytes 0..3 through the TZK2 entry points give what the TZK1 entry points give, and the two files of a stack without
    a gray frame differ in the magic alone and decode to the same frames."""
    from tezip_amd import keycoder, keycoderg
    stack = colour_stack(3, h, w, h * 13 + w)
    stack[:, 0, 0, 1] = stack[:, 0, 0, 0] ^ 0x55                         # (a random 1 x 1 frame could be gray)
    rng = np.random.default_rng(h + w)
    for preds in [[p] * 3 for p in range(4)] + [[3, 0, 2], [1, 2, 3]]:
        sym = ctx.keys_residual_buf(stack, preds)
        assert (ctx.keysg_residual_buf(stack, preds) == sym).all(), "residuals %r at %dx%d" % (preds, h, w)
        noisy = (sym | (rng.integers(0, 2, sym.size) * 0x4100).astype(np.int16)).astype(np.int16)   # the high bytes must not count
        back = ctx.keys_unresidual_buf(noisy, preds, h, w)
        assert (back == stack).all() and (ctx.keysg_unresidual_buf(noisy, preds, h, w) == back).all(), "inverse %r at %dx%d" % (preds, h, w)
    keys = [0, 2]
    k1, k2 = keycoder.encode_file(stack, keys, 3), keycoderg.encode_file(stack, keys, 3)
    assert k1[:4] == b"TZK1" and k2[:4] == b"TZK2" and k1[4:] == k2[4:]
    p1, p2 = keycoder.parse(k1), keycoderg.parse(k2)
    want = np.zeros_like(stack)
    want[keys] = stack[keys]
    b1, b2 = np.ascontiguousarray(p1.body), np.ascontiguousarray(p2.body)
    ctx.keys_begin(b1.size, p1.nt, p1.H, p1.W, p1.idx, p1.pred, p1.lengths)
    ctx.keys_put(0, b1)
    ctx.keys_decode()
    got1 = ctx.frames_get(0, 3)
    ctx.keysg_begin(b2.size, p2.nt, p2.H, p2.W, p2.idx, p2.pred, p2.lengths)
    ctx.keysg_put(0, b2)
    ctx.keysg_decode()
    got2 = ctx.frames_get(0, 3)
    assert (got1 == want).all() and (got2 == got1).all()


# ------------------------------------------------------------ scope counts, digests and refusal texts of the parent
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "key_coder_parent.json")


class _OddAddress:
    """A device array of n int16 symbols at an odd address, as _lib takes buffers (numel / is_contiguous / data_ptr)."""

    def __init__(self, n):
        import torch
        self.hold = torch.zeros(2 * n + 16, dtype=torch.uint8, device="cuda")
        self.n = n

    def numel(self):
        return self.n

    def is_contiguous(self):
        return True

    def data_ptr(self):
        return self.hold.data_ptr() + 1


def record():
    """The job of test_resident_forms_match_numpy_and_refuse_the_other_format through a context of its own -> {"calls": {call:
    {"scopes": scope count of the 'huffman' profiling class, "digest": TZD64 of what the call left}}, "refusals": {case: text}}."""
    from tezip_amd import _lib, digest, huff, keycoder, keycoderg
    stack, keys = mixed_stack()
    nt, h, w = stack.shape[:3]
    calls, refusals = {}, {}
    sym3 = np.zeros(4 * h * w * 3, np.int16)
    odd = _OddAddress(sym3.size)
    c = _lib.Context(0)

    def counted(name, call, left):
        c.prof_reset()
        call()
        scopes = int(c.prof_get()["huffman"][1])
        calls[name] = {"scopes": scopes, "digest": "%016x" % digest.frame_digest(np.ascontiguousarray(left()).reshape(-1).view(np.uint8))}

    def refused(name, call):
        with pytest.raises(_lib.TezipError) as e:
            call()
        refusals[name] = str(e.value)

    try:
        c.prof_enable(True)
        _resident(c, stack)
        state = {}
        counted("keys_counts", lambda: state.update(counts=c.keys_counts(keys)), lambda: state["counts"])
        counted("keys_gray", lambda: state.update(gray=c.keys_gray(keys)), lambda: state["gray"].astype(np.uint8))
        pred = keycoder.choose_predictors(state["counts"])
        len1 = huff.code_lengths(keycoder.chosen_counts(state["counts"], pred))
        counted("keys_encode", lambda: state.update(n1=c.keys_encode(keys, pred, len1)), lambda: c.keys_get(0, state["n1"]))
        body1 = c.keys_get(0, state["n1"])
        gcounts = keycoderg.gray_counts(state["counts"], state["gray"])
        predg = keycoderg.pred_bytes(gcounts, state["gray"])
        len2 = huff.code_lengths(keycoderg.chosen_counts(gcounts, predg))
        counted("keysg_encode", lambda: state.update(n2=c.keysg_encode(keys, predg, len2)), lambda: c.keysg_get(0, state["n2"]))
        body2 = c.keysg_get(0, state["n2"])
        # ---- refusals of the encoder's entry points (the stack is resident)
        bad4, bad8 = [0, 1, 4, 2], [0, 1, 8, 2]
        refused("keys_encode pred 4", lambda: c.keys_encode(keys, bad4, len1))
        refused("keysg_encode pred 8", lambda: c.keysg_encode(keys, bad8, len2))
        refused("keys_residual_buf pred 4", lambda: c.keys_residual_buf(stack[keys], bad4))
        refused("keysg_residual_buf pred 8", lambda: c.keysg_residual_buf(stack[keys], bad8))
        refused("keys_unresidual_buf pred 4", lambda: c.keys_unresidual_buf(sym3, bad4, h, w))
        refused("keysg_unresidual_buf pred 8", lambda: c.keysg_unresidual_buf(sym3, bad8, h, w))
        refused("keys_begin pred 4", lambda: c.keys_begin(body1.size, nt, h, w, keys, bad4, len1))
        refused("keysg_begin pred 8", lambda: c.keysg_begin(body2.size, nt, h, w, keys, bad8, len2))
        for name, idx in (("indices not ascending", [0, 4, 1, 6]), ("nkeys 0", [])):
            ok = [0] * len(idx)
            refused("keys_counts " + name, lambda: c.keys_counts(idx))
            refused("keys_gray " + name, lambda: c.keys_gray(idx))
            refused("keys_encode " + name, lambda: c.keys_encode(idx, ok, len1))
            refused("keysg_encode " + name, lambda: c.keysg_encode(idx, ok, len2))
            refused("keys_begin " + name, lambda: c.keys_begin(body1.size, nt, h, w, idx, ok, len1))
            refused("keysg_begin " + name, lambda: c.keysg_begin(body2.size, nt, h, w, idx, ok, len2))
        refused("keys_residual_buf misaligned symbols", lambda: c.keys_residual_buf(stack[keys], [0, 1, 2, 3], out=odd))
        refused("keysg_residual_buf misaligned symbols", lambda: c.keysg_residual_buf(stack[keys], [0, 1, 2, 3], out=odd))
        refused("keys_unresidual_buf misaligned symbols", lambda: c.keys_unresidual_buf(odd, [0, 1, 2, 3], h, w))
        refused("keysg_unresidual_buf misaligned symbols", lambda: c.keysg_unresidual_buf(odd, [0, 1, 2, 3], h, w))
        # ---- the decoders, and the refusals of a staged stream
        for kind, body, pr, ln in (("keys", body1, pred, len1), ("keysg", body2, predg, len2)):
            begin, put, decode = (getattr(c, "%s_%s" % (kind, f)) for f in ("begin", "put", "decode"))
            begin(body.size, nt, h, w, keys, pr, ln)
            put(0, body[:100])
            refused(kind + "_put outside the stream", lambda: put(body.size - 10, body[:100]))
            refused(kind + "_decode after an incomplete put", decode)
            put(100, body[100:])
            counted(kind + "_decode", decode, lambda: c.frames_get(0, nt))
    finally:
        c.close()
    return {"calls": calls, "refusals": refusals}


def test_scopes_digests_and_refusal_texts_are_the_parents():
    """tests/golden/key_coder_parent.json holds record() as the commit before the two coders were put behind one residual
    path gave it (tests/golden/make_key_coder_parent.py)."""
    import json
    with open(FIXTURE) as f:
        want = json.load(f)
    got = record()
    for part in ("calls", "refusals"):
        assert sorted(got[part]) == sorted(want[part])
        for name in sorted(want[part]):
            assert got[part][name] == want[part][name], "%s: %s" % (part, name)


def test_a_bad_index_is_named_before_a_bad_pred_byte(ctx):
    """Both formats check the whole key list, then the pred bytes: a call that is wrong in both names
    the index, whichever entry comes first."""
    from tezip_amd import _lib
    stack, _ = mixed_stack()
    _resident(ctx, stack)
    lengths = np.full(256, 8, np.uint8)
    want = "tezip_hip status -1: key frames: index 1 (entry 2) is not ascending inside [0, 7)"
    for encode, begin, bad in ((ctx.keys_encode, ctx.keys_begin, 4), (ctx.keysg_encode, ctx.keysg_begin, 8)):
        for call in (lambda: encode([0, 4, 1, 6], [bad, 0, 0, 0], lengths),
                     lambda: begin(4096, 7, 21, 30, [0, 4, 1, 6], [bad, 0, 0, 0], lengths)):
            with pytest.raises(_lib.TezipError) as e:
                call()
            assert str(e.value) == want


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
