"""The opt-in key-frame coder on the GPU: k_key_resid / k_key_unresid_* give the numpy residuals and their inverses bit for
bit, k_key_hist the numpy counts, tz_keys_encode behind keycoder.pack_front the bytes of keycoder.encode_file, and
tz_keys_begin / put / decode the zero-except-keys stack (tezip_amd/keycoder.py is the specification); `-c --key-coder huff`
then `-u` writes what `-c` then `-u` writes.  No test feeds a kernel a corrupted body: the container's validation and the
decoder's clamps are tested on the CPU (tests/test_keycoder.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

NT, H, W, KEYS = 7, 21, 30, [0, 1, 4, 6]


@pytest.fixture(scope="module")
def ctx():
    from tezip_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _stack(nt=NT, h=H, w=W, seed=1):
    """Smooth rows with noise on top: every predictor has a distribution of its own, and sums wrap."""
    rng = np.random.default_rng(seed)
    base = np.cumsum(rng.integers(-3, 4, (nt, h, w, 3)), axis=2) + np.cumsum(rng.integers(-3, 4, (nt, h, w, 3)), axis=1)
    return (base + rng.integers(0, 2, (nt, h, w, 3)) * 200).astype(np.uint8)


@pytest.mark.parametrize("h,w", [(1, 1), (3, 5), (21, 30), (61, 90), (64, 64), (3, 300)])
@pytest.mark.parametrize("k", [1, 3])
def test_buffer_forms_are_the_numpy_functions(ctx, h, w, k):
    """61 x 90 x 3 = 16 470 symbols cross a chunk boundary; W * 3 is odd or no multiple of 16 in most shapes, and with
    k = 3 the second and third frame start off a 16-byte boundary.  3 x 300: a row of five 64-column steps of the row
    kernel, more than one workgroup of columns in the column kernel."""
    from tezip_amd import keycoder
    frames = _stack(k, h, w, seed=h * 7 + w)
    for preds in [[p] * k for p in range(4)] + ([[3, 0, 2], [1, 2, 3]] if k == 3 else []):
        want = np.concatenate([keycoder.residual(f, p) for f, p in zip(frames, preds)])
        got = ctx.keys_residual_buf(frames, preds)
        assert got.dtype == np.int16 and (got == want).all(), "residuals %r at %dx%d" % (preds, h, w)
        back = ctx.keys_unresidual_buf(want, preds, h, w)
        assert (back == frames).all(), "inverse %r at %dx%d" % (preds, h, w)
        for j, p in enumerate(preds):
            assert (keycoder.unresidual(got[j * h * w * 3: (j + 1) * h * w * 3], p, h, w) == frames[j]).all()


def test_buffer_forms_at_512(ctx):
    from tezip_amd import keycoder, synth
    frames = np.ascontiguousarray(synth.turbulence(nt=3)[:3])
    for preds in ([3], [1, 2, 3], [0, 3, 3]):
        fr = frames[: len(preds)]
        want = np.concatenate([keycoder.residual(f, p) for f, p in zip(fr, preds)])
        assert (ctx.keys_residual_buf(fr, preds) == want).all(), preds
        assert (ctx.keys_unresidual_buf(want, preds, 512, 512) == fr).all(), preds


def test_device_buffers_off_alignment(ctx):
    import torch
    from tezip_amd import keycoder
    h, w, k = 21, 30, 2
    frames = _stack(k, h, w, seed=9)
    n = frames.size
    for shift in (1, 5, 16):
        dev = torch.zeros(n + 64, dtype=torch.uint8, device="cuda")
        view = dev[shift: shift + n]
        view.copy_(torch.from_numpy(frames.reshape(-1)))
        sym = torch.zeros(n + 16, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        ctx.keys_residual_buf(view.view(k, h, w, 3), [3, 1], out=sym[1: 1 + n])
        torch.cuda.synchronize()
        res = sym.cpu().numpy()
        want = np.concatenate([keycoder.residual(frames[0], 3), keycoder.residual(frames[1], 1)])
        assert (res[1: 1 + n] == want).all() and res[0] == 0 and (res[1 + n:] == 0).all(), shift
        out = torch.zeros(n + 64, dtype=torch.uint8, device="cuda")
        ctx.keys_unresidual_buf(sym[1: 1 + n], [3, 1], h, w, out=out[shift: shift + n])
        torch.cuda.synchronize()
        o = out.cpu().numpy()
        assert (o[shift: shift + n] == frames.reshape(-1)).all() and (o[:shift] == 0).all() and (o[shift + n:] == 0).all(), shift


def _resident_round_trip(ctx, stack, keys):
    """counts, file bytes and decoded stack of the resident forms against the numpy statement; returns the file."""
    from tezip_amd import huff, keycoder
    nt, h, w = stack.shape[:3]
    ctx.frames_begin(nt, h, w)
    ctx.frames_put(0, stack[:3])
    ctx.frames_put(3, stack[3:])
    counts = ctx.keys_counts(keys)
    want_counts = keycoder.predictor_counts(stack[keys])
    assert counts.shape == want_counts.shape and (counts == want_counts).all(), "k_key_hist against numpy"
    pred = keycoder.choose_predictors(counts)
    lengths = huff.code_lengths(keycoder.chosen_counts(counts, pred))
    nbytes = ctx.keys_encode(keys, pred, lengths)
    body = np.concatenate([ctx.keys_get(0, 100), ctx.keys_get(100, nbytes - 100)])
    n = len(keys) * h * w * 3
    front = keycoder.pack_front(nt, h, w, keys, pred, lengths, huff.geometry(n)[1], (nbytes - huff.body_bytes(n, 0)) // 4)
    data = front + body.tobytes()
    assert data == keycoder.encode_file(stack, keys, nt), "the GPU file differs from the numpy encoder's"
    want = np.zeros_like(stack)
    want[keys] = stack[keys]
    p = keycoder.parse(data)
    b = np.ascontiguousarray(p.body)
    for cuts in ([b.size], [7, b.size // 2 + 1, b.size]):              # whole, and three uneven pieces
        ctx.keys_begin(b.size, p.nt, p.H, p.W, p.idx, p.pred, p.lengths)
        lo = 0
        for hi in cuts:
            ctx.keys_put(lo, b[lo:hi])
            lo = hi
        ctx.keys_decode()
        assert (ctx.frames_get(0, nt) == want).all(), "decoded stack, pieces %r" % (cuts,)
    return data


def test_resident_forms_match_numpy(ctx):
    _resident_round_trip(ctx, _stack(), KEYS)
    every = _stack(NT, 5, 3, seed=4)                                     # every frame a key frame (-w 1): nothing to zero
    _resident_round_trip(ctx, every, list(range(NT)))


_POISON_SCRIPT = r"""
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
from tezip_amd import _lib
import test_gpu_keycoder as t
ctx = _lib.Context(0)
for rep in range(2):      # (the second pass reuses buffers the first one filled)
    t._resident_round_trip(ctx, t._stack(seed=rep), t.KEYS)
ctx.close()
print("poison ok")
"""


def test_same_stack_under_poison(tmp_path):
    """TEZIP_POISON fills every device buffer handed out before its use: the non-key frames must be zeroed by the decoder,
    and nothing may depend on what a buffer held."""
    script = tmp_path / "poison_job.py"
    script.write_text(_POISON_SCRIPT % (ROOT, os.path.join(ROOT, "tests")))
    env = dict(os.environ, TEZIP_POISON="0xA5")
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, str(script)], cwd=ROOT, capture_output=True, text=True, env=env,
                       timeout=330)
    assert r.returncode == 0 and "poison ok" in r.stdout, r.stdout + r.stderr


def test_a_staged_entropy_stream_survives_the_key_coder(ctx):
    """decompress.run stages entropy.dat's front before the key frames: tz_huff_begin / tz_huff_put, then a complete
    tz_keys_* sequence, then tz_huff_decode."""
    from tezip_amd import huff
    rng = np.random.default_rng(6)
    pay = np.minimum(rng.geometric(0.2, NT * H * W * 3) - 1, 300).astype(np.int16)
    ln = huff.code_lengths(np.bincount(pay))
    body = np.frombuffer(huff.pack_body(*huff.encode_body(pay, ln, 0)), np.uint8)
    ctx.huff_begin(body.size, pay.size, ln, 0)
    ctx.huff_put(0, body)
    _resident_round_trip(ctx, _stack(seed=12), KEYS)
    ctx.huff_decode()
    assert (ctx.payload_get(0, pay.size) == pay).all()


def test_bad_arguments_are_refused(ctx):
    from tezip_amd import _lib, huff, keycoder
    stack = _stack()
    data = _resident_round_trip(ctx, stack, KEYS)
    p = keycoder.parse(data)
    b = np.ascontiguousarray(p.body)

    def refused(status, call):
        with pytest.raises(_lib.TezipError) as e:
            call()
        assert e.value.status == status

    ctx.frames_begin(NT, H, W)
    ctx.frames_put(0, stack)
    ok_pred, ok_len = [0] * 4, p.lengths
    for idx in ([], [1, 1, 4, 6], [0, 4, 1, 6], [0, 1, 4, 7], [-1, 1, 4, 6]):   # none, not ascending, out of range
        refused(-1, lambda: ctx.keys_counts(idx))
        refused(-1, lambda: ctx.keys_encode(idx, [0] * len(idx), ok_len))
        refused(-1, lambda: ctx.keys_begin(b.size, NT, H, W, idx, [0] * len(idx), ok_len))
    refused(-1, lambda: ctx.keys_encode(KEYS, [0, 1, 4, 2], ok_len))                   # a predictor id above 3
    refused(-1, lambda: ctx.keys_begin(b.size, NT, H, W, KEYS, [0, 1, 4, 2], ok_len))
    kraft = np.array(ok_len)
    kraft[:3] = 1
    too_long = np.array(ok_len)
    too_long[0] = 13
    for bad_len in (kraft, too_long, np.zeros(256, np.uint8)):                          # Kraft > 1, a length of 13, no symbol
        refused(-1, lambda: ctx.keys_encode(KEYS, ok_pred, bad_len))
        refused(-1, lambda: ctx.keys_begin(b.size, NT, H, W, KEYS, ok_pred, bad_len))
    one = np.zeros(256, np.uint8)
    one[0] = 1
    refused(-1, lambda: ctx.keys_encode(KEYS, ok_pred, one))                           # the frames hold values without a code
    refused(-1, lambda: ctx.keys_begin(b.size + 2, NT, H, W, KEYS, ok_pred, ok_len))   # no whole words
    refused(-1, lambda: ctx.keys_begin(16, NT, H, W, KEYS, ok_pred, ok_len))           # shorter than the index
    refused(-1, lambda: ctx.keys_begin(b.size, 0, H, W, KEYS, ok_pred, ok_len))
    ctx.keys_begin(b.size, p.nt, p.H, p.W, p.idx, p.pred, p.lengths)
    ctx.keys_put(0, b[:100])
    refused(-1, lambda: ctx.keys_put(b.size - 10, b[:100]))                            # past the stream's end
    refused(-4, ctx.keys_decode)                                                       # not every byte was put
    ctx.keys_put(100, b[100:])
    ctx.keys_decode()
    fresh = _lib.Context(0)
    refused_fresh = [lambda: fresh.keys_counts(KEYS), lambda: fresh.keys_encode(KEYS, ok_pred, ok_len), fresh.keys_decode]
    for call in refused_fresh:                                                         # no frames resident / nothing staged
        with pytest.raises(_lib.TezipError) as e:
            call()
        assert e.value.status == -4
    fresh.close()
    want = np.zeros_like(stack)
    want[KEYS] = stack[KEYS]
    assert (ctx.frames_get(0, NT) == want).all()                                       # the context still works
    assert huff.MAX_LEN == 12


# ------------------------------------------------------------------------------------------- compress.run / decompress.run
@pytest.fixture(scope="module")
def jobs(tmp_path_factory):
    """Two image directories with a model each: 20 frames of synth.moving_blobs at 64 x 64, 12 frames at 61 x 90."""
    from PIL import Image
    from tezip_amd import synth, weights
    from tezip_amd.prednet import PredNetConfig
    tmp = tmp_path_factory.mktemp("keycoder")
    cfg = PredNetConfig(stack_sizes=(3, 16, 32))
    wts = cfg.init_weights(seed=4, bias_scale=0.2)
    out = {}
    for name, frames, hp, wp in (("blobs", synth.moving_blobs(20, 64, 64), 64, 64),
                                 ("odd", synth.translating_scene(12, 61, 90, seed=5), 64, 96)):
        mdir, ddir = str(tmp / (name + "_model")), tmp / (name + "_data")
        weights.save_model(mdir, cfg, wts, hp, wp)
        ddir.mkdir()
        names = ["f_%03d.png" % t for t in range(len(frames))]
        for t, f in enumerate(frames):
            Image.fromarray(f).save(ddir / names[t])
        out[name] = (mdir, str(ddir), names, frames)
    return tmp, out


def _read(d, n):
    with open(os.path.join(d, n), "rb") as f:
        return f.read()


@pytest.mark.parametrize("data,bound,coder", [
    ("blobs", 0.0, "zstd"), ("blobs", 0.0, "huff"), ("blobs", 0.0, "huffr"),
    ("blobs", 2.0, "zstd"), ("blobs", 2.0, "huff"), ("blobs", 2.0, "huffr"),
    ("odd", 2.0, "huffr"),
])
def test_key_coder_job_decodes_to_the_zstd_jobs_images(jobs, monkeypatch, capsys, data, bound, coder):
    from tezip_amd import compress, decompress, keycoder, zstd
    tmp, sets = jobs
    mdir, ddir, names, frames = sets[data]
    nt, h, w = frames.shape[:3]
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("TEZIP_NO_STREAMING", raising=False)
    tag = "%s_%g_%s" % (data, bound, coder)
    cz, ck = str(tmp / ("cz_" + tag)), str(tmp / ("ck_" + tag))
    compress.run(mdir, ddir, cz, 1, 5, None, "abs", [bound], True, False, True, CODER=coder)
    capsys.readouterr()
    compress.run(mdir, ddir, ck, 1, 5, None, "abs", [bound], True, True, True, CODER=coder, KEY_CODER="huff")
    assert any(ln.startswith("key_coding:") and ln.endswith("[sec]") for ln in capsys.readouterr().out.splitlines())
    for n in ("filename.txt", "entropy.dat", "tezip_amd.json"):
        assert _read(cz, n) == _read(ck, n), n
    kz, kk = _read(cz, "key_frame.dat"), _read(ck, "key_frame.dat")
    assert kk[:4] == b"TZK1" and kz[:4] != b"TZK1"
    key_stack = np.frombuffer(zstd.decompress(kz), np.uint8).reshape(nt, h, w, 3)
    p = keycoder.parse(kk)
    assert (p.nt, p.H, p.W) == (nt, h, w) and p.nkeys >= 3
    assert p.idx.tolist() == np.nonzero(key_stack.reshape(nt, -1).any(axis=1))[0].tolist()
    assert (keycoder.decode_file(kk) == key_stack).all()
    assert kk == keycoder.encode_file(key_stack, p.idx, nt)             # byte for byte the numpy encoder's file
    print("%s: TZK1 %d bytes, zstd-9 %d bytes" % (tag, len(kk), len(kz)))
    uz, uk, ur, un = (str(tmp / (k + tag)) for k in ("uz_", "uk_", "ur_", "un_"))
    decompress.run(mdir, cz, uz, True, False)
    decompress.run(mdir, ck, uk, True, False)
    assert sorted(os.listdir(uk)) == names
    for n in names:
        assert _read(uz, n) == _read(uk, n), n
    decompress.run(mdir, ck, ur, True, False, frames=(7, 9))
    assert sorted(os.listdir(ur)) == names[7:9]
    for n in names[7:9]:
        assert _read(ur, n) == _read(uz, n), n
    monkeypatch.setenv("TEZIP_NO_STREAMING", "1")                        # the whole-array path reads the same file
    decompress.run(mdir, ck, un, True, False)
    for n in names:
        assert _read(un, n) == _read(uz, n), n
