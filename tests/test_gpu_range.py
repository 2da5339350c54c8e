"""Range decode on a MI355X (`-u --frames A:B`, tz_rollout_decode_range / tz_undelta_carry / tz_decode_range): frames
[A, B) of a stream must be byte-identical to the same frames of a whole decode, while the predictor runs only from the
range's restart frame on and the inverse scan starts from a carry computed over the payload prefix."""
import os
import subprocess
import sys

import numpy as np
import pytest

import fake_predictor
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

SMALL_STACKS = (3, 16, 32)


@pytest.fixture(scope="module")
def ctx():
    from tezip_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


# ---------------------------------------------------------------------------------------------------- 1. reference seam
RUNS = {}
for _f in ("ref_runs.npz", "ref_runs2.npz", "ref_runs3.npz", "ref_runs4.npz"):
    _R = np.load(os.path.join(GOLDEN, _f))
    RUNS.update({str(n): _R for n in _R["run_names"]})


def _load(name):
    R, pre = RUNS[name], "run_%s_" % name
    f = R[pre + "frames"]
    frames = np.ascontiguousarray(f if f.ndim == 4 else np.repeat(f[..., None], 3, axis=-1))
    nt, h, w, _ = frames.shape
    p, win, gray, entropy = (int(v) for v in R[pre + "params"])
    stream = R[pre + "entropy"]
    tlen = int(stream[-7])
    payload = np.ascontiguousarray(stream[: nt * h * w * 3])
    table = np.ascontiguousarray(stream[nt * h * w * 3: -7]) if tlen >= 0 else None
    key_frames = np.ascontiguousarray(R[pre + "key_frame"].reshape(nt, h, w, 3))
    key = np.array([bool(key_frames[i].any()) for i in range(nt)])
    return dict(frames=frames, p=p, payload=payload, table=table, key_frames=key_frames, key=key, decoded=R[pre + "decoded"])


def _predictions(frames, key, p):
    """Copy of tests/test_gpu_ref_runs.py::_predictions: the reference's predictor seam rebuilt with the fake predictor."""
    nt, h, w, _ = frames.shape
    hp, wp = (h + 7) // 8 * 8, (w + 7) // 8 * 8
    x_pad = np.zeros((nt, hp, wp, 3), np.float32)
    x_pad[:, :h, :w] = frames.astype(np.float32) / np.float32(255)
    c0 = fake_predictor.c0_image(hp, wp)
    pred = np.empty((nt, hp, wp, 3), np.float32)
    for i in range(nt):
        if i < p or key[i]:
            pred[i] = c0
        else:
            pred[i] = fake_predictor.g_next(x_pad[i - 1] if key[i - 1] else pred[i - 1])
    return pred


@pytest.mark.parametrize("name", sorted(RUNS))
def test_carry_seam_reproduces_the_reference_images(ctx, name):
    r = _load(name)
    frames, key, p = r["frames"], r["key"], r["p"]
    nt, h, w, _ = frames.shape
    fe = h * w * 3
    pred = _predictions(frames, key, p)
    x = ctx.unmap(r["payload"], r["table"], offset=True) if r["table"] is not None else r["payload"]
    idx = np.arange(nt)
    base_is_key = ((idx == 0) | ((idx >= p) & key)).astype(np.uint8)
    for a in range(1, nt):
        carry = ctx.undelta_carry(x, a * fe)
        assert carry == ctx.undelta_carry(r["payload"], a * fe, r["table"])   # the remap inside the carry kernel
        for b in sorted({a + 1, min(nt, a + 3), nt}):
            d = ctx.spatial_undelta(np.ascontiguousarray(x[a * fe: b * fe]), carry).reshape(b - a, h, w, 3)
            out = ctx.reconstruct(np.ascontiguousarray(pred[a:b]), np.ascontiguousarray(r["key_frames"][a:b]),
                                  base_is_key[a:b], d)
            np.testing.assert_array_equal(out, r["decoded"][a:b], err_msg="frames [%d, %d)" % (a, b))


# ------------------------------------------------------------------------------------------ 2. carry kernel vs numpy
def _dec_lut(table):
    """The decoder's LUT as include/tezip_hip.h states it (decompress.py:31-36 + 1600 - x of :236): the chained
    sequential `where` passes, values outside [0, 2111] passed through as 1600 - x."""
    T = len(table)
    lut = np.empty(2112, np.int64)
    for v in range(2112):
        cur, last = v, -1
        while 0 <= cur < T and cur > last:
            last, cur = cur, int(table[cur])
        lut[v] = 1600 - cur
    return lut


def _expected_carry(x, n0, lut=None):
    """x[n0-1] of decompress.py:22-29 = -(sum s'[0..n0)) mod 2^16, s'[0] = -s[0]; x a torch or numpy int16 vector."""
    import torch
    total = 0
    first = None
    step = 1 << 27
    for o in range(0, n0, step):
        c = x[o: min(n0, o + step)]
        if not torch.is_tensor(c):
            c = torch.from_numpy(np.ascontiguousarray(c))
        c = c.to(torch.int64)
        if lut is not None:
            lt = torch.as_tensor(lut, device=c.device)
            inside = (c >= 0) & (c <= 2111)
            c = torch.where(inside, lt[c.clamp(0, 2111)], 1600 - c)
        if first is None:
            first = int(c[0])
        total += int(c.sum())
    total -= 2 * first
    v = (-total) & 0xFFFF
    return v - 0x10000 if v >= 0x8000 else v


SMALL_N = [1, 2, 7, 8, 15, 16, 17, 4095, 4096, 4097, (1 << 20) + 3]
TABLE = np.random.default_rng(3).permutation(np.arange(1300, 1900))[:400].astype(np.int16)
TABLE[5], TABLE[9] = 3, 12       # entries inside [0, T): the chained passes of decompress.py:31-36


@pytest.mark.parametrize("with_table", [False, True])
def test_carry_kernel_small_prefixes(ctx, with_table):
    import torch
    rng = np.random.default_rng(11)
    n = (1 << 20) + 64
    if with_table:
        x = rng.integers(0, len(TABLE), n).astype(np.int16)
        x[rng.integers(0, n, 200)] = rng.integers(-300, 3000, 200)     # outside the table / the LUT: passed through
    else:
        x = rng.integers(-32768, 32768, n).astype(np.int16)
    table = TABLE if with_table else None
    lut = _dec_lut(TABLE) if with_table else None
    if with_table:   # the LUT restatement agrees with the library's own unmap
        np.testing.assert_array_equal(ctx.unmap(x[:4096], TABLE, offset=True).astype(np.int64),
                                      np.where((x[:4096] >= 0) & (x[:4096] <= 2111), lut[np.clip(x[:4096], 0, 2111)],
                                               1600 - x[:4096].astype(np.int64)).astype(np.int16))
    xd = torch.from_numpy(x).cuda()
    for n0 in SMALL_N:
        want = _expected_carry(x, n0, lut)
        assert ctx.undelta_carry(x, n0, table) == want, ("host", n0)
        assert ctx.undelta_carry(xd, n0, table) == want, ("device", n0)
        # a device pointer 2 bytes past a 16-byte boundary: scalar head, then the vectors
        assert ctx.undelta_carry(xd[1:], n0, table) == _expected_carry(x[1:], n0, lut), ("misaligned", n0)
        assert ctx.undelta_carry(xd[7:], n0, table) == _expected_carry(x[7:], n0, lut), ("misaligned 14 B", n0)
    torch.cuda.synchronize()


@pytest.mark.parametrize("with_table", [False, True])
def test_carry_kernel_large_prefixes(ctx, with_table):
    import torch
    g = torch.Generator(device="cuda").manual_seed(5)
    table = TABLE if with_table else None
    lut = _dec_lut(TABLE) if with_table else None
    hi = len(TABLE) if with_table else 32767
    lo = 0 if with_table else -32768
    for n0 in (62_914_560, (1 << 31) + 4099):       # a cfg3-sized prefix (80 x 512 x 512 x 3), one above 2^31 elements
        x = torch.randint(lo, hi, (n0 + 8,), dtype=torch.int16, device="cuda", generator=g)
        torch.cuda.synchronize()
        assert ctx.undelta_carry(x, n0, table) == _expected_carry(x, n0, lut), n0
        assert ctx.undelta_carry(x[1:], n0, table) == _expected_carry(x[1:], n0, lut), ("misaligned", n0)
        del x
        torch.cuda.empty_cache()


def test_carry_refuses_the_stream_start(ctx):
    from tezip_amd import _lib
    with pytest.raises(_lib.TezipError) as e:
        ctx.undelta_carry(np.zeros(8, np.int16), 0)
    assert e.value.status == -1


# ---------------------------------------------------------------------------------- 3. end to end through the library
def _job(ctx, nt, h, w, p, window, thr, mode, bound, entropy, seed=1, stacks=SMALL_STACKS, contract=None):
    from tezip_amd import _lib, synth
    from tezip_amd.prednet import PredNetConfig
    cfg = PredNetConfig(stack_sizes=stacks)
    ctx.load_model(cfg, cfg.init_weights(seed=seed, bias_scale=0.2))
    if contract:
        ctx.set_contract(contract)
    ctx.prepare(_lib.pad8(h), _lib.pad8(w), max_batch=4)
    frames = synth.translating_scene(nt, h, w, seed=seed)
    if thr == "auto":   # a DWP threshold inside the observed MSE range: windows of mixed lengths
        _, mse = ctx.rollout(frames, p, None, 1e9, want_mse=True)
        thr = float(np.median(mse[p + 1:]))
    key, _ = ctx.rollout(frames, p, window, thr)
    payload, table, _ = ctx.encode(mode, bound, entropy)
    keys = np.where(key[:, None, None, None], frames, 0).astype(np.uint8)
    kd = ctx.rollout_decode(keys, p)
    full = ctx.decode(payload, table).copy()
    if bound[0] == 0 and mode == "abs":
        np.testing.assert_array_equal(full, frames)
    return keys, kd, payload, table, full


def _ranges(nt, p, key):
    out = {(a, a + 1) for a in range(nt)} if nt <= 16 else set()
    ks = [k for k in range(nt) if key[k] and k > p]
    out |= {(0, nt), (0, 1), (p, nt), (p, min(nt, p + 3)), (nt - 1, nt)}
    if p > 1:
        out.add((1, p))                                   # inside the warm-up
    for k in ks:
        out |= {(k, nt), (k, min(nt, k + 2)), (max(0, k - 2), min(nt, k + 2))}
    if len(ks) >= 2:
        out.add((max(0, ks[0] - 1), min(nt, ks[-1] + 1)))  # two or more windows
    return sorted(out)


def _check_ranges(ctx, keys, kd, payload, table, full, p, ranges):
    for a, b in ranges:
        km = ctx.rollout_decode_range(keys, p, a, b - a)
        np.testing.assert_array_equal(km, kd)
        got = ctx.decode_range(payload, table, a, b - a)
        np.testing.assert_array_equal(got, full[a:b], err_msg="frames [%d, %d)" % (a, b))


E2E = [  # nt, h, w, p, window, thr, mode, bound, entropy
    (16, 24, 32, 0, 3, None, "abs", [0.0], True),       # 24 x 32: the fused scan + reconstruct tail
    (16, 21, 30, 1, 5, None, "abs", [2.0], True),       # padded frames: scan + k_recon
    (15, 24, 32, 2, 5, None, "rel", [1e-3], False),
    (14, 21, 30, 3, 3, None, "abs", [0.0], False),
    (16, 24, 32, 1, None, "auto", "abs", [2.0], True),  # DWP
    (13, 16, 24, 0, None, "auto", "rel", [1e-3], True),
    (12, 16, 24, 2, 20, None, "abs", [0.0], True),      # one window longer than the sequence
    (40, 24, 32, 1, 20, None, "abs", [2.0], True),
    (40, 24, 32, 3, 5, None, "abs", [0.0], True),
]


@pytest.mark.parametrize("nt,h,w,p,window,thr,mode,bound,entropy", E2E)
def test_range_equals_slice_of_full_decode(ctx, nt, h, w, p, window, thr, mode, bound, entropy):
    keys, kd, payload, table, full = _job(ctx, nt, h, w, p, window, thr, mode, bound, entropy)
    _check_ranges(ctx, keys, kd, payload, table, full, p, _ranges(nt, p, kd))


@pytest.mark.parametrize("contract", [1, 2])
def test_range_at_256_under_each_contract(ctx, contract):
    keys, kd, payload, table, full = _job(ctx, 9, 256, 256, 1, 3, None, "abs", [0.0], True, contract=contract)
    try:
        assert ctx.rollout_contract() == contract
        _check_ranges(ctx, keys, kd, payload, table, full, 1, [(0, 9), (4, 5), (3, 8), (8, 9)])
        assert ctx.rollout_contract() == contract
    finally:
        ctx.set_contract(0)


def test_range_streaming_entries_and_resident_frames(ctx):
    nt, h, w, p = 14, 24, 32, 1
    keys, kd, payload, table, full = _job(ctx, nt, h, w, p, 4, None, "abs", [2.0], True)
    for a, b in ((6, 9), (0, 3), (13, 14)):
        ctx.frames_begin(nt, h, w)
        ctx.frames_put(0, keys[:7])
        ctx.frames_put(7, keys[7:])
        ctx.payload_begin(payload.size)
        ctx.payload_put(0, payload[:5000])
        ctx.payload_put(5000, payload[5000:])
        ctx.rollout_decode_range(None, p, a, b - a)
        ctx.decode_range(None, table, a, b - a, out="resident")
        np.testing.assert_array_equal(ctx.decoded_get(a, b - a), full[a:b])
        np.testing.assert_array_equal(ctx.decoded_get(b - 1, 1), full[b - 1:b])
        if a > 0:   # outside the resident range
            from tezip_amd import _lib
            with pytest.raises(_lib.TezipError):
                ctx.decoded_get(a - 1, 1)


def test_range_errors(ctx):
    from tezip_amd import _lib
    nt, h, w, p = 10, 24, 32, 1
    keys, kd, payload, table, full = _job(ctx, nt, h, w, p, 4, None, "abs", [2.0], True)
    for a, n in ((-1, 2), (0, 0), (nt, 1), (8, 3)):
        with pytest.raises(_lib.TezipError) as e:
            ctx.rollout_decode_range(keys, p, a, n)
        assert e.value.status == -1
    ctx.frames_begin(nt, h, w)
    ctx.frames_put(0, keys)
    km = np.zeros(nt, np.uint8)   # a range call whose stack differs from the staged one
    assert ctx.lib.tz_rollout_decode_range(ctx.h, None, nt - 1, h, w, p, 0, 1, km.ctypes.data) == -1
    assert ctx.lib.tz_rollout_decode_range(ctx.h, None, nt, h + 8, w, p, 0, 1, km.ctypes.data) == -1
    ctx.rollout_decode_range(keys, p, 5, 2)
    with pytest.raises(_lib.TezipError) as e:   # outside what the range rollout covered
        ctx.decode_range(payload, table, 8, 2)
    assert e.value.status == -1
    with pytest.raises(_lib.TezipError) as e:   # the short prediction stack serves no whole-stack decode
        ctx.decode(payload, table)
    assert e.value.status == -4
    np.testing.assert_array_equal(ctx.decode_range(payload, table, 5, 2), full[5:7])


def test_whole_rollout_decode_at_the_warm_up_edge(ctx):
    """What tz_rollout_decode accepts and refuses where the warm-up reaches the end of the stack or a key frame is missing
    inside it (the range entry refuses warm_up >= nt; the whole one accepts warm_up == nt: every frame a C0 copy)."""
    from tezip_amd import _lib
    nt, h, w, p = 8, 24, 32, 1
    keys, kd, payload, table, full = _job(ctx, nt, h, w, p, 3, None, "abs", [2.0], True)
    c0 = ctx.get_predictions()[0].copy()                      # warm-up slot 0 of the p = 1 rollout: C0
    km = ctx.rollout_decode(keys, nt)
    np.testing.assert_array_equal(km, kd)
    pred = ctx.get_predictions()
    for i in range(nt):
        np.testing.assert_array_equal(pred[i], c0)
    got = ctx.decode(payload, table)                          # only frame 0 reconstructs from its key bytes
    np.testing.assert_array_equal(got[0], full[0])
    with pytest.raises(_lib.TezipError) as e:
        ctx.rollout_decode(keys, nt + 1)
    assert e.value.status == -1
    assert "key frames do not cover the sequence (%d of %d frames)" % (nt + 1, nt) in str(e.value)
    holed = keys.copy()
    holed[1] = 0                                              # frames 0..2 must be key frames for warm_up 2
    ks = [i for i in range(nt) if holed[i].any()]
    with pytest.raises(_lib.TezipError) as e:
        ctx.rollout_decode(holed, 2)
    assert e.value.status == -1
    assert "key frames do not cover the sequence (frame %d)" % ks[2] in str(e.value)
    with pytest.raises(_lib.TezipError) as e:                 # the refused rollout leaves no prediction stack behind
        ctx.get_predictions()
    assert e.value.status == -4


def test_whole_and_range_rollouts_serve_each_others_decodes(ctx):
    """A whole decoder rollout and a range rollout of [0, nt) leave the same prediction stack, so each serves the other's
    decode entry points with the same bytes."""
    nt, h, w, p = 12, 24, 32, 1
    keys, kd, payload, table, full = _job(ctx, nt, h, w, p, 4, None, "abs", [2.0], True)
    pred = ctx.get_predictions().copy()
    ks = [k for k in range(nt) if kd[k] and k > p]
    for a, b in ((0, nt), (0, 3), (ks[0], nt), (ks[0] + 1, ks[0] + 3)):   # a whole rollout, then range decodes
        np.testing.assert_array_equal(ctx.decode_range(payload, table, a, b - a), full[a:b], err_msg="frames [%d, %d)" % (a, b))
    np.testing.assert_array_equal(ctx.rollout_decode_range(keys, p, 0, nt), kd)
    np.testing.assert_array_equal(ctx.get_predictions(), pred)
    np.testing.assert_array_equal(ctx.decode(payload, table), full)
    ctx.decode(payload, table, out="resident")
    np.testing.assert_array_equal(ctx.decoded_get(0, nt), full)


def test_decode_refuses_a_table_length_below_minus_one(ctx):
    nt, h, w, p = 6, 24, 32, 1
    keys, kd, payload, table, full = _job(ctx, nt, h, w, p, 3, None, "abs", [2.0], True)
    out = np.zeros_like(full)
    assert ctx.lib.tz_decode(ctx.h, payload.ctypes.data, payload.size, None, -7, out.ctypes.data) == -1
    assert b"bad table" in ctx.lib.tz_last_error(ctx.h)
    assert ctx.lib.tz_decode_range(ctx.h, payload.ctypes.data, payload.size, None, -7, 0, nt, out.ctypes.data) == -1
    assert not out.any()
    np.testing.assert_array_equal(ctx.decode(payload, table), full)   # the context still decodes


# --------------------------------------------------------------------------------------------------- 4. work proof
def test_range_runs_only_the_predictor_steps_from_its_restart(ctx):
    from tezip_amd import _lib
    nt, h, w, p = 16, 24, 32, 1
    keys, kd, payload, table, full = _job(ctx, nt, h, w, p, 5, None, "abs", [2.0], True)
    # the predictor advances every window in one batched call per depth: a range that ends one step after the last key
    # frame needs one depth, the whole decode the longest window's
    last = int(np.flatnonzero(kd)[-1])
    assert nt - last >= 3
    a, n = last + 1, 1
    r = _lib.range_restart(kd, p, a)
    assert r == last and r > p

    def conv_launches(fn):
        ctx.prof_enable(True)
        ctx.prof_reset()
        fn()
        launches = ctx.prof_get()["conv3x3_mfma"][1]
        ctx.prof_enable(False)
        return launches

    rng = conv_launches(lambda: ctx.rollout_decode_range(keys, p, a, n))
    got = ctx.decode_range(payload, table, a, n)
    np.testing.assert_array_equal(got, full[a:a + n])
    sub = conv_launches(lambda: ctx.rollout_decode(np.ascontiguousarray(keys[r:a + n]), 0))
    whole = conv_launches(lambda: ctx.rollout_decode(keys, p))
    assert rng == sub and 0 < rng < whole, (rng, sub, whole)


# ---------------------------------------------------------------------------------------------------------- 5. CLI
def _cli(args, env_extra=None, timeout=300):
    env = dict(os.environ)
    env.update(env_extra or {})
    return subprocess.run(["timeout", "-k", "10", str(timeout), sys.executable, "-m", "tezip_amd.tezip"] + args, cwd=ROOT,
                          env=env, capture_output=True, text=True, timeout=timeout + 30)


@pytest.fixture(scope="module")
def cli_job(tmp_path_factory):
    from PIL import Image
    from tezip_amd import synth, weights
    from tezip_amd.prednet import PredNetConfig
    tmp = tmp_path_factory.mktemp("range_cli")
    cfg = PredNetConfig(stack_sizes=SMALL_STACKS)
    nt, h, w = 16, 29, 43          # nt*H*W*3 a multiple of 8: -c --shuffle refuses other stacks
    frames = synth.translating_scene(nt, h, w, seed=5)
    mdir = str(tmp / "model")
    weights.save_model(mdir, cfg, cfg.init_weights(seed=4, bias_scale=0.1), 32, 48)
    ddir = tmp / "data"
    ddir.mkdir()
    for t in range(nt):
        Image.fromarray(frames[t]).save(ddir / ("f_%03d.png" % t))
    out = {}
    for shuffle in (False, True):
        cdir, udir = str(tmp / ("comp%d" % shuffle)), str(tmp / ("full%d" % shuffle))
        r = _cli(["-c", mdir, str(ddir), cdir, "-p", "1", "-w", "4", "-m", "abs", "-b", "1"] + (["--shuffle"] if shuffle else []))
        assert r.returncode == 0, r.stdout + r.stderr
        r = _cli(["-u", mdir, cdir, udir])
        assert r.returncode == 0, r.stdout + r.stderr
        out[shuffle] = (cdir, {n: open(os.path.join(udir, n), "rb").read() for n in os.listdir(udir)})
    names = ["f_%03d.png" % t for t in range(nt)]
    assert sorted(out[False][1]) == names and sorted(out[True][1]) == names
    return tmp, mdir, names, out


@pytest.mark.parametrize("spec,env,shuffle", [
    ("3:7", {}, False),
    ("12", {}, False),
    (":2", {"TEZIP_NO_STREAMING": "1"}, False),
    ("5:", {"TEZIP_NO_EARLY_ROLLOUT": "1"}, False),
    ("4:9", {}, True),
])
def test_cli_frames_writes_exactly_the_range(cli_job, spec, env, shuffle):
    from tezip_amd import tezip
    tmp, mdir, names, out = cli_job
    cdir, full = out[shuffle]
    a, b = tezip.parse_frames(spec)
    want = names[a: len(names) if b is None else b]
    udir = str(tmp / ("r_%s_%d_%d" % (spec.replace(":", "-"), len(env), shuffle)))
    r = _cli(["-u", mdir, cdir, udir, "--frames", spec], env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert sorted(os.listdir(udir)) == want, r.stdout
    for n in want:
        assert open(os.path.join(udir, n), "rb").read() == full[n], n


@pytest.mark.parametrize("spec", ["16:17", "2:40", "16"])
def test_cli_frames_out_of_range_exits_2_and_writes_nothing(cli_job, spec):
    tmp, mdir, names, out = cli_job
    udir = str(tmp / ("bad_" + spec.replace(":", "-")))
    r = _cli(["-u", mdir, out[False][0], udir, "--frames", spec])
    assert r.returncode == 2, r.stdout + r.stderr
    assert "ERROR" in r.stdout
    assert not os.path.exists(udir) or os.listdir(udir) == []


# -------------------------------------------------------------------------------------------------------- 6. poison
POISON_JOB = r'''
import hashlib, sys
import numpy as np
sys.path.insert(0, %r)
from tezip_amd import _lib, synth
from tezip_amd.prednet import PredNetConfig
cfg = PredNetConfig(stack_sizes=(3, 16, 32))
ctx = _lib.Context(0)
ctx.load_model(cfg, cfg.init_weights(seed=2, bias_scale=0.2))
h = hashlib.sha256()
for (nt, H, W) in [(14, 24, 32), (14, 21, 30)]:
    frames = synth.translating_scene(nt, H, W, seed=3)
    ctx.prepare(_lib.pad8(H), _lib.pad8(W), max_batch=4)
    key, _ = ctx.rollout(frames, 1, 4, None)
    payload, table, _ = ctx.encode("abs", [2.0], True)
    keys = np.where(key[:, None, None, None], frames, 0).astype(np.uint8)
    ctx.rollout_decode_range(keys, 1, 6, 5)
    h.update(ctx.decode_range(payload, table, 6, 5).tobytes())
    h.update(np.int16(ctx.undelta_carry(payload, 1000, table)).tobytes())
print("digest", h.hexdigest())
''' % ROOT


def test_range_decode_does_not_depend_on_device_memory_contents():
    digests = []
    for poison in (None, "165"):
        env = dict(os.environ)
        env.pop("TEZIP_POISON", None)
        if poison:
            env["TEZIP_POISON"] = poison
        r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, "-c", POISON_JOB], env=env, capture_output=True,
                           text=True, timeout=270)
        assert r.returncode == 0, r.stdout + r.stderr
        digests.append([l for l in r.stdout.splitlines() if l.startswith("digest")][-1])
    assert digests[0] == digests[1]
