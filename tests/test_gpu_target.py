"""`-c --target-psnr` on a MI355X (definition TZ-TPSNR-1, tezip_amd/target.py): k_bound_err against its slow statement,
tz_bound_probe against tz_encode + tz_encode_quality record for record, the search on the GPU against the same search over
the Python oracle's quantiser, and the command line end to end.  Integers throughout."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

SMALL_STACKS = (3, 16, 32)


def _model(seed=1):
    """Random weights whose predictions are worth something to these tests: glorot weights with small biases predict
    trunc(pred * 255) == 0 nearly everywhere, so that orig + d is 0, no clamp can fire behind a rollout and the three
    channels agree trivially.  With level 0's prediction convolution scaled up and a bias per channel the integer
    predictions span 0 .. 200 and differ between the channels at nearly every pixel (_nontrivial asserts it)."""
    from tezip_amd.prednet import PredNetConfig
    cfg = PredNetConfig(stack_sizes=SMALL_STACKS)
    wts = cfg.init_weights(seed=seed, bias_scale=0.2)
    names = [n for n, _ in cfg.weight_shapes()]
    wts[names.index("ahat0/kernel")] = wts[names.index("ahat0/kernel")] * np.float32(6.0)
    wts[names.index("ahat0/bias")] = np.array([0.35, 0.5, 0.65], np.float32)
    return cfg, wts


def _nontrivial(ctx, frames, key):
    """the integer predictions of the predicted frames span a range and their channels differ"""
    nt, h, w, _ = frames.shape
    xi = (ctx.get_predictions()[:, :h, :w] * np.float32(255.0)).astype(np.int64)[~np.asarray(key, bool)]
    assert len(xi) and xi.max() - xi.min() >= 100 and xi.max() <= 255
    assert (xi[..., 0] != xi[..., 1]).mean() > 0.5 and (xi[..., 0] != xi[..., 2]).mean() > 0.5


@pytest.fixture(scope="module")
def ctx():
    from tezip_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _records(q):
    return np.stack([q["sse"].astype(np.int64), q["max_abs"].astype(np.int64), q["n_changed"].astype(np.int64)], axis=1)


def _blobs():
    from tezip_amd import synth
    return np.ascontiguousarray(synth.moving_blobs(7, 32, 32)[:, :21, :30])


def _scene():
    from tezip_amd import synth
    return synth.translating_scene(6, 61, 90)


def _scene160():
    from tezip_amd import synth
    return synth.translating_scene(6, 128, 160)


def _rollout(ctx, frames, p, window, thr=None):
    """-> key mask; thr "auto": a DWP threshold inside the observed MSE range"""
    from tezip_amd import _lib
    cfg, wts = _model()
    ctx.load_model(cfg, wts)
    ctx.prepare(_lib.pad8(frames.shape[1]), _lib.pad8(frames.shape[2]), max_batch=4)
    if thr == "auto":   # the first of the frames' one-step MSEs (what a threshold of nearly 0 logs: every frame opens a window)
        # under which the job has two windows and two predicted frames
        _, mse = ctx.rollout(frames, p, None, 1e-12, want_mse=True)
        for thr in sorted(float(m) * 1.0001 for m in mse[p + 1:]):
            key, _ = ctx.rollout(frames, p, None, thr)
            if int(key[p:].sum()) >= 2 and int((~key).sum()) >= 2:
                return key
        pytest.fail("no DWP threshold with two windows and two predicted frames: %r" % (mse,))
    key, _ = ctx.rollout(frames, p, window, thr)
    return key


# ------------------------------------------------------------------------------------------------ 1. the kernel alone
def _stacks(nframes, fe, seed, zero_frames=()):
    """orig, d, q with predictions outside [0, 255] on both sides, so that both clamps fire, and q off d by up to 6"""
    rng = np.random.default_rng(seed)
    orig = rng.integers(0, 256, (nframes, fe)).astype(np.uint8)
    orig[rng.random((nframes, fe)) < 0.1] = 0
    orig[rng.random((nframes, fe)) < 0.1] = 255
    xh = rng.integers(-20, 276, (nframes, fe))
    d = (xh - orig).astype(np.int16)
    q = (d + rng.integers(-6, 7, (nframes, fe)) * (rng.random((nframes, fe)) < 0.7)).astype(np.int16)
    for f in zero_frames:
        d[f] = 0
        q[f] = 0
    return orig, d, q


SEAM_CASES = [   # nframes, frame elements, all-zero frames
    (3, 21 * 30 * 3, (1,)),          # frame ends inside 16-byte loads
    (5, 1, ()),
    (37, 1, (0, 36)),
    (1, 21 * 30 * 3, ()),
    (1, 5, ()),                      # fewer elements than one lane's load
    (5, 72 * 88 * 3, (0, 3)),        # 95040 elements: 47 tiles, several workgroups
]


@pytest.mark.parametrize("nframes,fe,zero", SEAM_CASES)
def test_bound_err_equals_its_slow_statement(ctx, nframes, fe, zero):
    import torch
    from tezip_amd import target
    orig, d, q = _stacks(nframes, fe, seed=nframes * 131 + fe, zero_frames=zero)
    want = target.errors_of(orig, d, q)
    if nframes * fe > 100:
        r = orig.astype(np.int64) + d - q
        assert (r < 0).any() and (r > 255).any() and want[:, 0].sum() > 0   # both clamps fire
        assert all(tuple(want[f]) == (0, 0, 0) for f in zero)
    np.testing.assert_array_equal(_records(ctx.bound_err(orig, d, q, nframes, fe)), want)   # host stacks (staged, aligned)
    # device stacks at every kind of alignment: a head in front of the first aligned element, and no common alignment at all
    n = nframes * fe
    for off_o, off_d, off_q in ((0, 0, 0), (3, 3, 3), (5, 5, 13), (1, 2, 2), (0, 0, 4), (7, 7, 7)):
        to = torch.zeros(n + 16, dtype=torch.uint8, device="cuda")
        td = torch.zeros(n + 16, dtype=torch.int16, device="cuda")
        tq = torch.zeros(n + 16, dtype=torch.int16, device="cuda")
        to[off_o: off_o + n] = torch.from_numpy(orig.reshape(-1)).cuda()
        td[off_d: off_d + n] = torch.from_numpy(d.reshape(-1)).cuda()
        tq[off_q: off_q + n] = torch.from_numpy(q.reshape(-1)).cuda()
        torch.cuda.synchronize()
        got = ctx.bound_err(to[off_o: off_o + n], td[off_d: off_d + n], tq[off_q: off_q + n], nframes, fe)
        np.testing.assert_array_equal(_records(got), want, err_msg="offsets %r" % ((off_o, off_d, off_q),))


GRAY_SEAM_CASES = [(3, 21 * 30 * 3, (1,)), (4, 3, ()), (1, 6, ()), (1, 21 * 30 * 3, ()), (5, 72 * 88 * 3, (0, 3))]


@pytest.mark.parametrize("nframes,fe,zero", GRAY_SEAM_CASES)
def test_bound_err_of_a_one_channel_payload(ctx, nframes, fe, zero):
    """gray originals, deltas that differ between the channels: channel 0's reconstruction in all three channels"""
    import torch
    from tezip_amd import _lib, target
    orig, d, q = _stacks(nframes, fe, seed=nframes * 17 + fe, zero_frames=zero)
    orig = np.repeat(orig[:, 0::3], 3, axis=1)                     # three equal channels
    want = target.errors_of(orig, d, q, channels=1)
    n = nframes * fe
    if n > 100:
        assert (want != target.errors_of(orig, d, q)).any() and want[:, 0].sum() > 0   # not the three-channel records
        assert all(tuple(want[f]) == (0, 0, 0) for f in zero)
    try:
        ctx.set_payload_channels(1)
        np.testing.assert_array_equal(_records(ctx.bound_err(orig, d, q, nframes, fe)), want)
        for off_o, off_d, off_q in ((0, 0, 0), (3, 3, 3), (5, 5, 13), (1, 2, 2), (0, 0, 4), (7, 7, 7), (6, 6, 6)):
            to = torch.zeros(n + 16, dtype=torch.uint8, device="cuda")
            td = torch.zeros(n + 16, dtype=torch.int16, device="cuda")
            tq = torch.zeros(n + 16, dtype=torch.int16, device="cuda")
            to[off_o: off_o + n] = torch.from_numpy(orig.reshape(-1)).cuda()
            td[off_d: off_d + n] = torch.from_numpy(d.reshape(-1)).cuda()
            tq[off_q: off_q + n] = torch.from_numpy(q.reshape(-1)).cuda()
            torch.cuda.synchronize()
            got = ctx.bound_err(to[off_o: off_o + n], td[off_d: off_d + n], tq[off_q: off_q + n], nframes, fe)
            np.testing.assert_array_equal(_records(got), want, err_msg="offsets %r" % ((off_o, off_d, off_q),))
        out = np.zeros(2, _lib.QUALITY_DTYPE)
        assert ctx.lib.tz_bound_err(ctx.h, orig.ctypes.data, d.ctypes.data, q.ctypes.data, 1, 4, out.ctypes.data) == -1   # no whole pixels
    finally:
        ctx.set_payload_channels(3)


def test_bound_err_of_nothing(ctx):
    from tezip_amd import _lib
    e8, e16 = np.zeros(0, np.uint8), np.zeros(0, np.int16)
    assert len(ctx.bound_err(e8, e16, e16, 0, 1890)) == 0
    assert _records(ctx.bound_err(e8, e16, e16, 3, 0)).tolist() == [[0, 0, 0]] * 3
    out = np.full(2, 7, _lib.QUALITY_DTYPE)
    assert ctx.lib.tz_bound_err(ctx.h, None, None, None, -1, 8, out.ctypes.data) == 0 and (out["sse"] == 7).all()   # nothing is done
    assert ctx.lib.tz_bound_err(ctx.h, None, None, None, 2, 8, out.ctypes.data) == -1


# --------------------------------------------------------------------------- 2. a probe is encode + encode_quality
BOUNDS = [("abs", [k / 2]) for k in (0, 1, 2, 5, 16, 64, 510)] + [("rel", [0.01]), ("absrel", [3.0, 0.02]), ("pwrel", [0.1])]


def _probe_equals_encode(ctx):
    some = 0
    for mode, bound in BOUNDS:
        got = _records(ctx.bound_probe(mode, bound))
        payload, table, _ = ctx.encode(mode, bound, True)
        want = _records(ctx.encode_quality(payload, table))
        np.testing.assert_array_equal(got, want, err_msg="%s %r" % (mode, bound))
        some += int(want[:, 0].sum() > 0)
    assert not _records(ctx.bound_probe("abs", [0.0])).any()
    assert some >= 6   # (the jobs exercise the lossy path)


PROBE_JOBS = {   # frames, warm_up, window, threshold, payload channels, delta stride
    "blobs_p2_w3": (_blobs, 2, 3, None, 3, 0),
    "scene_p0_w4": (_scene, 0, 4, None, 3, 0),
    "scene_p0_dwp": (_scene, 0, None, "auto", 3, 0),
    "scene160_p1": (_scene160, 1, 3, None, 3, 0),   # several quantiser tiles per slab
    "blobs_one_channel": (_blobs, 2, 3, None, 1, 0),
    "scene_channel_stride": (_scene, 0, 4, None, 3, 1),
}


@pytest.mark.parametrize("job", sorted(PROBE_JOBS))
def test_probe_equals_encode_and_encode_quality(ctx, job):
    make, p, window, thr, channels, stride = PROBE_JOBS[job]
    frames = make()
    try:
        ctx.set_payload_channels(channels)
        ctx.set_delta_stride(stride)
        key = _rollout(ctx, frames, p, window, thr)
        if thr is not None:
            assert int(key[p:].sum()) >= 2, "the threshold gives at least two windows"
        _nontrivial(ctx, frames, key)
        _probe_equals_encode(ctx)
        if channels == 1:   # the one-channel job is another job than the three-channel one on the same rollout
            one = _records(ctx.bound_probe("abs", [8.0]))
            ctx.set_payload_channels(3)
            three = _records(ctx.bound_probe("abs", [8.0]))
            print("%s abs 8: sse one channel %d, three channels %d" % (job, one[:, 0].sum(), three[:, 0].sum()))
            assert (one != three).any()
        else:   # behind the rollout of a mostly black stack the decoder's clamp matters: the predictions are positive there,
            # the runs' midpoints lie on both sides of them, and what falls below 0 is clamped (translating_scene's samples
            # are mid-range: at this bound nothing of it leaves [0, 255], and the kernel's clamps are the seam tests')
            _, _, d = ctx.encode("abs", [0.0], True, want_delta=True)
            d = d.astype(np.int64)
            _, _, q = ctx.encode("abs", [32.0], True, want_delta=True)
            r = frames.astype(np.int64) + d - q
            print("%s abs 32: %d samples clamped at 0, %d at 255" % (job, (r < 0).sum(), (r > 255).sum()))
            assert (r < 0).any() or (frames == 0).mean() < 0.5
    finally:
        ctx.set_payload_channels(3)
        ctx.set_delta_stride(0)


@pytest.mark.parametrize("channels", [3, 1])
def test_probes_leave_the_context_as_it_was(ctx, channels):
    frames = _blobs()
    try:
        ctx.set_payload_channels(channels)
        _leave_as_it_was(ctx, frames)
    finally:
        ctx.set_payload_channels(3)


def _leave_as_it_was(ctx, frames):
    _rollout(ctx, frames, 2, 3)
    host, table0, _ = ctx.encode("abs", [2.0], True)            # what an encode returns without probes
    host = np.array(host, copy=True)
    _, table, _ = ctx.encode("abs", [2.0], True, payload="resident")
    q0 = _records(ctx.encode_quality("resident", table))
    before = ctx.payload_get(0, host.size).copy()
    preds = ctx.get_predictions().copy()
    for mode, bound in BOUNDS:
        ctx.bound_probe(mode, bound)
    np.testing.assert_array_equal(ctx.payload_get(0, host.size), before)
    np.testing.assert_array_equal(_records(ctx.encode_quality("resident", table)), q0)   # (still resident: enc_kind untouched)
    np.testing.assert_array_equal(ctx.get_predictions(), preds)
    again, t2, _ = ctx.encode("abs", [2.0], True)
    np.testing.assert_array_equal(again, host)
    np.testing.assert_array_equal(t2, table0)


def test_probe_state_and_argument_errors():
    from tezip_amd import _lib
    c = _lib.Context(0)
    try:
        out = np.zeros(16, _lib.QUALITY_DTYPE)
        assert c.lib.tz_bound_probe(c.h, 0, 2.0, 0.0, out.ctypes.data) == -4   # no rollout
        frames = _blobs()
        key = _rollout(c, frames, 2, 3)
        assert c.lib.tz_bound_probe(c.h, 0, 2.0, 0.0, out.ctypes.data) == 0
        assert c.lib.tz_bound_probe(c.h, 0, 2.0, 0.0, None) == -1
        assert c.lib.tz_bound_probe(c.h, 4, 2.0, 0.0, out.ctypes.data) == -1
        assert c.lib.tz_bound_probe(c.h, 0, float("nan"), 0.0, out.ctypes.data) == -1
        assert c.lib.tz_bound_probe(c.h, 1, -0.5, 0.0, out.ctypes.data) == -1
        assert c.lib.tz_bound_probe(c.h, 0, 2.0, 0.0, out.ctypes.data) == 0        # a refused call leaves it usable
        c.set_payload_channels(1)
        assert c.lib.tz_bound_probe(c.h, 0, 2.0, 0.0, out.ctypes.data) == 0        # a gray stack
        colour = _scene()
        _rollout(c, colour, 0, 4)
        assert c.lib.tz_bound_probe(c.h, 0, 2.0, 0.0, out.ctypes.data) == -1       # colour: refused as tz_encode refuses it
        c.set_payload_channels(3)
        assert c.lib.tz_bound_probe(c.h, 0, 2.0, 0.0, out.ctypes.data) == 0
        key = _rollout(c, frames, 2, 3)
        keys = np.where(key[:, None, None, None], frames, 0).astype(np.uint8)
        c.rollout_decode(keys, 2)     # a decoder rollout
        assert c.lib.tz_bound_probe(c.h, 0, 2.0, 0.0, out.ctypes.data) == -4
    finally:
        c.close()


# ------------------------------------------------------------------------------- 3. the search against the oracle
def _oracle_probe(frames, preds, key, p, channels=3):
    """k -> SSE(k) from the Python oracle: delta_group, error_bound per frame and channel as the encoder applies them
    (group 0 of a job with warm-up is not quantised), reconstruct_int from the bases the decoder has.  channels 1: the
    decoder of a one-channel payload reconstructs channel 0 and writes the sample to all three channels."""
    from oracle import oracle as O
    nt, h, w, _ = frames.shape
    starts = sorted({0} | {i for i in range(p, nt) if key[i]})
    groups = list(zip(starts, starts[1:] + [nt]))
    memo = {}

    def probe(k):
        if k not in memo:
            sse = 0
            for g, (s, e) in enumerate(groups):
                orig = frames[s:e].astype(np.int64)
                d = O.delta_group(preds[s:e], frames[s:e])
                q = d.copy()
                if not (p != 0 and g == 0):
                    for j in range(1, e - s):
                        for c in range(3):
                            q[j, :, :, c] = O.error_bound(orig[j, :, :, c], d[j, :, :, c], "abs", [k / 2])
                base = (np.asarray(preds[s:e], np.float32)[:, :h, :w] * np.float32(255.0)).astype(np.int64)
                base[0] = orig[0]                          # a group starts with a key frame: its own bytes
                rec = O.reconstruct_int(base, q).astype(np.int64)
                if channels == 1:
                    rec = np.repeat(rec[..., :1], 3, axis=-1)
                sse += int(((rec - orig) ** 2).sum())
            memo[k] = sse
        return memo[k]

    return probe


@pytest.mark.parametrize("job", ["blobs_p2_w3", "scene_p0_w4", "blobs_one_channel"])
def test_search_on_the_gpu_equals_the_search_over_the_oracle(ctx, job):
    make, p, window, thr, channels, _ = PROBE_JOBS[job]
    try:
        ctx.set_payload_channels(channels)
        _search_equals_oracle(ctx, job, make(), p, window, thr, channels)
    finally:
        ctx.set_payload_channels(3)


def _search_equals_oracle(ctx, job, frames, p, window, thr, channels):
    from tezip_amd import target
    key = _rollout(ctx, frames, p, window, thr)
    _nontrivial(ctx, frames, key)
    cpu = _oracle_probe(frames, ctx.get_predictions(), key, p, channels)
    gpu_memo = {}

    def gpu(k):
        if k not in gpu_memo:
            gpu_memo[k] = int(ctx.bound_probe("abs", [k / 2])["sse"].sum())
        return gpu_memo[k]

    for T in (30, 40, 50):
        limit = target.sse_limit(T, frames.size)
        k_gpu, trace_gpu = target.search(gpu, limit)
        k_cpu, trace_cpu = target.search(cpu, limit)
        print("%s T=%d limit=%d k=%d/%d" % (job, T, limit, k_gpu, k_cpu))
        assert trace_gpu == trace_cpu and k_gpu == k_cpu
        assert 1 <= k_gpu <= 509, "a target this job meets losslessly or never: the case shows nothing"
        assert gpu(k_gpu) <= limit < gpu(k_gpu + 1)


# ---------------------------------------------------------------------------------------------------------- 4. CLI
def _cli(args, timeout=300):
    return subprocess.run(["timeout", "-k", "10", str(timeout), sys.executable, "-m", "tezip_amd.tezip"] + args, cwd=ROOT,
                          capture_output=True, text=True, timeout=timeout + 30)


@pytest.fixture(scope="module")
def cli_job(tmp_path_factory):
    """model directory, image directory, names and frames of the first job, on disk once for both CLI tests"""
    from PIL import Image
    from tezip_amd import weights
    root = tmp_path_factory.mktemp("target_cli")
    frames = _blobs()
    cfg, wts = _model()
    mdir = str(root / "model")
    weights.save_model(mdir, cfg, wts, 24, 32)
    ddir = root / "data"
    ddir.mkdir()
    names = ["f_%03d.png" % t for t in range(len(frames))]
    for t, n in enumerate(names):
        Image.fromarray(frames[t]).save(ddir / n)
    return mdir, str(ddir), names, frames


JOB = ["-p", "2", "-w", "3"]


def _images(directory, names):
    from PIL import Image
    return np.stack([np.asarray(Image.open(os.path.join(directory, n)).convert("RGB")) for n in names]).astype(np.int64)


def test_cli_target_psnr_is_the_abs_job_it_finds(tmp_path, cli_job):
    from tezip_amd import target
    mdir, ddir, names, frames = cli_job
    found, plain = str(tmp_path / "comp_t"), str(tmp_path / "comp")
    r = _cli(["-c", mdir, ddir, found] + JOB + ["--target-psnr", "40", "--report"])
    assert r.returncode == 0, r.stdout + r.stderr
    doc = json.load(open(os.path.join(found, "bound_search.json")))
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("target: ")]
    assert line == [target.stdout_line(doc)] and "abs" in r.stdout.splitlines()
    limit = target.sse_limit(40, frames.size)
    k = doc["result"]["k"]
    assert doc["sse_limit"] == limit and doc["samples"] == frames.size and doc["target_psnr_db"] == 40.0 and 1 <= k <= 509
    assert doc["result"]["bound"] == k / 2 and 1 <= len(doc["trace"]) <= 9
    by_k = {t["k"]: t for t in doc["trace"]}
    assert all(t["pass"] == (t["sse"] <= limit) and t["bound"] == t["k"] / 2 for t in doc["trace"])
    assert by_k[k]["pass"] and by_k[k]["sse"] == doc["result"]["sse"] and not by_k[k + 1]["pass"]   # the guarantee
    r = _cli(["-c", mdir, ddir, plain] + JOB + ["-m", "abs", "-b", repr(k / 2), "--report"])
    assert r.returncode == 0, r.stdout + r.stderr
    assert sorted(os.listdir(plain)) == ["entropy.dat", "filename.txt", "key_frame.dat", "quality.json", "tezip_amd.json"]
    assert sorted(os.listdir(found)) == sorted(os.listdir(plain) + ["bound_search.json"])
    for n in ("filename.txt", "key_frame.dat", "entropy.dat", "tezip_amd.json", "quality.json"):
        assert open(os.path.join(found, n), "rb").read() == open(os.path.join(plain, n), "rb").read(), n
    quality = json.load(open(os.path.join(found, "quality.json")))
    assert sum(f["sse"] for f in quality["per_frame"]) == doc["result"]["sse"] <= limit
    udir, udir0 = str(tmp_path / "dec_t"), str(tmp_path / "dec")
    for src, dst in ((found, udir), (plain, udir0)):
        r = _cli(["-u", mdir, src, dst])
        assert r.returncode == 0, r.stdout + r.stderr
    assert sorted(os.listdir(udir)) == names
    for n in names:   # -u ignores bound_search.json
        assert open(os.path.join(udir, n), "rb").read() == open(os.path.join(udir0, n), "rb").read(), n
    assert int(((_images(udir, names) - frames) ** 2).sum()) == doc["result"]["sse"]


def test_cli_target_psnr_with_the_opt_in_formats(tmp_path, cli_job):
    """--coder huffd --key-coder huffg --gray --sdelta channel --digests: the same search, and the job decodes and verifies"""
    from tezip_amd import target
    mdir, ddir, names, frames = cli_job
    other, udir = str(tmp_path / "comp_o"), str(tmp_path / "dec_o")
    r = _cli(["-c", mdir, ddir, other] + JOB + ["--target-psnr", "40", "--coder", "huffd", "--key-coder", "huffg", "--gray",
                                                "--sdelta", "channel", "--digests"])
    assert r.returncode == 0, r.stdout + r.stderr
    doc = json.load(open(os.path.join(other, "bound_search.json")))
    limit = target.sse_limit(40, frames.size)
    assert doc["sse_limit"] == limit and 1 <= doc["result"]["k"] <= 509 and doc["result"]["sse"] <= limit
    assert sorted(os.listdir(other)) == ["bound_search.json", "entropy.dat", "filename.txt", "frame_digests.json", "key_frame.dat",
                                         "tezip_amd.json"]
    r = _cli(["-u", mdir, other, udir, "--verify", "require"])
    assert r.returncode == 0 and "verified: %d frames" % len(names) in r.stdout, r.stdout + r.stderr
    assert int(((_images(udir, names) - frames) ** 2).sum()) == doc["result"]["sse"]   # what the search said the bound does
