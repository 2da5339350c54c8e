"""Contexts on concurrent threads (include/tezip_hip.h: a context is not thread-safe, distinct contexts are independent).

The rule of every test: a job run on its own context, on a thread, at the same time as other jobs, gives byte for byte
what the same job gives run alone on one thread.  Each test runs the serial baseline and the concurrent run in the same
process and, where the job has one, checks an independent reference too: the C oracle for lossless jobs and for the
predictor at the shapes tests/test_gpu_parity.py and tests/test_gpu_wino.py hold bit-exact, the mode's error bound and
numpy's statistics of the decoded frames for lossy jobs.

_lib binds the library with ctypes.CDLL, which releases the GIL for every call, so these Python threads really do
overlap inside the library.  No test opens more than 4 contexts at once.  State the library keeps beyond one context:
the k_wino attribute flags (launch_wino_t), the function-local static env knobs, and the GPU itself, which a
neighbour's launches slow down (epart_measure times fused against split steps)."""
import concurrent.futures
import gc
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from conftest import ROOT
from oracle import coracle
from oracle import oracle as O
from tezip_amd import _lib, synth
from tezip_amd.prednet import PredNetConfig

pytestmark = pytest.mark.gpu

SMALL = PredNetConfig(stack_sizes=(3, 16, 32))
FULL = PredNetConfig()
MAX_CONTEXTS = 4
JOIN_S = 240


def _concurrently(fns, timeout=JOIN_S):
    """Run each fn on a thread of its own, all released together, and return their results in order.  A thread that
    raises fails the test with its own exception; threads that do not finish within `timeout` fail it too."""
    assert 2 <= len(fns) <= MAX_CONTEXTS
    gc.collect()                                  # (contexts other tests dropped without close() go now, not mid-test)
    start = threading.Barrier(len(fns))

    def run(fn):
        start.wait(timeout=60)
        return fn()

    ex = concurrent.futures.ThreadPoolExecutor(max_workers=len(fns))
    try:
        futs = [ex.submit(run, fn) for fn in fns]
        done, pending = concurrent.futures.wait(futs, timeout=timeout, return_when=concurrent.futures.FIRST_EXCEPTION)
        for f in futs:
            if f in done and f.exception() is not None:
                start.abort()                     # (a thread still at the barrier gives up instead of waiting for ever)
                raise f.exception()
        if pending:
            done, pending = concurrent.futures.wait(pending, timeout=timeout)
        assert not pending, "%d of %d threads did not finish within %d s" % (len(pending), len(fns), 2 * timeout)
        return [f.result() for f in futs]
    finally:
        ex.shutdown(wait=False, cancel_futures=True)


def _serially(fns):
    gc.collect()
    return [fn() for fn in fns]


def _assert_same(got, want, what):
    assert got.keys() == want.keys(), what
    for k in want:
        if want[k] is None:
            assert got[k] is None, (what, k)
        elif isinstance(want[k], np.ndarray):
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
            assert np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)), "%s: %s differs from the serial run" % (what, k)
        else:
            assert got[k] == want[k], (what, k, got[k], want[k])


def _numpy_stats(dec, frames):
    d = (dec.astype(np.int64) - frames.astype(np.int64)).reshape(len(frames), -1)
    return np.stack([(d * d).sum(1), np.abs(d).max(1), (d != 0).sum(1)], axis=1)


def _records(q):
    return np.stack([q["sse"].astype(np.int64), q["max_abs"].astype(np.int64), q["n_changed"].astype(np.int64)], axis=1)


def _worst_tolerance(mode, bound, frames):
    """Per element, an upper bound of the tolerance E the quantiser may use (compress.py:28-48): a decoded element is
    within E + 1 of the original (the run value lies in [d - E, d + E] and is truncated towards 0; the clamp only
    shrinks the error)."""
    if mode == "abs":
        return np.full(frames.shape, abs(bound[0]))
    if mode == "rel":
        return np.full(frames.shape, 255.0 * bound[0])
    if mode == "absrel":
        return np.full(frames.shape, min(abs(bound[0]), 255.0 * bound[1]))
    return frames.astype(np.float64) * bound[0]


class _OraclePredictor:
    def __init__(self, net):
        self.net = net

    def c0(self, hp, wp):
        return self.net.c0()

    def next(self, frame):
        return self.net.next(np.asarray(frame, dtype=np.float32))


# ------------------------------------------------------------------------------ 2. different models and shapes at once
MODELS = [  # stack_sizes, R_stack_sizes, hp, wp, bias: bit-exact to the C oracle under TZ-PA2 in tests/test_gpu_wino.py
    ((3, 48, 96, 192), None, 64, 64, 0.1),
    ((3, 48, 96, 192), None, 24, 40, 0.3),
    ((3, 32, 64), (3, 48, 32), 40, 56, 0.25),
    ((3, 16), None, 24, 40, 0.25),
]


def _predictor(stack, rstack, hp, wp, bias):
    def job():
        cfg = PredNetConfig(stack_sizes=stack, R_stack_sizes=rstack)
        w = cfg.init_weights(seed=11, bias_scale=bias)
        frames = np.random.default_rng(hp * 31 + wp).integers(0, 256, (3, hp, wp, 3)).astype(np.float32) / np.float32(255)
        ctx = _lib.Context(0)
        try:
            ctx.load_model(cfg, w)
            ctx.set_contract(2)
            ctx.prepare(hp, wp, max_batch=2)
            c0 = ctx.predict_c0()
            nxt = ctx.predict_next(frames)            # 3 frames through a batch of 2
            again = ctx.predict_next(nxt[:1])
            return dict(c0=c0, next=nxt, again=again, contract=ctx.get_contract())
        finally:
            ctx.close()
    return job


def test_different_models_and_shapes_at_once():
    """Four models whose k_wino launches are different template instantiations (column-block widths, upsampled or not)
    are loaded, prepared and run at the same time.  The concurrent run goes FIRST here, and this test is the first of the
    file: in a process where no test has launched these instantiations yet, their first launches race on launch_wino_t's
    attribute flags."""
    jobs = [_predictor(*m) for m in MODELS]
    got = _concurrently(jobs)
    base = _serially(jobs)
    for m, g, b in zip(MODELS, got, base):
        _assert_same(g, b, "model %r" % (m,))
        stack, rstack, hp, wp, bias = m
        cfg = PredNetConfig(stack_sizes=stack, R_stack_sizes=rstack)
        w = cfg.init_weights(seed=11, bias_scale=bias)
        net = coracle.CPredNet(w, cfg.stack_sizes, cfg.R_stack_sizes, hp, wp).set_contract(2)
        frames = np.random.default_rng(hp * 31 + wp).integers(0, 256, (3, hp, wp, 3)).astype(np.float32) / np.float32(255)
        assert g["contract"] == 2
        np.testing.assert_array_equal(g["c0"], net.c0())
        for i in range(3):
            np.testing.assert_array_equal(g["next"][i], net.next(frames[i]), err_msg="%r frame %d" % (m, i))
        np.testing.assert_array_equal(g["again"][0], net.next(g["next"][0]))


# ------------------------------------------------------------------------------------------------- 1. mixed pipelines
def _pipeline(nt, h, w, p, window, thr, mode, bound, entropy, shuffle, seed):
    """rollout -> encode (+ encode_quality) -> rollout_decode -> decode, in a context of its own."""
    def job():
        frames = synth.translating_scene(nt, h, w, seed=seed)
        wts = SMALL.init_weights(seed=seed, bias_scale=0.2)
        ctx = _lib.Context(0)
        try:
            ctx.load_model(SMALL, wts)
            ctx.prepare(_lib.pad8(h), _lib.pad8(w), max_batch=4)
            t = thr
            if t in ("auto", "above"):            # DWP: the median of the probed MSEs (on these scenes the MSE falls with
                _, mse = ctx.rollout(frames, p, None, 1e9, want_mse=True)      # depth, so every frame restarts a window),
                t = float(np.median(mse[p + 1:])) if t == "auto" else 2.0 * float(mse[p + 1:].max())   # or one long window
            key, _ = ctx.rollout(frames, p, window, t)
            pred = ctx.get_predictions()
            payload, table, _ = ctx.encode(mode, bound, entropy, shuffle=shuffle)
            payload = np.array(payload, copy=True)
            q = _records(ctx.encode_quality(payload, table, shuffle=shuffle))
            keys = np.where(key[:, None, None, None], frames, 0).astype(np.uint8)
            kd = ctx.rollout_decode(keys, p)
            sym = ctx.byte_unshuffle(payload.view(np.uint8)) if shuffle else payload
            dec = np.array(ctx.decode(sym, table), copy=True)
            return dict(key=key, kd=kd, pred=pred, payload=payload, table=table, quality=q, dec=dec, thr=t)
        finally:
            ctx.close()
    return job


PIPELINES = [  # nt, h, w, p, window, thr, mode, bound, entropy, shuffle, seed
    (11, 21, 30, 2, 4, None, "abs", [0.0], True, False, 9),          # padded, lossless, warm-up 2: the C oracle below
    (12, 16, 24, 0, 5, None, "abs", [4.0], True, False, 9),          # lossy, warm-up 0: the C oracle below
    (12, 64, 64, 0, None, "above", "rel", [5e-2], False, True, 7),   # DWP, one window, no table, byte shuffle
    (12, 61, 90, 2, 3, None, "absrel", [3.0, 0.05], True, False, 3),
    (12, 64, 64, 2, None, "auto", "pwrel", [0.05], True, True, 4),
    (13, 61, 90, 0, 4, None, "abs", [2.0], False, False, 5),
    (12, 64, 96, 2, 5, None, "abs", [0.0], False, True, 6),          # lossless, no table, shuffle
]
ORACLE_CHECKED = (0, 1)


def _pipeline_oracle(nt, h, w, p, window, thr, mode, bound, entropy, shuffle, seed, res):
    """The C oracle's whole job (tests/test_gpu_parity.py CASES holds these shapes bit-exact)."""
    frames = synth.translating_scene(nt, h, w, seed=seed)
    wts = SMALL.init_weights(seed=seed, bias_scale=0.2)
    pred = _OraclePredictor(coracle.CPredNet(wts, SMALL.stack_sizes, SMALL.R_stack_sizes, _lib.pad8(h), _lib.pad8(w)))
    ref = O.compress_oracle(frames, p, window, None, mode, bound, pred, entropy)
    payload, table, _, _ = O.parse_stream(ref["stream"])
    np.testing.assert_array_equal(res["key"], ref["key"])
    np.testing.assert_array_equal(res["payload"], payload)
    if entropy:
        np.testing.assert_array_equal(res["table"], table)
    np.testing.assert_array_equal(res["dec"], O.decode_stream(ref["stream"], ref["key_frame"], pred))


def test_mixed_pipelines_on_concurrent_contexts():
    jobs = [_pipeline(*spec) for spec in PIPELINES]
    base = _serially(jobs)
    for i, (spec, res) in enumerate(zip(PIPELINES, base)):        # the baseline itself against independent references
        nt, h, w, p, window, thr, mode, bound, entropy, shuffle, seed = spec
        frames = synth.translating_scene(nt, h, w, seed=seed)
        np.testing.assert_array_equal(res["kd"], res["key"])
        np.testing.assert_array_equal(res["quality"], _numpy_stats(res["dec"], frames), err_msg="job %d" % i)
        if mode == "abs" and bound[0] == 0:
            np.testing.assert_array_equal(res["dec"], frames, err_msg="job %d" % i)
        else:
            err = np.abs(res["dec"].astype(np.int64) - frames.astype(np.int64))
            assert (err < _worst_tolerance(mode, bound, frames) + 1).all(), "job %d breaks its %s bound" % (i, mode)
            if not res["key"][p + 1:].all():      # (a frame that is not a key frame carries quantisation error)
                assert err.any(), "job %d: the lossy path did not run" % i
        if i in ORACLE_CHECKED:
            _pipeline_oracle(*spec, res)
    # at most MAX_CONTEXTS jobs at once: two rounds, each mixing SWP / DWP, padded / unpadded, table / none, shuffle
    for group in ([0, 2, 3, 4], [1, 5, 6]):
        got = _concurrently([jobs[i] for i in group])
        for i, res in zip(group, got):
            _assert_same(res, base[i], "job %d" % i)


# ------------------------------------------------------------------------------------------ 3. different contracts
def _contract_job(contract, frames, p, window):
    nt, h, w, _ = frames.shape

    def job():
        ctx = _lib.Context(0)
        try:
            ctx.load_model(FULL, FULL.init_weights(seed=6, bias_scale=0.1))
            ctx.set_contract(contract)
            ctx.prepare(_lib.pad8(h), _lib.pad8(w), max_batch=4)
            key, _ = ctx.rollout(frames, p, window)
            stamp = ctx.rollout_contract()
            pred = ctx.get_predictions()
            payload, table, _ = ctx.encode("abs", [0.0], True)
            payload = np.array(payload, copy=True)
            keys = np.where(key[:, None, None, None], frames, 0).astype(np.uint8)
            ctx.rollout_decode(keys, p)
            stamp_dec = ctx.rollout_contract()
            dec = np.array(ctx.decode(payload, table), copy=True)
            return dict(key=key, pred=pred, payload=payload, table=table, dec=dec, stamp=stamp, stamp_dec=stamp_dec,
                        contract=ctx.get_contract())
        finally:
            ctx.close()
    return job


def test_different_contracts_at_once():
    """TZ-PA1 on one context, TZ-PA2 on another, the same lossless job of the FULL model at 64x96 (where the two contracts
    differ in their bits, tests/test_gpu_contract.py).  Neither may adopt the other's contract."""
    frames = synth.translating_scene(9, 64, 96, seed=21)
    jobs = [_contract_job(1, frames, 1, 4), _contract_job(2, frames, 1, 4), _contract_job(1, frames, 0, 3),
            _contract_job(2, frames, 0, 3)]
    base = _serially(jobs)
    got = _concurrently(jobs)
    for i, (g, b) in enumerate(zip(got, base)):
        _assert_same(g, b, "job %d" % i)
        want = 1 + i % 2
        assert g["contract"] == g["stamp"] == g["stamp_dec"] == want, (i, g["contract"], g["stamp"], g["stamp_dec"])
        np.testing.assert_array_equal(g["dec"], frames)       # lossless
    # the two contracts really differ here, so a context that took the other's would show above
    assert not np.array_equal(base[0]["pred"], base[1]["pred"])


# -------------------------------------------------------------------------- 4. E-part measurement under contention
_EPART_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from tezip_amd import _lib, synth
from tezip_amd.prednet import PredNetConfig
FULL = PredNetConfig()
frames = synth.turbulence(4, 512, 512, seed=9)
ctx = _lib.Context(0)
ctx.load_model(FULL, FULL.init_weights(seed=123))
ctx.prepare(512, 512, max_batch=1)
assert ctx.get_contract() == 2
key, _ = ctx.rollout(frames, 0, 4)
payload, table, _ = ctx.encode("abs", [1.0], True)
np.savez(sys.argv[2], key=key, pred=ctx.get_predictions(), payload=np.array(payload), table=table)
ctx.close()
"""


def _epart_job():
    def job():
        frames = synth.turbulence(4, 512, 512, seed=9)
        ctx = _lib.Context(0)
        try:
            ctx.load_model(FULL, FULL.init_weights(seed=123))
            ctx.prepare(512, 512, max_batch=1)    # one window of 512x512: the measurement runs (test_gpu_epart.py)
            assert ctx.get_contract() == 2
            key, _ = ctx.rollout(frames, 0, 4)
            payload, table, _ = ctx.encode("abs", [1.0], True)
            return dict(key=key, pred=ctx.get_predictions(), payload=np.array(payload, copy=True), table=table)
        finally:
            ctx.close()
    return job


def test_epart_measurement_under_contention(tmp_path):
    """TEZIP_EPART unset: fresh contexts measure fused against split steps while their neighbours load the GPU, so the
    cached choice may differ from run to run (it is not asserted on).  The bits must not: they equal a run forced fused
    (TEZIP_EPART=0) and one forced split (=1), each in a child process of its own, run one at a time after the threads."""
    assert "TEZIP_EPART" not in os.environ
    jobs = [_epart_job() for _ in range(3)]
    base = _serially(jobs[:1])[0]
    got = _concurrently(jobs)
    for i, g in enumerate(got):
        _assert_same(g, base, "context %d" % i)
    for mode in ("0", "1"):
        env = dict(os.environ, TEZIP_EPART=mode)
        out = str(tmp_path / ("epart_%s.npz" % mode))
        r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, "-c", _EPART_CHILD, ROOT, out], env=env, cwd=ROOT,
                           capture_output=True, text=True, timeout=270)
        assert r.returncode == 0, "TEZIP_EPART=%s child: %d\n%s" % (mode, r.returncode, (r.stdout + r.stderr)[-3000:])
        forced = dict(np.load(out))
        _assert_same(forced, base, "TEZIP_EPART=%s" % mode)


# ------------------------------------------------------------------------------------------------- 5. streaming at once
def _stream_encoder(frames, pinned, piece=5):
    """frames_begin / frames_put in pieces, rollout from the staged stack, resident payload delivered by payload_get in
    pieces -- from pageable host arrays, or from / into pinned_empty buffers."""
    nt, h, w, _ = frames.shape

    def job():
        src = _lib.pinned_copy(frames) if pinned else frames
        ctx = _lib.Context(0)
        try:
            ctx.load_model(SMALL, SMALL.init_weights(seed=3, bias_scale=0.2))
            ctx.prepare(_lib.pad8(h), _lib.pad8(w), max_batch=4)
            ctx.frames_begin(nt, h, w)
            for f0 in range(0, nt, piece):
                ctx.frames_put(f0, src[f0:f0 + piece])
            ctx.frames_fence()
            key, _ = ctx.rollout(None, 1, 4)
            _, table, _ = ctx.encode("abs", [2.0], True, payload="resident")
            n = nt * h * w * 3
            out = _lib.pinned_empty(n, np.int16) if pinned else np.empty(n, np.int16)
            step = n // 3 + 5
            for off in range(0, n, step):
                ctx.payload_get(off, min(step, n - off), out=out[off:off + step])
            return dict(key=key, table=table, payload=np.array(out, copy=True))
        finally:
            ctx.close()
    return job


def _stream_decoder(keys, payload, table, pinned):
    nt, h, w, _ = keys.shape

    def job():
        ks, pl = (_lib.pinned_copy(keys), _lib.pinned_copy(payload)) if pinned else (keys, payload)
        ctx = _lib.Context(0)
        try:
            ctx.load_model(SMALL, SMALL.init_weights(seed=3, bias_scale=0.2))
            ctx.prepare(_lib.pad8(h), _lib.pad8(w), max_batch=4)
            ctx.frames_begin(nt, h, w)
            ctx.frames_put(0, ks[:6])
            ctx.frames_put(6, ks[6:])
            ctx.payload_begin(pl.size)
            step = pl.size // 4 + 3
            for off in range(0, pl.size, step):
                ctx.payload_put(off, pl[off:off + step])
            kd = ctx.rollout_decode(None, 1)
            ctx.decode(None, table, out="resident")
            dec = _lib.pinned_empty((nt, h, w, 3), np.uint8) if pinned else np.empty((nt, h, w, 3), np.uint8)
            for f0 in range(0, nt, 4):
                c = min(4, nt - f0)
                ctx.decoded_get(f0, c, out=dec[f0:f0 + c])
            return dict(kd=kd, dec=np.array(dec, copy=True))
        finally:
            ctx.close()
    return job


def _deferred_encoder(seqs):
    """set_payload_deferred(True): each payload's transfer runs under the next sequence's rollout; payload_wait ends it."""
    nt, h, w, _ = seqs[0].shape

    def job():
        ctx = _lib.Context(0)
        try:
            ctx.load_model(SMALL, SMALL.init_weights(seed=3, bias_scale=0.2))
            ctx.prepare(_lib.pad8(h), _lib.pad8(w), max_batch=4)
            ctx.set_payload_deferred(True)
            bufs = [_lib.pinned_empty(nt * h * w * 3, np.int16) for _ in range(2)]
            src = [_lib.pinned_copy(f) for f in seqs]
            out = {}
            for i, f in enumerate(src):
                ctx.rollout(f, 0, 5)
                ctx.payload_wait()
                if i > 0:
                    out["payload%d" % (i - 1)] = np.array(bufs[(i - 1) & 1], copy=True)
                _, out["table%d" % i], _ = ctx.encode("abs", [1.0], True, payload=bufs[i & 1])
            ctx.payload_wait()
            out["payload%d" % (len(seqs) - 1)] = np.array(bufs[(len(seqs) - 1) & 1], copy=True)
            return out
        finally:
            ctx.close()
    return job


def test_streaming_contexts_at_once():
    nt, h, w = 16, 128, 160
    frames = synth.translating_scene(nt, h, w, seed=31)
    seqs = [synth.translating_scene(10, 96, 128, seed=40 + i) for i in range(3)]
    # the decoder's input: a job encoded beforehand (its own check: lossy within the bound, key frames exact)
    enc = _stream_encoder(frames, False)()
    keys = np.where(enc["key"][:, None, None, None], frames, 0).astype(np.uint8)
    jobs = [_stream_encoder(frames, False), _stream_encoder(frames, True),
            _stream_decoder(keys, enc["payload"], enc["table"], False), _deferred_encoder(seqs)]
    base = _serially(jobs)
    dec = base[2]["dec"]
    assert int(np.abs(dec.astype(int) - frames.astype(int)).max()) <= 2
    np.testing.assert_array_equal(dec[enc["key"]], frames[enc["key"]])
    _assert_same(base[1], base[0], "pinned against pageable")
    for i, f in enumerate(seqs):                  # deferred against the blocking form
        c = _lib.Context(0)
        try:
            c.load_model(SMALL, SMALL.init_weights(seed=3, bias_scale=0.2))
            c.prepare(96, 128, max_batch=4)
            c.rollout(f, 0, 5)
            p, t, _ = c.encode("abs", [1.0], True)
            np.testing.assert_array_equal(base[3]["payload%d" % i], p)
            np.testing.assert_array_equal(base[3]["table%d" % i], t)
        finally:
            c.close()
    for round_ in (jobs, [jobs[0], jobs[1], _stream_decoder(keys, enc["payload"], enc["table"], True)]):
        got = _concurrently(round_)
        for i, g in enumerate(got):
            _assert_same(g, base[i], "streaming context %d" % i)


# -------------------------------------------------------------------------- 6. range decode and quality report at once
def test_range_decode_and_quality_report_at_once():
    nt, h, w, p = 16, 64, 96, 1
    frames = synth.translating_scene(nt, h, w, seed=12)
    wts = SMALL.init_weights(seed=12, bias_scale=0.2)
    c = _lib.Context(0)
    try:
        c.load_model(SMALL, wts)
        c.prepare(h, w, max_batch=4)
        key, _ = c.rollout(frames, p, 5)
        payload, table, _ = c.encode("abs", [2.0], True)
        payload = np.array(payload, copy=True)
    finally:
        c.close()
    keys = np.where(key[:, None, None, None], frames, 0).astype(np.uint8)
    ranges = [(0, nt), (0, 1), (3, 9), (6, 7), (11, 16), (nt - 1, nt), (p, p + 3)]

    def ranger():
        ctx = _lib.Context(0)
        try:
            ctx.load_model(SMALL, wts)
            ctx.prepare(h, w, max_batch=4)
            ctx.rollout_decode(keys, p)
            out = {"full": np.array(ctx.decode(payload, table), copy=True)}
            for a, b in ranges:
                ctx.rollout_decode_range(keys, p, a, b - a)
                out["%d:%d" % (a, b)] = np.array(ctx.decode_range(payload, table, a, b - a), copy=True)
            return out
        finally:
            ctx.close()

    def reporter(mode, bound, entropy, shuffle):
        def job():
            ctx = _lib.Context(0)
            try:
                ctx.load_model(SMALL, wts)
                ctx.prepare(h, w, max_batch=4)
                ctx.rollout(frames, p, 4)
                pl, tb, _ = ctx.encode(mode, bound, entropy, payload="resident", shuffle=shuffle)
                q1 = _records(ctx.encode_quality("resident", tb, shuffle=shuffle))
                n = nt * h * w * 3
                host = np.array(ctx.payload_get(0, n), copy=True)
                q2 = _records(ctx.encode_quality(host, tb, shuffle=shuffle))
                return dict(resident=q1, host=q2)
            finally:
                ctx.close()
        return job

    jobs = [ranger, reporter("abs", [2.0], True, False), reporter("rel", [1e-2], False, True),
            reporter("abs", [0.0], True, False)]
    base = _serially(jobs)
    full = base[0]["full"]
    assert int(np.abs(full.astype(int) - frames.astype(int)).max()) <= 2
    for a, b in ranges:
        np.testing.assert_array_equal(base[0]["%d:%d" % (a, b)], full[a:b], err_msg="frames [%d, %d)" % (a, b))
    for r in base[1:]:
        np.testing.assert_array_equal(r["resident"], r["host"])
    assert base[1]["resident"][:, 0].sum() > 0 and not base[3]["resident"].any()   # lossy reports errors, lossless none
    assert int(base[1]["resident"][:, 1].max()) <= 2
    got = _concurrently(jobs)
    for i, (g, b) in enumerate(zip(got, base)):
        _assert_same(g, b, "job %d" % i)


# ----------------------------------------------------------------------------------- 7. per-context switches stay
def test_per_context_switches_stay_per_context():
    """Context B runs a job in two halves.  Between them, context A turns profiling on, switches the convolution kernels,
    sets a small scan poll limit (no epoch skew: nothing is made to fail) and provokes argument errors.  B's results, B's
    profile counters (zero: B never enabled them) and B's last error (empty) must be what they are when B runs alone;
    A's last error must be A's own message."""
    nt, h, w, p = 12, 128, 160, 1
    frames = synth.translating_scene(nt, h, w, seed=14)
    wts = SMALL.init_weights(seed=14, bias_scale=0.2)

    def b_job(mid=None):
        ctx = _lib.Context(0)
        try:
            ctx.load_model(SMALL, wts)
            ctx.prepare(h, w, max_batch=4)
            key, _ = ctx.rollout(frames, p, 4)
            if mid:
                mid()
            pred = ctx.get_predictions()
            payload, table, _ = ctx.encode("abs", [2.0], True)
            payload = np.array(payload, copy=True)
            keys = np.where(key[:, None, None, None], frames, 0).astype(np.uint8)
            ctx.rollout_decode(keys, p)
            dec = np.array(ctx.decode(payload, table), copy=True)
            key2, _ = ctx.rollout(frames, p, 4)
            prof = ctx.prof_get()
            return dict(key=key, key2=key2, pred=pred, payload=payload, table=table, dec=dec,
                        prof_calls=np.array([v[1] for v in prof.values()], np.int64),
                        last_error=ctx.lib.tz_last_error(ctx.h).decode())
        finally:
            ctx.close()

    def a_job(started, switched):
        ctx = _lib.Context(0)
        try:
            ctx.load_model(SMALL, wts)
            ctx.prepare(h, w, max_batch=4)
            if started is not None:
                assert started.wait(timeout=120), "B never started"
            ctx.prof_enable(True)
            ctx.set_conv_impl(0, "always")
            ctx.scan_fault_inject(0, 64)
            msgs = []
            out = np.zeros(nt, _lib.QUALITY_DTYPE)
            # call order: no rollout yet
            assert ctx.lib.tz_encode_quality(ctx.h, None, 0, None, -1, 0, out.ctypes.data) == -4
            msgs.append(ctx.lib.tz_last_error(ctx.h).decode())
            ctx.rollout(frames[:6], 0, 3)
            payload, table, _ = ctx.encode("abs", [2.0], True)
            tb = np.ascontiguousarray(table)
            # a wrong payload length
            assert ctx.lib.tz_encode_quality(ctx.h, payload.ctypes.data, payload.size - 1, tb.ctypes.data, len(tb), 0,
                                             out.ctypes.data) == -1
            msgs.append(ctx.lib.tz_last_error(ctx.h).decode())
            # a range outside the sequence
            km = np.zeros(6, np.uint8)
            ks = np.ascontiguousarray(frames[:6])
            assert ctx.lib.tz_rollout_decode_range(ctx.h, ks.ctypes.data, 6, h, w, 0, -1, 2, km.ctypes.data) == -1
            msgs.append(ctx.lib.tz_last_error(ctx.h).decode())
            if switched is not None:
                switched.set()
            ctx.scan_fault_inject(0, 0)
            return msgs
        finally:
            if switched is not None:
                switched.set()                    # (B never waits for ever, whatever happened here)
            ctx.close()

    base_b = b_job()
    base_a = a_job(None, None)
    assert all(base_a) and len(set(base_a)) == 3, base_a
    assert not base_b["prof_calls"].any() and base_b["last_error"] not in base_a

    started, switched = threading.Event(), threading.Event()

    def b_concurrent():
        def mid():
            started.set()
            assert switched.wait(timeout=120), "A never finished its switches"
        return b_job(mid)

    got_b, got_a = _concurrently([b_concurrent, lambda: a_job(started, switched)])
    _assert_same(got_b, base_b, "B")           # (its last error included: A's messages stay in A)
    assert got_a == base_a


# ----------------------------------------------------------------------------- 8. create and destroy while others run
def test_create_and_destroy_while_others_run():
    long_specs = [(24, 256, 320, 1, 6, None, "abs", [1.0], True, False, 50),
                  (24, 256, 320, 0, None, "auto", "abs", [0.0], True, True, 51)]
    long_jobs = [_pipeline(*s) for s in long_specs]
    short = _pipeline(6, 16, 24, 0, 3, None, "abs", [2.0], True, False, 52)
    base = _serially(long_jobs + [short])
    for s, b in zip(long_specs, base):
        frames = synth.translating_scene(*s[:3], seed=s[-1])
        np.testing.assert_array_equal(b["quality"], _numpy_stats(b["dec"], frames))
    np.testing.assert_array_equal(base[1]["dec"], synth.translating_scene(24, 256, 320, seed=51))

    def churn():
        out = []
        for _ in range(8):                        # Context(0), a small job, close(): 3 contexts open at most
            out.append(short())
        return out

    got = _concurrently(long_jobs + [churn])
    for i in range(2):
        _assert_same(got[i], base[i], "long job %d" % i)
    for k, r in enumerate(got[2]):
        _assert_same(r, base[2], "short job %d" % k)
