"""The compression report on a MI355X (tz_encode_quality, `-c --report`): its per-frame records must equal, as integers,
numpy's statistics of the frames a FRESH context decodes from the same payload (tz_rollout_decode + tz_decode), for SWP
and DWP, warm-up 0 and 2, every error-bound mode and lossless, with and without the rank table and with the byte
shuffle, on flat and padded frames; and the call must change nothing an encode leaves behind."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

SMALL_STACKS = (3, 16, 32)


def _model(seed):
    from tezip_amd.prednet import PredNetConfig
    cfg = PredNetConfig(stack_sizes=SMALL_STACKS)
    return cfg, cfg.init_weights(seed=seed, bias_scale=0.2)


@pytest.fixture(scope="module")
def ctx():
    from tezip_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def dctx():
    """The independent decoder: a context of its own, which never saw the encoder's rollout."""
    from tezip_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _numpy_stats(dec, frames):
    d = dec.astype(np.int64) - frames.astype(np.int64)
    nt = len(frames)
    d = d.reshape(nt, -1)
    return np.stack([(d * d).sum(1), np.abs(d).max(1), (d != 0).sum(1)], axis=1)


def _records(q):
    return np.stack([q["sse"].astype(np.int64), q["max_abs"].astype(np.int64), q["n_changed"].astype(np.int64)], axis=1)


def _encode(ctx, nt, h, w, p, window, thr, mode, bound, entropy, shuffle=False, seed=1):
    from tezip_amd import _lib, synth
    cfg, wts = _model(seed)
    ctx.load_model(cfg, wts)
    ctx.prepare(_lib.pad8(h), _lib.pad8(w), max_batch=4)
    frames = synth.translating_scene(nt, h, w, seed=seed)
    if thr == "auto":   # a DWP threshold inside the observed MSE range: windows of mixed lengths
        _, mse = ctx.rollout(frames, p, None, 1e9, want_mse=True)
        thr = float(np.median(mse[p + 1:]))
    key, _ = ctx.rollout(frames, p, window, thr)
    payload, table, _ = ctx.encode(mode, bound, entropy, shuffle=shuffle)
    payload = np.array(payload, copy=True)
    return frames, key, payload, table


def _decode_fresh(dctx, frames, key, payload, table, p, shuffle=False, seed=1):
    from tezip_amd import _lib
    nt, h, w, _ = frames.shape
    cfg, wts = _model(seed)
    dctx.load_model(cfg, wts)
    dctx.prepare(_lib.pad8(h), _lib.pad8(w), max_batch=4)
    if shuffle:
        payload = dctx.byte_unshuffle(payload.view(np.uint8))
    keys = np.where(key[:, None, None, None], frames, 0).astype(np.uint8)
    kd = dctx.rollout_decode(keys, p)
    np.testing.assert_array_equal(kd, key)
    return dctx.decode(payload, table).copy()


JOBS = [  # nt, h, w, p, window, thr, mode, bound, entropy, shuffle
    (12, 64, 64, 0, 5, None, "abs", [2.0], True, False),
    (12, 64, 64, 2, 4, None, "abs", [2.0], True, True),
    (12, 61, 90, 0, 5, None, "abs", [2.0], True, False),       # padded: the unfused tail, unaligned frame sizes
    (12, 61, 90, 2, 3, None, "rel", [1e-2], False, False),
    (12, 64, 64, 2, None, "auto", "absrel", [3.0, 0.01], True, False),
    (12, 61, 90, 0, None, "auto", "pwrel", [0.05], True, True),
    (13, 61, 90, 2, None, "auto", "abs", [2.0], False, False),
    (12, 64, 64, 0, 4, None, "rel", [1e-2], False, True),
    (12, 64, 64, 2, 5, None, "abs", [0.0], True, False),        # lossless
    (12, 61, 90, 2, None, "auto", "abs", [0.0], False, True),
    (12, 61, 90, 0, 4, None, "abs", [0.0], True, False),
    (12, 64, 64, 0, None, "auto", "pwrel", [0.05], False, False),
]


@pytest.mark.parametrize("nt,h,w,p,window,thr,mode,bound,entropy,shuffle", JOBS)
def test_records_equal_an_independent_decode(ctx, dctx, nt, h, w, p, window, thr, mode, bound, entropy, shuffle):
    frames, key, payload, table = _encode(ctx, nt, h, w, p, window, thr, mode, bound, entropy, shuffle)
    q = ctx.encode_quality(payload, table, shuffle=shuffle)
    dec = _decode_fresh(dctx, frames, key, payload, table, p, shuffle)
    want = _numpy_stats(dec, frames)
    np.testing.assert_array_equal(_records(q), want)
    lossless = mode == "abs" and bound[0] == 0
    if lossless:   # 3. a lossless job reports zeros everywhere
        assert not want.any()
    if mode == "abs":   # 4. |q - d| < E + 1, the error is an integer, the clamp only shrinks it
        assert int(q["max_abs"].max()) <= math.ceil(bound[0])
    # warm-up frames and key frames (group 0 / the bytes of key_frame.dat) carry no error
    for i in range(nt):
        if i < p or key[i]:
            assert tuple(_records(q)[i]) == (0, 0, 0), i
    if not lossless and mode == "abs":
        assert want[:, 0].sum() > 0   # (the job exercises the lossy path)


def test_cfg3_sized_job(ctx, dctx):
    frames, key, payload, table = _encode(ctx, 80, 512, 512, 0, 20, None, "abs", [2.0], True, seed=3)
    q = ctx.encode_quality(payload, table)
    dec = _decode_fresh(dctx, frames, key, payload, table, 0, seed=3)
    np.testing.assert_array_equal(_records(q), _numpy_stats(dec, frames))
    assert int(q["max_abs"].max()) <= 2 and int(q["sse"].sum()) > 0


def test_it_decodes_the_bytes_it_is_given(ctx):
    nt, h, w, p = 12, 61, 90, 1
    frames, key, payload, table = _encode(ctx, nt, h, w, p, 4, None, "abs", [2.0], True)
    clean = _records(ctx.encode_quality(payload, table))
    fe = h * w * 3
    f = next(i for i in range(nt // 2, nt) if not key[i])
    i = f * fe + fe // 2
    bad = payload.copy()
    bad[i] = bad[i] + 1 if bad[i] < 5 else bad[i] - 1
    got = _records(ctx.encode_quality(bad, table))
    assert (got != clean).any()
    np.testing.assert_array_equal(got[:f], clean[:f])   # the inverse scan propagates forward only
    assert (got[f] != clean[f]).any()


def test_resident_payload_is_left_as_it_was(ctx):
    nt, h, w, p = 12, 64, 64, 2
    frames, key, payload, table = _encode(ctx, nt, h, w, p, 5, None, "abs", [2.0], True)
    n = payload.size
    _, t2, _ = ctx.encode("abs", [2.0], True, payload="resident")
    np.testing.assert_array_equal(t2, table)
    before = ctx.payload_get(0, n).copy()
    np.testing.assert_array_equal(before, payload)
    q_res = ctx.encode_quality("resident", table)
    np.testing.assert_array_equal(ctx.payload_get(0, n), before)
    np.testing.assert_array_equal(_records(q_res), _records(ctx.encode_quality(payload, table)))
    again, t3, _ = ctx.encode("abs", [2.0], True)   # a following encode behaves as it would have
    np.testing.assert_array_equal(again, payload)
    np.testing.assert_array_equal(t3, table)


def test_records_do_not_depend_on_the_launch_shape():
    from tezip_amd import _lib
    cases = [(12, 61, 90, 2, 4, "abs", [2.0], True), (9, 64, 64, 0, 3, "rel", [1e-2], False)]
    got = {}
    before = os.environ.get("TEZIP_QUALITY_GRID")
    try:
        for grid in ("0", "1", "3", "7", "100000"):
            os.environ["TEZIP_QUALITY_GRID"] = grid   # read when a context is made
            c = _lib.Context(0)
            try:
                got[grid] = [_records(c.encode_quality(pl, tb)) for (_, _, pl, tb) in
                             (_encode(c, nt, h, w, p, win, None, m, b, e) for nt, h, w, p, win, m, b, e in cases)]
            finally:
                c.close()
    finally:
        if before is None:
            os.environ.pop("TEZIP_QUALITY_GRID", None)
        else:
            os.environ["TEZIP_QUALITY_GRID"] = before
    for grid, recs in got.items():
        for a, b in zip(recs, got["0"]):
            np.testing.assert_array_equal(a, b, err_msg="grid %s" % grid)
    assert all(r[:, 0].sum() > 0 for r in got["0"])


def test_state_and_argument_errors():
    from tezip_amd import _lib
    c = _lib.Context(0)
    try:
        out = np.zeros(16, _lib.QUALITY_DTYPE)
        assert c.lib.tz_encode_quality(c.h, None, 0, None, -1, 0, out.ctypes.data) == -4   # no rollout
        nt, h, w, p = 6, 64, 64, 1
        frames, key, payload, table = _encode(c, nt, h, w, p, 3, None, "abs", [2.0], True)
        n = payload.size
        tb = np.ascontiguousarray(table)
        # a host payload is fine, but no resident one was written by this encode
        assert c.lib.tz_encode_quality(c.h, None, n, tb.ctypes.data, len(tb), 0, out.ctypes.data) == -4
        assert c.lib.tz_encode_quality(c.h, payload.ctypes.data, n - 1, tb.ctypes.data, len(tb), 0, out.ctypes.data) == -1
        assert c.lib.tz_encode_quality(c.h, payload.ctypes.data, n, tb.ctypes.data, len(tb), 0, out.ctypes.data) == 0
        c.encode("abs", [2.0], True, payload="resident")
        assert c.lib.tz_encode_quality(c.h, None, n, tb.ctypes.data, len(tb), 0, out.ctypes.data) == 0
        c.rollout(frames, p, 3)       # a rollout without an encode: the resident payload belongs to the one before
        assert c.lib.tz_encode_quality(c.h, None, n, tb.ctypes.data, len(tb), 0, out.ctypes.data) == -4
        keys = np.where(key[:, None, None, None], frames, 0).astype(np.uint8)
        c.rollout_decode(keys, p)     # a decoder rollout
        assert c.lib.tz_encode_quality(c.h, payload.ctypes.data, n, tb.ctypes.data, len(tb), 0, out.ctypes.data) == -4
        with pytest.raises(_lib.TezipError) as e:
            c.encode_quality(payload, table)
        assert e.value.status == -4
    finally:
        c.close()


# ---------------------------------------------------------------------------------------------------------- CLI
def _cli(args, timeout=300):
    return subprocess.run(["timeout", "-k", "10", str(timeout), sys.executable, "-m", "tezip_amd.tezip"] + args, cwd=ROOT,
                          capture_output=True, text=True, timeout=timeout + 30)


def test_cli_report_end_to_end(tmp_path):
    from PIL import Image
    from tezip_amd import synth, weights
    nt, h, w = 16, 29, 43
    cfg, wts = _model(4)
    frames = synth.translating_scene(nt, h, w, seed=5)
    mdir = str(tmp_path / "model")
    weights.save_model(mdir, cfg, wts, 32, 48)
    ddir = tmp_path / "data"
    ddir.mkdir()
    names = ["f_%03d.png" % t for t in range(nt)]
    for t in range(nt):
        Image.fromarray(frames[t]).save(ddir / names[t])
    job = ["-p", "1", "-w", "4", "-m", "abs", "-b", "2"]
    with_r, without = str(tmp_path / "comp_r"), str(tmp_path / "comp")
    r = _cli(["-c", mdir, str(ddir), with_r] + job + ["--report"])
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert any(ln.startswith("max_abs_err:") for ln in lines) and any(ln.startswith("PSNR:") for ln in lines)
    assert any(ln.startswith("ratio:") for ln in lines)
    r = _cli(["-c", mdir, str(ddir), without] + job)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PSNR:" not in r.stdout
    assert sorted(os.listdir(without)) == ["entropy.dat", "filename.txt", "key_frame.dat", "tezip_amd.json"]
    assert sorted(os.listdir(with_r)) == sorted(os.listdir(without) + ["quality.json"])
    for n in os.listdir(without):   # the report changes nothing that -c writes
        assert open(os.path.join(with_r, n), "rb").read() == open(os.path.join(without, n), "rb").read(), n
    doc = json.load(open(os.path.join(with_r, "quality.json")))
    stored = sum(os.path.getsize(os.path.join(with_r, n)) for n in ("filename.txt", "key_frame.dat", "entropy.dat"))
    assert doc["ratio"] == nt * h * w * 3 / stored
    assert [f["name"] for f in doc["per_frame"]] == names
    # -u of the directory that holds quality.json: its images against the inputs are what the report says
    udir, udir0 = str(tmp_path / "dec_r"), str(tmp_path / "dec")
    r = _cli(["-u", mdir, with_r, udir])
    assert r.returncode == 0, r.stdout + r.stderr
    r = _cli(["-u", mdir, without, udir0])
    assert r.returncode == 0, r.stdout + r.stderr
    assert sorted(os.listdir(udir)) == names
    dec = np.stack([np.asarray(Image.open(os.path.join(udir, n)).convert("RGB")) for n in names])
    want = _numpy_stats(dec, frames)
    got = np.array([[f["sse"], f["max_abs_err"], f["n_changed"]] for f in doc["per_frame"]], np.int64)
    np.testing.assert_array_equal(got, want)
    assert doc["max_abs_err"] == int(want[:, 1].max()) <= 2 and doc["n_changed"] == int(want[:, 2].sum())
    for n in names:   # decompress ignores quality.json
        assert open(os.path.join(udir, n), "rb").read() == open(os.path.join(udir0, n), "rb").read(), n
