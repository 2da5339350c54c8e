#!/usr/bin/env python3
"""Device and wall time of the per-frame digests (`-c --digests`, `-u --verify`; k_digest, format TZD64) on cfg3's job: 80
frames of 512x512 synthetic turbulence, random weights (seed 3), window 20, `abs 2`.
Device times are HIP-event sums of the 'digest' profiling class (tz_prof_get), 7 runs, median, next to k_quality's over
the same stacks in the same process.  Wall times are compress.run / decompress.run with and without the records, the two
settings alternating in one process, first round dropped, median of 3.
Usage: python scripts/digest_profile.py out.json [work_dir]
       python scripts/digest_profile.py --decompress-only out.json [work_dir]
The second form times decompress.run of a directory WITHOUT records only (4 rounds, first dropped), with whatever
tezip_amd package stands next to this script's parent directory: run it from two checkouts to compare commits."""
import contextlib
import io
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tezip_amd import _lib, compress, decompress, synth, weights  # noqa: E402
from tezip_amd.prednet import PredNetConfig  # noqa: E402


def timed(ctx, cls, fn, runs=7):
    ms, launches = [], 0
    for _ in range(runs):
        ctx.prof_reset()
        fn()
        ms_, launches = ctx.prof_get()[cls]
        ms.append(ms_)
    return float(np.median(ms)), ms, int(launches)


def device_part(cfg, wts, frames, window):
    from tezip_amd import digest
    nt, h, w = frames.shape[:3]
    nbytes = frames.size
    enc, dec = _lib.Context(0), _lib.Context(0)
    for c in (enc, dec):
        c.load_model(cfg, wts)
        c.prepare(h, w, 20)
    key, _ = enc.rollout(frames, 0, window)
    _, table, _ = enc.encode("abs", [2.0], True, payload="resident")
    payload = enc.payload_get(0, nbytes).copy()
    enc.prof_enable(True)
    state = {}
    e_ms, e_all, e_n = timed(enc, "digest", lambda: state.update(dig=enc.encode_digests("resident", table)))
    q_ms, q_all, q_n = timed(enc, "quality", lambda: state.update(q=enc.encode_quality("resident", table)))
    d_dec, d_org = state["dig"]
    assert (d_org == digest.stack_digests(frames)).all()
    assert ((d_dec != d_org) == (state["q"]["n_changed"] > 0)).all()
    keys = np.where(key[:, None, None, None], frames, 0).astype(np.uint8)
    dec.rollout_decode(keys, 0)
    dec.decode(payload, table, out="resident")
    dec.prof_enable(True)
    u_ms, u_all, u_n = timed(dec, "digest", lambda: state.update(u=dec.decoded_digests(0, nt)))
    assert (state["u"] == d_dec).all()
    enc.close()
    dec.close()
    return dict(stack_bytes=int(nbytes),
                encode_digests=dict(device_ms=e_ms, device_ms_all=e_all, launches=e_n, bytes_read=int(2 * nbytes),
                                    bytes_per_second=2 * nbytes / (e_ms * 1e-3), us_per_launch=e_ms * 1e3 / max(e_n, 1)),
                decoded_digests=dict(device_ms=u_ms, device_ms_all=u_all, launches=u_n, bytes_read=int(nbytes),
                                     bytes_per_second=nbytes / (u_ms * 1e-3)),
                k_quality_same_process=dict(device_ms=q_ms, device_ms_all=q_all, launches=q_n, bytes_read=int(2 * nbytes),
                                            bytes_per_second=2 * nbytes / (q_ms * 1e-3)),
                frames_changed_by_abs2=int((d_dec != d_org).sum()))


def make_job(cfg, wts, frames, work):
    from PIL import Image
    nt, h, w = frames.shape[:3]
    mdir, ddir = os.path.join(work, "model"), os.path.join(work, "data")
    weights.save_model(mdir, cfg, wts, h, w)
    os.makedirs(ddir)
    for t in range(nt):
        Image.fromarray(frames[t]).save(os.path.join(ddir, "f_%03d.png" % t))
    return mdir, ddir


def _summary(r):
    for k in [k for k in r if k.endswith("_s")]:
        r[k + "_median"] = float(np.median(r[k]))
        r[k + "_spread"] = [float(min(r[k])), float(max(r[k]))]
    return r


def wall_part(mdir, ddir, window, work):
    res = {"plain": dict(compress_s=[], decompress_s=[]), "digests": dict(compress_s=[], decompress_s=[])}
    for rep in range(4):               # (the first round warms the process up and is dropped)
        for name, flag in (("plain", False), ("digests", True)):
            out, dec = os.path.join(work, "c_%s_%d" % (name, rep)), os.path.join(work, "u_%s_%d" % (name, rep))
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf):
                t0 = time.perf_counter()
                if flag:
                    compress.run(mdir, ddir, out, 0, window, None, "abs", [2.0], True, False, True, DIGESTS=True)
                else:
                    compress.run(mdir, ddir, out, 0, window, None, "abs", [2.0], True, False, True)
                t1 = time.perf_counter()
                decompress.run(mdir, out, dec, True, False)
                t2 = time.perf_counter()
            assert ("verified: 80 frames" in buf.getvalue()) == flag
            if rep:
                res[name]["compress_s"].append(t1 - t0)
                res[name]["decompress_s"].append(t2 - t1)
            shutil.rmtree(dec)
            shutil.rmtree(out)
    return {k: _summary(r) for k, r in res.items()}


def decompress_only(mdir, ddir, window, work):
    out = os.path.join(work, "c_plain")
    res = dict(decompress_s=[])
    with contextlib.redirect_stdout(io.StringIO()):
        compress.run(mdir, ddir, out, 0, window, None, "abs", [2.0], True, False, True)
        for rep in range(4):
            dec = os.path.join(work, "u_plain_%d" % rep)
            t0 = time.perf_counter()
            decompress.run(mdir, out, dec, True, False)
            t1 = time.perf_counter()
            if rep:
                res["decompress_s"].append(t1 - t0)
            shutil.rmtree(dec)
    return _summary(res)


def main():
    args = sys.argv[1:]
    only = bool(args) and args[0] == "--decompress-only"
    if only:
        args = args[1:]
    cfg = PredNetConfig()
    wts = cfg.init_weights(seed=3)
    nt, h, w, window = 80, 512, 512, 20
    frames = synth.turbulence(nt, h, w, seed=3)
    doc = dict(frames=[nt, h, w], weights="random (seed 3)", data="synth.turbulence", window=window, mode="abs 2", root=ROOT)
    work = args[1] if len(args) > 1 else tempfile.mkdtemp(prefix="digest_profile_")
    os.makedirs(work, exist_ok=True)
    try:
        if not only:
            doc["device"] = device_part(cfg, wts, frames, window)
            print(json.dumps(doc["device"]), flush=True)
        mdir, ddir = make_job(cfg, wts, frames, work)
        if only:
            doc["wall_decompress_without_records"] = decompress_only(mdir, ddir, window, work)
        else:
            doc["wall_abs2"] = wall_part(mdir, ddir, window, work)
        print(json.dumps(doc.get("wall_abs2") or doc["wall_decompress_without_records"]), flush=True)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    doc["notes"] = ("One process, one device.  Device times are HIP-event sums of the 'digest' (k_digest) and 'quality' (k_quality) "
                    "profiling classes, 7 runs, median; the decoder's tail that tz_encode_digests / tz_encode_quality run first is "
                    "counted in its own classes.  Wall times: compress.run / decompress.run on PNG files, abs 2, zstd coders, the "
                    "settings alternating, first round dropped, median of 3, spread = [min, max].")
    with open(args[0], "w") as f:
        json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
