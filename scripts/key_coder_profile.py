#!/usr/bin/env python3
"""Size and time of the GPU coder of key_frame.dat (`--key-coder huff`, format TZK1) next to zstd-9 over the reference's
zero-except-keys stack, from the same frames: 80 frames of 512x512 synthetic turbulence, random weights (seed 3), window 20.
Device times are HIP-event sums of the 'huffman' profiling class (tz_prof_get), 7 runs, median.  Wall times are
compress.run / decompress.run of `--coder huffr` with and without `--key-coder huff`, alternating, 3 runs each, median.
Usage: python scripts/key_coder_profile.py out.json [work_dir]"""
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
from tezip_amd import _lib, compress, decompress, huff, keycoder, synth, weights, zstd  # noqa: E402
from tezip_amd.prednet import PredNetConfig  # noqa: E402


def timed(ctx, fn, runs=7):
    ms = []
    for _ in range(runs):
        ctx.prof_reset()
        fn()
        ms.append(ctx.prof_get()["huffman"][0])
    return float(np.median(ms)), ms


def device_part(cfg, wts, frames, window):
    nt, h, w = frames.shape[:3]
    ctx = _lib.Context(0)
    ctx.load_model(cfg, wts)
    ctx.prepare(h, w, 20)
    key, _ = ctx.rollout(frames, 0, window)
    idx = [int(i) for i in np.nonzero(key)[0]]
    ctx.prof_enable(True)
    state = {}

    def enc():
        counts = ctx.keys_counts(idx)
        pred = keycoder.choose_predictors(counts)
        ln = huff.code_lengths(keycoder.chosen_counts(counts, pred))
        state.update(pred=pred, ln=ln, nbytes=ctx.keys_encode(idx, pred, ln))

    enc_ms, enc_all = timed(ctx, enc)
    n = len(idx) * h * w * 3
    body = ctx.keys_get(0, state["nbytes"])
    front = keycoder.pack_front(nt, h, w, idx, state["pred"], state["ln"], huff.geometry(n)[1],
                                (state["nbytes"] - huff.body_bytes(n, 0)) // 4)
    data = front + body.tobytes()
    stack = np.zeros_like(frames)
    stack[idx] = frames[idx]
    t0 = time.perf_counter()
    z = len(zstd.compress_array(stack, 9, 16))
    zs = time.perf_counter() - t0
    p = keycoder.parse(data)
    b = np.ascontiguousarray(p.body)

    def dec():
        ctx.keys_begin(b.size, nt, h, w, p.idx, p.pred, p.lengths)
        ctx.keys_put(0, b)
        ctx.keys_decode()

    dec_ms, dec_all = timed(ctx, dec)
    assert (ctx.frames_get(0, nt) == stack).all()
    ctx.close()
    return dict(key_frames=idx, predictor_ids=[int(v) for v in state["pred"]], tzk1_bytes=len(data), zstd9_bytes=z,
                tzk1_over_zstd9=len(data) / z, zstd9_seconds_16_threads=zs,
                encode_device_ms_hist_resid_size_scan_enc=enc_ms, encode_device_ms_all=enc_all,
                decode_device_ms_dec_unresid=dec_ms, decode_device_ms_all=dec_all)


def wall_part(cfg, wts, frames, window, work):
    from PIL import Image
    nt, h, w = frames.shape[:3]
    mdir, ddir = os.path.join(work, "model"), os.path.join(work, "data")
    weights.save_model(mdir, cfg, wts, h, w)
    os.makedirs(ddir)
    for t in range(nt):
        Image.fromarray(frames[t]).save(os.path.join(ddir, "f_%03d.png" % t))
    res = {"huffr": dict(compress_s=[], decompress_s=[]), "huffr+key_huff": dict(compress_s=[], decompress_s=[])}
    for rep in range(4):               # (the first round warms the process up and is dropped)
        for name, kc in (("huffr", "zstd"), ("huffr+key_huff", "huff")):
            out, dec = os.path.join(work, "c_%s_%d" % (kc, rep)), os.path.join(work, "u_%s_%d" % (kc, rep))
            with contextlib.redirect_stdout(io.StringIO()):
                t0 = time.perf_counter()
                compress.run(mdir, ddir, out, 0, window, None, "abs", [2.0], True, False, True, CODER="huffr", KEY_CODER=kc)
                t1 = time.perf_counter()
                decompress.run(mdir, out, dec, True, False)
                t2 = time.perf_counter()
            if rep:
                res[name]["compress_s"].append(t1 - t0)
                res[name]["decompress_s"].append(t2 - t1)
            res[name]["bytes"] = {n: os.path.getsize(os.path.join(out, n)) for n in ("key_frame.dat", "entropy.dat")}
            shutil.rmtree(dec)
            shutil.rmtree(out)
    for r in res.values():
        r["compress_s_median"] = float(np.median(r["compress_s"]))
        r["decompress_s_median"] = float(np.median(r["decompress_s"]))
    return res


def main():
    cfg = PredNetConfig()
    wts = cfg.init_weights(seed=3)
    nt, h, w, window = 80, 512, 512, 20
    frames = synth.turbulence(nt, h, w, seed=3)
    doc = dict(frames=[nt, h, w], weights="random (seed 3)", data="synth.turbulence", window=window)
    doc["device"] = device_part(cfg, wts, frames, window)
    print(json.dumps(doc["device"]), flush=True)
    work = sys.argv[2] if len(sys.argv) > 2 else tempfile.mkdtemp(prefix="key_coder_profile_")
    os.makedirs(work, exist_ok=True)
    try:
        doc["wall_abs2"] = wall_part(cfg, wts, frames, window, work)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    print(json.dumps(doc["wall_abs2"]), flush=True)
    doc["notes"] = ("One process, one device.  Device times are HIP-event sums of the 'huffman' profiling class, 7 runs, median: encode = "
                    "k_key_hist + k_key_resid + the Huffman size / scan / pack kernels, decode = the Huffman expand kernel + "
                    "k_key_unresid_row / k_key_unresid_col (the memset of the other frames is not in the class).  Wall times: compress.run / "
                    "decompress.run on PNG files, abs 2, the two settings alternating, first round dropped, median of 3.")
    with open(sys.argv[1], "w") as f:
        json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
