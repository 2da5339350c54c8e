#!/usr/bin/env python3
"""Size and device time of the two GPU coders of entropy.dat, `--coder huffr` (TZR1) next to `--coder huff` (TZH1), and the
zstd-9 size, all from the same payload: 80 frames of 512x512 synthetic turbulence, random weights (seed 3), window 20,
lossless and `abs 2`.  Device times are HIP-event sums of the 'huffman' profiling class (tz_prof_get), 6 runs, median.
Usage: python scripts/huffr_profile.py out.json"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tezip_amd import _lib, huff, huffr, synth, zstd  # noqa: E402
from tezip_amd.prednet import PredNetConfig  # noqa: E402

HBM_PEAK = 8e12


def timed(ctx, fn, runs=6):
    ms = []
    for _ in range(runs):
        ctx.prof_reset()
        fn()
        ms.append(ctx.prof_get()["huffman"][0])
    return float(np.median(ms)), ms


def main():
    cfg = PredNetConfig()
    nt, h, w = 80, 512, 512
    frames = synth.turbulence(nt, h, w, seed=3)
    ctx = _lib.Context(0)
    ctx.load_model(cfg, cfg.init_weights(seed=3))
    ctx.prepare(h, w, 20)
    ctx.prof_enable(True)
    n = nt * h * w * 3
    jobs = []
    for bound in ([0.0], [2.0]):
        ctx.rollout(frames, 0, 20)
        _, table, _ = ctx.encode("abs", bound, True, payload="resident")
        pay = ctx.payload_get(0, n)
        trailer = huff.reference_trailer(table, (1, nt, h, w, 3), 0)
        t0 = time.perf_counter()
        z = len(zstd.compress_array(np.concatenate([pay, trailer.astype(np.int16)]), 9, 16))
        zs = time.perf_counter() - t0
        rec = dict(mode="abs", bound=bound, zstd9_bytes=z, zstd9_seconds_16_threads=zs)
        for name, fmt, counts, encode, begin, put, decode in (
                ("huff", huff, ctx.huff_counts, ctx.huff_encode, ctx.huff_begin, ctx.huff_put, ctx.huff_decode),
                ("huffr", huffr, ctx.huffr_counts, ctx.huffr_encode, ctx.huffr_begin, ctx.huffr_put, ctx.huffr_decode)):
            cnt, base = counts()
            ln = fmt.code_lengths(cnt)
            state = {}

            def enc():
                c, b = counts()
                state["nbytes"] = encode(ln, b)

            enc_ms, enc_all = timed(ctx, enc)
            nbytes = state["nbytes"]
            body = ctx.huff_get(0, nbytes)
            front = fmt.pack_front(trailer, ln, base, n, huff.geometry(n)[1], (nbytes - huff.body_bytes(n, 0)) // 4)
            size = len(front) + nbytes

            def dec():
                begin(nbytes, n, ln, base)
                put(0, body)
                decode()

            dec_ms, dec_all = timed(ctx, dec)
            assert (ctx.payload_get(0, n) == pay).all(), name     # (the payload buffer now holds the decoded stream)
            rec[name] = dict(bytes=size, over_zstd9=size / z, bits_per_element=8.0 * size / n,
                             encode_device_ms_count_size_scan_enc=enc_ms, encode_device_ms_all=enc_all,
                             decode_device_ms=dec_ms, decode_device_ms_all=dec_all,
                             encode_fraction_of_8TBps_hbm_peak=(3 * 2 * n + nbytes) / (enc_ms * 1e-3) / HBM_PEAK,
                             decode_fraction_of_8TBps_hbm_peak=(2 * n + nbytes) / (dec_ms * 1e-3) / HBM_PEAK)
            if name == "huffr":
                rec[name]["token_counts_T0_T7"] = [int(c) for c in cnt[-8:]]
                rec[name]["literals"] = int(cnt[:-8].sum())
        rec["huffr_over_huff_bytes"] = rec["huffr"]["bytes"] / rec["huff"]["bytes"]
        rec["huffr_over_huff_encode_ms"] = rec["huffr"]["encode_device_ms_count_size_scan_enc"] / rec["huff"]["encode_device_ms_count_size_scan_enc"]
        rec["huffr_over_huff_decode_ms"] = rec["huffr"]["decode_device_ms"] / rec["huff"]["decode_device_ms"]
        jobs.append(rec)
        print(json.dumps(rec), flush=True)
    ctx.close()
    doc = dict(frames=[nt, h, w], weights="random (seed 3)", data="synth.turbulence", window=20, jobs=jobs,
               notes="Both coders measured in one process on one device from the same resident payload. Device times are HIP-event sums "
                     "of the 'huffman' profiling class (tz_prof_get), 6 runs, median. encode = count + size + scan + pack kernels, bytes "
                     "moved = 3 reads of the payload + the coded stream; decode = the expand kernel, coded stream in + payload out.")
    with open(sys.argv[1], "w") as f:
        json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
