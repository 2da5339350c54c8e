#!/usr/bin/env python3
"""Size of entropy.dat and device time of the encoder's and the decoder's tail under the flat spatial delta and under the
channel stride (`-c --sdelta channel`, tz_set_delta_stride(1), tezip_amd/sdelta.py), random weights (seed 3), lossless (abs 0)
and at abs 2:
  turbulence          80 frames of 512x512 synth.turbulence, -w 20 (cfg3's job)
  translating_scene   40 frames of 128x160 synth.translating_scene, -w 10 (cfg2's job)
Per job, bound and stride mode, all from the same resident rollout: the bytes of entropy.dat under zstd-9, huffr and huffd
(with the distance huffd picks); the HIP-event time (tz_timer_start / tz_timer_stop on the context's stream) of the whole
tz_encode call (front + table + remap: the encode tail, which includes the one host wait for the histogram) and of tz_decode
on the staged payload (the decoder's tail), RUNS runs each, median; and from a separate profiled pass the library's own
per-kernel event times (spatial delta + histogram, inverse scan, reconstruct).
When parent_tree is given (a checkout of the PARENT commit with its library built) the FLAT tails are also taken from that
build: children run in the order this tree, parent, parent, this tree, so that each build is measured once early and once
late, and the parent's two medians give the A/A spread that serves as margin.
One GPU process at a time, each under a time limit; the script stops at the first child that fails.
No ratio is asserted anywhere: the strided scan publishes three sums, reads the payload twice and reconstructs in a second
kernel, so it is expected to be slower than the fused flat tail.
Usage: python scripts/sdelta_profile.py out.json [parent_tree]"""
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JOBS = (dict(name="turbulence", gen="turbulence", nt=80, h=512, w=512, window=20),
        dict(name="translating_scene", gen="translating_scene", nt=40, h=128, w=160, window=10))
BOUNDS = {"lossless": [0.0], "abs2": [2.0]}
RUNS = 7
HBM_PEAK = 8.0e12   # bytes / s (spec)


def timed(ctx, fn):
    ms = []
    for _ in range(RUNS):
        ctx.synchronize()
        ctx.timer_start()
        fn()
        ms.append(ctx.timer_stop())
    return float(np.median(ms)), ms


def child(root):
    """Measure with the package of the tree `root`; prints one JSON line."""
    sys.path.insert(0, root)
    from tezip_amd import _lib, huff, huffr, huffd, synth, zstd
    from tezip_amd.prednet import PredNetConfig
    has_stride = hasattr(_lib.Context, "set_delta_stride")
    cfg = PredNetConfig()
    wts = cfg.init_weights(seed=3)
    out = {}
    for j in JOBS:
        frames = getattr(synth, j["gen"])(j["nt"], j["h"], j["w"])
        nt, h, w = frames.shape[:3]
        n = nt * h * w * 3
        ctx = _lib.Context(0)
        try:
            ctx.load_model(cfg, wts)
            ctx.prepare(_lib.pad8(h), _lib.pad8(w), min(j["window"], 20))
            for bname, bound in BOUNDS.items():
                key = ctx.rollout(frames, 0, j["window"])[0]
                recs, pays = {}, {}
                for mode in ("flat", "channel") if has_stride else ("flat",):
                    if has_stride:
                        ctx.set_delta_stride(1 if mode == "channel" else 0)
                    state = {}

                    def enc():
                        state["table"] = ctx.encode("abs", bound, True, payload="resident")[1]

                    enc()                                                       # warm: buffers, lazy allocations
                    enc_ms, enc_all = timed(ctx, enc)
                    table = state["table"]
                    pay = ctx.payload_get(0, n)
                    one = 4 if mode == "channel" else 1
                    trailer = huff.reference_trailer(table, (one, nt, h, w, 3), 0)
                    rec = dict(n=n, encode_ms=enc_ms, encode_ms_all=enc_all,
                               zstd9_bytes=len(zstd.compress_array(np.concatenate([pay, trailer.astype(np.int16)]), 9, 16)))
                    cnt, base = ctx.huffr_counts()
                    ln = huffr.code_lengths(cnt)
                    nbytes = ctx.huffr_encode(ln, base)
                    rec["huffr_bytes"] = len(huffr.pack_front(trailer, ln, base, n, huff.geometry(n)[1], (nbytes - huff.body_bytes(n, 0)) // 4)) + nbytes
                    c3, base = ctx.huffd_counts()
                    dist, ln, costs = huffd.choose(c3)
                    nbytes = ctx.huffd_encode(ln, base, dist)
                    rec["huffd_bytes"] = len(huffd.pack_front(trailer, ln, base, n, huff.geometry(n)[1], (nbytes - huff.body_bytes(n, 0)) // 4, dist)) + nbytes
                    rec["huffd_D"] = int(dist)
                    rec["huffd_cost_bits"] = [int(c) for c in costs]
                    # the library's own per-kernel events, one profiled encode
                    ctx.prof_enable(True)
                    ctx.prof_reset()
                    enc()
                    prof = ctx.prof_get()
                    ctx.prof_enable(False)
                    rec["encode_kernels_ms"] = {k: v[0] for k, v in prof.items() if v[1] and k in ("delta", "quant", "spatial_delta_hist", "lut_remap", "table_create")}
                    recs[mode], pays[mode] = rec, (pay, table)
                # the decoder's tail, on the decoder's own rollout of the same job
                key_stack = np.where(key[:, None, None, None], frames, 0).astype(np.uint8)
                ctx.rollout_decode(key_stack, 0)
                decoded = {}
                for mode, (pay, table) in pays.items():
                    if has_stride:
                        ctx.set_delta_stride(1 if mode == "channel" else 0)
                    ctx.payload_begin(n)
                    ctx.payload_put(0, pay)

                    def dec():
                        ctx.decode(None, table, out="resident")

                    dec()
                    dec_ms, dec_all = timed(ctx, dec)
                    decoded[mode] = ctx.decoded_digests(0, nt)
                    ctx.prof_enable(True)
                    ctx.prof_reset()
                    dec()
                    prof = ctx.prof_get()
                    ctx.prof_enable(False)
                    recs[mode].update(decode_ms=dec_ms, decode_ms_all=dec_all,
                                      decode_kernels_ms={k: v[0] for k, v in prof.items() if v[1] and k in ("undelta_scan", "reconstruct", "lut_remap")})
                if has_stride:
                    assert (decoded["flat"] == decoded["channel"]).all(), "the two modes decode to different frames"
                    ctx.set_delta_stride(0)
                out["%s/%s" % (j["name"], bname)] = recs
                print(json.dumps({j["name"]: bname, "rec": recs}), file=sys.stderr, flush=True)
        finally:
            ctx.close()
    print("SDELTA_PROFILE " + json.dumps(out), flush=True)


def run_child(root):
    r = subprocess.run(["timeout", "-k", "10", "420", sys.executable, os.path.abspath(__file__), "--child", root], capture_output=True, text=True)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("SDELTA_PROFILE ")]
    if r.returncode != 0 or not lines:
        raise SystemExit("the measurement in %s ended with status %d:\n%s\n%s" % (root, r.returncode, r.stdout[-2000:], r.stderr[-4000:]))
    return json.loads(lines[-1][len("SDELTA_PROFILE "):])


def main():
    if sys.argv[1] == "--child":
        return child(sys.argv[2])
    out_path = sys.argv[1]
    parent = os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else None
    runs = [("this", run_child(HERE))]                      # (one after the other: a child that failed ends the script
    if parent:                                              #  before the next starts)
        runs.append(("parent", run_child(parent)))
        runs.append(("parent", run_child(parent)))
        runs.append(("this", run_child(HERE)))
    new = runs[0][1]
    summary = {}
    for key, r in new.items():
        f, c = r["flat"], r["channel"]
        n = f["n"]
        s = dict(zstd9_channel_over_flat=c["zstd9_bytes"] / f["zstd9_bytes"], huffr_channel_over_flat=c["huffr_bytes"] / f["huffr_bytes"],
                 huffd_channel_over_flat=c["huffd_bytes"] / f["huffd_bytes"], huffd_D_flat=f["huffd_D"], huffd_D_channel=c["huffd_D"],
                 encode_channel_over_flat=c["encode_ms"] / f["encode_ms"], decode_channel_over_flat=c["decode_ms"] / f["decode_ms"],
                 # decoder tail, bytes that must move: flat fused 2 payload + 4 prediction + 1 frame; channel 2 + 2 (payload read
                 # twice) + 2 + 2 (temporary written and read) + 4 + 1
                 decode_flat_hbm_fraction=7.0 * n / (f["decode_ms"] * 1e-3) / HBM_PEAK,
                 decode_channel_hbm_fraction=13.0 * n / (c["decode_ms"] * 1e-3) / HBM_PEAK)
        if parent:
            this = [x[1][key]["flat"] for x in runs if x[0] == "this"]
            par = [x[1][key]["flat"] for x in runs if x[0] == "parent"]
            for leg in ("encode_ms", "decode_ms"):
                s["flat_%s_this" % leg] = [t[leg] for t in this]
                s["flat_%s_parent" % leg] = [p[leg] for p in par]
                s["flat_%s_margin_parent_AA" % leg] = abs(par[0][leg] - par[1][leg])
                s["flat_%s_this_minus_parent" % leg] = float(np.median([v for t in this for v in t[leg + "_all"]])
                                                             - np.median([v for p in par for v in p[leg + "_all"]]))
        summary[key] = s
    doc = dict(jobs=JOBS, weights="random (seed 3)", bounds=BOUNDS, runs=RUNS, results=new,
               all_runs=[dict(build=b, results=r) for b, r in runs] if parent else None, summary=summary,
               notes="One device, one GPU process at a time.  Key: job / bound, then the stride mode.  *_bytes: the entropy.dat "
                     "each coder writes for the resident payload (front + stream; zstd-9 of payload | trailer).  encode_ms: HIP "
                     "events around the whole tz_encode (payload resident); decode_ms: around tz_decode of the staged payload, "
                     "frames resident; medians of %d runs after one warm call.  *_kernels_ms: the library's per-kernel events of "
                     "one more, profiled call.  hbm_fraction: bytes that must move (see the script) over the time over 8 TB/s.  "
                     "With a parent tree: children in the order this, parent, parent, this; margin = the difference of the "
                     "parent's two run medians; this_minus_parent = difference of the medians of all samples of each build." % RUNS)
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(summary, indent=1))


if __name__ == "__main__":
    main()
