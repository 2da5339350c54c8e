#!/usr/bin/env python3
"""Size of entropy.dat and device time of the encoder and of the decoder's tail under the flat spatial delta, the channel
stride and the 2-D plane delta (`-c --sdelta plane`, tz_set_delta_plane(1), definition TZ-SD2, tezip_amd/sdelta.py), random
weights (seed 3):
  turbulence          80 frames of 512x512 synth.turbulence, -w 20 (cfg3's job)
  translating_scene   40 frames of 128x160 synth.translating_scene, -w 10 (cfg2's job)
Per job, all from the same resident rollout: lossless, and abs 2 and abs 6 under the greedy and the lattice quantiser; per
spatial delta the bytes of entropy.dat under zstd-9 and huffd (with the distance huffd picks), the HIP-event time
(tz_timer_start / tz_timer_stop on the context's stream) of the whole tz_encode call (payload resident; it includes the one
host wait for the histogram) and of tz_decode on the staged payload (the decoder's tail), RUNS runs each after one warm call,
median.  The three payloads of a configuration must decode to the same frames (TZD64 digests), else the script stops.
When parent_tree is given (a checkout of the PARENT commit with its library built) the FLAT times of the lossless and the
abs 2 greedy configuration are also taken from that build: children run in the order this tree (everything), parent, parent,
this tree (flat times only), so that the parent's two medians give the A/A spread.
One GPU process at a time, each under a time limit; the script stops at the first child that fails.  No ratio is asserted.
Usage: python scripts/plane_profile.py out.json [parent_tree]"""
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JOBS = (dict(name="turbulence", gen="turbulence", nt=80, h=512, w=512, window=20),
        dict(name="translating_scene", gen="translating_scene", nt=40, h=128, w=160, window=10))
CONFIGS = (("lossless", "greedy", [0.0]), ("abs2-greedy", "greedy", [2.0]), ("abs2-lattice", "lattice", [2.0]),
           ("abs6-greedy", "greedy", [6.0]), ("abs6-lattice", "lattice", [6.0]))
FLAT_ONLY = ("lossless", "abs2-greedy")     # what the parent build is asked for
MODES = ("flat", "channel", "plane")
MARK = {"flat": 1, "channel": 4, "plane": 8}
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


def set_mode(ctx, mode):
    if hasattr(ctx, "set_delta_plane"):
        ctx.set_delta_plane(0)
    if hasattr(ctx, "set_delta_stride"):
        ctx.set_delta_stride(1 if mode == "channel" else 0)
    if mode == "plane":
        ctx.set_delta_plane(1)


def child(root, flat_only):
    """Measure with the package of the tree `root`; prints one JSON line."""
    sys.path.insert(0, root)
    from tezip_amd import _lib, huff, huffd, synth, zstd
    from tezip_amd.prednet import PredNetConfig
    cfg = PredNetConfig()
    wts = cfg.init_weights(seed=3)
    out = {}
    for j in JOBS:
        frames = getattr(synth, j["gen"])(j["nt"], j["h"], j["w"])
        nt, h, w = frames.shape[:3]
        n = nt * h * w * 3
        enc, dec = _lib.Context(0), _lib.Context(0)
        try:
            for c in (enc, dec):
                c.load_model(cfg, wts)
                c.prepare(_lib.pad8(h), _lib.pad8(w), min(j["window"], 20))
            key = enc.rollout(frames, 0, j["window"])[0]
            dec.rollout_decode(np.where(key[:, None, None, None], frames, 0).astype(np.uint8), 0)
            for cname, quant, bound in CONFIGS:
                if flat_only and cname not in FLAT_ONLY:
                    continue
                if hasattr(enc, "set_quantiser"):
                    enc.set_quantiser(quant)
                recs, digests = {}, {}
                for mode in ("flat",) if flat_only else MODES:
                    set_mode(enc, mode)
                    set_mode(dec, mode)
                    state = {}

                    def encode():
                        state["table"] = enc.encode("abs", bound, True, payload="resident")[1]

                    encode()                                                    # warm: buffers, lazy allocations
                    enc_ms, enc_all = timed(enc, encode)
                    table = state["table"]
                    pay = enc.payload_get(0, n)
                    rec = dict(n=n, encode_ms=enc_ms, encode_ms_all=enc_all, table_len=int(len(table)))
                    if not flat_only:
                        trailer = huff.reference_trailer(table, (MARK[mode], nt, h, w, 3), 0)
                        rec["zstd9_bytes"] = len(zstd.compress_array(np.concatenate([pay, trailer.astype(np.int16)]), 9, 16))
                        c3, base = enc.huffd_counts()
                        dist, ln, _ = huffd.choose(c3)
                        nbytes = enc.huffd_encode(ln, base, dist)
                        rec["huffd_bytes"] = len(huffd.pack_front(trailer, ln, base, n, huff.geometry(n)[1],
                                                                  (nbytes - huff.body_bytes(n, 0)) // 4, dist)) + nbytes
                        rec["huffd_D"] = int(dist)
                    dec.payload_begin(n)
                    dec.payload_put(0, pay)

                    def decode():
                        dec.decode(None, table, out="resident")

                    decode()
                    rec["decode_ms"], rec["decode_ms_all"] = timed(dec, decode)
                    digests[mode] = dec.decoded_digests(0, nt)
                    dec.prof_enable(True)
                    dec.prof_reset()
                    decode()
                    prof = dec.prof_get()
                    dec.prof_enable(False)
                    rec["decode_kernels_ms"] = {k: v[0] for k, v in prof.items() if v[1] and k in ("undelta_scan", "reconstruct", "lut_remap")}
                    recs[mode] = rec
                for mode in recs:
                    assert (digests[mode] == digests["flat"]).all(), "%s decodes to other frames than flat" % mode
                out["%s/%s" % (j["name"], cname)] = recs
                print(json.dumps({j["name"]: cname, "rec": recs}), file=sys.stderr, flush=True)
        finally:
            enc.close()
            dec.close()
    print("PLANE_PROFILE " + json.dumps(out), flush=True)


def run_child(root, flat_only):
    r = subprocess.run(["timeout", "-k", "10", "540", sys.executable, os.path.abspath(__file__), "--child", root, "1" if flat_only else "0"],
                       capture_output=True, text=True)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("PLANE_PROFILE ")]
    if r.returncode != 0 or not lines:
        raise SystemExit("the measurement in %s ended with status %d:\n%s\n%s" % (root, r.returncode, r.stdout[-2000:], r.stderr[-4000:]))
    return json.loads(lines[-1][len("PLANE_PROFILE "):])


def main():
    if sys.argv[1] == "--child":
        return child(sys.argv[2], sys.argv[3] == "1")
    out_path = sys.argv[1]
    parent = os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else None
    runs = [("this", run_child(HERE, False))]               # (one after the other: a child that failed ends the script
    if parent:                                              #  before the next starts)
        runs.append(("parent", run_child(parent, True)))
        runs.append(("parent", run_child(parent, True)))
        runs.append(("this", run_child(HERE, True)))
    new = runs[0][1]
    summary = {}
    for key, r in new.items():
        f, c, p = r["flat"], r["channel"], r["plane"]
        n = f["n"]
        s = dict(zstd9_bytes=[m["zstd9_bytes"] for m in (f, c, p)], huffd_bytes=[m["huffd_bytes"] for m in (f, c, p)],
                 huffd_D=[m["huffd_D"] for m in (f, c, p)],
                 zstd9_plane_over_channel=p["zstd9_bytes"] / c["zstd9_bytes"], huffd_plane_over_channel=p["huffd_bytes"] / c["huffd_bytes"],
                 zstd9_plane_over_flat=p["zstd9_bytes"] / f["zstd9_bytes"], huffd_plane_over_flat=p["huffd_bytes"] / f["huffd_bytes"],
                 encode_ms=[m["encode_ms"] for m in (f, c, p)], decode_ms=[m["decode_ms"] for m in (f, c, p)],
                 # decoder tail, bytes that must move per element: flat fused 2 payload + 4 prediction + 1 frame; channel 2 + 2 (the
                 # payload read twice) + 2 + 2 (temporary written and read) + 4 + 1; plane with the fused reconstruct 2 + 2 (the
                 # payload read twice where a frame has more than one band) + 2 + 2 (temporary) + 4 + 1
                 decode_bytes_per_element=[7, 13, 13],
                 decode_hbm_fraction=[b * n / (m["decode_ms"] * 1e-3) / HBM_PEAK for b, m in ((7.0, f), (13.0, c), (13.0, p))])
        if parent and key.split("/")[1] in FLAT_ONLY:
            this = [x[1][key]["flat"] for x in runs if x[0] == "this"]
            par = [x[1][key]["flat"] for x in runs if x[0] == "parent"]
            for leg in ("encode_ms", "decode_ms"):
                s["flat_%s_this" % leg] = [t[leg] for t in this]
                s["flat_%s_parent" % leg] = [q[leg] for q in par]
                s["flat_%s_margin_parent_AA" % leg] = abs(par[0][leg] - par[1][leg])
        summary[key] = s
    doc = dict(jobs=JOBS, weights="random (seed 3)", configs=[list(c) for c in CONFIGS], runs=RUNS, results=new,
               all_runs=[dict(build=b, results=r) for b, r in runs] if parent else None, summary=summary,
               notes="One device, one GPU process at a time.  Key: job / configuration, then the spatial delta; lists in the summary "
                     "are in the order flat, channel, plane.  *_bytes: the entropy.dat each coder writes for the resident payload "
                     "(zstd-9 of payload | trailer; huffd front + stream).  encode_ms: HIP events around the whole tz_encode (payload "
                     "resident); decode_ms: around tz_decode of the staged payload, frames resident; medians of %d runs after one warm "
                     "call.  decode_kernels_ms: the library's per-kernel events of one more, profiled call.  hbm_fraction: bytes that "
                     "must move (see the script) over the time over 8 TB/s.  With a parent tree: children in the order this, parent, "
                     "parent, this; margin = the difference of the parent's two run medians." % RUNS)
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(summary, indent=1))


if __name__ == "__main__":
    main()
