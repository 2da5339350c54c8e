#!/usr/bin/env python3
"""Size of entropy.dat under the four coders and device time of the GPU coders' passes, `--coder huffd` (TZR2: the match distance
none / 1 / 3 chosen per file, tezip_amd/huffd.py) next to `--coder huff` (TZH1), `--coder huffr` (TZR1) and zstd-9, all from the
same resident payload, random weights (seed 3), lossless (abs 0) and at abs 2:
  turbulence     80 frames of 512x512 synth.turbulence, -w 20 (cfg3's job), three payload channels
  moving_blobs   40 frames of 64x64 synth.moving_blobs, -w 20 (cfg1's job), three channels and one (--gray)
  detector       8 frames of 1024x1024 synth.detector, -w 4, three channels and one (--gray)
Per payload: the bytes of the entropy.dat each coder writes (front + stream; zstd-9 of payload | trailer), the D huffd chooses
with its three costs in bits, and the HIP-event time (tz_timer_start / tz_timer_stop on the context's stream) of the count
call, of the encode call (size + scan + pack) and of the decode call (stage + expand), 3 runs each, median.  When parent_tree
is given (a checkout of the PARENT commit with its library built), huff's and huffr's times are also taken from that build in a
child process of its own, so that huffr is compared with the kernels it launched before they took a distance parameter.
One GPU process at a time, each under a time limit; the script stops at the first child that fails.
The expectation this records (no threshold anywhere): huffd's count pass costs more than huffr's (three histograms from one
read), its pack and expand cost no more than huffr's, and its file is never larger than the smaller of huff's and huffr's by
more than 4 bytes per chunk + 12.
Usage: python scripts/huffd_profile.py out.json [parent_tree]"""
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JOBS = (dict(name="turbulence", gen="turbulence", nt=80, h=512, w=512, window=20, channels=(3,)),
        dict(name="moving_blobs", gen="moving_blobs", nt=40, h=64, w=64, window=20, channels=(3, 1)),
        dict(name="detector", gen="detector", nt=8, h=1024, w=1024, window=4, channels=(3, 1)))
BOUNDS = {"lossless": [0.0], "abs2": [2.0]}
RUNS = 3


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
    from tezip_amd import _lib, huff, huffr, synth, zstd
    from tezip_amd.prednet import PredNetConfig
    has_huffd = hasattr(_lib.Context, "huffd_counts")
    if has_huffd:
        from tezip_amd import huffd
    cfg = PredNetConfig()
    wts = cfg.init_weights(seed=3)
    out = {}
    for j in JOBS:
        frames = getattr(synth, j["gen"])(j["nt"], j["h"], j["w"])
        nt, h, w = frames.shape[:3]
        ctx = _lib.Context(0)
        try:
            ctx.load_model(cfg, wts)
            ctx.prepare(_lib.pad8(h), _lib.pad8(w), min(j["window"], 20))
            for ch in j["channels"]:
                for bname, bound in BOUNDS.items():
                    ctx.rollout(frames, 0, j["window"])
                    ctx.set_payload_channels(ch)
                    _, table, _ = ctx.encode("abs", bound, True, payload="resident")
                    n = nt * h * w * ch
                    pay = ctx.payload_get(0, n)
                    trailer = huff.reference_trailer(table, (1, nt, h, w, ch), 0)
                    rec = dict(n=n, chunks=huff.geometry(n)[1])
                    if has_huffd:
                        rec["zstd9_bytes"] = len(zstd.compress_array(np.concatenate([pay, trailer.astype(np.int16)]), 9, 16))
                    coders = [("huff", ctx.huff_counts, lambda c: (huff.code_lengths(c), ()), ctx.huff_encode, ctx.huff_begin, ctx.huff_put,
                               ctx.huff_decode, huff.pack_front),
                              ("huffr", ctx.huffr_counts, lambda c: (huffr.code_lengths(c), ()), ctx.huffr_encode, ctx.huffr_begin, ctx.huffr_put,
                               ctx.huffr_decode, huffr.pack_front)]
                    if has_huffd:
                        def pick(c3):
                            dist, ln, costs = huffd.choose(c3)
                            rec["huffd_choice"] = dict(D=dist, cost_bits_none=costs[0], cost_bits_1=costs[1], cost_bits_3=costs[2])
                            return ln, (dist,)
                        coders.append(("huffd", ctx.huffd_counts, pick, ctx.huffd_encode, ctx.huffd_begin, ctx.huffd_put, ctx.huffd_decode,
                                       huffd.pack_front))
                    for name, counts, lengths_of, encode, begin, put, decode, pack_front in coders:
                        cnt, base = counts()
                        ln, dist = lengths_of(cnt)
                        state = {}
                        count_ms, count_all = timed(ctx, counts)

                        def enc():
                            state["nbytes"] = encode(ln, base, *dist)

                        enc_ms, enc_all = timed(ctx, enc)
                        nbytes = state["nbytes"]
                        body = ctx.huff_get(0, nbytes)
                        front = pack_front(trailer, ln, base, n, huff.geometry(n)[1], (nbytes - huff.body_bytes(n, 0)) // 4, *dist)

                        def dec():
                            begin(nbytes, n, ln, base, *dist)
                            put(0, body)
                            decode()

                        dec_ms, dec_all = timed(ctx, dec)
                        assert (ctx.payload_get(0, n) == pay).all(), name     # (the payload buffer now holds the decoded stream)
                        rec[name] = dict(bytes=len(front) + nbytes, count_ms=count_ms, count_ms_all=count_all, encode_ms=enc_ms,
                                         encode_ms_all=enc_all, decode_ms=dec_ms, decode_ms_all=dec_all)
                    out["%s/%dch/%s" % (j["name"], ch, bname)] = rec
                    print(json.dumps({j["name"]: ch, bname: rec}), file=sys.stderr, flush=True)
        finally:
            ctx.close()
    print("HUFFD_PROFILE " + json.dumps(out), flush=True)


def run_child(root):
    r = subprocess.run(["timeout", "-k", "10", "540", sys.executable, os.path.abspath(__file__), "--child", root], capture_output=True, text=True)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("HUFFD_PROFILE ")]
    if r.returncode != 0 or not lines:
        raise SystemExit("the measurement in %s ended with status %d:\n%s\n%s" % (root, r.returncode, r.stdout[-2000:], r.stderr[-4000:]))
    return json.loads(lines[-1][len("HUFFD_PROFILE "):])


def main():
    if sys.argv[1] == "--child":
        return child(sys.argv[2])
    out_path = sys.argv[1]
    parent = os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else None
    new = run_child(HERE)                                   # (one after the other: a child that failed ends the script
    old = run_child(parent) if parent else None             #  before the next starts)
    ratios = {}
    for key, r in new.items():
        best = min(r["huff"]["bytes"], r["huffr"]["bytes"])
        ratios[key] = dict(D=r["huffd_choice"]["D"], huffd_over_best_of_huff_huffr_bytes=r["huffd"]["bytes"] / best,
                           huffd_over_huffr_bytes=r["huffd"]["bytes"] / r["huffr"]["bytes"],
                           huffd_over_zstd9_bytes=r["huffd"]["bytes"] / r["zstd9_bytes"],
                           size_guarantee_holds=r["huffd"]["bytes"] <= best + 4 * r["chunks"] + 12,
                           count_huffd_over_huffr=r["huffd"]["count_ms"] / r["huffr"]["count_ms"],
                           encode_huffd_over_huffr=r["huffd"]["encode_ms"] / r["huffr"]["encode_ms"],
                           decode_huffd_over_huffr=r["huffd"]["decode_ms"] / r["huffr"]["decode_ms"])
        if old:
            ratios[key]["huffr_encode_over_parent"] = r["huffr"]["encode_ms"] / old[key]["huffr"]["encode_ms"]
            ratios[key]["huffr_decode_over_parent"] = r["huffr"]["decode_ms"] / old[key]["huffr"]["decode_ms"]
    doc = dict(jobs=JOBS, weights="random (seed 3)", bounds=BOUNDS, results=new, parent_results=old, ratios=ratios,
               notes="One device, one GPU process at a time.  Key: job / payload channels / bound.  bytes: front + stream of the "
                     "entropy.dat the coder writes for the resident payload.  count_ms / encode_ms / decode_ms: HIP events on the "
                     "context's stream around the counts call, the encode call (size + scan + pack; it waits once for the stream's "
                     "size) and begin + put + decode (host-to-device copy of the stream + expand), %d runs, median.  parent_results: "
                     "huff's and huffr's figures from a build of the parent commit (null when no tree was given).  Expectation "
                     "recorded, not tested: count_huffd_over_huffr above 1, the encode and decode ratios at or below 1 when D is 1 or 3." % RUNS)
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(ratios, indent=1))


if __name__ == "__main__":
    main()
