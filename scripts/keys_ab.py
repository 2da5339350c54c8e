#!/usr/bin/env python3
"""A/B of the key-frame coders (TZK1 `--key-coder huff`, TZK2 `--key-coder huffg`) between this tree's library and another
build of it (the parent commit's libtezip_hip.so): HIP-event time (tz_timer_start / tz_timer_stop on the context's stream)
of the encoder's calls on a resident stack -- TZK1: tz_keys_counts + tz_keys_encode, TZK2: tz_keys_gray + tz_keys_counts +
tz_keysg_encode, the host's choice of predictors and code lengths between them included -- and of tz_keys_decode /
tz_keysg_decode of a staged body.  Jobs (the key frames of -w W are every W-th frame):
  turbulence     80 frames of 512x512 synth.turbulence, -w 20                                     (TZK1 and TZK2, no gray frame)
  moving_blobs   40 frames of 64x64 synth.moving_blobs, -w 20                                     (TZK2, every frame gray)
  detector       8 frames of 1024x1024 synth.detector, -w 4                                       (TZK2, every frame gray)
  mixed          the turbulence job with channel 0 in all three channels of key frames 0 and 40   (TZK2)
RUNS samples per entry after one warm call, median.
Four runs, each a pair of child processes one after the other (never two GPU processes at once, each under a time limit, the
script stops at the first child that fails), in the order this/parent, parent/this, parent/this, this/parent: each build goes
first twice.  The margin of an entry is the parent build's own spread over its four run medians (max - min); an entry is
accepted when this build's median of run medians is inside that margin of the parent's, or faster, and listed otherwise.
Usage: python scripts/keys_ab.py PARENT_LIB.so out.json"""
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNS = 7
JOBS = {"turbulence": dict(gen="turbulence", nt=80, h=512, w=512, window=20, coders=("tzk1", "tzk2")),
        "moving_blobs": dict(gen="moving_blobs", nt=40, h=64, w=64, window=20, coders=("tzk2",)),
        "detector": dict(gen="detector", nt=8, h=1024, w=1024, window=4, coders=("tzk2",)),
        "mixed": dict(gen="turbulence", nt=80, h=512, w=512, window=20, coders=("tzk2",), gray_keys=(0, 40))}


def child(lib_path):
    sys.path.insert(0, HERE)
    from tezip_amd import _lib, huff, keycoder, keycoderg, synth
    _lib.LIB_PATH = lib_path
    out = {}

    def timed(ctx, fn):
        fn()                                                                # warm: buffers, lazy allocations
        ms = []
        for _ in range(RUNS):
            ctx.synchronize()
            ctx.timer_start()
            fn()
            ms.append(ctx.timer_stop())
        return float(np.median(ms))

    made = {}
    ctx = _lib.Context(0)
    try:
        for job, j in JOBS.items():
            shape = (j["gen"], j["nt"], j["h"], j["w"])
            if shape not in made:
                made[shape] = np.ascontiguousarray(getattr(synth, shape[0])(*shape[1:]))
            frames = made[shape].copy()
            for k in j.get("gray_keys", ()):
                frames[k] = frames[k][..., :1]
            nt, h, w = frames.shape[:3]
            idx = list(range(0, nt, j["window"]))
            want = np.zeros_like(frames)
            want[idx] = frames[idx]
            for coder in j["coders"]:
                g = "g" if coder == "tzk2" else ""
                begin, put, decode, get = (getattr(ctx, "keys%s_%s" % (g, f)) for f in ("begin", "put", "decode", "get"))
                state = {}

                def enc():
                    if coder == "tzk1":
                        counts = ctx.keys_counts(idx)
                        pred = keycoder.choose_predictors(counts)
                        ln = huff.code_lengths(keycoder.chosen_counts(counts, pred))
                        state.update(pred=pred, ln=ln, nbytes=ctx.keys_encode(idx, pred, ln))
                    else:
                        gray = ctx.keys_gray(idx)
                        counts = keycoderg.gray_counts(ctx.keys_counts(idx), gray)
                        pred = keycoderg.pred_bytes(counts, gray)
                        ln = huff.code_lengths(keycoderg.chosen_counts(counts, pred))
                        state.update(pred=pred, ln=ln, nbytes=ctx.keysg_encode(idx, pred, ln))

                ctx.frames_begin(nt, h, w)
                ctx.frames_put(0, frames)
                out["%s/%s_encode" % (job, coder)] = timed(ctx, enc)
                body = get(0, state["nbytes"])
                begin(body.size, nt, h, w, idx, state["pred"], state["ln"])
                put(0, body)
                out["%s/%s_decode" % (job, coder)] = timed(ctx, decode)
                assert (ctx.frames_get(0, nt) == want).all(), "%s %s: the decoded stack" % (job, coder)
    finally:
        ctx.close()
    print("KEYS_AB " + json.dumps(out), flush=True)


def run_child(lib_path):
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--child", lib_path],
                       capture_output=True, text=True)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("KEYS_AB ")]
    if r.returncode != 0 or not lines:
        raise SystemExit("the measurement with %s ended with status %d:\n%s\n%s" % (lib_path, r.returncode, r.stdout[-2000:], r.stderr[-4000:]))
    return json.loads(lines[-1][len("KEYS_AB "):])


def main():
    if sys.argv[1] == "--child":
        return child(sys.argv[2])
    libs = {"this": os.path.join(HERE, "tezip_amd", "csrc", "libtezip_hip.so"), "parent": os.path.abspath(sys.argv[1])}
    order = [("this", "parent"), ("parent", "this"), ("parent", "this"), ("this", "parent")]
    runs = {"this": [], "parent": []}
    for pair in order:
        for build in pair:
            runs[build].append(run_child(libs[build]))
            print(build, json.dumps(runs[build][-1]), file=sys.stderr, flush=True)
    entries, outside = {}, []
    for k in runs["this"][0]:
        t, p = [r[k] for r in runs["this"]], [r[k] for r in runs["parent"]]
        margin = max(p) - min(p)
        e = dict(this_ms=t, parent_ms=p, this_median_ms=float(np.median(t)), parent_median_ms=float(np.median(p)), margin_ms=margin)
        e["outside_margin"] = e["this_median_ms"] - e["parent_median_ms"] > margin
        entries[k] = e
        if e["outside_margin"]:
            outside.append(k)
    doc = dict(jobs=JOBS, runs_per_build=4, samples=RUNS, run_order=["%s first" % a for a, _ in order], entries=entries,
               outside_margin=outside,
               notes="HIP events on the context's stream around the calls of an entry, median of %d samples after one warm call, per "
                     "run; margin_ms: the parent build's max - min over its four run medians; outside_margin: this build's median "
                     "of run medians is slower than the parent's by more than margin_ms." % RUNS)
    with open(sys.argv[2], "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({k: (round(e["this_median_ms"], 4), round(e["parent_median_ms"], 4), round(e["margin_ms"], 4)) for k, e in entries.items()}, indent=1))
    print("outside the parent's spread:", outside or "none")


if __name__ == "__main__":
    main()
