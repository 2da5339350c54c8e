#!/usr/bin/env python3
"""A/B of the host paths of the three payload layouts (flat, gray, channel stride) between this tree's library and another
build of it (the parent commit's libtezip_hip.so): HIP-event time (tz_timer_start / tz_timer_stop on the context's stream)
of tz_encode lossless and at abs 2 (entropy on, payload resident), tz_decode of the staged payload and tz_decode_range of the
last quarter of the stream, on the 80-frame 512x512 turbulence job of scripts/sdelta_profile.py (gray: its channel 0 in all
three channels), random weights (seed 3).  RUNS samples per entry after one warm call, median.
Four runs, each a pair of child processes one after the other (never two GPU processes at once, each under a time limit, the
script stops at the first child that fails), in the order this/parent, parent/this, parent/this, this/parent: each build goes
first twice.  The margin of an entry is the parent build's own spread over its four run medians (max - min); every entry whose
median over this build's runs differs from the parent's by more than that is listed.
Usage: python scripts/layouts_ab.py PARENT_LIB.so out.json"""
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NT, H, W, WINDOW, RUNS = 80, 512, 512, 20, 7
RANGE = (60, 20)
LAYOUTS = {"flat": (3, 0), "gray": (1, 0), "stride": (3, 1)}


def child(lib_path):
    sys.path.insert(0, HERE)
    from tezip_amd import _lib, synth
    from tezip_amd.prednet import PredNetConfig
    _lib.LIB_PATH = lib_path
    cfg = PredNetConfig()
    wts = cfg.init_weights(seed=3)
    colour = synth.turbulence(NT, H, W)
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

    for name, (channels, stride) in LAYOUTS.items():
        frames = np.ascontiguousarray(np.repeat(colour[..., :1], 3, axis=-1)) if channels == 1 else colour
        n = NT * H * W * channels
        ctx = _lib.Context(0)
        try:
            ctx.load_model(cfg, wts)
            ctx.prepare(H, W, WINDOW)
            ctx.set_payload_channels(channels)
            ctx.set_delta_stride(stride)
            key = ctx.rollout(frames, 0, WINDOW)[0]
            state = {}
            out[name + "/encode_lossless"] = timed(ctx, lambda: ctx.encode("abs", [0.0], True, payload="resident"))

            def enc():
                state["table"] = ctx.encode("abs", [2.0], True, payload="resident")[1]

            out[name + "/encode_abs2"] = timed(ctx, enc)
            pay = ctx.payload_get(0, n)
            key_stack = np.where(key[:, None, None, None], frames, 0).astype(np.uint8)
            ctx.rollout_decode(key_stack, 0)
            ctx.payload_begin(n)
            ctx.payload_put(0, pay)
            out[name + "/decode"] = timed(ctx, lambda: ctx.decode(None, state["table"], out="resident"))
            ctx.rollout_decode_range(key_stack, 0, *RANGE)
            ctx.payload_begin(n)
            ctx.payload_put(0, pay)
            out[name + "/decode_range"] = timed(ctx, lambda: ctx.decode_range(None, state["table"], RANGE[0], RANGE[1], out="resident"))
        finally:
            ctx.close()
    print("LAYOUTS_AB " + json.dumps(out), flush=True)


def run_child(lib_path):
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--child", lib_path],
                       capture_output=True, text=True)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("LAYOUTS_AB ")]
    if r.returncode != 0 or not lines:
        raise SystemExit("the measurement with %s ended with status %d:\n%s\n%s" % (lib_path, r.returncode, r.stdout[-2000:], r.stderr[-4000:]))
    return json.loads(lines[-1][len("LAYOUTS_AB "):])


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
        e["outside_margin"] = abs(e["this_median_ms"] - e["parent_median_ms"]) > margin
        entries[k] = e
        if e["outside_margin"]:
            outside.append(k)
    doc = dict(job="turbulence %d x %d x %d, -w %d, random weights (seed 3)" % (NT, H, W, WINDOW), runs_per_build=4, samples=RUNS,
               run_order=["%s first" % a for a, _ in order], range=list(RANGE), entries=entries, outside_margin=outside,
               notes="HIP events on the context's stream around the whole call, median of %d samples after one warm call, per run; "
                     "margin_ms: the parent build's max - min over its four run medians; outside_margin: this build's median of run "
                     "medians differs from the parent's by more than margin_ms." % RUNS)
    with open(sys.argv[2], "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({k: (round(e["this_median_ms"], 4), round(e["parent_median_ms"], 4), round(e["margin_ms"], 4)) for k, e in entries.items()}, indent=1))
    print("outside the parent's spread:", outside or "none")


if __name__ == "__main__":
    main()
