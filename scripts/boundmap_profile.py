#!/usr/bin/env python3
"""What a bound map (`-c -m abs --bound-map FILE`, definition TZ-BM1, tezip_amd/boundmap.py) buys and costs on cfg3's job: 80 frames
of 512x512 synth.turbulence, `-p 0 -w 20`, random weights (seed 3), `--coder huffd`.  The map is 0 inside a centred 128x128 box and
6 outside.

  python scripts/boundmap_profile.py run OUT.json
      one process, HIP events on the context's stream (tz_timer_start / tz_timer_stop), profiling off while a time is taken:
      sizes   entropy.dat under huffd (ratetarget.file_bytes of the flat record of tz_sdelta_probe: the exact size of the file) of
              the lossless job, `abs 6` and the map job, greedy and lattice, from the one rollout;
      encode  device time of the whole tz_encode (payload resident), 7 calls, median: the map job, a `pwrel` job of the same
              tolerances' range (b0 = 6 / 255) and `abs 6`, greedy and lattice.
      On a build without tz_set_bound_map (the parent commit's) the map rows are left out: the same file serves both builds.
  python scripts/boundmap_profile.py merge OUT.json NEW1.json [NEW2.json ...] --parent P1.json [P2.json ...]
      the medians over the processes of each build (run them alternating), the parent's run-to-run spread of its pwrel figure and
      whether the map job lies inside it, and by how much the uniform abs job is faster.  Default OUT: profiles/bound_map_<date>.json

No figure is fixed in advance.  The expectations, and whether they held, are recorded: the map job runs the per-element (float64)
walk, so pwrel's time is the yardstick and the map job should lie inside the parent's own spread of it; the uniform abs job is
expected to be faster than both -- that gap is the case for an all-integer walk under a map."""
import datetime
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RUNS = 7
BOX, OUTSIDE = 128, 6
PWREL_B0 = OUTSIDE / 255.0


def roi_map(h, w):
    m = np.full((h, w), OUTSIDE, np.uint8)
    m[(h - BOX) // 2:(h + BOX) // 2, (w - BOX) // 2:(w + BOX) // 2] = 0
    return m


def _timed(ctx, fn, runs=RUNS):
    fn()   # (the first call warms pools and code objects)
    ms = []
    for _ in range(runs):
        ctx.timer_start()
        fn()
        ms.append(float(ctx.timer_stop()))
    return dict(median_ms=float(np.median(ms)), spread_ms=[min(ms), max(ms)], all_ms=ms)


def run(out):
    from tezip_amd import _lib, ratetarget, synth
    from tezip_amd.prednet import PredNetConfig
    cfg = PredNetConfig()
    wts = cfg.init_weights(seed=3)
    frames = synth.turbulence(80, 512, 512, seed=3)
    nt, h, w, _ = frames.shape
    ctx = _lib.Context(0)
    has_map = hasattr(ctx, "set_bound_map")
    M = roi_map(h, w)
    doc = dict(definition="TZ-BM1", frames=[nt, h, w], window=20, has_bound_map=has_map, pwrel_b0=PWREL_B0,
               map="0 inside a centred %dx%d box, %d outside" % (BOX, BOX, OUTSIDE), quant={})
    try:
        ctx.load_model(cfg, wts)
        ctx.prepare(h, w, 4)
        ctx.rollout(frames, 0, 20)
        ctx.prof_enable(False)
        size = lambda mode, b: int(ratetarget.file_bytes(ctx.sdelta_probe(mode, b, True, "huffd")[0], "huffd"))  # noqa: E731
        for q, quant in enumerate(("greedy", "lattice")):
            ctx.set_quantiser(q)
            cell = dict(bytes=dict(lossless=size("abs", [0.0]), abs6=size("abs", [float(OUTSIDE)])), encode={})
            cell["encode"]["abs6"] = _timed(ctx, lambda: ctx.encode("abs", [float(OUTSIDE)], True, payload="resident"))
            cell["encode"]["pwrel"] = _timed(ctx, lambda: ctx.encode("pwrel", [PWREL_B0], True, payload="resident"))
            cell["encode"]["lossless"] = _timed(ctx, lambda: ctx.encode("abs", [0.0], True, payload="resident"))
            if has_map:
                ctx.set_bound_map(M)
                cell["bytes"]["map"] = size("abs", [0.0])
                cell["encode"]["map"] = _timed(ctx, lambda: ctx.encode("abs", [0.0], True, payload="resident"))
                rec = ctx.encode_map_check("resident", ctx.encode("abs", [0.0], True, payload="resident")[1])
                cell["map_violations"] = int(rec["violations"].sum())
                ctx.set_bound_map(None)
            doc["quant"][quant] = cell
    finally:
        ctx.close()
    print(json.dumps(doc))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


def _med(docs, quant, what):
    xs = [d["quant"][quant]["encode"][what]["median_ms"] for d in docs if what in d["quant"][quant]["encode"]]
    return dict(median_ms=float(np.median(xs)), processes_ms=xs) if xs else None


def merge(out, new, parent):
    new, parent = [json.load(open(p)) for p in new], [json.load(open(p)) for p in parent]
    doc = dict(date=datetime.date.today().isoformat(), definition="TZ-BM1", frames=new[0]["frames"], window=new[0]["window"], map=new[0]["map"],
               pwrel_b0=new[0]["pwrel_b0"], quant={},
               runs="per process %d calls behind one warm-up call, median; then the median over %d fresh processes of this build and %d of "
                    "the parent's, alternating" % (RUNS, len(new), len(parent)))
    for quant in ("greedy", "lattice"):
        cell = dict(bytes=new[0]["quant"][quant]["bytes"], map_violations=new[0]["quant"][quant].get("map_violations"),
                    this_build={k: _med(new, quant, k) for k in ("map", "pwrel", "abs6", "lossless")},
                    parent_build={k: _med(parent, quant, k) for k in ("pwrel", "abs6", "lossless")} if parent else None)
        b = cell["bytes"]
        cell["map_over_lossless_bytes"] = b["map"] / b["lossless"]
        cell["map_over_abs6_bytes"] = b["map"] / b["abs6"]
        t = cell["this_build"]
        cell["map_over_abs6_time"] = t["map"]["median_ms"] / t["abs6"]["median_ms"]
        cell["map_over_pwrel_time"] = t["map"]["median_ms"] / t["pwrel"]["median_ms"]
        if parent:
            ps = cell["parent_build"]["pwrel"]["processes_ms"]
            cell["parent_pwrel_spread_ms"] = [min(ps), max(ps)]
            cell["map_inside_parent_pwrel_spread"] = bool(min(ps) <= t["map"]["median_ms"] <= max(ps))
        doc["quant"][quant] = cell
    doc["notes"] = ("encode: HIP events on the context's stream around tz_encode(payload = NULL), entropy on: front, histogram download, table "
                    "and remap.  bytes: the exact size of the entropy.dat the huffd job writes in the flat layout.  Not measured: a trained "
                    "model, -t jobs, other frame sizes, other maps.")
    print(json.dumps(doc))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", out)


def main(argv):
    if len(argv) >= 2 and argv[0] == "run":
        return run(argv[1])
    if len(argv) >= 3 and argv[0] == "merge":
        rest = argv[2:]
        cut = rest.index("--parent") if "--parent" in rest else len(rest)
        return merge(argv[1] or os.path.join(ROOT, "profiles", "bound_map_%s.json" % datetime.date.today().isoformat()), rest[:cut], rest[cut + 1:])
    print(__doc__)
    return 2


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
