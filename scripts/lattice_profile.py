#!/usr/bin/env python3
"""What the lattice quantiser (`-c --quant lattice`, definition TZ-QL1, tezip_amd/lattice.py) costs and buys next to the reference's
greedy one, on two jobs with random weights (seed 3): cfg3's (80 frames of 512x512 synth.turbulence, `-p 0 -w 20`) and 8 frames of
1024x1024 synth.detector (`-p 0 -w 4`), at abs 2 and abs 6, flat and `--sdelta channel`, under zstd and `--coder huffd`.
One process per run of this script, HIP events on the context's stream (tz_timer_start / tz_timer_stop), profiling off while a time
is taken.  Per job, bound and layout:
  bytes     entropy.dat under huffd (ratetarget.file_bytes of tz_size_probe's record: the exact size of the file) and under zstd
            (the stream compress.build_stream makes of tz_encode's payload, through tezip_amd/zstd.py at level 9), and the
            sequence PSNR of tz_bound_probe's records (what --report prints), greedy against lattice;
  encode    device time of the whole tz_encode (payload resident), 7 runs, first two dropped, median: lattice, greedy, and the
            lossless front (abs 0) of the same build;
  search    device time of a `--target-psnr 40` search (target.search over tz_bound_probe) under each quantiser, and every probe
            again on its own: the slowest is named.
No figure is fixed in advance.  The expectations, and whether they held, are recorded: the lattice encode within the run-to-run
spread of the lossless front (it moves the same bytes); no lattice probe standing out the way the greedy probe at E = 63.5 does.
Usage: python scripts/lattice_profile.py [out.json]      (default: profiles/lattice_<date>.json)"""
import datetime
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tezip_amd import _lib, compress, ratetarget, synth, target, zstd  # noqa: E402
from tezip_amd.prednet import PredNetConfig  # noqa: E402

RUNS = 7
TARGET = 40.0
JOBS = (("cfg3_turbulence", lambda: synth.turbulence(80, 512, 512, seed=3), 20),
        ("detector_1024", lambda: synth.detector(8, 1024, 1024), 4))
BOUNDS = (2.0, 6.0)


def _timed(ctx, fn, runs=RUNS, drop=2):
    ms, out = [], None
    for _ in range(runs):
        ctx.timer_start()
        out = fn()
        ms.append(float(ctx.timer_stop()))
    xs = ms[drop:]   # (the first runs warm pools and code objects)
    return out, dict(median_ms=float(np.median(xs)), spread_ms=[min(xs), max(xs)], all_ms=ms)


def _psnr(sse, n):
    return None if sse == 0 else float(10.0 * np.log10(65025.0 * n / sse))


def _bytes(ctx, frames, bound, strided, with_zstd):
    nt, h, w, _ = frames.shape
    rec = ctx.size_probe("abs", [bound], True, "huffd")
    sse = int(ctx.bound_probe("abs", [bound])["sse"].astype(np.int64).sum())
    out = dict(huffd_entropy_dat_bytes=int(ratetarget.file_bytes(rec, "huffd")), huffd_match_distance=int(rec["dist"]),
               sequence_psnr_db=_psnr(sse, int(frames.size)))
    if with_zstd:
        payload, table, _ = ctx.encode("abs", [bound], True)
        stream = compress.build_stream(np.asarray(payload).reshape(-1), table, (4 if strided else 1, nt, h, w, 3), 0)
        out["zstd_entropy_dat_bytes"] = len(zstd.compress_array(stream, 9, zstd.default_threads()))
    return out


def _search(ctx, n):
    limit = target.sse_limit(TARGET, n)
    probe = lambda k: int(ctx.bound_probe("abs", [target.bound_of(k)])["sse"].astype(np.int64).sum())  # noqa: E731
    (k, trace), t = _timed(ctx, lambda: target.search(probe, limit), 5, 1)
    per_probe = []
    for tr in trace:
        _, tp = _timed(ctx, lambda: probe(tr["k"]), 3, 1)
        per_probe.append(dict(k=tr["k"], bound=tr["bound"], median_ms=tp["median_ms"]))
    slow = max(per_probe, key=lambda p: p["median_ms"])
    rest = [p["median_ms"] for p in per_probe if p is not slow]
    return dict(t, k=k, bound=target.bound_of(k), probes=len(trace), per_probe=per_probe, slowest_probe=slow,
                other_probes_ms=[min(rest), max(rest)] if rest else None)


def main():
    date = datetime.date.today().isoformat()
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "lattice_%s.json" % date)
    with_zstd = os.environ.get("LATTICE_PROFILE_ZSTD", "1") != "0"
    cfg = PredNetConfig()
    wts = cfg.init_weights(seed=3)
    doc = dict(date=date, definition="TZ-QL1", target_psnr_db=TARGET, jobs={},
               runs="%d per encode, first two dropped, median; spread = [min, max]; 5 per search, 3 per probe, first dropped" % RUNS)
    for name, make, window in JOBS:
        frames = make()
        nt, h, w, _ = frames.shape
        ctx = _lib.Context(0)
        try:
            ctx.load_model(cfg, wts)
            ctx.prepare(h, w, min(20, max(1, nt // window)))
            ctx.rollout(frames, 0, window)
            ctx.prof_enable(False)
            job = dict(frames=[nt, h, w], window=window, layouts={}, search={})
            for layout, stride in (("flat", 0), ("channel", 1)):
                ctx.set_delta_stride(stride)
                ctx.set_quantiser(0)
                _, lossless = _timed(ctx, lambda: ctx.encode("abs", [0.0], True, payload="resident"))
                cells = dict(lossless_front_encode=lossless, bounds={})
                for bound in BOUNDS:
                    cell = {}
                    for q, quant in enumerate(("greedy", "lattice")):
                        ctx.set_quantiser(q)
                        _, t = _timed(ctx, lambda: ctx.encode("abs", [bound], True, payload="resident"))
                        cell[quant] = dict(_bytes(ctx, frames, bound, bool(stride), with_zstd), encode=t)
                    lat, gre = cell["lattice"], cell["greedy"]
                    cell["lattice_over_greedy_huffd_bytes"] = lat["huffd_entropy_dat_bytes"] / gre["huffd_entropy_dat_bytes"]
                    if with_zstd:
                        cell["lattice_over_greedy_zstd_bytes"] = lat["zstd_entropy_dat_bytes"] / gre["zstd_entropy_dat_bytes"]
                    lo, hi = lossless["spread_ms"]
                    cell["lattice_encode_within_lossless_spread"] = bool(lo <= lat["encode"]["median_ms"] <= hi)
                    cell["lattice_encode_over_lossless_front"] = lat["encode"]["median_ms"] / lossless["median_ms"]
                    cells["bounds"]["abs %g" % bound] = cell
                job["layouts"][layout] = cells
            ctx.set_delta_stride(0)
            for q, quant in enumerate(("greedy", "lattice")):
                ctx.set_quantiser(q)
                job["search"][quant] = _search(ctx, int(frames.size))
            s = job["search"]["lattice"]
            job["search"]["lattice_probe_stands_out"] = bool(s["other_probes_ms"] and s["slowest_probe"]["median_ms"] > 2.0 * s["other_probes_ms"][1])
            doc["jobs"][name] = job
        finally:
            ctx.close()
    doc["notes"] = ("encode: HIP events on the context's stream around tz_encode(payload = NULL), entropy on: front, histogram download, "
                    "table and remap.  bytes: huffd is the exact size of the file the job writes; zstd is the reference's file, made on "
                    "the host from the device's payload.  search: around the Python search, including the host's steps between probes.  "
                    "lattice_probe_stands_out: the slowest probe takes more than twice the slowest of the others.")
    print(json.dumps(doc))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
