#!/usr/bin/env python3
"""What per-frame bounds cost and buy (`-c --target-psnr DB --per-frame`, definition TZ-TPSNR-F1, tezip_amd/frametarget.py) on
cfg3's job: 80 frames of 512x512 synthetic turbulence, random weights (seed 3), `-p 0 -w 20`, target 40 dB, `--coder huffd`.
One process, HIP events on the context's stream (tz_timer_start / tz_timer_stop), profiling off while a time is taken:
  search    the per-frame search next to the sequence search (`--target-psnr 40`, TZ-TPSNR-1) of the same build, 5 runs each,
            first dropped, median; then every probe of both on its own, with the chains its quantiser sent through the serial
            fallback (quant_serial_chains: the slow case at E = 63.5 shows there).
  jobs      the per-frame job, the sequence job (a weaker guarantee) and `-m abs -b min(frame_bounds)`, the uniform bound that
            gives the SAME floor: bytes of entropy.dat (tz_size_probe's exact size of the huffd file, ratetarget.file_bytes) and
            the worst PSNR over the frames that are not stored exactly (tz_bound_probe's records, which are --report's per_frame).
No threshold is set in advance: the figures are recorded.
Usage: python scripts/frame_bounds_profile.py [out.json]      (default: profiles/frame_bounds_<date>.json)"""
import datetime
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tezip_amd import _lib, frametarget, ratetarget, synth, target  # noqa: E402
from tezip_amd.prednet import PredNetConfig  # noqa: E402

RUNS = 5
TARGET = 40.0
NT, H, W, WINDOW = 80, 512, 512, 20
CODER = "huffd"


def _timed(ctx, fn, runs):
    ms, out = [], None
    for _ in range(runs):
        ctx.timer_start()
        out = fn()
        ms.append(float(ctx.timer_stop()))
    xs = ms[1:]   # (the first run warms pools and code objects)
    return out, dict(median_ms=float(np.median(xs)), spread_ms=[min(xs), max(xs)], all_ms=ms)


def _serial(ctx, fn):
    """-> (median ms of fn with profiling off, chains the quantiser sent through k_q_serial in one run of fn)"""
    _, t = _timed(ctx, fn, 3)
    ctx.prof_enable(True)
    ctx.prof_reset()
    fn()
    n = int(ctx.prof_get()["quant_serial_chains"][1])
    ctx.prof_enable(False)
    return t["median_ms"], n


def _psnr(sse, n):
    return None if sse == 0 else float(10.0 * np.log10(65025.0 * n / sse))


def _job(ctx, fixed, frame_n):
    """entropy.dat's bytes and the worst predicted frame of the job the context is set up for (frame bounds, or none: abs b)"""
    def of(bound):
        rec = ctx.size_probe("abs", [bound], True, CODER)
        sse = ctx.bound_probe("abs", [bound])["sse"].astype(np.int64)
        worst = max(int(s) for s, fx in zip(sse, fixed) if not fx)
        return dict(entropy_dat_bytes=int(ratetarget.file_bytes(rec, CODER)), match_distance=int(rec["dist"]),
                    worst_predicted_frame_sse=worst, worst_predicted_frame_psnr_db=_psnr(worst, frame_n),
                    sequence_psnr_db=_psnr(int(sse.sum()), frame_n * len(sse)))
    return of


def main():
    date = datetime.date.today().isoformat()
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "frame_bounds_%s.json" % date)
    cfg = PredNetConfig()
    wts = cfg.init_weights(seed=3)
    frames = synth.turbulence(NT, H, W, seed=3)
    ctx = _lib.Context(0)
    ctx.load_model(cfg, wts)
    ctx.prepare(H, W, 20)
    doc = dict(date=date, definition=frametarget.DEFINITION, target_psnr_db=TARGET, coder=CODER,
               job="cfg3: 512x512, 80 frames, -p 0 -w 20, entropy on, random weights (seed 3), synth.turbulence",
               runs="%d per search, first dropped, median; spread = [min, max]; 3 per probe" % RUNS)
    try:
        key, _ = ctx.rollout(frames, 0, WINDOW)
        fixed = frametarget.fixed_frames(key, 0)
        frame_n, n = H * W * 3, int(frames.size)
        limit_f, limit_s = target.sse_limit(TARGET, frame_n), target.sse_limit(TARGET, n)

        def frame_probe(cand):
            ctx.set_frame_bounds([target.bound_of(c) for c in cand])
            return ctx.bound_probe("abs", [0.0])["sse"]

        def seq_probe(k):
            return int(ctx.bound_probe("abs", [target.bound_of(k)])["sse"].sum())

        ctx.prof_enable(False)
        (ks, sse, trace), t_frame = _timed(ctx, lambda: frametarget.search(frame_probe, limit_f, fixed), RUNS)
        ctx.set_frame_bounds(None)
        (k_seq, trace_seq), t_seq = _timed(ctx, lambda: target.search(seq_probe, limit_s), RUNS)
        per_probe = []
        for t in trace:
            cand = [0 if c is None else c for c in t["k"]]
            ms, serial = _serial(ctx, lambda: frame_probe(cand))
            searched = [c for c in t["k"] if c is not None]
            per_probe.append(dict(k_min=min(searched), k_max=max(searched), frames_at_k127=sum(c == 127 for c in searched), median_ms=ms,
                                  quant_serial_chains=serial))
        ctx.set_frame_bounds(None)
        per_probe_seq = []
        for t in trace_seq:
            ms, serial = _serial(ctx, lambda: seq_probe(t["k"]))
            per_probe_seq.append(dict(k=t["k"], bound=t["bound"], median_ms=ms, quant_serial_chains=serial))
        doc["search"] = dict(per_frame=dict(t_frame, probes=len(trace), sse_limit=limit_f, per_probe=per_probe),
                             sequence=dict(t_seq, probes=len(trace_seq), sse_limit=limit_s, k=k_seq, bound=target.bound_of(k_seq),
                                           per_probe=per_probe_seq))
        bounds = [0.0 if fx else target.bound_of(k) for k, fx in zip(ks, fixed)]
        searched = [b for b, fx in zip(bounds, fixed) if not fx]
        doc["frame_bounds"] = bounds
        doc["frames_searched"] = len(searched)
        job = _job(ctx, fixed, frame_n)
        ctx.set_frame_bounds(bounds)
        jobs = {"per_frame": dict(job(0.0), bounds="%g..%g" % (min(searched), max(searched)))}
        ctx.set_frame_bounds(None)
        jobs["sequence_target"] = dict(job(target.bound_of(k_seq)), bound=target.bound_of(k_seq))
        jobs["uniform_same_floor"] = dict(job(min(searched)), bound=min(searched))
        doc["jobs"] = jobs
        doc["per_frame_bytes_over_uniform_same_floor"] = jobs["per_frame"]["entropy_dat_bytes"] / jobs["uniform_same_floor"]["entropy_dat_bytes"]
    finally:
        ctx.close()
    doc["notes"] = ("search: HIP events on the context's stream around the Python call, profiling off; it includes the host's steps between "
                    "the probes (every probe returns its records to the host, a per-frame probe also uploads its bounds).  per_probe: each "
                    "probe again on its own; quant_serial_chains from one more run with profiling on.  jobs: entropy_dat_bytes is "
                    "ratetarget.file_bytes of tz_size_probe's record, the exact size of the huffd file the job writes; the PSNR figures "
                    "are from tz_bound_probe's per-frame sse, the records --report prints; worst_predicted_frame is over the frames "
                    "that are not stored exactly.")
    print(json.dumps(doc))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
