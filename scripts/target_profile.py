#!/usr/bin/env python3
"""Cost of `-c --target-psnr` (definition TZ-TPSNR-1, tezip_amd/target.py) on cfg3's job: 80 frames of 512x512 synthetic
turbulence, random weights (seed 3), `-p 0 -w 20`, target 40 dB.
Part 1, in one process, HIP events on the context's stream (tz_timer_start / tz_timer_stop): the rollout, one tz_bound_probe
(at the bound the search finds; the profiling classes inside it: delta, quantiser, k_bound_err), the whole search
(every probe plus the host's steps between them), 7 runs each, first dropped, median, and every probe of the search on its own.
Part 2, optional: wall time of the command line with the flag against `-m abs -b <found>` run by ANOTHER tree (a checkout
of the parent commit with its library built), as fresh processes on the same PNG files, alternating, median of 3 after one
warm-up each; the two output directories must hold the same three files.
Usage: python scripts/target_profile.py [--parent TREE] [out.json]      (default: profiles/target_psnr_<date>.json)"""
import datetime
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tezip_amd import _lib, synth, target, weights  # noqa: E402
from tezip_amd.prednet import PredNetConfig  # noqa: E402

RUNS = 7
TARGET = 40.0
NT, H, W, WINDOW = 80, 512, 512, 20


def _timed(ctx, fn):
    ctx.prof_reset()
    ctx.timer_start()
    out = fn()
    ms = float(ctx.timer_stop())
    return out, ms, {k: (float(v[0]), int(v[1])) for k, v in ctx.prof_get().items() if v[1]}


def _med(xs):
    xs = list(xs)[1:]   # (the first run warms pools and code objects)
    return dict(median_ms=float(np.median(xs)), spread_ms=[min(xs), max(xs)], all_ms=xs)


def device_part(ctx, frames):
    n = int(frames.size)
    limit = target.sse_limit(TARGET, n)
    probe = lambda k: int(ctx.bound_probe("abs", [target.bound_of(k)])["sse"].sum())   # noqa: E731
    ctx.prof_enable(False)   # (profiling on puts events around every launch: rollout, search and probe are timed without it)
    rollout_ms = []
    for _ in range(4):
        ctx.timer_start()
        ctx.rollout(frames, 0, WINDOW)
        rollout_ms.append(float(ctx.timer_stop()))
    search_ms, k, trace = [], None, None
    for _ in range(RUNS):
        ctx.timer_start()
        k, trace = target.search(probe, limit)
        search_ms.append(float(ctx.timer_stop()))
    probe_ms = []
    for _ in range(RUNS):
        ctx.timer_start()
        probe(k)
        probe_ms.append(float(ctx.timer_stop()))
    per_probe = []   # every probe of the search on its own: the quantiser's time depends on the bound
    for t in trace:
        ms = []
        for _ in range(4):
            ctx.timer_start()
            probe(t["k"])
            ms.append(float(ctx.timer_stop()))
        per_probe.append(dict(k=t["k"], bound=t["bound"], median_ms=float(np.median(ms[1:]))))
    ctx.prof_enable(True)
    classes = None
    for _ in range(3):
        _, _, classes = _timed(ctx, lambda: probe(k))
    for t in per_probe:
        _, _, c = _timed(ctx, lambda: probe(t["k"]))
        t["classes_ms_with_profiling_on"] = {name: v[0] for name, v in c.items()}
    # what the found bound does, by the entry points the definition rests on
    _, table, _ = ctx.encode("abs", [target.bound_of(k)], True, payload="resident")
    q = ctx.encode_quality("resident", table)
    sse = int(q["sse"].astype(np.int64).sum())
    by_k = {t["k"]: t for t in trace}
    assert by_k[k]["sse"] == sse <= limit and (k == target.K_MAX or by_k[k + 1]["sse"] > limit)
    r, s, p = _med(rollout_ms), _med(search_ms), _med(probe_ms)
    return dict(samples=n, sse_limit=limit, k=k, bound=target.bound_of(k), sse=sse, probes=len(trace), trace=trace,
                psnr_db_of_result=10.0 * np.log10(65025.0 * n / sse) if sse else None,
                rollout=r, search=s, one_probe=p, search_over_rollout=s["median_ms"] / r["median_ms"],
                per_probe=per_probe, sum_of_per_probe_ms=float(sum(t["median_ms"] for t in per_probe)),
                one_probe_classes_ms_with_profiling_on={c: v[0] for c, v in classes.items()},
                one_probe_launches={c: v[1] for c, v in classes.items()},
                k_bound_err_tb_per_s=5.0 * n / (classes["quality"][0] * 1e-3) / 1e12)


CLI_LIMIT_S = 180   # a command-line job here takes about 3 s: a hung one ends the script instead of holding the GPU


def _cli(tree, args):
    t0 = time.perf_counter()
    r = subprocess.run(["timeout", "-k", "10", str(CLI_LIMIT_S), sys.executable, "-m", "tezip_amd.tezip"] + args, cwd=tree,
                       capture_output=True, text=True, env=dict(os.environ, TEZIP_TIMING="1"), timeout=CLI_LIMIT_S + 30)
    dt = time.perf_counter() - t0
    if r.returncode != 0:
        raise RuntimeError("%s %r failed:\n%s\n%s" % (tree, args, r.stdout[-2000:], r.stderr[-2000:]))
    stage = [ln for ln in r.stderr.splitlines() if "bound search" in ln]
    return dt, (float(stage[0].split()[-5]) if stage else None)


def wall_part(parent, frames, cfg, wts, bound):
    from PIL import Image
    tmp = tempfile.mkdtemp(prefix="target_profile_")
    try:
        mdir, ddir = os.path.join(tmp, "model"), os.path.join(tmp, "data")
        weights.save_model(mdir, cfg, wts, H, W)
        os.mkdir(ddir)
        for t in range(len(frames)):
            Image.fromarray(frames[t]).save(os.path.join(ddir, "f_%03d.png" % t))
        job = ["-p", "0", "-w", str(WINDOW)]
        flag, plain = [], []
        for i in range(4):   # (run 0 of each warms the file cache and the code-object cache)
            out_f, out_p = os.path.join(tmp, "out_flag_%d" % i), os.path.join(tmp, "out_parent_%d" % i)
            flag.append(_cli(ROOT, ["-c", mdir, ddir, out_f] + job + ["--target-psnr", repr(TARGET)]))
            plain.append(_cli(parent, ["-c", mdir, ddir, out_p] + job + ["-m", "abs", "-b", repr(bound)])[0])
            same = all(open(os.path.join(out_f, n), "rb").read() == open(os.path.join(out_p, n), "rb").read()
                       for n in ("filename.txt", "key_frame.dat", "entropy.dat"))
            assert same, "the flagged job and the parent's -m abs -b %r wrote different files" % bound
        f, p = [x[0] for x in flag[1:]], plain[1:]
        return dict(with_flag_s=f, with_flag_median_s=float(np.median(f)), parent_abs_s=p, parent_abs_median_s=float(np.median(p)),
                    extra_s=float(np.median(f) - np.median(p)), bound_search_stage_s=[x[1] for x in flag[1:]],
                    files_identical=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    args = sys.argv[1:]
    parent = None
    if args and args[0] == "--parent":
        parent, args = os.path.abspath(args[1]), args[2:]
    date = datetime.date.today().isoformat()
    out = args[0] if args else os.path.join(ROOT, "profiles", "target_psnr_%s.json" % date)
    cfg = PredNetConfig()
    wts = cfg.init_weights(seed=3)
    frames = synth.turbulence(NT, H, W, seed=3)
    ctx = _lib.Context(0)
    ctx.load_model(cfg, wts)
    ctx.prepare(H, W, 20)
    doc = dict(date=date, definition=target.DEFINITION, target_psnr_db=TARGET,
               job="cfg3: 512x512, 80 frames, -p 0 -w 20, entropy on, random weights (seed 3), synth.turbulence",
               runs="%d per figure (rollout 4), first dropped, median; spread = [min, max]" % RUNS)
    try:
        doc["device"] = device_part(ctx, frames)
    finally:
        ctx.close()
    print("device", json.dumps(doc["device"]), flush=True)
    if parent:
        doc["wall"] = wall_part(parent, frames, cfg, wts, doc["device"]["bound"])
        print("wall", json.dumps(doc["wall"]), flush=True)
    else:
        doc["wall"] = "not measured (no --parent tree given)"
    doc["notes"] = ("rollout / search / one_probe: HIP events on the context's stream around the Python call(s), profiling off for the "
                    "search and the probe; the search includes the host's steps between its probes (each probe returns its records "
                    "to the host).  one_probe_classes: the profiling classes of one probe with profiling on (events around every "
                    "launch): delta = tzk_delta, quant = the quantiser's launches, quality = k_bound_err alone; k_bound_err_tb_per_s "
                    "= 5 B per element over that time.  wall: fresh processes of the command line, PNG decoding, model load, "
                    "zstd-9 and file writes included; bound_search_stage_s is the TEZIP_TIMING stage of the flagged run.")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
