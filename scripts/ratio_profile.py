#!/usr/bin/env python3
"""Cost of `-c --target-ratio` (definition TZ-TRATIO-1, tezip_amd/ratetarget.py) on cfg3's job: 80 frames of 512x512 synthetic
turbulence, random weights (seed 3), `-p 0 -w 20 --coder huffd`, two targets.
Part 1, the command line: both targets as fresh processes on the same PNG files (wall time, bound_search.json: the probes).
Part 2, one process, HIP events on the context's stream: every probe of both searches on its own (tz_size_probe, profiling off,
4 runs, first dropped, median), its profiling classes with profiling on (delta, quant, huffman = k_size_count + k_size_bits), and
the two kernels alone through their seams on the probe's own quantised delta stack (k_size_count, k_size_bits: time and bytes
per element moved -- each reads the 2-byte stack once).
Part 3, the baseline of a probe: the chain a host loop over the existing entry points would run for one candidate -- tz_encode
(resident payload) + tz_huffd_counts + the host's choice + tz_huffd_encode -- against tz_size_probe, as ALTERNATING FRESH
PROCESSES (`--child chain|probe`), median of 3 after one warm-up pair.  With --parent TREE the chain runs in that tree (a checkout
of the parent commit with its library built), else in this one.  tz_huffd_encode cannot stop behind its size pass, so the chain
includes the pack pass a size-only loop would not need: the baseline is an upper bound of it.
Usage: python scripts/ratio_profile.py [--parent TREE] [out.json]      (default: profiles/target_ratio_<date>.json)"""
import datetime
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.environ.get("TEZIP_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tezip_amd import _lib, huffd, synth, weights  # noqa: E402
from tezip_amd.prednet import PredNetConfig  # noqa: E402

NT, H, W, WINDOW = 80, 512, 512, 20
TARGETS = (4.0, 8.0)
CODER = "huffd"
CLI_LIMIT_S = 240   # a command-line job here takes a few seconds: a hung one ends the script instead of holding the GPU


def _job():
    cfg = PredNetConfig()
    return cfg, cfg.init_weights(seed=3), synth.turbulence(NT, H, W, seed=3)


def _context(cfg, wts, frames):
    ctx = _lib.Context(0)
    ctx.load_model(cfg, wts)
    ctx.prepare(H, W, 20)
    ctx.rollout(frames, 0, WINDOW)
    return ctx


def _ms(ctx, fn, runs=4):
    out = []
    for _ in range(runs):
        ctx.timer_start()
        fn()
        out.append(float(ctx.timer_stop()))
    return dict(median_ms=float(np.median(out[1:])), spread_ms=[min(out[1:]), max(out[1:])])


def _chain(ctx, bound):
    """one candidate by the existing entry points -> the bytes of its stream"""
    ctx.encode("abs", [bound], True, payload="resident")
    counts, base = ctx.huffd_counts()
    dist, lengths, _ = huffd.choose(counts)
    return ctx.huffd_encode(lengths, base, dist)


def child(kind, bounds):
    """a fresh process: the rollout, then per bound the device time of one candidate (4 runs, first dropped, median)"""
    cfg, wts, frames = _job()
    ctx = _context(cfg, wts, frames)
    try:
        out = {}
        for b in bounds:
            fn = (lambda: _chain(ctx, b)) if kind == "chain" else (lambda: ctx.size_probe("abs", [b], True, CODER))
            got = fn()
            out[repr(b)] = dict(_ms(ctx, fn), bytes=int(got if kind == "chain" else got["bytes"]))
        print("RESULT " + json.dumps(out))
    finally:
        ctx.close()


def _child(tree, kind, bounds):
    r = subprocess.run(["timeout", "-k", "10", str(CLI_LIMIT_S), sys.executable, os.path.abspath(__file__), "--child", kind] + [repr(b) for b in bounds],
                       capture_output=True, text=True, env=dict(os.environ, TEZIP_TREE=tree), timeout=CLI_LIMIT_S + 30)
    if r.returncode != 0:
        raise RuntimeError("%s child in %s failed:\n%s\n%s" % (kind, tree, r.stdout[-2000:], r.stderr[-2000:]))
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def baseline_part(parent, bounds):
    rounds = []
    for i in range(4):   # (pair 0 warms the code-object cache)
        rounds.append((_child(ROOT, "probe", bounds), _child(parent or ROOT, "chain", bounds)))
    out = {}
    for b in bounds:
        p = [r[0][repr(b)]["median_ms"] for r in rounds[1:]]
        c = [r[1][repr(b)]["median_ms"] for r in rounds[1:]]
        assert len({r[0][repr(b)]["bytes"] for r in rounds} | {r[1][repr(b)]["bytes"] for r in rounds}) == 1, "probe and chain disagree"
        out[repr(b)] = dict(probe_ms=p, probe_median_ms=float(np.median(p)), chain_ms=c, chain_median_ms=float(np.median(c)),
                            probe_over_chain=float(np.median(p) / np.median(c)), stream_bytes=rounds[0][0][repr(b)]["bytes"])
    return dict(chain_tree="parent commit" if parent else "this tree (no --parent given)", per_bound=out)


def _cli(args):
    t0 = time.perf_counter()
    r = subprocess.run(["timeout", "-k", "10", str(CLI_LIMIT_S), sys.executable, "-m", "tezip_amd.tezip"] + args, cwd=ROOT,
                       capture_output=True, text=True, env=dict(os.environ, TEZIP_TIMING="1"), timeout=CLI_LIMIT_S + 30)
    dt = time.perf_counter() - t0
    if r.returncode != 0:
        raise RuntimeError("%r failed:\n%s\n%s" % (args, r.stdout[-2000:], r.stderr[-2000:]))
    stage = [ln for ln in r.stderr.splitlines() if "bound search" in ln]
    return dt, (float(stage[0].split()[-5]) if stage else None), [ln for ln in r.stdout.splitlines() if ln.startswith("target: ")]


def cli_part(cfg, wts, frames):
    from PIL import Image
    tmp = tempfile.mkdtemp(prefix="ratio_profile_")
    try:
        mdir, ddir = os.path.join(tmp, "model"), os.path.join(tmp, "data")
        weights.save_model(mdir, cfg, wts, H, W)
        os.mkdir(ddir)
        for t in range(len(frames)):
            Image.fromarray(frames[t]).save(os.path.join(ddir, "f_%03d.png" % t))
        out = {}
        for R in TARGETS:
            runs = []
            for i in range(4):   # (run 0 warms the file cache and the code-object cache)
                odir = os.path.join(tmp, "out_%g_%d" % (R, i))
                runs.append(_cli(["-c", mdir, ddir, odir, "-p", "0", "-w", str(WINDOW), "--coder", CODER, "--target-ratio", repr(R)]))
            doc = json.load(open(os.path.join(odir, "bound_search.json")))
            assert os.path.getsize(os.path.join(odir, "entropy.dat")) == doc["result"]["entropy_bytes"]
            out[repr(R)] = dict(wall_s=[r[0] for r in runs[1:]], wall_median_s=float(np.median([r[0] for r in runs[1:]])),
                                search_stage_s=[r[1] for r in runs[1:]], line=runs[-1][2], bound_search=doc)
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def device_part(ctx, searches):
    n = NT * H * W * 3
    ks = sorted({t["k"] for doc in searches for t in doc["trace"]})
    per_probe = {}
    for k in ks:
        b = k / 2.0
        ctx.prof_enable(False)
        rec = dict(bound=b, probe=_ms(ctx, lambda: ctx.size_probe("abs", [b], True, CODER)))
        ctx.prof_enable(True)
        for _ in range(2):
            ctx.prof_reset()
            ctx.size_probe("abs", [b], True, CODER)
        prof = {c: v for c, v in ctx.prof_get().items() if v[1]}
        rec["classes_ms_with_profiling_on"] = {c: float(v[0]) for c, v in prof.items()}
        rec["launches"] = {c: int(v[1]) for c, v in prof.items()}
        # the two kernels alone, on this candidate's quantised delta stack (staged to the device outside the timed scope: the
        # profiling class brackets the kernel alone)
        _, table, q = ctx.encode("abs", [b], True, want_delta=True)
        tq = np.ascontiguousarray(q).reshape(-1)
        lens = np.full(_lib.SIZE_BINS + 8, 8, np.uint8)
        for name, fn in (("k_size_count", lambda: ctx.size_count_buf(tq, 3, 1, True)), ("k_size_bits", lambda: ctx.size_bits_buf(tq, lens, 3, 3, 1, True))):
            for _ in range(3):
                ctx.prof_reset()
                fn()
            ms = float(ctx.prof_get()["huffman"][0])
            rec[name] = dict(ms=ms, bytes_per_element=2.0, tb_per_s=2.0 * n / (ms * 1e-3) / 1e12)
        del tq
        per_probe[str(k)] = rec
    ctx.prof_enable(False)
    return dict(elements=n, per_probe=per_probe)


def main():
    args = sys.argv[1:]
    if args and args[0] == "--child":
        return child(args[1], [float(a) for a in args[2:]])
    parent = None
    if args and args[0] == "--parent":
        parent, args = os.path.abspath(args[1]), args[2:]
    date = datetime.date.today().isoformat()
    out = args[0] if args else os.path.join(ROOT, "profiles", "target_ratio_%s.json" % date)
    cfg, wts, frames = _job()
    doc = dict(date=date, definition="TZ-TRATIO-1", targets=list(TARGETS), coder=CODER,
               job="cfg3: 512x512, 80 frames, -p 0 -w 20, entropy on, --coder huffd, random weights (seed 3), synth.turbulence")
    doc["cli"] = cli_part(cfg, wts, frames)
    print("cli", json.dumps({R: (v["line"], v["wall_median_s"]) for R, v in doc["cli"].items()}), flush=True)
    ctx = _context(cfg, wts, frames)
    try:
        doc["device"] = device_part(ctx, [v["bound_search"] for v in doc["cli"].values()])
    finally:
        ctx.close()
    print("device", json.dumps(doc["device"]), flush=True)
    bounds = sorted({v["bound_search"]["result"]["bound"] for v in doc["cli"].values() if v["bound_search"]["result"]} | {0.0})
    doc["baseline"] = baseline_part(parent, bounds)
    print("baseline", json.dumps(doc["baseline"]), flush=True)
    doc["notes"] = ("cli: fresh processes of the command line, PNG decoding, model load, key-frame zstd-9 and file writes included; "
                    "search_stage_s is the TEZIP_TIMING stage `key_frame.dat + bound search (device)`.  device.per_probe: tz_size_probe "
                    "at every candidate either search visited, HIP events around the Python call, profiling off; classes with "
                    "profiling on: delta = tzk_delta, quant = the quantiser's launches, huffman = k_size_count + k_size_bits; "
                    "k_size_count / k_size_bits: each kernel alone through its seam on the candidate's quantised delta stack, 2 B per "
                    "element read, nothing written but counters.  baseline: device time of one candidate by tz_size_probe against the "
                    "chain tz_encode (resident) + tz_huffd_counts + huffd.choose + tz_huffd_encode, alternating fresh processes, median "
                    "of 3 process medians after a warm-up pair; the chain includes tz_huffd_encode's pack pass.")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
