#!/usr/bin/env python3
"""What a PSNR floor found inside the closed loop (`-c --loop closed --quant lattice --loop-psnr DB`, definition TZ-CLF1,
tezip_amd/closedframes.py) costs and buys with the closed-loop profile's TRAINED model (scripts/closedloop_profile.py train) on
cfg2's job (40 frames of 128x160 synth.translating_scene) and cfg3's (80 frames of 512x512 synth.turbulence), `-p 0 -w 20`, at 36
and 40 dB.

  python scripts/closedframes_profile.py run OUT.json MODEL_DIR JOB
      one process of this build.  Device time (HIP events on the context's stream, 7 calls behind one warm-up call, median) of
      tz_rollout_closed_frames searching at 36 and 40 dB, and of tz_rollout_closed at abs median(found bounds) for the same
      process; the bounds found; the files of the closed job under them and of what a user could do before for the same floor,
      the OPEN-loop `--target-psnr DB --per-frame --quant lattice` job: entropy.dat + key_frame.dat in the default format (flat,
      zstd-9: compress.pack_outputs) and under `--coder huffd --sdelta auto` (the exact size of the smallest layout's file from
      tz_sdelta_probe; key_frame.dat zstd-9).
  python scripts/closedframes_profile.py parent OUT.json MODEL_DIR JOB NEW.json --root TREE
      one process of a build of the parent commit in TREE: tz_rollout_closed at abs median(the bounds NEW.json found), timed the
      same way.
  python scripts/closedframes_profile.py merge OUT.json NEW1.json [...] --parent P1.json [...]
      the medians over the processes of each build (run them alternating).  Default OUT: profiles/closed_frames_<date>.json

Expected, written down before the first run and nobody has measured it: the search adds 9 small launches a step, about 170 on
cfg3, a few ms on a 43 ms rollout; each probe reads 5 B/sample, which should hit in the last-level cache after the first round.
The files: smaller than the open-loop per-frame job's, as the closed-loop tables suggest."""
import datetime
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from closedloop_profile import JOBS, RUNS, _timed, job_frames  # noqa: E402

TARGETS = (36.0, 40.0)
WINDOW = 20


def _files(ctx, frames, key):
    """[entropy.dat, key_frame.dat] in the default format and under huffd + auto, of the job the context is set up for"""
    from tezip_amd import compress, sdauto
    payload, table, _ = ctx.encode("abs", [0.0], True)
    kb, eb = compress.pack_outputs(frames, key, np.asarray(payload), table, 0)
    chosen, sizes = sdauto.choose(ctx.sdelta_probe("abs", [0.0], True, "huffd"), "huffd")
    return dict(zstd=[len(eb), len(kb)], huffd_auto=[int(min(s for s in sizes if s is not None)), len(kb), chosen])


def _context(model_dir, frames):
    from tezip_amd import _lib, weights
    cfg, wts, _ = weights.load_model(model_dir)
    nt, h, w, _ = frames.shape
    ctx = _lib.Context(0)
    ctx.load_model(cfg, wts)
    ctx.prepare(_lib.pad8(h), _lib.pad8(w), max(1, (nt + WINDOW - 1) // WINDOW))
    ctx.prof_enable(False)
    ctx.set_quantiser("lattice")
    return ctx


def _dump(out, doc):
    print(json.dumps(doc))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


def run(out, model_dir, job):
    from tezip_amd import frametarget, target
    frames = job_frames(job)
    nt, h, w, _ = frames.shape
    ctx = _context(model_dir, frames)
    doc = dict(definition="TZ-CLF1", job=job, frames=[nt, h, w], window=WINDOW, targets={})
    try:
        for db in TARGETS:
            limit = target.sse_limit(db, h * w * 3)
            cell = dict(sse_limit=limit)
            ctx.set_frame_bounds(None)
            cell["rollout_closed_frames_search"] = _timed(ctx, lambda: ctx.rollout_closed_frames(frames, 0, WINDOW, sse_limit=limit))
            key = ctx.rollout_closed_frames(frames, 0, WINDOW, sse_limit=limit)
            found, sse = ctx.loop_frame_bounds()
            searched = found[~key]
            cell["bounds"] = dict(min=float(searched.min()), median=float(np.median(searched)), max=float(searched.max()),
                                  worst_sse=int(sse.max()))
            ctx.set_frame_bounds(found)
            cell["closed"] = _files(ctx, frames, key)
            ctx.set_frame_bounds(None)
            cell["rollout_closed_frames_given"] = _timed(ctx, lambda: ctx.rollout_closed_frames(frames, 0, WINDOW, bounds=found))
            med = [float(np.median(searched))]
            cell["rollout_closed_at_median"] = _timed(ctx, lambda: ctx.rollout_closed(frames, 0, WINDOW, "abs", med))
            # the open-loop job for the same floor (TZ-TPSNR-F1)
            key, _ = ctx.rollout(frames, 0, WINDOW)
            fixed = frametarget.fixed_frames(key, 0)

            def probe(cand):
                ctx.set_frame_bounds([target.bound_of(c) for c in cand])
                return ctx.bound_probe("abs", [0.0])["sse"]

            ks, _, _ = frametarget.search(probe, limit, fixed)
            ctx.set_frame_bounds([0.0 if fx else target.bound_of(k) for fx, k in zip(fixed, ks)])
            open_b = np.array([target.bound_of(k) for fx, k in zip(fixed, ks) if not fx])
            cell["open_bounds"] = dict(min=float(open_b.min()), median=float(np.median(open_b)), max=float(open_b.max()))
            cell["open"] = _files(ctx, frames, key)
            for fmt in ("zstd", "huffd_auto"):
                cell["closed_over_open_" + fmt] = sum(cell["closed"][fmt][:2]) / sum(cell["open"][fmt][:2])
            doc["targets"]["%g" % db] = cell
    finally:
        ctx.close()
    _dump(out, doc)


def parent(out, model_dir, job, new):
    frames = job_frames(job)
    new = json.load(open(new))
    ctx = _context(model_dir, frames)
    doc = dict(job=job, parent=True, targets={})
    try:
        for db, cell in new["targets"].items():
            med = [cell["bounds"]["median"]]
            doc["targets"][db] = dict(rollout_closed_at_median=_timed(ctx, lambda: ctx.rollout_closed(frames, 0, WINDOW, "abs", med)))
    finally:
        ctx.close()
    _dump(out, doc)


def merge(out, new, old):
    new, old = [json.load(open(p)) for p in new], [json.load(open(p)) for p in old]
    doc = dict(date=datetime.date.today().isoformat(), definition="TZ-CLF1", jobs={},
               model="the closed-loop profile's: PredNet (3,48,96,192), tezip_amd/train.py's default 100 x 5 steps on ten held-out 128x128 sequences of the job's generator",
               runs="per process %d calls behind one warm-up call, median; then the median over the fresh processes of each build, alternating" % RUNS)
    for job in sorted({d["job"] for d in new}):
        mine, theirs = [d for d in new if d["job"] == job], [d for d in old if d["job"] == job]
        cell = dict(frames=mine[0]["frames"], window=mine[0]["window"], targets={})
        for db, first in mine[0]["targets"].items():
            t = {k: v for k, v in first.items() if not k.startswith("rollout_")}
            for what in ("rollout_closed_frames_search", "rollout_closed_frames_given", "rollout_closed_at_median"):
                xs = [d["targets"][db][what]["median_ms"] for d in mine]
                t[what] = dict(median_ms=float(np.median(xs)), processes_ms=xs)
            if theirs:
                xs = [d["targets"][db]["rollout_closed_at_median"]["median_ms"] for d in theirs]
                t["parent_rollout_closed_at_median"] = dict(median_ms=float(np.median(xs)), processes_ms=xs)
                t["search_over_parent"] = t["rollout_closed_frames_search"]["median_ms"] / float(np.median(xs))
                t["search_minus_parent_ms"] = t["rollout_closed_frames_search"]["median_ms"] - float(np.median(xs))
            cell["targets"][db] = t
        doc["jobs"][job] = cell
    doc["notes"] = ("times: HIP events on the context's stream, the whole entry point from host frames.  bytes: [entropy.dat, key_frame.dat]; "
                    "zstd = the default format's files, huffd_auto = the exact size of the smallest layout's TZR2 file (tz_sdelta_probe) + "
                    "the zstd key_frame.dat.  open = the open-loop --target-psnr DB --per-frame --quant lattice job.  Not measured: real "
                    "data, other models, -p > 0.")
    _dump(out, doc)
    print("wrote", out)


def main(argv):
    root = ROOT
    if "--root" in argv:
        i = argv.index("--root")
        root = os.path.abspath(argv[i + 1])
        argv = argv[:i] + argv[i + 2:]
    sys.path.insert(0, root)
    if len(argv) == 4 and argv[0] == "run" and argv[3] in JOBS:
        return run(argv[1], argv[2], argv[3])
    if len(argv) == 5 and argv[0] == "parent" and argv[3] in JOBS:
        return parent(argv[1], argv[2], argv[3], argv[4])
    if len(argv) >= 3 and argv[0] == "merge":
        rest = argv[2:]
        cut = rest.index("--parent") if "--parent" in rest else len(rest)
        return merge(argv[1] or os.path.join(ROOT, "profiles", "closed_frames_%s.json" % datetime.date.today().isoformat()), rest[:cut], rest[cut + 1:])
    print(__doc__)
    return 2


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
