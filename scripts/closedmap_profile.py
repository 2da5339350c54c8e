#!/usr/bin/env python3
"""What one abs bound per pixel inside the closed loop (`-c --loop closed --quant lattice -m abs --loop-map FILE`, definition
TZ-CLM1, tezip_amd/closedmap.py) costs and buys with the closed-loop profile's TRAINED model (scripts/closedloop_profile.py train)
on cfg3's job (80 frames of 512x512 synth.turbulence, `-p 0 -w 20`) under the bound-map profile's map: 0 inside a centred 128x128
box, 6 outside.

  python scripts/closedmap_profile.py run OUT.json MODEL_DIR
      one process of this build.  Device time (HIP events on the context's stream, 7 calls behind one warm-up call, median) of
      tz_rollout_closed_map under the box map and under a map that is 6 everywhere, and of tz_rollout_closed at abs 6; whether the
      uniform-6 map gives tz_rollout_closed's payload; the files of the map job and of what a user could do before for the same
      region of interest, the OPEN-loop `--bound-map --quant lattice` job: entropy.dat + key_frame.dat in the default format (flat,
      zstd-9: compress.pack_outputs) and under `--coder huffd --sdelta auto` (the exact size of the smallest layout's file from
      tz_sdelta_probe; key_frame.dat zstd-9).
  python scripts/closedmap_profile.py parent OUT.json MODEL_DIR --root TREE
      one process of a build of the parent commit in TREE: tz_rollout_closed at abs 6, timed the same way.
  python scripts/closedmap_profile.py merge OUT.json NEW1.json [...] --parent P1.json [...]
      the medians over the processes of each build (run them alternating).  Default OUT: profiles/closed_map_<date>.json

Expected, written down before the first run: the files land in the closed-loop profile's range for abs 6 against the open loop
(0.50-0.75x in the default format); tz_rollout_closed_map stays inside the parent's spread of tz_rollout_closed at abs 6 plus the
extra map read (H*W bytes a frame on top of 5 bytes a sample: under 7 % of the step kernel's traffic, which is itself a few
percent of a 43 ms rollout), under the box map and under the uniform one alike."""
import datetime
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from closedloop_profile import RUNS, _timed, job_frames  # noqa: E402

JOB, WINDOW, BOUND, BOX = "cfg3", 20, 6, 128


def box_map(h, w):
    m = np.full((h, w), BOUND, np.uint8)
    m[(h - BOX) // 2:(h + BOX) // 2, (w - BOX) // 2:(w + BOX) // 2] = 0
    return m


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


def run(out, model_dir):
    frames = job_frames(JOB)
    nt, h, w, _ = frames.shape
    ctx = _context(model_dir, frames)
    box, flat = box_map(h, w), np.full((h, w), BOUND, np.uint8)
    doc = dict(definition="TZ-CLM1", job=JOB, frames=[nt, h, w], window=WINDOW, map=dict(box=BOX, inside=0, outside=BOUND), times={})
    try:
        t = doc["times"]
        ctx.set_bound_map(None)
        t["rollout_closed_abs6"] = _timed(ctx, lambda: ctx.rollout_closed(frames, 0, WINDOW, "abs", [float(BOUND)]))
        payload, table, _ = ctx.encode("abs", [float(BOUND)], True)
        payload = np.asarray(payload).copy()
        ctx.set_bound_map(flat)
        t["rollout_closed_map_uniform6"] = _timed(ctx, lambda: ctx.rollout_closed_map(frames, 0, WINDOW))
        again, table2, _ = ctx.encode("abs", [0.0], True)
        doc["uniform6_equals_abs6"] = bool(np.array_equal(np.asarray(again), payload) and np.array_equal(table2, table))
        ctx.set_bound_map(box)
        t["rollout_closed_map_box"] = _timed(ctx, lambda: ctx.rollout_closed_map(frames, 0, WINDOW))
        key = ctx.rollout_closed_map(frames, 0, WINDOW)
        doc["closed"] = _files(ctx, frames, key)
        _, table, _ = ctx.encode("abs", [0.0], True, payload="resident")
        rec = ctx.encode_map_check("resident", table)
        doc["violations"] = int(rec["violations"].sum())
        key, _ = ctx.rollout(frames, 0, WINDOW)                      # the open-loop --bound-map --quant lattice job
        doc["open"] = _files(ctx, frames, key)
        for fmt in ("zstd", "huffd_auto"):
            doc["closed_over_open_" + fmt] = sum(doc["closed"][fmt][:2]) / sum(doc["open"][fmt][:2])
    finally:
        ctx.close()
    _dump(out, doc)


def parent(out, model_dir):
    frames = job_frames(JOB)
    ctx = _context(model_dir, frames)
    try:
        doc = dict(job=JOB, parent=True,
                   times=dict(rollout_closed_abs6=_timed(ctx, lambda: ctx.rollout_closed(frames, 0, WINDOW, "abs", [float(BOUND)]))))
    finally:
        ctx.close()
    _dump(out, doc)


def merge(out, new, old):
    new, old = [json.load(open(p)) for p in new], [json.load(open(p)) for p in old]
    doc = dict(date=datetime.date.today().isoformat(), **{k: v for k, v in new[0].items() if k != "times"})
    doc["model"] = "the closed-loop profile's: PredNet (3,48,96,192), tezip_amd/train.py's default 100 x 5 steps on ten held-out 128x128 sequences of the job's generator"
    doc["runs"] = "per process %d calls behind one warm-up call, median; then the median over the fresh processes of each build, alternating" % RUNS
    doc["uniform6_equals_abs6"] = all(d["uniform6_equals_abs6"] for d in new)
    doc["times"] = {}
    for what in new[0]["times"]:
        xs = [d["times"][what]["median_ms"] for d in new]
        doc["times"][what] = dict(median_ms=float(np.median(xs)), processes_ms=xs,
                                  spread_ms=[min(d["times"][what]["spread_ms"][0] for d in new), max(d["times"][what]["spread_ms"][1] for d in new)])
    if old:
        xs = [d["times"]["rollout_closed_abs6"]["median_ms"] for d in old]
        base = float(np.median(xs))
        doc["times"]["parent_rollout_closed_abs6"] = dict(
            median_ms=base, processes_ms=xs, spread_ms=[min(d["times"]["rollout_closed_abs6"]["spread_ms"][0] for d in old),
                                                        max(d["times"]["rollout_closed_abs6"]["spread_ms"][1] for d in old)])
        for what in ("rollout_closed_map_box", "rollout_closed_map_uniform6", "rollout_closed_abs6"):
            doc[what + "_over_parent"] = doc["times"][what]["median_ms"] / base
    doc["notes"] = ("times: HIP events on the context's stream, the whole entry point from host frames.  bytes: [entropy.dat, key_frame.dat]; "
                    "zstd = the default format's files, huffd_auto = the exact size of the smallest layout's TZR2 file (tz_sdelta_probe) + "
                    "the zstd key_frame.dat.  open = the open-loop --bound-map --quant lattice job under the same map.  Not measured: "
                    "--pred select under the map, real data, other models and maps, -p > 0.")
    _dump(out, doc)
    print("wrote", out)


def main(argv):
    root = ROOT
    if "--root" in argv:
        i = argv.index("--root")
        root = os.path.abspath(argv[i + 1])
        argv = argv[:i] + argv[i + 2:]
    sys.path.insert(0, root)
    if len(argv) == 3 and argv[0] == "run":
        return run(argv[1], argv[2])
    if len(argv) == 3 and argv[0] == "parent":
        return parent(argv[1], argv[2])
    if len(argv) >= 3 and argv[0] == "merge":
        rest = argv[2:]
        cut = rest.index("--parent") if "--parent" in rest else len(rest)
        return merge(argv[1] or os.path.join(ROOT, "profiles", "closed_map_%s.json" % datetime.date.today().isoformat()), rest[:cut], rest[cut + 1:])
    print(__doc__)
    return 2


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
