#!/usr/bin/env python3
"""What motion-compensated tiles (`-c --loop closed --pred motion`, definition TZ-PM1, tezip_amd/predmotion.py) buy and cost on
cfg2's job (40 frames of 128x160 synth.translating_scene) and cfg3's job (80 frames of 512x512 synth.turbulence), `-p 0 -w 20`,
with RANDOM weights (PredNetConfig().init_weights(seed=123), bench.py's model) and with the model scripts/closedloop_profile.py
trains -- against `--pred select` and against `--loop closed` alone.

  python scripts/closedloop_profile.py train MODEL_DIR JOB
      the trained model (see that script).
  python scripts/predmotion_profile.py run OUT.json JOB [--model MODEL_DIR] [--root TREE] [--sizes]
      one process; the model of MODEL_DIR, random weights without one.  --root: import tezip_amd from another tree (a build of the
      parent commit: the rows that need tz_set_pred_motion are then left out, the same file serves both builds).
      times   HIP events on the context's stream, 7 calls behind one warm-up call, median: tz_rollout_closed lossless and at abs 6
              lattice and tz_rollout_decode_closed of both, without a second candidate ("net"), under selection ("select") and --
              this build -- under motion ("motion").
      --sizes entropy.dat + key_frame.dat (+ pred_modes.dat) of the three jobs, lossless and at abs 2 / abs 6 under the lattice
              quantiser: under the default format (flat layout, zstd-9) and under `--coder huffd --sdelta auto` (the exact size of
              the smallest layout's file from tz_sdelta_probe; key_frame.dat zstd-9); the tiles taken from the frame in front and
              how many of them are displaced.
  python scripts/predmotion_profile.py merge OUT.json NEW1.json [...] --parent P1.json [...]
      the sizes of the first NEW file of each (job, model) that has them, the medians of the times over the processes of each build
      (run them alternating) and the parent's run-to-run spread.  Default OUT: profiles/pred_motion_<date>.json

No threshold is fixed in advance.  Expected, to be confirmed or refuted in writing: motion's rollout within about 1 ms of select's
on cfg3 (2.5 M wave instructions per 512x512 frame by arithmetic); cfg2 with the trained model takes displaced tiles and gets
smaller; turbulence gains nothing."""
import datetime
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import closedloop_profile as CL  # noqa: E402  (JOBS, BOUNDS, job_frames, _timed, _key_stack)
import predselect_profile as PS  # noqa: E402  (_model, WINDOW)

WINDOW = PS.WINDOW


def _preds(ctx):
    return ("net",) + (("select",) if hasattr(ctx, "set_pred_select") else ()) + (("motion",) if hasattr(ctx, "set_pred_motion") else ())


def _set(ctx, pred):
    if hasattr(ctx, "set_pred_motion"):
        ctx.set_pred_motion(0)
    if hasattr(ctx, "set_pred_select"):
        ctx.set_pred_select(pred == "select")
    if pred == "motion":
        ctx.set_pred_motion(7)


def _sizes(ctx, frames):
    """{bound: {pred: {zstd: [entropy, key, modes], huffd_auto: [entropy, key, modes, layout], prev_tiles, displaced_tiles, tiles}}}"""
    from tezip_amd import compress, predselect, sdauto
    out = {}
    for name, bound, quant in CL.BOUNDS:
        cell = {}
        ctx.set_quantiser(quant)
        for pred in _preds(ctx):
            _set(ctx, pred)
            key = ctx.rollout_closed(frames, 0, WINDOW, "abs", bound)
            msize, extra = 0, {}
            if pred != "net":
                modes = ctx.pred_modes()
                extra = dict(tiles=int(modes[~key].size), prev_tiles=int(np.count_nonzero(modes)))
                if pred == "motion":
                    from tezip_amd import predmotion   # (not in a build of the parent commit, which never gets here)
                    vectors = ctx.pred_vectors()
                    msize = len(predmotion.pack(modes, vectors))
                    extra["displaced_tiles"] = int(np.count_nonzero(vectors.any(axis=-1)))
                else:
                    msize = len(predselect.pack(modes))
            payload, table, _ = ctx.encode("abs", bound, True)
            kb, eb = compress.pack_outputs(frames, key, np.asarray(payload), table, 0)
            chosen, sizes = sdauto.choose(ctx.sdelta_probe("abs", bound, True, "huffd"), "huffd")
            best = min(s for s in sizes if s is not None)
            cell[pred] = dict(zstd=[len(eb), len(kb), msize], huffd_auto=[int(best), len(kb), msize, chosen], **extra)
        if "motion" in cell:
            for fmt in ("zstd", "huffd_auto"):
                for other in ("net", "select"):
                    cell["motion_over_%s_%s" % (other, fmt)] = sum(cell["motion"][fmt][:3]) / sum(cell[other][fmt][:3])
        out[name] = cell
    ctx.set_quantiser("greedy")
    _set(ctx, "net")
    return out


def run(out, job, model_dir, sizes):
    from tezip_amd import _lib
    cfg, wts, model = PS._model(model_dir)
    frames = CL.job_frames(job)
    nt, h, w, _ = frames.shape
    ctx = _lib.Context(0)
    doc = dict(definition="TZ-PM1", job=job, model=model, frames=[nt, h, w], window=WINDOW, preds=list(_preds(ctx)), times={})
    try:
        ctx.load_model(cfg, wts)
        ctx.prepare(_lib.pad8(h), _lib.pad8(w), max(1, (nt + WINDOW - 1) // WINDOW))
        ctx.prof_enable(False)
        t = doc["times"]
        ctx.set_quantiser("lattice")
        for pred in _preds(ctx):
            _set(ctx, pred)
            for name, bound in (("lossless", [0.0]), ("abs6", [6.0])):
                t["rollout_closed_%s_%s" % (name, pred)] = CL._timed(ctx, lambda bound=bound: ctx.rollout_closed(frames, 0, WINDOW, "abs", bound))
                key = ctx.rollout_closed(frames, 0, WINDOW, "abs", bound)
                kf = CL._key_stack(frames, key)
                payload, table, _ = ctx.encode("abs", bound, True)
                payload = np.asarray(payload).copy()
                if pred != "net":
                    ctx.put_pred_modes(ctx.pred_modes())
                if pred == "motion":
                    ctx.put_pred_vectors(ctx.pred_vectors())
                t["decode_closed_%s_%s" % (name, pred)] = CL._timed(ctx, lambda kf=kf, payload=payload, table=table:
                                                                    ctx.rollout_decode_closed(kf, 0, payload, table))
        ctx.set_quantiser("greedy")
        _set(ctx, "net")
        if sizes:
            doc["bytes"] = _sizes(ctx, frames)
    finally:
        ctx.close()
    print(json.dumps(doc))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


def merge(out, new, parent):
    new, parent = [json.load(open(p)) for p in new], [json.load(open(p)) for p in parent]
    doc = dict(date=datetime.date.today().isoformat(), definition="TZ-PM1", jobs={},
               models="random: PredNet (3,48,96,192) glorot seed 123; trained: scripts/closedloop_profile.py train",
               runs="per process %d calls behind one warm-up call, median; then the median over the fresh processes of each build, alternating" % CL.RUNS)
    for job, model in sorted({(d["job"], d["model"]) for d in new}):
        mine = [d for d in new if (d["job"], d["model"]) == (job, model)]
        theirs = [d for d in parent if (d["job"], d["model"]) == (job, model)]
        cell = dict(frames=mine[0]["frames"], window=mine[0]["window"],
                    this_build={k: CL._med(mine, k) for k in sorted(mine[0]["times"])},
                    parent_build={k: CL._med(theirs, k) for k in sorted(theirs[0]["times"])} if theirs else None)
        with_bytes = [d for d in mine if "bytes" in d]
        if with_bytes:
            cell["bytes"] = with_bytes[0]["bytes"]
        if theirs:
            t, p = cell["this_build"], cell["parent_build"]
            for k in sorted(k for k in p if k.endswith("_select")):
                ps = p[k]["processes_ms"]
                base = k[:-len("_select")]
                cell["parent_select_spread_ms_" + base] = [min(ps), max(ps)]
                cell["motion_over_parent_select_" + base] = t[base + "_motion"]["median_ms"] / p[k]["median_ms"]
                cell["motion_minus_parent_select_ms_" + base] = t[base + "_motion"]["median_ms"] - p[k]["median_ms"]
        doc["jobs"]["%s_%s" % (job, model)] = cell
    doc["notes"] = ("times: HIP events on the context's stream; rollout_closed_*: tz_rollout_closed from host frames; decode_closed_*: "
                    "tz_rollout_decode_closed; _net without a second candidate, _select with tz_set_pred_select(1), _motion with "
                    "tz_set_pred_motion(7).  bytes: [entropy.dat, key_frame.dat, pred_modes.dat] per job; zstd = the default format's files, "
                    "huffd_auto = the exact size of the smallest layout's TZR2 file (tz_sdelta_probe) + the zstd key_frame.dat.  Not measured: "
                    "other models and real data, -p > 0, the command line's wall time.")
    print(json.dumps(doc))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", out)


def main(argv):
    root = ROOT
    if "--root" in argv:
        i = argv.index("--root")
        root = os.path.abspath(argv[i + 1])
        argv = argv[:i] + argv[i + 2:]
    sys.path.insert(0, root)
    model_dir = None
    if "--model" in argv:
        i = argv.index("--model")
        model_dir = argv[i + 1]
        argv = argv[:i] + argv[i + 2:]
    sizes = "--sizes" in argv
    argv = [a for a in argv if a != "--sizes"]
    if len(argv) == 3 and argv[0] == "run" and argv[2] in CL.JOBS:
        return run(argv[1], argv[2], model_dir, sizes)
    if len(argv) >= 3 and argv[0] == "merge":
        rest = argv[2:]
        cut = rest.index("--parent") if "--parent" in rest else len(rest)
        return merge(argv[1] or os.path.join(ROOT, "profiles", "pred_motion_%s.json" % datetime.date.today().isoformat()), rest[:cut], rest[cut + 1:])
    print(__doc__)
    return 2


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
