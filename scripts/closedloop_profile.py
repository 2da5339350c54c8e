#!/usr/bin/env python3
"""What closed-loop prediction (`-c --loop closed`, definition TZ-CL1, tezip_amd/closedloop.py) buys and costs with a TRAINED model
(with random weights the output hardly depends on the input and closed equals open) on cfg2's job (40 frames of 128x160
synth.translating_scene) and cfg3's job (80 frames of 512x512 synth.turbulence), `-p 0`.

  python scripts/closedloop_profile.py train MODEL_DIR JOB
      the reference's model (3, 48, 96, 192) trained with the reference's schedule (tezip_amd/train.py: 100 epochs x 5 samples, Adam
      1e-3 -> 1e-4, as tests/test_gpu_train.py and bench.py's trained leg do) on ten held-out 128x128 sequences of the job's
      generator (seeds 100-109; the jobs are the generators' default seeds).  JOB: cfg2 or cfg3.
  python scripts/closedloop_profile.py run OUT.json MODEL_DIR JOB [--root TREE] [--sizes]
      one process, the model of MODEL_DIR.  --root: import tezip_amd from another tree (a build of the parent commit; the rows that
      need tz_rollout_closed are then left out: the same file serves both builds).
      times   HIP events on the context's stream (tz_timer_start / tz_timer_stop), 7 calls behind one warm-up call, median, at
              -w 20: tz_rollout, tz_rollout_decode + tz_decode, and -- this build -- tz_rollout_closed lossless and at abs 6
              lattice, tz_rollout_decode_closed of both.
      --sizes entropy.dat + key_frame.dat of the open and the closed job at -w 20 and -w 40, lossless and at abs 2 / abs 6 under the
              lattice quantiser: under the default format (flat layout, zstd-9: the files compress.pack_outputs makes) and under
              `--coder huffd --sdelta auto` (the exact size of the smallest layout's file from tz_sdelta_probe; key_frame.dat zstd-9).
  python scripts/closedloop_profile.py merge OUT.json NEW1.json [...] --parent P1.json [...]
      the sizes of the first NEW file that has them, the medians of the times over the processes of each build (run them
      alternating) and the parent's run-to-run spread.  Default OUT: profiles/closed_loop_<date>.json

No ratio is fixed in advance.  Expected, to be confirmed or refuted in writing: the lossless closed rollout no slower than the
parent's tz_rollout (the same number of predictor steps, but no step is fed the level-0 error maps its predecessor could fuse);
the lossy closed rollout and the closed decoder slower by one elementwise launch per step."""
import datetime
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNS = 7
JOBS = {"cfg2": ("translating_scene", 40, 128, 160), "cfg3": ("turbulence", 80, 512, 512)}
BOUNDS = (("lossless", [0.0], "greedy"), ("abs2", [2.0], "lattice"), ("abs6", [6.0], "lattice"))


def job_frames(job):
    from tezip_amd import synth
    gen, nt, h, w = JOBS[job]
    return np.ascontiguousarray(getattr(synth, gen)(nt, h, w))


def train(model_dir, job):
    import tempfile
    from tezip_amd import synth, train as tztrain
    gen = JOBS[job][0]
    data = tempfile.mkdtemp(prefix="tz_cl_set_")
    seqs = [getattr(synth, gen)(12, 128, 128, seed=100 + k) for k in range(10)]
    np.save(os.path.join(data, "X_train.npy"), np.concatenate(seqs[:9]))
    np.save(os.path.join(data, "sources_train.npy"), np.repeat(["train-%d" % k for k in range(9)], 12))
    np.save(os.path.join(data, "X_val.npy"), seqs[9])
    np.save(os.path.join(data, "sources_val.npy"), np.repeat(["val-9"], 12))
    tztrain.run(model_dir, data, False)
    print("trained", model_dir)


def _timed(ctx, fn, runs=RUNS):
    fn()   # (the first call warms pools and code objects)
    ms = []
    for _ in range(runs):
        ctx.timer_start()
        fn()
        ms.append(float(ctx.timer_stop()))
    return dict(median_ms=float(np.median(ms)), spread_ms=[min(ms), max(ms)], all_ms=ms)


def _key_stack(frames, key):
    kf = np.zeros_like(frames)
    kf[key] = frames[key]
    return kf


def _sizes(ctx, frames, closed_ok):
    """{window: {bound: {loop: {zstd: [entropy, key], huffd_auto: [entropy, key, layout]}}}}"""
    from tezip_amd import compress, ratetarget, sdauto
    out = {}
    for window in (20, 40):
        out["w%d" % window] = {}
        for name, bound, quant in BOUNDS:
            cell = {}
            ctx.set_quantiser(quant)
            for loop in ("open", "closed") if closed_ok else ("open",):
                if loop == "closed":
                    key = ctx.rollout_closed(frames, 0, window, "abs", bound)
                else:
                    key, _ = ctx.rollout(frames, 0, window)
                payload, table, _ = ctx.encode("abs", bound, True)
                kb, eb = compress.pack_outputs(frames, key, np.asarray(payload), table, 0)
                chosen, sizes = sdauto.choose(ctx.sdelta_probe("abs", bound, True, "huffd"), "huffd")
                best = min(s for s in sizes if s is not None)
                cell[loop] = dict(zstd=[len(eb), len(kb)], huffd_auto=[int(best), len(kb), chosen])
            if "closed" in cell:
                for fmt in ("zstd", "huffd_auto"):
                    cell["closed_over_open_" + fmt] = sum(cell["closed"][fmt][:2]) / sum(cell["open"][fmt][:2])
            out["w%d" % window][name] = cell
    ctx.set_quantiser("greedy")
    return out


def run(out, model_dir, job, sizes):
    from tezip_amd import _lib, weights
    cfg, wts, _ = weights.load_model(model_dir)
    frames = job_frames(job)
    nt, h, w, _ = frames.shape
    window = 20
    ctx = _lib.Context(0)
    closed_ok = hasattr(ctx, "rollout_closed")
    doc = dict(definition="TZ-CL1", job=job, frames=[nt, h, w], window=window, has_closed_loop=closed_ok, times={})
    try:
        ctx.load_model(cfg, wts)
        ctx.prepare(_lib.pad8(h), _lib.pad8(w), max(1, (nt + window - 1) // window))
        ctx.prof_enable(False)
        t = doc["times"]
        t["rollout_open"] = _timed(ctx, lambda: ctx.rollout(frames, 0, window))
        key, _ = ctx.rollout(frames, 0, window)
        kf = _key_stack(frames, key)
        ctx.set_quantiser("lattice")
        streams = {}
        for name, bound in (("lossless", [0.0]), ("abs6", [6.0])):
            ctx.rollout(frames, 0, window)
            payload, table, _ = ctx.encode("abs", bound, True)
            payload = np.asarray(payload).copy()

            def decode_open(payload=payload, table=table):
                ctx.rollout_decode(kf, 0)
                ctx.decode(payload, table, out="resident")
            t["decode_open_" + name] = _timed(ctx, decode_open)
            if closed_ok:
                t["rollout_closed_" + name] = _timed(ctx, lambda bound=bound: ctx.rollout_closed(frames, 0, window, "abs", bound))
                payload, table, _ = ctx.encode("abs", bound, True)
                streams[name] = (np.asarray(payload).copy(), table)
        for name, (payload, table) in streams.items():
            t["decode_closed_" + name] = _timed(ctx, lambda payload=payload, table=table: ctx.rollout_decode_closed(kf, 0, payload, table))
        ctx.set_quantiser("greedy")
        if sizes:
            doc["bytes"] = _sizes(ctx, frames, closed_ok)
    finally:
        ctx.close()
    print(json.dumps(doc))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


def _med(docs, what):
    xs = [d["times"][what]["median_ms"] for d in docs if what in d["times"]]
    return dict(median_ms=float(np.median(xs)), processes_ms=xs) if xs else None


def merge(out, new, parent):
    new, parent = [json.load(open(p)) for p in new], [json.load(open(p)) for p in parent]
    doc = dict(date=datetime.date.today().isoformat(), definition="TZ-CL1", jobs={},
               model="PredNet (3,48,96,192), tezip_amd/train.py's default 100 x 5 steps on ten held-out 128x128 sequences of the job's generator",
               runs="per process %d calls behind one warm-up call, median; then the median over the fresh processes of each build, alternating" % RUNS)
    for job in sorted({d["job"] for d in new}):
        mine, theirs = [d for d in new if d["job"] == job], [d for d in parent if d["job"] == job]
        cell = dict(frames=mine[0]["frames"], window=mine[0]["window"],
                    this_build={k: _med(mine, k) for k in sorted(mine[0]["times"])},
                    parent_build={k: _med(theirs, k) for k in sorted(theirs[0]["times"])} if theirs else None)
        with_bytes = [d for d in mine if "bytes" in d]
        if with_bytes:
            cell["bytes"] = with_bytes[0]["bytes"]
        if theirs:
            t, p = cell["this_build"], cell["parent_build"]
            ps = p["rollout_open"]["processes_ms"]
            cell["parent_rollout_spread_ms"] = [min(ps), max(ps)]
            cell["closed_lossless_over_parent_rollout"] = t["rollout_closed_lossless"]["median_ms"] / p["rollout_open"]["median_ms"]
            cell["closed_abs6_over_parent_rollout"] = t["rollout_closed_abs6"]["median_ms"] / p["rollout_open"]["median_ms"]
            for name in ("lossless", "abs6"):
                cell["decode_closed_%s_over_parent_decode" % name] = (t["decode_closed_" + name]["median_ms"] /
                                                                      p["decode_open_" + name]["median_ms"])
        doc["jobs"][job] = cell
    doc["notes"] = ("times: HIP events on the context's stream; rollout_*: the whole entry point from host frames; decode_open: tz_rollout_decode + "
                    "tz_decode(frames resident); decode_closed: tz_rollout_decode_closed.  bytes: [entropy.dat, key_frame.dat] per loop; zstd = "
                    "the default format's files, huffd_auto = the exact size of the smallest layout's TZR2 file (tz_sdelta_probe) + the zstd "
                    "key_frame.dat.  Not measured: other models and data, -p > 0, the command line's wall time.")
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
    sizes = "--sizes" in argv
    argv = [a for a in argv if a != "--sizes"]
    if len(argv) == 3 and argv[0] == "train" and argv[2] in JOBS:
        return train(argv[1], argv[2])
    if len(argv) == 4 and argv[0] == "run" and argv[3] in JOBS:
        return run(argv[1], argv[2], argv[3], sizes)
    if len(argv) >= 3 and argv[0] == "merge":
        rest = argv[2:]
        cut = rest.index("--parent") if "--parent" in rest else len(rest)
        return merge(argv[1] or os.path.join(ROOT, "profiles", "closed_loop_%s.json" % datetime.date.today().isoformat()), rest[:cut], rest[cut + 1:])
    print(__doc__)
    return 2


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
