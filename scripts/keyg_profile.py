#!/usr/bin/env python3
"""Size and device time of the coders of key_frame.dat on gray jobs: `--key-coder zstd`, `huff` (TZK1) and `huffg` (TZK2, a
gray key frame coded once), from the same frames, random weights (seed 3), abs 2:
  moving_blobs   40 frames of 64x64 synth.moving_blobs, -w 20 (cfg1's job)
  detector       8 frames of 1024x1024 synth.detector, -w 4
`zstd` and `huffg` are measured in this tree; `huff` in a build of the PARENT commit (a checkout with its library built,
given as parent_tree), in a child process of its own, so that the comparison is with the coder as it was, not with a switch
inside the new build.  Device times are HIP-event sums of the 'huffman' profiling class (tz_prof_get) over the key-coder
stage -- for huffg k_key_gray + k_key_hist + k_key_resid + the Huffman size / scan / pack kernels -- 7 runs, median.
File sizes are those of compress.run's directory.
The expectation this records (no threshold anywhere): huffg's device time on a gray job does not exceed huff's on the same
job, since it codes a third of the symbols after one extra read.
Usage: python scripts/keyg_profile.py out.json parent_tree [work_dir]"""
import contextlib
import io
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JOBS = {"moving_blobs": dict(gen="moving_blobs", nt=40, h=64, w=64, window=20),
        "detector": dict(gen="detector", nt=8, h=1024, w=1024, window=4)}
FILES = ("key_frame.dat", "entropy.dat", "filename.txt", "tezip_amd.json")


def timed(ctx, fn, runs=7):
    ms = []
    for _ in range(runs):
        ctx.prof_reset()
        fn()
        ms.append(ctx.prof_get()["huffman"][0])
    return float(np.median(ms)), ms


def child(root, work, coders):
    """Measure `coders` with the package of the tree `root`; prints one JSON line."""
    sys.path.insert(0, root)
    from PIL import Image
    from tezip_amd import _lib, compress, huff, keycoder, synth, weights
    from tezip_amd.prednet import PredNetConfig
    cfg = PredNetConfig()
    wts = cfg.init_weights(seed=3)
    out = {}
    for job, j in JOBS.items():
        frames = getattr(synth, j["gen"])(j["nt"], j["h"], j["w"])
        nt, h, w = frames.shape[:3]
        mdir, ddir = os.path.join(work, job + "_model"), os.path.join(work, job + "_data")
        weights.save_model(mdir, cfg, wts, _lib.pad8(h), _lib.pad8(w))
        os.makedirs(ddir)
        for t in range(nt):
            Image.fromarray(frames[t]).save(os.path.join(ddir, "f_%03d.png" % t))
        res = {}
        for coder in coders:
            cdir = os.path.join(work, "%s_%s" % (job, coder))
            with contextlib.redirect_stdout(io.StringIO()):
                compress.run(mdir, ddir, cdir, 0, j["window"], None, "abs", [2.0], True, False, True, KEY_CODER=coder)
            res[coder] = dict(bytes={n: os.path.getsize(os.path.join(cdir, n)) for n in FILES if os.path.exists(os.path.join(cdir, n))})
            shutil.rmtree(cdir)
        ctx = _lib.Context(0)
        ctx.load_model(cfg, wts)
        ctx.prepare(_lib.pad8(h), _lib.pad8(w), min(j["window"], 20))
        key, _ = ctx.rollout(frames, 0, j["window"])
        idx = [int(i) for i in np.nonzero(key)[0]]
        ctx.prof_enable(True)

        def enc_huff():
            counts = ctx.keys_counts(idx)
            pred = keycoder.choose_predictors(counts)
            ctx.keys_encode(idx, pred, huff.code_lengths(keycoder.chosen_counts(counts, pred)))

        def enc_huffg():
            from tezip_amd import keycoderg
            gray = ctx.keys_gray(idx)
            counts = keycoderg.gray_counts(ctx.keys_counts(idx), gray)
            predg = keycoderg.pred_bytes(counts, gray)
            ctx.keysg_encode(idx, predg, huff.code_lengths(keycoderg.chosen_counts(counts, predg)))

        for coder, fn in (("huff", enc_huff), ("huffg", enc_huffg)):
            if coder in coders:
                med, every = timed(ctx, fn)
                res[coder].update(key_frames=idx, encode_device_ms=med, encode_device_ms_all=every)
        ctx.close()
        shutil.rmtree(mdir)
        shutil.rmtree(ddir)
        out[job] = res
    print("KEYG_PROFILE " + json.dumps(out), flush=True)


def run_child(root, work, coders):
    os.makedirs(work)
    r = subprocess.run(["timeout", "-k", "10", "400", sys.executable, os.path.abspath(__file__), "--child", root, work] + list(coders),
                       capture_output=True, text=True)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("KEYG_PROFILE ")]
    if r.returncode != 0 or not lines:
        raise SystemExit("the measurement in %s ended with status %d:\n%s\n%s" % (root, r.returncode, r.stdout[-2000:], r.stderr[-4000:]))
    return json.loads(lines[-1][len("KEYG_PROFILE "):])


def main():
    if sys.argv[1] == "--child":
        return child(sys.argv[2], sys.argv[3], sys.argv[4:])
    out_path, parent = sys.argv[1], os.path.abspath(sys.argv[2])
    work = sys.argv[3] if len(sys.argv) > 3 else tempfile.mkdtemp(prefix="keyg_profile_")
    try:
        new = run_child(HERE, os.path.join(work, "new"), ["zstd", "huffg"])     # (one after the other: a child that failed
        old = run_child(parent, os.path.join(work, "parent"), ["huff"])         #  ends the script before the next starts)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    doc = dict(jobs=JOBS, weights="random (seed 3)", bound="abs 2", results={})
    for job in JOBS:
        r = dict(new[job], huff=old[job]["huff"])
        z = r["zstd"]["bytes"]["key_frame.dat"]
        for c in ("huff", "huffg"):
            r[c]["key_frame_over_zstd9"] = r[c]["bytes"]["key_frame.dat"] / z
        r["huffg_device_ms_over_huff"] = r["huffg"]["encode_device_ms"] / r["huff"]["encode_device_ms"]
        doc["results"][job] = r
    doc["notes"] = ("One device, one process per tree: zstd and huffg from this tree, huff from a build of the parent commit.  "
                    "encode_device_ms: HIP-event sum of the 'huffman' profiling class over the key-coder stage (huff: k_key_hist + "
                    "k_key_resid + Huffman size / scan / pack; huffg: k_key_gray + k_key_hist + k_key_resid + the same Huffman kernels "
                    "over a third of the symbols), 7 runs, median.  bytes: the files compress.run wrote.  Expectation recorded, not "
                    "tested: huffg_device_ms_over_huff <= 1 on a gray job.")
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps({j: {c: (r[c]["bytes"]["key_frame.dat"], r[c].get("encode_device_ms")) for c in ("zstd", "huff", "huffg")}
                      for j, r in doc["results"].items()}))


if __name__ == "__main__":
    main()
