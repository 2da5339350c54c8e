"""Cost of the compression report (`-c --report`, tz_encode_quality) on the cfg3 job (512 x 512, 80 frames, -w 20, -p 0)
with `abs 2` and lossless: device time of the call by HIP events, its split into the decoder's tail and k_quality (the
library's per-kernel-class event timings), k_quality's fraction of HBM bandwidth, and the wall time of the `-c` CLI
with and without --report.

    python scripts/quality_bench.py [--out FILE] [--no-cli] [--reps N]

--out defaults to profiles/quality_<date>.json.  The records are checked against a fresh context's decode before
anything is timed.  Prints one JSON document."""
import argparse
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

HBM_PEAK_TBS = 8.0            # MI355X HBM3E specification
HBM_COPY_TBS = 6.29           # measured float4 copy (the practical roof)
NT, H, W, WARM, WIN = 80, 512, 512, 0, 20
MODES = {"abs2": ("abs", [2.0]), "lossless": ("abs", [0.0])}


def check(cfg, wts, frames, key, payload, table, q):
    from tezip_amd import _lib
    d = _lib.Context(0)
    try:
        d.load_model(cfg, wts)
        d.prepare(H, W, max_batch=4)
        keys = np.where(key[:, None, None, None], frames, 0).astype(np.uint8)
        d.rollout_decode(keys, WARM)
        dec = d.decode(payload, table)
        diff = (dec.astype(np.int16) - frames.astype(np.int16)).reshape(NT, -1).astype(np.int64)
        want = np.stack([(diff * diff).sum(1), np.abs(diff).max(1), (diff != 0).sum(1)], 1)
        got = np.stack([q["sse"], q["max_abs"], q["n_changed"]], 1).astype(np.int64)
        assert (got == want).all(), "tz_encode_quality disagrees with a fresh decode"
    finally:
        d.close()


def library(ctx, table, reps):
    """tz_encode_quality on the resident payload: HIP events around the call, and the kernel classes inside it."""
    ctx.encode_quality("resident", table)              # warms pools and code objects
    ev, classes = [], {}
    for _ in range(reps):
        ctx.timer_start()
        ctx.encode_quality("resident", table)
        ev.append(ctx.timer_stop())
    ctx.prof_enable(True)
    ctx.prof_reset()
    for _ in range(reps):
        ctx.encode_quality("resident", table)
    prof = ctx.prof_get()
    ctx.prof_enable(False)
    for k, (ms, n) in prof.items():
        if n and k in ("undelta_scan", "reconstruct", "quality"):
            classes[k] = dict(us_per_call=round(ms / reps * 1e3, 2), launches_per_call=n / reps)
    q_us = prof["quality"][0] / prof["quality"][1] * 1e3
    tbs = 2 * NT * H * W * 3 / (q_us * 1e-6) / 1e12
    return dict(device_ms_hip_events=round(float(np.median(ev)), 4), device_ms_min=round(float(np.min(ev)), 4),
                classes=classes,
                k_quality=dict(bytes_read=2 * NT * H * W * 3, us_event_timed=round(q_us, 2), tb_per_s=round(tbs, 3),
                               fraction_of_hbm_peak=round(tbs / HBM_PEAK_TBS, 3),
                               fraction_of_measured_copy=round(tbs / HBM_COPY_TBS, 3)))


def cli_times(mdir, frames, tmp, bound, reps):
    from PIL import Image
    ddir = os.path.join(tmp, "data")
    if not os.path.isdir(ddir):
        os.makedirs(ddir)
        for t in range(NT):
            Image.fromarray(frames[t]).save(os.path.join(ddir, "t_%03d.png" % t))

    def run(args):
        t0 = time.perf_counter()
        r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, "-m", "tezip_amd.tezip"] + args, cwd=ROOT,
                           capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("CLI failed (%d): %s" % (r.returncode, (r.stdout + r.stderr)[-2000:]))
        return (time.perf_counter() - t0) * 1e3

    out = {}
    for label, extra in (("without_report", []), ("with_report", ["--report"])):
        walls = []
        for i in range(reps):
            cdir = os.path.join(tmp, "c_%s_%d" % (label, i))
            walls.append(run(["-c", mdir, ddir, cdir, "-p", str(WARM), "-w", str(WIN), "-m", "abs", "-b", str(bound)] + extra))
            shutil.rmtree(cdir)
        out[label] = dict(cli_wall_ms=[round(v, 1) for v in walls], median=round(float(np.median(walls)), 1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-cli", action="store_true")
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    from tezip_amd import _lib, synth, weights
    from tezip_amd.prednet import PredNetConfig
    cfg = PredNetConfig()
    wts = cfg.init_weights(seed=123)
    frames = synth.turbulence(NT, H, W, seed=3)
    doc = {"date": datetime.date.today().isoformat(),
           "job": "cfg3: %dx%d, %d frames, -p %d -w %d, entropy on" % (H, W, NT, WARM, WIN), "modes": {}}
    ctx = _lib.Context(0)
    try:
        ctx.load_model(cfg, wts)
        ctx.prepare(H, W, max_batch=4)
        key, _ = ctx.rollout(frames, WARM, WIN)
        for label, (mode, bound) in MODES.items():
            payload, table, _ = ctx.encode(mode, bound, True)
            payload = np.array(payload, copy=True)
            q = ctx.encode_quality(payload, table)
            check(cfg, wts, frames, key, payload, table, q)       # what is timed is right
            ctx.encode(mode, bound, True, payload="resident")
            res = library(ctx, table, args.reps)
            res.update(max_abs_err=int(q["max_abs"].max()), sse=int(q["sse"].sum()), n_changed=int(q["n_changed"].sum()))
            doc["modes"][label] = res
    finally:
        ctx.close()
    if not args.no_cli:
        tmp = tempfile.mkdtemp(prefix="quality_bench_")
        try:
            mdir = os.path.join(tmp, "model")
            weights.save_model(mdir, cfg, wts, H, W)
            for label, (mode, bound) in MODES.items():
                doc["modes"][label]["cli"] = cli_times(mdir, frames, tmp, bound[0], 2)
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    text = json.dumps(doc, indent=1)
    print(text)
    out = args.out or os.path.join(ROOT, "profiles", "quality_%s.json" % doc["date"])
    with open(out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
