"""Range decode (`-u --frames A:B`) against the whole decode on the cfg3 job (512 x 512, 80 frames, -w 20, -p 0,
lossless): device time of the library calls and wall time of the CLI for the full decode, one frame at the end of a
window, one whole window and a 10-frame range across a window boundary; and the prefix-carry kernel alone on a
cfg3-sized prefix (62.9 M elements) with its fraction of HBM bandwidth.

    python scripts/range_decode_bench.py [--out FILE] [--no-cli] [--reps N]

Device time = the sum of the library's per-kernel-class event timings (tz_prof_*; the sub-classes of the convolution
class are not added twice), library time = wall time of the two calls with host payload in and host frames out.
Prints one JSON document."""
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
TOP_CLASSES = ("conv3x3_mfma", "err0", "delta", "quant", "spatial_delta_hist", "lut_remap", "undelta_scan", "reconstruct",
               "sse", "undelta_carry")
NT, H, W, WARM, WIN = 80, 512, 512, 0, 20
RANGES = {"full": (0, NT), "one_frame_window_end": (NT - 1, NT), "one_window": (NT - WIN, NT),
          "ten_frames_across_boundary": (2 * WIN - 5, 2 * WIN + 5)}


def device_ms(prof):
    return sum(prof[k][0] for k in TOP_CLASSES if k in prof)


def library_times(ctx, keys, payload, table, reps):
    out = {}
    for name, (a, b) in RANGES.items():
        dev, wall, conv = [], [], 0
        for _ in range(reps + 1):                    # the first pass warms pools and code objects
            ctx.prof_enable(True)
            ctx.prof_reset()
            t0 = time.perf_counter()
            if name == "full":
                ctx.rollout_decode(keys, WARM)
                ctx.decode(payload, table)
            else:
                ctx.rollout_decode_range(keys, WARM, a, b - a)
                ctx.decode_range(payload, table, a, b - a)
            wall.append((time.perf_counter() - t0) * 1e3)
            prof = ctx.prof_get()
            dev.append(device_ms(prof))
            conv = prof["conv3x3_mfma"][1]
            ctx.prof_enable(False)
        out[name] = dict(frames=[a, b], device_ms=round(float(np.median(dev[1:])), 3),
                         library_wall_ms=round(float(np.median(wall[1:])), 3), conv_launches=int(conv),
                         classes_ms={k: round(v[0], 4) for k, v in prof.items() if k in TOP_CLASSES and v[1]})
    return out


def carry_kernel(ctx, reps):
    """The carry kernel on a payload staged in HBM (tz_payload_begin / tz_payload_put): no host transfer in the loop."""
    n0 = NT * H * W * 3
    x = np.random.default_rng(1).integers(0, 600, n0).astype(np.int16)
    ctx.payload_begin(n0)
    ctx.payload_put(0, x)
    table = np.arange(1000, 1600, dtype=np.int16)
    res = {}
    for label, tb in (("no_table", None), ("table", table)):
        ctx.undelta_carry(None, n0, tb, staged=True)
        ctx.prof_enable(True)
        ctx.prof_reset()
        for _ in range(reps):
            ctx.undelta_carry(None, n0, tb, staged=True)
        ms, n = ctx.prof_get()["undelta_carry"]
        ctx.prof_enable(False)
        us = ms / n * 1e3
        tbs = n0 * 2 / (us * 1e-6) / 1e12
        res[label] = dict(elements=n0, us_per_launch_event_timed=round(us, 2), tb_per_s=round(tbs, 3),
                          fraction_of_hbm_peak=round(tbs / HBM_PEAK_TBS, 3), fraction_of_measured_copy=round(tbs / HBM_COPY_TBS, 3))
    return res


def cli_times(mdir, frames, tmp):
    from PIL import Image
    ddir = os.path.join(tmp, "data")
    os.makedirs(ddir)
    for t in range(NT):
        Image.fromarray(frames[t]).save(os.path.join(ddir, "t_%03d.png" % t))
    cdir = os.path.join(tmp, "comp")

    def run(args):
        t0 = time.perf_counter()
        r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, "-m", "tezip_amd.tezip"] + args, cwd=ROOT,
                           capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("CLI failed (%d): %s" % (r.returncode, (r.stdout + r.stderr)[-2000:]))
        return (time.perf_counter() - t0) * 1e3

    out = {"compress_wall_ms": round(run(["-c", mdir, ddir, cdir, "-p", str(WARM), "-w", str(WIN), "-m", "abs", "-b", "0"]), 1)}
    for name, (a, b) in RANGES.items():
        udir = os.path.join(tmp, "u_" + name)
        extra = [] if name == "full" else ["--frames", "%d:%d" % (a, b)]
        out[name] = dict(frames=[a, b], cli_wall_ms=round(run(["-u", mdir, cdir, udir] + extra), 1))
        shutil.rmtree(udir)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-cli", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    from tezip_amd import _lib, synth, weights
    from tezip_amd.prednet import PredNetConfig
    cfg = PredNetConfig()
    wts = cfg.init_weights(seed=123)
    frames = synth.turbulence(NT, H, W, seed=3)
    ctx = _lib.Context(0)
    ctx.load_model(cfg, wts)
    ctx.prepare(H, W, max_batch=4)
    key, _ = ctx.rollout(frames, WARM, WIN)
    payload, table, _ = ctx.encode("abs", [0.0], True)
    keys = np.where(key[:, None, None, None], frames, 0).astype(np.uint8)
    ctx.rollout_decode(keys, WARM)
    full = ctx.decode(payload, table).copy()
    for name, (a, b) in RANGES.items():               # what is timed is what is right
        ctx.rollout_decode_range(keys, WARM, a, b - a)
        assert (ctx.decode_range(payload, table, a, b - a) == full[a:b]).all(), name
    doc = {"date": datetime.date.today().isoformat(), "job": "cfg3: %dx%d, %d frames, -p %d -w %d, abs 0, entropy on" % (H, W, NT, WARM, WIN),
           "key_frames": [int(i) for i in np.flatnonzero(key)],
           "library": library_times(ctx, keys, payload, table, args.reps), "carry_kernel": carry_kernel(ctx, max(args.reps, 20))}
    ctx.close()
    if not args.no_cli:
        tmp = tempfile.mkdtemp(prefix="range_bench_")
        try:
            mdir = os.path.join(tmp, "model")
            weights.save_model(mdir, cfg, wts, H, W)
            doc["cli"] = cli_times(mdir, frames, tmp)
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
