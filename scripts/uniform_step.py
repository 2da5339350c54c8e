#!/usr/bin/env python3
"""The bench's timed step (cfg3: 80 frames of 512x512, four 20-frame windows, rollout + encode, frames resident in HBM) with
a model that HAS biases: init_weights(seed=123, bias_scale=...).  bench.py's glorot model has zero biases, so all its
per-model constants are 0 over the whole plane and every tile takes the uniform-constant shortcut (tz_prednet.hip
measure_uniform); with biases the outermost tile ring of every level keeps the per-pixel loads -- the figure that holds for
trained weights.  TEZIP_UNIFORM=0 / a mask of its parts and TEZIP_UNIFORM_LOG=1 apply (read at prepare time).
  python scripts/uniform_step.py [--bias-scale 0.1] [--steps 20] [--warmup 2] [--kernels]   -> one JSON line"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from tezip_amd import _lib  # noqa: E402
from tezip_amd.prednet import PredNetConfig  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--bias-scale", type=float, default=0.1)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--kernels", action="store_true", help="one more step under the library's per-class kernel timers")
args = ap.parse_args()

dev = torch.device("cuda", 0)
cfg = PredNetConfig()
ctx = _lib.Context(0)
ctx.load_model(cfg, cfg.init_weights(seed=123, bias_scale=args.bias_scale))
ctx.prepare(bench.H, bench.W, max_batch=(bench.NT - bench.WARM_UP + bench.WINDOW - 1) // bench.WINDOW)
frames = bench.turbulence_cuda(bench.NT, 0, bench.NT, bench.H, bench.W, 3, dev)
payload = torch.empty(bench.NT * bench.H * bench.W * 3, dtype=torch.int16, device=dev)


def step():
    ctx.rollout(frames, bench.WARM_UP, bench.WINDOW)
    ctx.encode(bench.MODE, bench.BOUND, True, payload=payload)


for _ in range(args.warmup):
    step()
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(args.steps):
    step()
torch.cuda.synchronize()
line = {"bias_scale": args.bias_scale, "TEZIP_UNIFORM": os.environ.get("TEZIP_UNIFORM", "default"), "steps": args.steps,
        "ms_per_step": (time.perf_counter() - t0) / args.steps * 1e3}
if args.kernels:
    ctx.prof_enable(True)
    ctx.prof_reset()
    step()
    line["kernel_ms_per_step"] = {k: round(v[0], 3) for k, v in ctx.prof_get().items() if v[1] and k in
                                  ("wino_pa2", "conv16b_level0", "conv_small_valu")}
    ctx.prof_enable(False)
print(json.dumps(line))
