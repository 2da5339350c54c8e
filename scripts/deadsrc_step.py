#!/usr/bin/env python3
"""The bench's timed step (cfg3: 80 frames of 512x512, four 20-frame windows, rollout + encode, frames resident in HBM) for
the dead-source skip of k_wino (tz_prednet.hip measure_dead), timed with HIP events on the context's stream.  bench.py's glorot
model has zero biases: the whole positive half of every error map is dead and half of the same-resolution stages are left
out.  This script runs the models for which that is NOT so -- where the step must cost what it did before:
  --bias-scale S   init_weights(seed=123, bias_scale=S) (default 0.1: no dead block anywhere)
  --trained        the model bench.py --full trains for compression_ratio_trained (the same data, the same schedule)
TEZIP_DEADSRC=0 and TEZIP_DEADSRC_LOG=1 apply (read at prepare time; the log lines go to stderr).
  python scripts/deadsrc_step.py [--bias-scale 0.1 | --trained] [--steps 20] [--warmup 2] [--repeats 3]   -> one JSON line"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from tezip_amd import _lib  # noqa: E402
from tezip_amd.prednet import PredNetConfig  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--bias-scale", type=float, default=0.1)
ap.add_argument("--trained", action="store_true")
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--kernels", action="store_true", help="one more step under the library's per-class kernel timers")
args = ap.parse_args()

dev = torch.device("cuda", 0)
cfg = PredNetConfig()
if args.trained:   # bench.py trained_ratio's model
    import tempfile
    from tezip_amd import synth, train, weights
    tmp = tempfile.mkdtemp(prefix="tz_deadsrc_model_")
    data = os.path.join(tmp, "set")
    os.makedirs(data)
    seqs = [synth.turbulence(12, 128, 128, seed=100 + k) for k in range(10)]
    np.save(os.path.join(data, "X_train.npy"), np.concatenate(seqs[:9]))
    np.save(os.path.join(data, "sources_train.npy"), np.repeat(["train-%d" % k for k in range(9)], 12))
    np.save(os.path.join(data, "X_val.npy"), seqs[9])
    np.save(os.path.join(data, "sources_val.npy"), np.repeat(["val-9"], 12))
    train.run(os.path.join(tmp, "model"), data, False)
    wts = weights.load_model(os.path.join(tmp, "model"))[1]
    model = "trained as bench.py --full does"
else:
    wts = cfg.init_weights(seed=123, bias_scale=args.bias_scale)
    model = "init_weights(seed=123, bias_scale=%g)" % args.bias_scale
ctx = _lib.Context(0)
ctx.load_model(cfg, wts)
ctx.prepare(bench.H, bench.W, max_batch=(bench.NT - bench.WARM_UP + bench.WINDOW - 1) // bench.WINDOW)
frames = bench.turbulence_cuda(bench.NT, 0, bench.NT, bench.H, bench.W, 3, dev)
payload = torch.empty(bench.NT * bench.H * bench.W * 3, dtype=torch.int16, device=dev)
stream = torch.cuda.ExternalStream(ctx.stream_ptr(), device=dev)   # the context's own stream: the events go where its kernels go


def step():
    ctx.rollout(frames, bench.WARM_UP, bench.WINDOW)
    ctx.encode(bench.MODE, bench.BOUND, True, payload=payload)


for _ in range(args.warmup):
    step()
torch.cuda.synchronize()
ms = []
for _ in range(args.repeats):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(args.steps):
        step()
    e1.record(stream)
    e1.synchronize()
    ms.append(e0.elapsed_time(e1) / args.steps)
line = {"model": model, "TEZIP_DEADSRC": os.environ.get("TEZIP_DEADSRC", "default"), "steps": args.steps,
        "ms_per_step": [round(v, 4) for v in ms]}
if args.kernels:
    ctx.prof_enable(True)
    ctx.prof_reset()
    step()
    line["kernel_ms_per_step"] = {k: round(v[0], 3) for k, v in ctx.prof_get().items() if v[1] and k in
                                  ("wino_pa2", "conv16b_level0", "conv_small_valu")}
    ctx.prof_enable(False)
ctx.close()
print(json.dumps(line))
