"""The abs bound that meets a PSNR target (`tezip.py -c ... --target-psnr DB`; not in the reference).

Definition TZ-TPSNR-1 (also DESIGN.md section 9).  The predictions of a job do not depend on its bound -- the quantiser runs
behind the rollout, and the decoder predicts from the key frames alone -- so one rollout serves every candidate bound and
a candidate costs one quantiser run and one comparison (tz_bound_probe).  All of it is integers:

  samples     N = nt * H * W * 3: every sample of the job, key frames included, as the sequence PSNR of --report counts them.
  limit       sse_limit(T, N) = min(N * 65025, floor(N * 65025.0 / 10.0 ** (T / 10.0))), in Python float64, computed HERE and
              nowhere else; T finite and > 0.  PSNR >= T  <=>  SSE <= N * 255^2 / 10^(T/10), up to that one rounding.
  candidates  k = 0 .. 510, bound E = k / 2.  Deltas lie in [-255, 255]: at E = 255 no run of the quantiser can close, so a
              larger bound changes nothing; on the half-integer grid every d +- E and the quantiser's midpoint are exact in
              fp64.  Other bounds are not searched.
  pass(k)     SSE(k) <= limit, SSE(k) the exact sum over all frames of what tz_encode_quality reports for a
              tz_encode("abs", k / 2) on the same rollout (tz_bound_probe gives the same records without a payload) -- of
              the job as it is stored: with --gray on an all-gray job that is the one-channel payload, whose decoder writes
              channel 0's reconstruction to all three channels, and its SSE(k) is not the three-channel job's.
  search      lo = 0, hi = 511; while hi - lo > 1: mid = (lo + hi) // 2, lo = mid if pass(mid) else hi = mid; the result is
              k = lo.  At most 9 probes.  limit == 0: k = 0 with no probe at all.  (k = 0 is lossless: SSE(0) = 0.)
  guarantee   SSE(k) <= limit, and k == 510 or SSE(k + 1) > limit.

NOT the largest passing bound: SSE is not monotone in the bound (a wider bound merges other runs, whose midpoints can lie
nearer the deltas, and the decoder's clamp to [0, 255] removes error the quantiser made), so the bisection finds A boundary
between a passing and a failing candidate; a larger candidate further up may pass as well.

The job then runs as the ordinary `-m abs -b E`: the decoder never sees a bound.  This module is pure numpy; the probes
come from the library (tezip_amd/_lib.py Context.bound_probe)."""
import json
import math
import os

import numpy as np

FILE_NAME = "bound_search.json"
DEFINITION = "TZ-TPSNR-1"
K_MAX = 510            # candidates k = 0 .. K_MAX, bound k / 2
PEAK2 = 65025          # 255^2


def check_target(target):
    """None, or why `target` is no PSNR target (the refusal of tezip.py and compress.run)."""
    try:
        t = float(target)
    except (TypeError, ValueError):
        return "--target-psnr takes a number of dB, got %r" % (target,)
    if math.isnan(t) or math.isinf(t) or t <= 0.0:
        return "--target-psnr must be a finite number of dB above 0, got %r" % (target,)
    return None


def sse_limit(target, n):
    """The largest sum of squared errors over n samples whose PSNR is still >= target dB (the one float computation of
    TZ-TPSNR-1)."""
    problem = check_target(target)
    if problem:
        raise ValueError(problem)
    n = int(n)
    if n < 0:
        raise ValueError("sample count %d" % n)
    return min(n * PEAK2, int(math.floor(n * 65025.0 / 10.0 ** (float(target) / 10.0))))


def bound_of(k):
    return k / 2.0


def search(probe, limit):
    """probe: k -> total sse of candidate k (an int).  -> (k, trace), trace = [{"k", "bound", "sse", "pass"}] in probe order."""
    limit = int(limit)
    trace = []
    if limit <= 0:
        return 0, trace
    lo, hi = 0, K_MAX + 1
    while hi - lo > 1:
        mid = (lo + hi) // 2
        sse = int(probe(mid))
        ok = sse <= limit
        trace.append({"k": mid, "bound": bound_of(mid), "sse": sse, "pass": ok})
        if ok:
            lo = mid
        else:
            hi = mid
    return lo, trace


def errors_of(orig, d, q, channels=3):
    """The slow statement of k_bound_err.  orig (uint8), d and q (int16: the deltas and what the quantiser made of them),
    all shaped (nframes, ...): -> (nframes, 3) int64 of (sse, max_abs, n_changed) of clamp(orig + d - q, 0, 255) against orig.
    channels=1: what a one-channel payload decodes to (tezip_amd/graypayload.py) -- the stacks are (..., 3) pixels, the job
    stores channel 0's q alone and its decoder writes clamp(orig_0 + d_0 - q_0, 0, 255) to all three channels of the pixel;
    the kernel's form of it is for gray originals (three equal channels), which is all such a job accepts."""
    o = np.asarray(orig).astype(np.int64)
    nf = o.shape[0] if o.ndim else 0
    o = o.reshape(nf, -1)
    dd = np.asarray(d).astype(np.int64).reshape(nf, -1)
    qq = np.asarray(q).astype(np.int64).reshape(nf, -1)
    if channels == 1:
        if o.shape[1] % 3:
            raise ValueError("frames of %d elements: a one-channel payload describes whole pixels" % o.shape[1])
        rec = np.clip(o[:, 0::3] + dd[:, 0::3] - qq[:, 0::3], 0, 255)
        e = np.repeat(rec, 3, axis=1) - o
    elif channels == 3:
        e = np.clip(o + dd - qq, 0, 255) - o
    else:
        raise ValueError("channels must be 3 or 1, not %r" % (channels,))
    out = np.zeros((nf, 3), np.int64)
    if o.shape[1]:
        out[:, 0] = (e * e).sum(axis=1)
        out[:, 1] = np.abs(e).max(axis=1)
        out[:, 2] = (e != 0).sum(axis=1)
    return out


def make(target, n, limit, trace, k):
    """bound_search.json as a JSON-ready dict."""
    sse = next((t["sse"] for t in trace if t["k"] == k), 0)   # (k = 0 is never probed: lossless)
    return {
        "definition": DEFINITION,
        "target_psnr_db": float(target),
        "samples": int(n),
        "sse_limit": int(limit),
        "probes": len(trace),
        "trace": [dict(t) for t in trace],
        "result": {"k": int(k), "mode": "abs", "bound": bound_of(k), "sse": int(sse)},
    }


def write(out_dir, doc):
    path = os.path.join(out_dir, FILE_NAME)
    with open(path, "w", encoding="UTF-8") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return path


def stdout_line(doc):
    r = doc["result"]
    return "target: PSNR >= %g dB -> abs bound %g (%d probes, sse %d <= %d)" % (doc["target_psnr_db"], r["bound"], doc["probes"],
                                                                                r["sse"], doc["sse_limit"])
