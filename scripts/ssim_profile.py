#!/usr/bin/env python3
"""Device time of the SSIM report (`-c --report --ssim`; k_ssim, definition TZ-SSIM-1) on cfg3's job: 80 frames of 512x512
synthetic turbulence, random weights (seed 3), `-p 0 -w 20`, lossless and `abs 2`.
Per mode, in one process: the HIP-event time of a whole tz_encode_ssim call and of a whole tz_encode_quality call on the same
resident payload (tz_timer_start / tz_timer_stop around the call: the decoder's tail both run first is included), the share
of the 'quality' profiling class in each (k_ssim_init + k_ssim, or k_quality, alone), 9 runs each, the two alternating, first
run dropped, median; the job's SSIM and worst window; and a check of the records against the numpy statement on 4 frames.
Usage: python scripts/ssim_profile.py [out.json]      (default: profiles/ssim_<date>.json)"""
import datetime
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tezip_amd import _lib, ssim, synth  # noqa: E402
from tezip_amd.prednet import PredNetConfig  # noqa: E402

RUNS = 9


def _call(ctx, fn):
    """(whole call in ms by HIP events on the context's stream, 'quality' class ms, its launches) of one call."""
    ctx.prof_reset()
    ctx.timer_start()
    out = fn()
    ms = ctx.timer_stop()
    cls_ms, launches = ctx.prof_get()["quality"]
    return out, float(ms), float(cls_ms), int(launches)


def _stats(rows):
    rows = rows[1:]   # (the first run warms the pool up)
    call, cls = [r[0] for r in rows], [r[1] for r in rows]
    return dict(call_ms_median=float(np.median(call)), call_ms_spread=[min(call), max(call)], call_ms_all=call,
                quality_class_us_median=float(np.median(cls)) * 1e3, quality_class_us_spread=[min(cls) * 1e3, max(cls) * 1e3],
                launches_in_class=rows[-1][2])


def mode_part(ctx, frames, bound):
    nt, h, w = frames.shape[:3]
    key, _ = ctx.rollout(frames, 0, 20)
    _, table, _ = ctx.encode("abs", [bound], True, payload="resident")
    s_rows, q_rows, rec, q = [], [], None, None
    for _ in range(RUNS):
        rec, ms, cms, n = _call(ctx, lambda: ctx.encode_ssim("resident", table))
        s_rows.append((ms, cms, n))
        q, ms, cms, n = _call(ctx, lambda: ctx.encode_quality("resident", table))
        q_rows.append((ms, cms, n))
    fig = ssim.figures(rec)
    # the records against the numpy statement, on the frames the context's own decoder yields (4 of them: numpy is slow)
    payload = ctx.payload_get(0, frames.size).copy()
    ctx.rollout_decode(np.where(key[:, None, None, None], frames, 0).astype(np.uint8), 0)
    dec = ctx.decode(payload, table)
    pick = [0, 1, nt // 2, nt - 1]
    want = ssim.frame_records(dec[pick], frames[pick])
    equal = all((rec[f][pick] == want[f]).all() for f in ("sum_q32", "min_q32", "windows", "reserved"))
    s, qs = _stats(s_rows), _stats(q_rows)
    stack = int(frames.size)
    windows = int(rec["windows"].astype(np.int64).sum())
    return dict(tz_encode_ssim=s, tz_encode_quality=qs,
                k_ssim_over_k_quality=s["quality_class_us_median"] / qs["quality_class_us_median"],
                call_ssim_over_call_quality=s["call_ms_median"] / qs["call_ms_median"],
                stack_bytes_read_by_both=2 * stack, k_ssim_bytes_with_aprons=int(2 * stack * (64 * 64) / (60 * 60)),
                k_ssim_tb_per_s_of_stack_bytes=2 * stack / (s["quality_class_us_median"] * 1e-6) / 1e12,
                windows=windows, ssim=fig["ssim"], ssim_min=fig["ssim_min"],
                ssim_per_frame_min=min(f["ssim"] for f in fig["per_frame"]),
                max_abs_err=int(q["max_abs"].max()), sse=int(q["sse"].astype(np.int64).sum()),
                records_equal_numpy_on_frames=pick, records_equal_numpy=bool(equal))


def main():
    date = datetime.date.today().isoformat()
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "ssim_%s.json" % date)
    cfg = PredNetConfig()
    wts = cfg.init_weights(seed=3)
    nt, h, w = 80, 512, 512
    frames = synth.turbulence(nt, h, w, seed=3)
    ctx = _lib.Context(0)
    ctx.load_model(cfg, wts)
    ctx.prepare(h, w, 20)
    ctx.prof_enable(True)
    doc = dict(date=date, job="cfg3: 512x512, 80 frames, -p 0 -w 20, entropy on, random weights (seed 3), synth.turbulence",
               runs="%d per call, alternating, first dropped, median; spread = [min, max]" % RUNS, modes={})
    try:
        for name, bound in (("lossless", 0.0), ("abs2", 2.0)):
            doc["modes"][name] = mode_part(ctx, frames, bound)
            print(name, json.dumps(doc["modes"][name]), flush=True)
    finally:
        ctx.close()
    doc["notes"] = ("call_ms: HIP events around the whole C call (the shared front -- mask upload, the decoder's tail k_scan2p into "
                    "scratch -- plus the statistics kernel and the copy of the records).  quality_class_us: the 'quality' profiling "
                    "class alone, i.e. k_ssim_init + k_ssim for tz_encode_ssim and k_quality for tz_encode_quality, HIP events around "
                    "the launches (profiling on adds a synchronisation per query, the same for both).  k_ssim reads the two stacks "
                    "per tile of 64x64 pixels, of which 60x60 are its own and the rest the apron of its neighbours.")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
