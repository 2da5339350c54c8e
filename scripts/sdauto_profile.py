#!/usr/bin/env python3
"""What `-c --sdelta auto` (definition TZ-SDA1, tezip_amd/sdauto.py) chooses and what the choice costs, random weights (seed 3),
--coder huffd:
  turbulence          80 frames of 512x512 synth.turbulence, -w 20 (cfg3's job)
  translating_scene   40 frames of 128x160 synth.translating_scene, -w 10 (cfg2's job)
Per job, all from the same resident rollout: lossless, and abs 2 and abs 6 under the greedy and the lattice quantiser.  A
`probe` child records the three sizes E(flat), E(channel), E(plane) and the choice, the HIP-event time (tz_timer_start /
tz_timer_stop on the context's stream) of the whole tz_sdelta_probe call -- it includes its six host waits -- as the median
of RUNS calls after one warm call, and the library's per-kernel events of one more, profiled call.  A `today` child measures
what a user does without the flag: tz_encode (payload resident) + tz_huffd_counts + the host's choice + tz_huffd_encode under
each of the three layouts, one HIP-event interval around all three.  It uses nothing this feature adds, so it runs from a
checkout of the PARENT commit with its library built (parent_tree) -- or from this tree when none is given, which the
document then says.  Children are fresh processes in the order probe, today, probe, today, probe, today; the document holds
every run and the median of the three.  The sizes of the probe must be the sizes of the three real chains, else the script stops.
One GPU process at a time, each under a time limit; the script stops at the first child that fails.  No ratio is asserted.
Usage: python scripts/sdauto_profile.py out.json [parent_tree]"""
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JOBS = (dict(name="turbulence", gen="turbulence", nt=80, h=512, w=512, window=20),
        dict(name="translating_scene", gen="translating_scene", nt=40, h=128, w=160, window=10))
CONFIGS = (("lossless", "greedy", [0.0]), ("abs2-greedy", "greedy", [2.0]), ("abs2-lattice", "lattice", [2.0]),
           ("abs6-greedy", "greedy", [6.0]), ("abs6-lattice", "lattice", [6.0]))
MODES = ("flat", "channel", "plane")
MARK = {"flat": 1, "channel": 4, "plane": 8}
CODER = "huffd"
RUNS = 7
PROCESSES = 3
HBM_PEAK = 8.0e12   # bytes / s (spec)


def timed(ctx, fn):
    ms = []
    for _ in range(RUNS):
        ctx.synchronize()
        ctx.timer_start()
        fn()
        ms.append(ctx.timer_stop())
    return float(np.median(ms)), ms


def set_mode(ctx, mode):
    ctx.set_delta_plane(0)
    ctx.set_delta_stride(1 if mode == "channel" else 0)
    if mode == "plane":
        ctx.set_delta_plane(1)


def child(root, kind):
    """Measure with the package of the tree `root`; prints one JSON line."""
    sys.path.insert(0, root)
    from tezip_amd import _lib, huff, huffd, synth
    from tezip_amd.prednet import PredNetConfig
    cfg = PredNetConfig()
    wts = cfg.init_weights(seed=3)
    out = {}
    for j in JOBS:
        frames = getattr(synth, j["gen"])(j["nt"], j["h"], j["w"])
        nt, h, w = frames.shape[:3]
        n = nt * h * w * 3
        ctx = _lib.Context(0)
        try:
            ctx.load_model(cfg, wts)
            ctx.prepare(_lib.pad8(h), _lib.pad8(w), min(j["window"], 20))
            ctx.rollout(frames, 0, j["window"])
            for cname, quant, bound in CONFIGS:
                ctx.set_quantiser(quant)
                set_mode(ctx, "flat")
                rec = dict(n=n)
                if kind == "probe":
                    from tezip_amd import sdauto
                    state = {}

                    def probe():
                        state["recs"] = ctx.sdelta_probe("abs", bound, True, CODER)

                    probe()                                                     # warm: buffers, lazy allocations
                    rec["probe_ms"], rec["probe_ms_all"] = timed(ctx, probe)
                    chosen, sizes = sdauto.choose(state["recs"], CODER)
                    rec.update(chosen=chosen, bytes=sizes, huffd_D=[int(r["dist"]) for r in state["recs"]])
                    ctx.prof_enable(True)
                    ctx.prof_reset()
                    probe()
                    prof = ctx.prof_get()
                    ctx.prof_enable(False)
                    rec["probe_kernels_ms"] = {k: [v[0], v[1]] for k, v in prof.items() if v[1]}   # [ms, launches]
                    # the six launches one by one, through the seams on this configuration's quantised delta stack (staged to
                    # the device outside the profiled scope: the stage brackets the kernel alone); any code of full support
                    q = np.ascontiguousarray(ctx.encode("abs", bound, True, want_delta=True)[2]).reshape(-1)
                    lens = np.full(_lib.SIZE_BINS + 8, 8, np.uint8)
                    split = {}
                    for mode, r in zip(MODES, state["recs"]):
                        d = int(r["dist"])
                        if mode == "plane":
                            calls = (("k_size_count", lambda: ctx.size_count_plane_buf(q, (nt, h, w), 3, True)),
                                     ("k_size_bits", lambda d=d: ctx.size_bits_plane_buf(q, (nt, h, w), lens, d, 3, True)))
                        else:
                            s = 3 if mode == "channel" else 1
                            calls = (("k_size_count", lambda s=s: ctx.size_count_buf(q, 3, s, True)),
                                     ("k_size_bits", lambda s=s, d=d: ctx.size_bits_buf(q, lens, d, 3, s, True)))
                        ctx.prof_enable(True)
                        for name, fn in calls:
                            for _ in range(3):
                                ctx.prof_reset()
                                fn()
                            ms = float(ctx.prof_get()["huffman"][0])
                            nbytes = 2.0 * n * (2 if mode == "plane" else 1)      # the plane walk reads the row above as well
                            split["%s/%s" % (mode, name)] = dict(ms=ms, bytes=nbytes, tb_per_s=nbytes / (ms * 1e-3) / 1e12)
                        ctx.prof_enable(False)
                    rec["size_kernels"] = split
                    del q
                else:
                    state = {}

                    def today():
                        for mode in MODES:
                            set_mode(ctx, mode)
                            table = ctx.encode("abs", bound, True, payload="resident")[1]
                            c3, base = ctx.huffd_counts()
                            dist, ln, _ = huffd.choose(c3)
                            nbytes = ctx.huffd_encode(ln, base, dist)
                            trailer = huff.reference_trailer(table, (MARK[mode], nt, h, w, 3), 0)
                            state[mode] = len(huffd.pack_front(trailer, ln, base, n, huff.geometry(n)[1],
                                                               (nbytes - huff.body_bytes(n, 0)) // 4, dist)) + nbytes

                    today()
                    rec["today_ms"], rec["today_ms_all"] = timed(ctx, today)
                    rec["bytes"] = [state[m] for m in MODES]
                out["%s/%s" % (j["name"], cname)] = rec
                print(json.dumps({j["name"]: cname, "rec": rec}), file=sys.stderr, flush=True)
        finally:
            ctx.close()
    print("SDAUTO_PROFILE " + json.dumps(out), flush=True)


def run_child(root, kind):
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--child", root, kind],
                       capture_output=True, text=True)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("SDAUTO_PROFILE ")]
    if r.returncode != 0 or not lines:
        raise SystemExit("the %s measurement in %s ended with status %d:\n%s\n%s" % (kind, root, r.returncode, r.stdout[-2000:], r.stderr[-4000:]))
    return json.loads(lines[-1][len("SDAUTO_PROFILE "):])


def main():
    if sys.argv[1] == "--child":
        return child(sys.argv[2], sys.argv[3])
    out_path = sys.argv[1]
    parent = os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else None
    runs = []
    for _ in range(PROCESSES):      # (one after the other: a child that failed ends the script before the next starts)
        for kind, root in (("probe", HERE), ("today", parent or HERE)):
            runs.append((kind, run_child(root, kind)))
            print("%s child %d of %d done" % (kind, len(runs), 2 * PROCESSES), file=sys.stderr, flush=True)
    probes = [r for k, r in runs if k == "probe"]
    todays = [r for k, r in runs if k == "today"]
    summary = {}
    for key, p in probes[0].items():
        t = todays[0][key]
        if p["bytes"] != t["bytes"] or any(q[key]["bytes"] != p["bytes"] for q in probes + todays):
            raise SystemExit("%s: the probe's sizes %r are not the real chains' %r" % (key, p["bytes"], t["bytes"]))
        probe_ms = [q[key]["probe_ms"] for q in probes]
        today_ms = [q[key]["today_ms"] for q in todays]
        kernels = p["probe_kernels_ms"]
        size_ms = kernels.get("huffman", [0.0, 0])[0]
        summary[key] = dict(bytes=p["bytes"], chosen=p["chosen"], huffd_D=p["huffd_D"],
                            chosen_over_flat=min(p["bytes"]) / p["bytes"][0], worst_over_chosen=max(p["bytes"]) / min(p["bytes"]),
                            probe_ms=float(np.median(probe_ms)), probe_ms_processes=probe_ms,
                            today_ms=float(np.median(today_ms)), today_ms_processes=today_ms,
                            today_over_probe=float(np.median(today_ms)) / float(np.median(probe_ms)),
                            probe_kernels_ms=kernels, size_kernels=p["size_kernels"],
                            # the six launches of the size kernels read the stack once each, the plane pair its row above once
                            # more: 2 bytes x n x (6 + 2)
                            size_kernels_tb_per_s=(2.0 * p["n"] * 8 / (size_ms * 1e-3) / 1e12) if size_ms else None)
    doc = dict(jobs=JOBS, weights="random (seed 3)", coder=CODER, configs=[list(c) for c in CONFIGS], runs=RUNS, processes=PROCESSES,
               today_build="parent commit" if parent else "this tree (no parent tree was given)",
               all_runs=[dict(kind=k, results=r) for k, r in runs], summary=summary,
               notes="One device, one GPU process at a time.  Key: job / configuration; lists of three are in the order flat, channel, "
                     "plane.  bytes: E(layout), the entropy.dat the job would write under --coder huffd; the `today` children write the "
                     "three streams and must agree.  probe_ms: HIP events around one tz_sdelta_probe call (delta, quantiser, and per "
                     "layout k_size_count, a host wait, k_size_bits, a host wait).  today_ms: HIP events around tz_encode (payload "
                     "resident) + tz_huffd_counts + tz_huffd_encode under the three layouts, host code choice included.  Medians of %d "
                     "calls after one warm call per process, then the median over %d fresh processes, probe and today alternating.  "
                     "probe_kernels_ms: the library's per-stage events of one more, profiled call, [ms, launches]; `huffman` holds the "
                     "six launches of k_size_count / k_size_bits.  size_kernels_tb_per_s: 2 bytes x n x 8 reads over that time.  "
                     "size_kernels: each of the six launches alone, through the seams on the configuration's quantised delta stack "
                     "(the third of three profiled calls), at the match distance of the probe's record under a code of full support; "
                     "bytes: 2 n, 4 n for the plane walk, which reads the row above as a second stream." % (RUNS, PROCESSES))
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(summary, indent=1))


if __name__ == "__main__":
    main()
