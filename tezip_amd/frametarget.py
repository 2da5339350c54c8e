"""One abs bound per frame: the PSNR floor of `tezip.py -c ... --target-psnr DB --per-frame` and the explicit list of
`-c -m abs --frame-bounds FILE` (not in the reference).

The reference's error_bound runs per frame and channel (compress.py:316-319), so a frame's quantised delta depends on that
frame's tolerance alone, and the decoder never sees a bound: a job with a different bound in every frame is an ordinary job
of the reference's format (tz_set_frame_bounds, include/tezip_hip.h).

Definition TZ-TPSNR-F1 (also DESIGN.md section 9).  It is TZ-TPSNR-1 (tezip_amd/target.py, whose sse_limit, bound_of, K_MAX and
check_target it uses) held per frame instead of over the sequence:

  samples     n = H * W * 3: the samples of ONE frame.
  limit       target.sse_limit(T, n), the same for every frame.
  fixed       the frames whose delta the encoder zeroes or never quantises -- frame 0, the warm-up frames, the key frames:
              they are stored exactly, their bound is 0 and they are not searched.
  searched    every other frame f, each with its own lo_f = 0, hi_f = 511.  One probe takes bounds[f] = mid_f / 2 for every
              frame whose interval is still open (mid_f = (lo_f + hi_f) // 2); finished frames ride along at lo_f / 2 and
              fixed frames at 0.  It is ONE tz_bound_probe under tz_set_frame_bounds and yields every frame's sse;
              pass_f <=> sse_f <= limit; lo_f = mid_f if pass_f else hi_f = mid_f.  Stop when every interval has closed: at
              most 9 probes for the whole job.  limit == 0: every k_f = 0 and no probe runs.
  guarantee   per searched frame: sse_f(k_f) <= limit, and k_f == 510 or sse_f(k_f + 1) > limit, where sse_f(k) is what the
              uniform job `-m abs -b k/2` reports for frame f (frame f's quantised delta under bounds[f] = k/2 is bit for bit
              that job's, whatever the other frames' bounds are).

NOT the largest passing bound: SSE is not monotone in the bound (a wider bound merges other runs, whose midpoints can lie
nearer the deltas, and the decoder's clamp to [0, 255] removes error the quantiser made), so the bisection finds A boundary
between a passing and a failing candidate; a larger candidate further up may pass as well.

With --gray on an all-gray job the records are the one-channel job's, as in TZ-TPSNR-1.  The job then runs under
tz_set_frame_bounds with the bounds found.  This module is pure numpy; the probe is passed in."""
import json
import math
import os

from . import target

FILE_NAME = target.FILE_NAME
DEFINITION = "TZ-TPSNR-F1"

NEEDS_TARGET = "--per-frame holds every frame to the PSNR of --target-psnr: add --target-psnr DB"
NOT_WITH_RATIO = "--per-frame cannot be combined with --target-ratio (a per-frame ratio target is not defined)"
BOUNDS_NEED_ABS = "--frame-bounds gives abs bounds: it goes with -m abs and takes the place of -b"
BOUNDS_NOT_WITH_TARGET = "--frame-bounds gives the bounds itself: it cannot be combined with --target-psnr or --target-ratio"
NOT_SHARDED = "per-frame bounds are not available for a sharded job (WORLD_SIZE > 1): run it on one GPU"


def check(per_frame, frame_bounds, mode, bound, target_psnr, target_ratio, sharded):
    """The refusals of --per-frame and --frame-bounds that tezip.py and a direct caller of compress.run share: None, or the
    message."""
    if per_frame:
        if target_ratio is not None:
            return NOT_WITH_RATIO
        if target_psnr is None:
            return NEEDS_TARGET
        if frame_bounds is not None:
            return BOUNDS_NOT_WITH_TARGET
    if frame_bounds is not None:
        if target_psnr is not None or target_ratio is not None:
            return BOUNDS_NOT_WITH_TARGET
        if mode != "abs" or bound:
            return BOUNDS_NEED_ABS
    if (per_frame or frame_bounds is not None) and sharded:
        return NOT_SHARDED
    return None


def fixed_frames(key, warm_up):
    """key: the rollout's key mask (nt).  -> nt bools, True for frame 0, the warm-up frames and the key frames."""
    fixed = [bool(k) for k in key]
    for f in range(min(len(fixed), max(1, int(warm_up)))):
        fixed[f] = True
    return fixed


def search(probe, limit, fixed):
    """probe: a list of nt candidates k (0 at fixed frames) -> the nt per-frame sse of the job under bounds k / 2.
    -> (ks, sse, trace): the nt results k_f (0 at fixed frames), sse_f(k_f) as the probes reported it, and per probe
    {"k", "sse", "pass"}, lists over all frames with None at fixed frames."""
    limit = int(limit)
    fixed = [bool(x) for x in fixed]
    nt = len(fixed)
    lo, hi = [0] * nt, [1 if fx else target.K_MAX + 1 for fx in fixed]
    sse_lo = [0] * nt   # (k = 0 is never probed: lossless)
    trace = []
    if limit <= 0:
        return lo, sse_lo, trace
    while any(hi[f] - lo[f] > 1 for f in range(nt)):
        is_open = [hi[f] - lo[f] > 1 for f in range(nt)]
        cand = [(lo[f] + hi[f]) // 2 if is_open[f] else lo[f] for f in range(nt)]
        sse = [int(s) for s in probe(list(cand))]
        if len(sse) != nt:
            raise ValueError("the probe returned %d records for %d frames" % (len(sse), nt))
        ok = [s <= limit for s in sse]
        trace.append({"k": [None if fixed[f] else cand[f] for f in range(nt)],
                      "sse": [None if fixed[f] else sse[f] for f in range(nt)],
                      "pass": [None if fixed[f] else ok[f] for f in range(nt)]})
        for f in range(nt):
            if not is_open[f]:
                continue
            if ok[f]:
                lo[f], sse_lo[f] = cand[f], sse[f]
            else:
                hi[f] = cand[f]
    return lo, sse_lo, trace


def make(target_db, frame_samples, limit, fixed, names, ks, sse, trace):
    """bound_search.json of a per-frame search as a JSON-ready dict."""
    nt = len(fixed)
    return {
        "definition": DEFINITION,
        "target_psnr_db": float(target_db),
        "frame_samples": int(frame_samples),
        "sse_limit": int(limit),
        "probes": len(trace),
        "trace": [{"k": list(t["k"]), "sse": list(t["sse"]), "pass": list(t["pass"])} for t in trace],
        "frames": [{"index": f, "name": None if names is None else str(names[f]), "fixed": bool(fixed[f]), "k": int(ks[f]),
                    "bound": target.bound_of(int(ks[f])), "sse": int(sse[f])} for f in range(nt)],
        "frame_bounds": [0.0 if fixed[f] else target.bound_of(int(ks[f])) for f in range(nt)],
    }


def write(out_dir, doc):
    return target.write(out_dir, doc)


def stdout_line(doc):
    searched = [fr["bound"] for fr in doc["frames"] if not fr["fixed"]]
    head = "target: PSNR >= %g dB in every frame -> " % doc["target_psnr_db"]
    if not searched:
        return head + "nothing to search"
    return head + "abs bounds %g..%g (%d probes, %d of %d frames searched)" % (min(searched), max(searched), doc["probes"],
                                                                              len(searched), len(doc["frames"]))


# ---- explicit bounds: --frame-bounds FILE, compress.run(FRAME_BOUNDS=...)
def _entries(seq, where):
    if not isinstance(seq, (list, tuple)):
        raise ValueError("%s: a list of numbers is wanted, or an object with a \"frame_bounds\" list" % where)
    out = []
    for i, v in enumerate(seq):
        if isinstance(v, bool) or not isinstance(v, (int, float)):
            raise ValueError("%s: entry %d is %r, not a number" % (where, i, v))
        v = float(v)
        if math.isnan(v) or math.isinf(v) or v < 0.0:
            raise ValueError("%s: entry %d is %r: a bound is finite and >= 0" % (where, i, v))
        out.append(v)
    if not out:
        raise ValueError("%s: no bounds" % where)
    return out


def load(spec, flag="--frame-bounds", name="FRAME_BOUNDS"):
    """spec: the path of a JSON file -- a list of numbers, or an object with a "frame_bounds" list (the bound_search.json of a
    per-frame search replays) -- or a sequence of numbers.  -> the list of floats.  ValueError names the file and the index.
    flag, name: what the messages call the command-line flag and compress.run's argument (--loop-bounds reads the same files)."""
    if isinstance(spec, (str, bytes, os.PathLike)):
        path = os.fspath(spec)
        where = "%s %s" % (flag, path)
        try:
            with open(path, "r", encoding="UTF-8") as f:
                doc = json.load(f)
        except OSError as e:
            raise ValueError("%s: cannot be read (%s)" % (where, e.strerror or e)) from None
        except (ValueError, UnicodeDecodeError) as e:
            raise ValueError("%s: not JSON (%s)" % (where, e)) from None
        if isinstance(doc, dict):
            if "frame_bounds" not in doc:
                raise ValueError("%s: the object has no \"frame_bounds\" list" % where)
            doc = doc["frame_bounds"]
        return _entries(doc, where)
    try:
        seq = [v.item() if hasattr(v, "item") else v for v in spec]
    except TypeError:
        raise ValueError("%s: a path or a sequence of numbers is wanted, got %r" % (name, spec)) from None
    return _entries(seq, name)


def where_of(spec, flag="--frame-bounds", name="FRAME_BOUNDS"):
    return "%s %s" % (flag, os.fspath(spec)) if isinstance(spec, (str, bytes, os.PathLike)) else name


def check_length(bounds, nt, spec, flag="--frame-bounds", name="FRAME_BOUNDS"):
    """None, or the refusal of a list that does not have one entry per image."""
    if len(bounds) != int(nt):
        return "%s: %d bounds for %d images" % (where_of(spec, flag, name), len(bounds), int(nt))
    return None


def explicit_line(bounds):
    return "frame bounds: %d frames, abs %g..%g" % (len(bounds), min(bounds), max(bounds))
