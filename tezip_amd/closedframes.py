"""The closed loop under one abs bound per frame (`tezip.py -c --loop closed --quant lattice --loop-psnr DB`, or `-m abs
--loop-bounds FILE`; tz_rollout_closed_frames; NOT a reference feature), definition TZ-CLF1 -- the slow statement of it in numpy,
the specification the GPU is tested against.

In a closed loop (TZ-CL1, tezip_amd/closedloop.py) the prediction of frame t depends on dec[t-1] only.  When the loop reaches
frame t, pred_t is fixed, so every candidate bound for frame t is priced by an elementwise pass over (pred_t, orig_t): no
predictor step is involved, and the bound is fixed before step t + 1 starts.  A PSNR floor in every frame therefore costs ONE
closed-loop rollout; the sequence-wide targets (--target-psnr without --per-frame, --target-ratio) would need a rollout per
candidate and stay refused.

TZ-CLF1 is TZ-CL1 except for the tolerance of a non-key frame:

  key mask, groups, fixed frames (frame 0, warm-up, key frames: stored exactly), the feeding rule, x = trunc(f32(pred * 255)),
  d = x - orig, dec[t] = clamp(x - q, 0, 255), the mark and the decoder: TZ-CL1's.
  quantiser     TZ-QL1 (tezip_amd/lattice.py) with the frame's own radius: E_t = min(255, floor(b_t)), q = Q_{E_t}(d); E_t = 0 is
                the identity.
  bounds given  b_t from a list of nt finite numbers >= 0; entries at fixed frames are taken as 0.  Every E_t = 0: the lossless
                closed job, one schedule, byte for byte.
  bounds searched
                limit = target.sse_limit(DB, H * W * 3), as everywhere else.  For each non-fixed frame t, in loop order, once
                pred_t exists:  sse_t(k) = sum (clamp(x - Q_{floor(k / 2)}(x - orig_t), 0, 255) - orig_t)^2 over the frame's
                H * W * 3 samples, exact integers.  The bisection is target.search's: lo = 0, hi = 511, mid = (lo + hi) // 2,
                pass iff sse_t(mid) <= limit, at most 9 probes.  k_t = lo, b_t = k_t / 2; dec[t] is formed with
                E_t = floor(k_t / 2) and fed to step t + 1.  limit == 0 is the lossless closed job, with no probe.
  guarantee     per searched frame: sse_t(k_t) <= limit, and k_t == 510 or sse_t(k_t + 1) > limit.  A boundary, not the largest
                passing bound, for the reasons TZ-TPSNR-1 gives (tezip_amd/target.py).  sse_t is taken GIVEN the dec[t-1] that the
                earlier frames' results produced: the search is greedy in time, it does not optimise the sequence.
  stored stream q is a pure function of (final pred, orig, b_t): the unchanged back half under tz_set_frame_bounds(b) with the
                lattice quantiser forms the loop's q again.  The stream is an ordinary closed-loop stream (marks 17/18/20/21/24/25)
                and `-u` takes no flag and no new code path.

This module is pure numpy; the predictor is passed in, as for closedloop.encode."""
import numpy as np

from . import closedloop, frametarget, lattice, target

DEFINITION = "TZ-CLF1"
FILE_NAME = target.FILE_NAME
ROUNDS = 9                      # 511 -> 1 by halving
NOT_RUN = 2 ** 64 - 1           # tz_loop_search_trace: the round did not run for the frame

FLAG_PSNR, FLAG_BOUNDS = "--loop-psnr", "--loop-bounds"


def _flag(loop_psnr):
    return FLAG_PSNR if loop_psnr is not None else FLAG_BOUNDS


def check_flags(loop_psnr, loop_bounds, loop, quant, mode, bound, pred=None, compressing=True, sweep=False, sharded=False, gray=False,
                threshold=None, target_psnr=None, target_ratio=None, per_frame=False, frame_bounds=None, bound_map=None):
    """The refusals of --loop-psnr and --loop-bounds that tezip.py and a direct caller of compress.run share: None, or the message.
    loop_bounds is only asked whether it is there (load() reads it).  Without either flag nothing is refused here."""
    if loop_psnr is None and loop_bounds is None:
        return None
    flag = _flag(loop_psnr)
    if not compressing:
        return "%s is valid with -c (--compress) only (-u decodes such a job without a flag)" % flag
    if loop_psnr is not None and loop_bounds is not None:
        return "%s finds the bounds, %s gives them: a job takes one of the two" % (FLAG_PSNR, FLAG_BOUNDS)
    if loop != "closed":
        return "%s sets the bounds of a closed loop: add --loop closed" % flag
    if quant != "lattice":
        return "%s needs a quantiser that is a function of one sample: add --quant lattice" % flag
    if pred in ("select", "motion"):
        return "%s cannot be combined with --pred %s (selection under a per-frame bound is out of scope)" % (flag, pred)
    for on, other, why in ((threshold is not None, "-t", "the closed loop runs fixed windows: use -w"),
                           (sweep, "--sweep", "run the job you want with -w"),
                           (gray, "--gray", "the loop decodes three channels"),
                           (target_psnr is not None, "--target-psnr", "a sequence-wide target needs a rollout per candidate"),
                           (target_ratio is not None, "--target-ratio", "a sequence-wide target needs a rollout per candidate"),
                           (per_frame, "--per-frame", "that is the open loop's search; %s is the closed loop's" % FLAG_PSNR),
                           (frame_bounds is not None, "--frame-bounds", "those are the open loop's bounds; %s gives the closed loop's" % FLAG_BOUNDS),
                           (bound_map is not None, "--bound-map", "the loop takes one bound per frame")):
        if on:
            return "%s cannot be combined with %s (%s)" % (flag, other, why)
    if sharded:
        return "%s is not available for a sharded job (WORLD_SIZE > 1): run it on one GPU" % flag
    if bound:
        return "%s takes the place of -b" % flag
    if loop_psnr is not None:
        if mode is not None:
            return "%s finds abs bounds: it takes the place of -m and -b" % FLAG_PSNR
        problem = target.check_target(loop_psnr)
        return problem.replace("--target-psnr", FLAG_PSNR) if problem else None
    if mode != "abs":
        return "%s gives abs bounds: it goes with -m abs and takes the place of -b" % FLAG_BOUNDS
    return None


def load(spec):
    """--loop-bounds FILE / LOOP_BOUNDS: what frametarget.load accepts (a search's bound_search.json replays)."""
    return frametarget.load(spec, FLAG_BOUNDS, "LOOP_BOUNDS")


def check_length(bounds, nt, spec):
    return frametarget.check_length(bounds, nt, spec, FLAG_BOUNDS, "LOOP_BOUNDS")


# ---------------------------------------------------------------------------------------------------- the slow statement
def radius(b):
    """E = min(255, floor(b)) of one bound."""
    return int(lattice.step_radius(float(b)))


def decode_under(x, orig, e):
    """(q, dec) of one frame under the radius e: q = Q_e(x - orig) (the identity for e = 0), dec = clamp(x - q, 0, 255)."""
    d = np.asarray(x, np.int64) - np.asarray(orig, np.int64)
    q = lattice.quantise_e(d, float(e))
    return q, np.clip(x - q, 0, 255)


def sse_of(x, orig, k):
    """sse_t(k): the squared error of the frame decoded under candidate k (bound k / 2), an exact int."""
    _, dec = decode_under(x, orig, k // 2)
    e = dec - np.asarray(orig, np.int64)
    return int((e * e).sum())


def normalise(bounds, key):
    """The bounds of the job: the list with 0 at fixed frames."""
    return [0.0 if k else float(b) for k, b in zip(key, bounds)]


def encode(frames, p, w, predictor, bounds=None, limit=None):
    """The encoder's loop.  frames, p, w, predictor as closedloop.encode; exactly one of bounds (nt finite numbers >= 0) and limit
    (the sse a frame may reach, >= 0; 0: the lossless job, no probe).  Returns dict(key, pred, q, dec) as closedloop.encode, plus
    bounds float64[nt] (0 at fixed frames), k int[nt] and sse int[nt] (the search's k_t and sse_t(k_t); zeros after given bounds)
    and trace (ROUNDS, nt) of python ints, NOT_RUN where a round did not run."""
    if (bounds is None) == (limit is None):
        raise ValueError("give the bounds or the limit to search them under, not %s" % ("both" if bounds is not None else "neither"))
    frames = np.asarray(frames, np.uint8)
    nt, h, wd, _ = frames.shape
    hp, wp = closedloop.pad8(h), closedloop.pad8(wd)
    key, gfirst = closedloop.key_mask(nt, p, w), closedloop.group_first(nt, p, w)
    if bounds is not None:
        b = np.asarray(bounds, np.float64)
        if b.shape != (nt,) or not np.isfinite(b).all() or (b < 0).any():
            raise ValueError("bounds must be %d finite numbers >= 0" % nt)
        bounds = normalise(b, key)
    c0 = np.asarray(predictor.c0(hp, wp), np.float32)
    pred = np.empty((nt, hp, wp, 3), np.float32)
    q = np.zeros((nt, h, wd, 3), np.int64)
    dec = np.zeros_like(frames)
    ks, sse = [0] * nt, [0] * nt
    trace = [[NOT_RUN] * nt for _ in range(ROUNDS)]
    for t in range(nt):
        orig = frames[t].astype(np.int64)
        if key[t]:
            pred[t] = c0
            dec[t] = frames[t]
            q[t] = 0 if gfirst[t] else closedloop.x_hat(c0, h, wd) - orig
            continue
        pred[t] = np.asarray(predictor.next(closedloop.u8_to_f32(dec[t - 1], hp, wp)), np.float32)
        x = closedloop.x_hat(pred[t], h, wd)
        if bounds is not None:
            e = radius(bounds[t])
        else:
            probes = []

            def probe(k):
                probes.append(sse_of(x, orig, k))
                return probes[-1]

            ks[t], tr = target.search(probe, limit)
            for r, s in enumerate(probes):
                trace[r][t] = s
            sse[t] = next((s["sse"] for s in tr if s["k"] == ks[t]), 0)
            e = ks[t] // 2
        q[t], d = decode_under(x, orig, e)
        dec[t] = d.astype(np.uint8)
    if bounds is None:
        bounds = [0.0 if key[t] else target.bound_of(ks[t]) for t in range(nt)]
    return dict(key=key, pred=pred, q=q.astype(np.int16), dec=dec, bounds=np.asarray(bounds, np.float64), k=ks, sse=sse, trace=trace)


def open_loop_q(pred, frames, p, w, bounds):
    """What the OPEN-loop formulas under per-frame bounds (delta, zeroed group firsts, TZ-QL1 with bounds[t] on every frame that is
    not skipped: lattice.quantise_stack) give on a prediction stack -- on the loop's final predictions this is encode()'s q."""
    frames = np.asarray(frames, np.uint8)
    nt, h, wd, _ = frames.shape
    gfirst = closedloop.group_first(nt, p, w)
    skip = gfirst.copy()
    skip[:p] = True
    d = np.zeros((nt, h, wd, 3), np.int64)
    for t in range(nt):
        if not gfirst[t]:
            d[t] = closedloop.x_hat(pred[t], h, wd) - frames[t].astype(np.int64)
    return lattice.quantise_stack(frames, d, "abs", [0.0], skip=skip, bounds=bounds)


# ---------------------------------------------------------------------------------------------------- the job's lines and file
def make(target_db, frame_samples, limit, fixed, names, bounds, sse, trace):
    """bound_search.json of a --loop-psnr job as a JSON-ready dict.  bounds: k / 2 per frame (0 at fixed frames); sse: sse_t(k_t);
    trace: (ROUNDS, nt), NOT_RUN where a round did not run."""
    nt = len(fixed)
    ks = [int(round(2 * float(b))) for b in bounds]
    rounds = []
    for row in trace:
        row = [None if int(s) == NOT_RUN else int(s) for s in row]
        if any(s is not None for s in row):
            rounds.append({"sse": row, "pass": [None if s is None else s <= int(limit) for s in row]})
    return {
        "definition": DEFINITION,
        "target_psnr_db": float(target_db),
        "frame_samples": int(frame_samples),
        "sse_limit": int(limit),
        "probes": len(rounds),
        "trace": rounds,
        "frames": [{"index": f, "name": None if names is None else str(names[f]), "fixed": bool(fixed[f]), "k": ks[f],
                    "bound": target.bound_of(ks[f]), "sse": int(sse[f])} for f in range(nt)],
        "frame_bounds": [0.0 if fixed[f] else target.bound_of(ks[f]) for f in range(nt)],
    }


def write(out_dir, doc):
    return target.write(out_dir, doc)


def stdout_line(doc):
    searched = [fr["bound"] for fr in doc["frames"] if not fr["fixed"]]
    head = "loop target: PSNR >= %g dB in every frame -> " % doc["target_psnr_db"]
    if not searched or doc["sse_limit"] <= 0:
        return head + "nothing to search"
    return head + "abs bounds %g..%g (%s, %d of %d frames searched)" % (min(searched), max(searched), DEFINITION, len(searched),
                                                                        len(doc["frames"]))


def explicit_line(bounds):
    return "loop bounds: %d frames, abs %g..%g" % (len(bounds), min(bounds), max(bounds))
