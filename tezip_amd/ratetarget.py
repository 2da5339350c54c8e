"""The abs bound that meets a compression-ratio target (`tezip.py -c ... --target-ratio R --coder huff|huffr|huffd`; not in the
reference).

Definition TZ-TRATIO-1 (also DESIGN.md section 9; the mirror image of TZ-TPSNR-1, tezip_amd/target.py).  The predictions of a job
do not depend on its bound, so one rollout serves every candidate; and with a GPU coder the size of entropy.dat is an exact
function of integer counts -- header + trailer + code lengths + index + the sum over the chunks of ceil(chunk bits / 32) words
-- so a candidate costs one quantiser run and two reads of its output (tz_size_probe), and no bit stream is written to know
it.  (zstd's size cannot be known without running zstd: the feature belongs to the GPU coders.)  All of it is integers:

  raw         nt * H * W * 3: the bytes of the frames.
  F           the bytes of filename.txt plus key_frame.dat, exactly as this job writes them; neither depends on the bound.
  budget      budget(raw, R) = floor(raw / R), in Python float64, computed HERE and nowhere else; R finite and > 0.
  candidates  k = 0 .. 510, bound k / 2: the grid of TZ-TPSNR-1 (at 255 no run of the quantiser can close).
  E(k)        the exact size in bytes of the entropy.dat that `-c -m abs -b k/2` would write with the job's other flags
              (--coder, --gray, --sdelta, -w / -t, -n): file_bytes of the record tz_size_probe returns.
  pass(k)     F + E(k) <= budget.
  search      1. probe k = 0; it passes: the result is 0, the job is lossless and took one probe.
              2. else probe k = 510; it fails: the target cannot be met (result None; the job writes no entropy.dat).
              3. else lo = 0 (fails), hi = 510 (passes); while hi - lo > 1: mid = (lo + hi) // 2, hi = mid if pass(mid) else
                 lo = mid; the result is hi.  At most 11 probes.
  guarantee   F + E(k) <= budget, and k == 0 or F + E(k - 1) > budget.

NOT the smallest passing bound: size is not monotone in the bound (a wider bound merges other runs of the quantiser, and the
Huffman code and huffd's match distance change with the counts), so the bisection finds A boundary between a failing and a
passing candidate; a smaller candidate further down may pass as well.

The job then runs as the ordinary `-m abs -b k/2`: every file is what that job writes, and the size of its entropy.dat is the
result probe's E(k).  This module is pure numpy; the probes come from the library (tezip_amd/_lib.py Context.size_probe).
count_of and bits_of are the slow statement of the two kernels behind them (k_size_count, k_size_bits in csrc/tz_codec.hip):
they work on the payload symbols IN FRONT of the rank remap, which is a bijection on the symbols present -- equality at a
distance is unchanged by it, and remapped_counts moves the literal counts to their ranks."""
import json
import math
import os

import numpy as np

from . import huff, huffd, huffr

FILE_NAME = "bound_search.json"
DEFINITION = "TZ-TRATIO-1"
K_MAX = 510             # candidates k = 0 .. K_MAX, bound k / 2
MAX_PROBES = 11
CODERS = {"huff": huff.TZH1, "huffr": huffr.TZR1, "huffd": huffd.TZR2}   # the coders whose file size is a function of counts
BINS, BIAS = 4096, 1024  # TZ_SIZE_BINS, TZ_SIZE_BIAS: literal bin = symbol + BIAS
NTOK = huffr.NTOK
OFFSET = 1600            # TZ_OFFSET (compress.py:348)
NBINS = huff.NBINS
EXIT_UNREACHABLE = 4     # the exit status of a job whose target cannot be met


def check_target(ratio):
    """None, or why `ratio` is no ratio target (the refusal of tezip.py and compress.run)."""
    try:
        r = float(ratio)
    except (TypeError, ValueError):
        return "--target-ratio takes a number, got %r" % (ratio,)
    if math.isnan(r) or math.isinf(r) or r <= 0.0:
        return "--target-ratio must be a finite number above 0, got %r" % (ratio,)
    return None


def budget(raw, ratio):
    """The most bytes the files of a job of `raw` frame bytes may take at a ratio of at least `ratio` (the one float
    computation of TZ-TRATIO-1)."""
    problem = check_target(ratio)
    if problem:
        raise ValueError(problem)
    raw = int(raw)
    if raw < 0:
        raise ValueError("raw size %d" % raw)
    return int(math.floor(raw / float(ratio)))


def bound_of(k):
    return k / 2.0


def search(probe, fixed, limit):
    """probe: k -> E(k), the bytes of candidate k's entropy.dat (an int); fixed: F; limit: the budget.
    -> (k or None, trace), trace = [{"k", "bound", "entropy_bytes", "pass"}] in probe order."""
    fixed, limit = int(fixed), int(limit)
    trace = []

    def ok(k):
        e = int(probe(k))
        trace.append({"k": k, "bound": bound_of(k), "entropy_bytes": e, "pass": fixed + e <= limit})
        return trace[-1]["pass"]

    if ok(0):
        return 0, trace
    if not ok(K_MAX):
        return None, trace
    lo, hi = 0, K_MAX
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if ok(mid):
            hi = mid
        else:
            lo = mid
    return hi, trace


# ---- the size of a file from the record of a probe
def trailer_len(table_len):
    """int16 values of the reference trailer: table | T (or -1 alone), five shape entries, warm_up."""
    return (int(table_len) + 1 if int(table_len) >= 0 else 1) + 6


def file_bytes(record, coder):
    """The bytes of the entropy.dat whose stream `record` describes (a tz_size_record: n, stream_words, A, table_len), by the
    format's own pack_front over empty sections of the right lengths and huff.body_bytes."""
    fmt = CODERS[coder]
    n, words, A = int(record["n"]), int(record["stream_words"]), int(record["A"])
    front = huff.pack_front_of(fmt, np.zeros(trailer_len(record["table_len"]), "<i2"), np.zeros(A + fmt.ntok, np.uint8), 0, n,
                               huff.geometry(n)[1], words)
    return len(front) + huff.body_bytes(n, words)


# ---- the slow statement of k_size_count and k_size_bits
def symbols_of(q, channels=3, stride=1, offset=True):
    """The payload symbols of the quantised delta stack q (int16, (frame, y, x, 3) order) in front of the rank remap, in the
    layout (channels, stride): (3, 1) flat, (3, 3) channel stride, (1, 1) channel 0 alone.  y[i] = x[i - stride] - x[i] in
    int16 (the first `stride`: x[i]), then 1600 - y when offset: the conventions of k_sdelta / k_sdelta_s3 / k_sdelta_gray."""
    x = np.asarray(q, np.int16).reshape(-1)
    if (channels, stride) not in ((3, 1), (3, 3), (1, 1)):
        raise ValueError("no payload layout of %r channels at stride %r" % (channels, stride))
    if channels == 1:
        if x.size % 3:
            raise ValueError("a one-channel payload describes whole pixels, not %d elements" % x.size)
        x = x[0::3]
    sd = x.copy()
    sd[stride:] = (x[:-stride].astype(np.int32) - x[stride:].astype(np.int32)).astype(np.int16)
    return (OFFSET - sd.astype(np.int32)).astype(np.int16) if offset else sd


def _stretches(sym, dist, run=huff.RUN):
    """-> (lit bool[n], start int64[s], m int64[s]): the literals, and the first element and the length of every maximal
    stretch of matches at the distance `dist` (0: no element matches); no match across a run start."""
    n = sym.size
    match = np.zeros(n, bool)
    if dist:
        match[dist:] = sym[dist:] == sym[:-dist]
        match &= (np.arange(n) % run) >= dist
    start = np.nonzero(match & ~np.concatenate([[False], match[:-1]]))[0]
    end = np.nonzero(match & ~np.concatenate([match[1:], [False]]))[0]
    return ~match, start, end - start + 1


def _log2(m):
    return ((m[:, None] >> np.arange(NTOK)) > 0).sum(axis=1) - 1


def count_of(q, channels=3, stride=1, offset=True):
    """k_size_count: (uint64[3][BINS + 8], bad) -- row i at the match distance huffd.DISTS[i]: the literals by bin = symbol +
    BIAS, then T_0..T_7; bad: a symbol outside the bins (it is counted nowhere)."""
    return count_of_symbols(symbols_of(q, channels, stride, offset))


def count_of_symbols(symbols):
    """count_of over ready-made payload symbols (in front of the rank remap), whatever spatial delta formed them."""
    sym = np.asarray(symbols).reshape(-1).astype(np.int64)
    b = sym + BIAS
    inside = (b >= 0) & (b < BINS)
    out = np.zeros((len(huffd.DISTS), BINS + NTOK), np.uint64)
    for i, dist in enumerate(huffd.DISTS):
        lit, _, m = _stretches(sym, dist)
        out[i, :BINS] = np.bincount(b[lit & inside], minlength=BINS)
        out[i, BINS:] = np.bincount(_log2(m), minlength=NTOK)
    return out, bool((~inside).any())


def bits_of(q, lens, dist, channels=3, stride=1, offset=True):
    """k_size_bits: (words, bits, bad) under lens (BINS + 8 code lengths: by bin, then the tokens) at the match distance dist --
    bits per run of 256, per chunk of 64 runs, every chunk rounded up to 32-bit words; bad: a literal or token of length 0."""
    return bits_of_symbols(symbols_of(q, channels, stride, offset), lens, dist)


def bits_of_symbols(symbols, lens, dist):
    """bits_of over ready-made payload symbols (in front of the rank remap), whatever spatial delta formed them."""
    sym = np.asarray(symbols).reshape(-1).astype(np.int64)
    ln = np.asarray(lens, np.int64).reshape(-1)
    if ln.size != BINS + NTOK:
        raise ValueError("%d code lengths, %d + %d wanted" % (ln.size, BINS, NTOK))
    huffd.check_dist(dist)
    b = sym + BIAS
    inside = (b >= 0) & (b < BINS)
    lit, start, m = _stretches(sym, dist)
    per = np.where(lit, np.where(inside, ln[np.clip(b, 0, BINS - 1)], 0), 0)
    bad = bool((per[lit] == 0).any())
    k = _log2(m)
    tok = ln[BINS + k]
    bad = bad or bool((tok == 0).any())
    per[start] += tok + k           # (a stretch is coded at its first element, which is no literal)
    chunk = huff.RUN * huff.CHUNK_RUNS
    cbits = np.add.reduceat(per, np.arange(0, sym.size, chunk)) if sym.size else np.zeros(0, np.int64)
    return int(((cbits + 31) >> 5).sum()), int(cbits.sum()), bad


def rank_of(table):
    """The rank remap as a function of the symbol value (k_lut under build_enc_lut: symbols of the table go to their ranks, every
    other value stays); table None: the identity."""
    lut = np.arange(NBINS + 1, dtype=np.int64)
    if table is not None:
        lut[np.asarray(table, np.int64)] = np.arange(len(table))

    def rank(v):
        v = np.asarray(v, np.int64)
        return np.where((v >= 0) & (v <= NBINS), lut[np.clip(v, 0, NBINS)], v)

    return rank


def table_of(counts):
    """compress.py:352-361 from row 0 of count_of: the symbols inside [0, NBINS) with a count, count descending, ascending symbol
    among equal counts (tz_build_table)."""
    h = np.asarray(counts)[0, BIAS: BIAS + NBINS].astype(np.int64)
    syms = np.nonzero(h)[0]
    return syms[np.argsort(-h[syms], kind="stable")].astype(np.int16)


def remapped_counts(counts, table):
    """count_of's rows -> (uint64[3][A + 8], base) of the payload BEHIND the rank remap by `table` (None: no remap), as
    tz_huffd_counts reports them: the literal counts moved to their ranks (a permutation: the remap is a bijection on the
    symbols present), the tokens as they are."""
    counts = np.asarray(counts, np.uint64)
    rank = rank_of(table)
    r = np.zeros_like(counts)
    bins = np.nonzero(counts[:, :BINS].any(axis=0))[0]
    to = rank(bins - BIAS) + BIAS
    if ((to < 0) | (to >= BINS)).any() or np.unique(to).size != to.size:
        raise ValueError("the rank remap is no bijection inside the bins on the symbols present")
    r[:, to] = counts[:, bins]
    r[:, BINS:] = counts[:, BINS:]
    present = np.nonzero(r[0, :BINS])[0]
    lo, hi = int(present[0]), int(present[-1])
    return np.concatenate([r[:, lo: hi + 1], r[:, BINS:]], axis=1), lo - BIAS


def code_of(counts3, coder):
    """The code the job's host chooses from the remapped counts (compress._huff_entropy_file): -> (dist, lengths uint8[A + ntok])."""
    if coder == "huffd":
        dist, lengths, _ = huffd.choose(counts3)
        return dist, lengths
    if coder == "huffr":
        return 3, huffr.code_lengths(counts3[2])
    return 0, huff.code_lengths(counts3[0][:-NTOK])


def lens_of(lengths, coder, dist, base, table):
    """The LUT of k_size_bits from the code lengths of `coder` (A, then its tokens): uint8[BINS + 8], by bin the code length of
    the symbol's rank, then the token lengths (0 at dist 0)."""
    lengths = np.asarray(lengths, np.uint8)
    A = lengths.size - CODERS[coder].ntok
    s = rank_of(table)(np.arange(BINS) - BIAS) - int(base)
    out = np.zeros(BINS + NTOK, np.uint8)
    ok = (s >= 0) & (s < A)
    out[:BINS][ok] = lengths[s[ok]]
    if dist:
        out[BINS:] = lengths[A: A + NTOK]
    return out


# ---- bound_search.json and the printed lines
def make(ratio, raw, limit, fixed, trace, k):
    """bound_search.json as a JSON-ready dict; k None: the target cannot be met."""
    result = None
    if k is not None:
        e = next(t["entropy_bytes"] for t in reversed(trace) if t["k"] == k)
        result = {"k": int(k), "mode": "abs", "bound": bound_of(k), "entropy_bytes": int(e)}
    return {
        "definition": DEFINITION,
        "target_ratio": float(ratio),
        "raw_bytes": int(raw),
        "budget_bytes": int(limit),
        "fixed_bytes": int(fixed),
        "probes": len(trace),
        "trace": [dict(t) for t in trace],
        "result": result,
    }


def write(out_dir, doc):
    path = os.path.join(out_dir, FILE_NAME)
    with open(path, "w", encoding="UTF-8") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return path


def stdout_line(doc):
    r = doc["result"]
    return "target: ratio >= %g -> abs bound %g (%d probes, %d + %d bytes <= %d)" % (doc["target_ratio"], r["bound"], doc["probes"],
                                                                                    doc["fixed_bytes"], r["entropy_bytes"], doc["budget_bytes"])


def unreachable_line(doc):
    """The message of a job whose loosest candidate still misses the budget."""
    last = next(t for t in doc["trace"] if t["k"] == K_MAX)
    total = doc["fixed_bytes"] + last["entropy_bytes"]
    return "ERROR: --target-ratio %g cannot be met: at abs %g the files take %d bytes (ratio %.6g)" % (
        doc["target_ratio"], bound_of(K_MAX), total, doc["raw_bytes"] / total)
