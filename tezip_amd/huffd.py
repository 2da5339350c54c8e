"""The Huffman-coded entropy.dat whose coder picks its match distance (`--coder huffd`; NOT a reference format): container,
validation, the choice rule and the numpy encoder / decoder of the stream the GPU kernels write (k_huffd_count, then k_huff_size /
k_huff_enc / k_huff_dec or k_huffr_size / k_huffr_enc / k_huffr_dec at the chosen distance, csrc/tz_codec.hip).  The stream has
ONE statement: huff.py's without tokens (D = 0), huffr.py's tokeniser, encoder and decode loop at the distance D = 1 or 3; this
module delegates to them.  The slow code is the specification the kernels are tested against (tests/test_huffd.py,
tests/test_gpu_huffd.py); the product never calls it on the hot path.  DESIGN.md section 9 holds the format as prose.

TZR2 is TZR1 (tezip_amd/huffr.py) with another magic and the match distance D in the header's last u32:
  header   48 bytes: "TZR2" | u16 version = 1 | u16 L = 12 | u64 n | i32 base | u32 A | u32 R | u32 chunk_runs |
           u32 nchunks | u32 stream_words | u32 trailer_len | u32 D          D is 0, 1 or 3
  trailer, lengths (always A + 8 bytes), index, bits: as in TZR1
D = 1 or 3: huffr.py's statement with 3 replaced by D.  Element j of a run is a MATCH when j >= D and s[j] == s[j - D]; every
maximal stretch of m matches (cut at the run's end, so m <= R - D <= 255: T_7 with 7 raw bits still holds it) is the token
T_k, k = floor(log2 m), followed by k raw bits; the imaginary history in front of a run is D elements equal to `base`.  For
D = 3 index and bits are TZR1's byte for byte.
D = 0: no element matches, the eight token lengths are 0, and index and bits are TZH1's (tezip_amd/huff.py) for the same
literal lengths.
The choice of D is part of the format's statement, so that the GPU's counts and numpy give the same file: counts_D is the token
histogram at distance D (D = 0: the plain histogram, eight zeros appended); len_D the length-limited code of counts_D
(tz_huff_lengths over the A literals for D = 0, tz_huffr_lengths over A + 8 counts otherwise); cost_D = sum_s counts_D[s] *
len_D[s] + sum_k k * counts_D[A + k] bits, an exact integer.  The smallest cost wins, a tie goes to the smaller D.
Size: cost_D is the number of stream bits before the chunks are padded to words, and every other section is shared, so a TZR2
file is at most min(TZH1 file, TZR1 file) + 4 * nchunks + 12 bytes (fewer than 32 padding bits per chunk, 8 token-length bytes
TZH1 does not store, 3 bytes of section padding)."""
import numpy as np

from . import huff, huffr
from .huff import (CHUNK_RUNS, HEADER, MAX_LEN, NBINS, RUN, _pad4, body_bytes, canonical_codes, decode_table,  # noqa: F401
                   geometry, kraft_sum, pack_body, parse_trailer, reference_trailer)
from .huffr import NTOK

MAGIC = b"TZR2"
VERSION = 1
DISTS = (0, 1, 3)       # the match distances a file may name, in the order of the rows of tz_huffd_counts
TZR2 = huff.Format(MAGIC, "huffd", NTOK)


def is_huffd(head):
    """The first bytes of an entropy.dat: this coder's magic (TZH1 is huff's, TZR1 huffr's, a zstd frame starts 28 B5 2F FD)."""
    return bytes(head[:4]) == MAGIC


def check_dist(dist):
    if dist not in DISTS:
        raise ValueError("entropy.dat (huffd): match distance D = %r, the format knows 0 (no tokens), 1 and 3" % (dist,))
    return int(dist)


def tokenise(sym, A, dist, run=RUN):
    """huffr.tokenise at the match distance `dist`; dist = 0: every element is a literal followed by no raw bits."""
    if check_dist(dist):
        return huffr.tokenise(sym, A, run, dist)
    sym = np.asarray(sym, np.int64).reshape(-1)
    return sym.copy(), np.zeros_like(sym), np.zeros_like(sym)


def token_counts(payload, base, A):
    """The three histograms the choice is made from: uint64[3][A + 8], row i at the distance DISTS[i], literals then T_0..T_7
    (what tz_huffd_counts returns; row 0 holds no token)."""
    sym = np.asarray(payload, np.int64).reshape(-1) - int(base)
    out = np.zeros((len(DISTS), A + NTOK), np.uint64)
    for i, dist in enumerate(DISTS):
        tok, _, _ = tokenise(sym, A, dist)
        out[i] = np.bincount(tok[tok >= 0], minlength=A + NTOK)
    return out


def lengths_of(counts, dist):
    """len_D: the code lengths uint8[A + 8] of one row of the counts at the distance `dist`."""
    counts = np.asarray(counts, np.uint64)
    if check_dist(dist) == 0:
        return np.concatenate([huff.code_lengths(counts[:-NTOK]), np.zeros(NTOK, np.uint8)])
    return huffr.code_lengths(counts)


def cost_bits(counts, lengths):
    """cost_D in bits, exact (Python integers): the codes of the literals and tokens, and the raw bits behind the tokens."""
    c = [int(v) for v in np.asarray(counts).reshape(-1)]
    ln = [int(v) for v in np.asarray(lengths).reshape(-1)]
    return sum(a * b for a, b in zip(c, ln)) + sum(k * c[len(c) - NTOK + k] for k in range(NTOK))


def choose(counts3):
    """counts3 uint64[3][A + 8] (token_counts / tz_huffd_counts) -> (D, lengths uint8[A + 8], costs): the distance of the
    smallest cost, a tie to the smaller D; costs = (cost_0, cost_1, cost_3) in bits."""
    counts3 = np.asarray(counts3, np.uint64)
    if counts3.ndim != 2 or counts3.shape[0] != len(DISTS) or counts3.shape[1] <= NTOK:
        raise ValueError("huffd: counts of shape %r, (3, A + %d) wanted" % (counts3.shape, NTOK))
    lens = [lengths_of(counts3[i], d) for i, d in enumerate(DISTS)]
    costs = tuple(cost_bits(counts3[i], lens[i]) for i in range(len(DISTS)))
    best = min(range(len(DISTS)), key=lambda i: (costs[i], DISTS[i]))
    return DISTS[best], lens[best], costs


def check_lengths_of(dist):
    """The check of the A + 8 code lengths of a file that names the distance `dist`."""
    def check(lengths):
        ln = np.asarray(lengths)
        if dist == 0:
            if ln.ndim != 1 or ln.size <= NTOK:
                raise ValueError("entropy.dat (huffd): %d code lengths, A + %d with A >= 1 wanted" % (ln.size, NTOK))
            if ln[-NTOK:].any():
                raise ValueError("entropy.dat (huffd): match distance D = 0 with a code length for a repeat token")
            huff.check_lengths(ln[:-NTOK])
        else:
            huffr.check_lengths(ln)
    return check


def encode_body(payload, lengths, base, dist, run=RUN, chunk_runs=CHUNK_RUNS):
    """int16 payload -> (chunk_off uint32[nchunks], run_bits uint16[nruns], words uint32[stream_words]) at the distance `dist`;
    lengths holds A + 8 entries.  huffr.encode_body at that distance; dist = 0: huff.encode_body over the literal lengths."""
    if check_dist(dist):
        return huffr.encode_body(payload, lengths, base, run, chunk_runs, dist, "huffd")
    sym = np.asarray(payload, np.int64).reshape(-1) - int(base)
    ln = np.asarray(lengths, np.int64)
    A = ln.size - NTOK
    if sym.size < 1:
        raise ValueError("huffd: an empty payload cannot be coded")
    if A < 1 or sym.min() < 0 or sym.max() >= A:
        raise ValueError("huffd: the payload holds a value outside the %d literals" % A)
    if ln[A:].any():
        raise ValueError("huffd: match distance 0 with a code length for a repeat token")
    if (ln[sym] == 0).any():
        raise ValueError("huffd: the payload needs a literal or a token without a code")
    return huff.encode_body(payload, ln[:A], base, run, chunk_runs, "huffd")


def decode_body(chunk_off, run_bits, words, n, lengths, base, dist, run=RUN, chunk_runs=CHUNK_RUNS):
    """The inverse of encode_body for ANY bits: huffr.decode_body at the distance `dist`; dist = 0: huff.decode_body over the
    literal lengths."""
    if check_dist(dist):
        return huffr.decode_body(chunk_off, run_bits, words, n, lengths, base, run, chunk_runs, dist)
    return huff.decode_body(chunk_off, run_bits, words, n, np.asarray(lengths)[:-NTOK], base, run, chunk_runs)


def pack_front(trailer, lengths, base, n, nchunks, stream_words, dist, run=RUN, chunk_runs=CHUNK_RUNS):
    """Header | trailer | lengths: everything of the file in front of the index.  The header's last u32 holds D."""
    front = huff.pack_front_of(TZR2, trailer, lengths, base, n, nchunks, stream_words, run, chunk_runs)
    return front[:HEADER.size - 4] + np.uint32(check_dist(dist)).astype("<u4").tobytes() + front[HEADER.size:]


def encode_file(payload, table, shape5, warm_up, lengths=None, base=None, dist=None):
    """The whole entropy.dat of a payload, on the CPU (tests, and the specification of compress.run's output).  dist None:
    chosen by the format's rule, and `lengths` then is the chosen code's; a given dist without lengths takes len_dist."""
    payload = np.asarray(payload, np.int16).reshape(-1)
    if base is None:
        base = int(payload.min())
    if dist is None or lengths is None:
        counts3 = token_counts(payload, base, int(payload.max()) - base + 1)
        if dist is None:
            dist, chosen, _ = choose(counts3)
            lengths = chosen if lengths is None else lengths
        else:
            lengths = lengths_of(counts3[DISTS.index(check_dist(dist))], dist)
    co, rb, words = encode_body(payload, lengths, base, dist)
    return pack_front(reference_trailer(table, shape5, warm_up), lengths, base, payload.size, co.size, words.size, dist) + pack_body(co, rb, words)


class Parsed:
    """A validated TZR2 entropy.dat: header fields (dist: the match distance D), the reference trailer's content, and views of
    the sections."""
    coder = "huffd"


def parse(data, key_len=None):
    """Validate a TZR2 entropy.dat (bytes / uint8 array) -> Parsed: huff.parse's checks over A + 8 code lengths, D in {0, 1, 3},
    and no token length under D = 0."""
    buf = huff.as_bytes(data)
    dist = None
    if buf.size >= HEADER.size and bytes(buf[:4]) == MAGIC:
        dist = int(buf[HEADER.size - 4: HEADER.size].view("<u4")[0])
        check_dist(dist)
    p = huff.parse_of(TZR2, Parsed(), check_lengths_of(dist), data, key_len)   # (another magic or a short file: refused there)
    p.dist = dist
    return p


def decode_file(data, key_len=None):
    """-> (payload int16[n], Parsed) on the CPU."""
    p = parse(data, key_len)
    return decode_body(p.chunk_off, p.run_bits, p.words, p.n, p.lengths, p.base, p.dist), p
