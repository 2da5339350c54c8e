"""The Huffman-coded entropy.dat with repeat tokens (`--coder huffr`; NOT a reference format): container, validation and a
plain numpy tokeniser / encoder / decoder of the stream the GPU kernels write (k_huffr_count / k_huffr_size / k_huff_scan /
k_huffr_enc / k_huffr_dec in csrc/tz_codec.hip).  The slow code here is the specification the kernels are tested against
(tests/test_huffr.py, tests/test_gpu_huffr.py); the product never calls it on the hot path.  DESIGN.md section 9 holds the
format as prose.  It is TZH1 (tezip_amd/huff.py) with another magic, eight more symbols and a tokeniser in front.

File layout, little-endian, every section padded with zero bytes to a multiple of 4:
  header   48 bytes: "TZR1" | u16 version = 1 | u16 L = 12 | u64 n | i32 base | u32 A | u32 R | u32 chunk_runs |
           u32 nchunks | u32 stream_words | u32 trailer_len | u32 0
  trailer  trailer_len int16: the reference trailer verbatim (table | T  or  -1, then 1, nt, H, W, 3, then warm_up)
  lengths  A + 8 bytes: code length of literal s (payload value = s + base) for s < A, then of the repeat tokens T_0..T_7
           (symbols A..A + 7); 0 = absent, else 1..L; codes are canonical over all A + 8 symbols
  index    nchunks u32 word offsets of the chunks in the bit stream, then nruns = ceil(n / R) u16 run sizes in bits
  bits     stream_words u32
A run is R consecutive payload ELEMENTS owned by one lane; a chunk is chunk_runs runs and starts on a word boundary.
Element j of a run is a MATCH when j >= 3 and s[j] == s[j - 3] (history never crosses a run boundary).  Every maximal
stretch of m consecutive matches (cut at the run's end, so 1 <= m <= R - 3) is coded as the token T_k, k = floor(log2 m),
followed by k raw bits holding m - 2^k, least significant bit first; every other element is a literal.  Codes are stored
bit-reversed as in TZH1.  A decoder clamps a stretch to the elements left in its run and copies from an imaginary history
of three elements equal to `base` where a token stands at j < 3, so every bit pattern decodes to n elements.
"""
import numpy as np

from . import huff
from .huff import (CHUNK_RUNS, HEADER, MAX_LEN, NBINS, RUN, _pad4, body_bytes, canonical_codes, decode_table,  # noqa: F401
                   geometry, kraft_sum, pack_body, parse_trailer, reference_trailer)   # (index | bits are laid out as in TZH1)

MAGIC = b"TZR1"
VERSION = 1
NTOK = 8                # repeat tokens T_0..T_7: stretches of 2^k .. 2^(k+1) - 1 matches
DIST = 3                # TZR1's match distance: one pixel of the interleaved (H, W, 3) payload
TZR1 = huff.Format(MAGIC, "huffr", NTOK)


def is_huffr(head):
    """The first bytes of an entropy.dat: this coder's magic (TZH1 is huff's, a zstd frame starts 28 B5 2F FD)."""
    return bytes(head[:4]) == MAGIC


def code_lengths(counts, max_len=MAX_LEN):
    """tz_huffr_lengths (host only): tz_huff_lengths' package-merge over A + 8 <= TZ_NBINS + 8 counts; uint8, 0 = absent."""
    import ctypes as C
    from . import _lib
    counts = np.ascontiguousarray(counts, np.uint64)
    out = np.zeros(counts.size, np.uint8)
    rc = _lib.load().tz_huffr_lengths(counts.ctypes.data, int(counts.size), int(max_len), out.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise ValueError("tz_huffr_lengths refused the counts (status %d): no symbol present, more symbols than 2^max_len "
                         "codes, or more than %d + %d of them" % (rc, NBINS, NTOK))
    return out


def check_lengths(lengths, max_len=MAX_LEN):
    ln = np.asarray(lengths)
    if ln.ndim != 1 or not NTOK + 1 <= ln.size <= NBINS + NTOK:
        raise ValueError("entropy.dat (huffr): %d code lengths, A + %d must lie in [%d, %d]" % (ln.size, NTOK, NTOK + 1, NBINS + NTOK))
    if int(ln.max()) > max_len:
        raise ValueError("entropy.dat (huffr): code lengths hold %d, the limit L is %d" % (int(ln.max()), max_len))
    if not (ln[:-NTOK] > 0).any():
        raise ValueError("entropy.dat (huffr): code lengths name no literal")
    if kraft_sum(ln, max_len) > (1 << max_len):
        raise ValueError("entropy.dat (huffr): Kraft sum of the code lengths exceeds 1 (not a prefix code)")


def tokenise_run(values):
    """The tokeniser as a loop over ONE run (<= R values): [("L", value) | ("T", k, m - 2^k)], the plain statement."""
    out, j, n = [], 0, len(values)
    while j < n:
        if j >= DIST and values[j] == values[j - DIST]:
            m = 1
            while j + m < n and values[j + m] == values[j + m - DIST]:
                m += 1
            k = m.bit_length() - 1
            out.append(("T", k, m - (1 << k)))
            j += m
        else:
            out.append(("L", int(values[j])))
            j += 1
    return out


def tokenise(sym, A, run=RUN, dist=DIST):
    """sym int64[n] (value - base) -> (tok, extra, nextra), int64[n] each: tok[i] is the symbol coded AT element i -- the
    literal sym[i], A + k at the first element of a stretch, -1 inside a stretch -- followed by nextra[i] raw bits `extra[i]`.
    dist >= 1: the match distance (TZR1: 3; a TZR2 file, tezip_amd/huffd.py, names 1 or 3)."""
    sym = np.asarray(sym, np.int64).reshape(-1)
    n = sym.size
    match = np.zeros(n, bool)
    match[dist:] = sym[dist:] == sym[:-dist]
    match &= (np.arange(n) % run) >= dist                            # (so a stretch never spans a run boundary)
    start = np.nonzero(match & ~np.concatenate([[False], match[:-1]]))[0]
    end = np.nonzero(match & ~np.concatenate([match[1:], [False]]))[0]
    m = end - start + 1
    k = np.zeros(m.size, np.int64)
    for t in range(1, NTOK):
        k += m >= (1 << t)
    tok = np.where(match, -1, sym)
    extra, nextra = np.zeros(n, np.int64), np.zeros(n, np.int64)
    tok[start], extra[start], nextra[start] = A + k, m - (np.int64(1) << k), k
    return tok, extra, nextra


def token_counts(payload, base, A):
    """The histogram the code lengths are built from: uint64[A + 8], literals then T_0..T_7 (what tz_huffr_counts returns)."""
    tok, _, _ = tokenise(np.asarray(payload, np.int64).reshape(-1) - int(base), A)
    return np.bincount(tok[tok >= 0], minlength=A + NTOK).astype(np.uint64)


def encode_body(payload, lengths, base, run=RUN, chunk_runs=CHUNK_RUNS, dist=DIST, tag="huffr"):
    """int16 payload -> (chunk_off uint32[nchunks], run_bits uint16[nruns], words uint32[stream_words]) at the match distance
    `dist` >= 1; `tag` names the coder in the messages."""
    sym = np.asarray(payload, np.int64).reshape(-1) - int(base)
    n = sym.size
    ln = np.asarray(lengths, np.int64)
    A = ln.size - NTOK
    if n < 1:
        raise ValueError("%s: an empty payload cannot be coded" % tag)
    if A < 1 or sym.min() < 0 or sym.max() >= A:
        raise ValueError("%s: the payload holds a value outside the %d literals" % (tag, A))
    tok, extra, nextra = tokenise(sym, A, run, dist)
    at = np.nonzero(tok >= 0)[0]                                     # the elements something is coded at
    tl = ln[tok[at]]
    if (tl == 0).any():
        raise ValueError("%s: the payload needs a literal or a token without a code" % tag)
    bits = np.zeros(n, np.int64)
    bits[at] = tl + nextra[at]
    chunk_off, run_bits, total, pos = huff.layout(tag, bits, at, run, chunk_runs)
    code = canonical_codes(ln).astype(np.int64)[tok[at]] | (extra[at] << tl)          # <= 12 + 7 bits
    return chunk_off, run_bits, huff.scatter(code, pos, total)


def decode_body(chunk_off, run_bits, words, n, lengths, base, run=RUN, chunk_runs=CHUNK_RUNS, dist=DIST):
    """The inverse of encode_body for ANY bits: every run is decoded from its own bit offset, all runs in lockstep as the
    lanes of k_huffr_dec do, one element per step -- a lane inside a stretch copies the element `dist` back, any other lane
    reads a symbol.  Reads past the stream's end see zeros; a stretch ends with its run."""
    ln = np.asarray(lengths, np.int64)
    A = ln.size - NTOK
    tab = decode_table(ln)
    pos, w, last = huff.run_positions(chunk_off, run_bits, words, n, run, chunk_runs)
    nruns = pos.size
    out = np.zeros(nruns * run, np.int16)
    hist = [np.full(nruns, int(base), np.int64)] * dist              # the imaginary history in front of a run, oldest first
    m = np.zeros(nruns, np.int64)                                    # elements the current stretch still has to copy
    for j in range(run):
        read = m == 0
        i = np.minimum(pos >> 5, last)
        window = ((w[i] | (w[i + 1] << np.uint64(32))) >> (pos & 31).astype(np.uint64)).astype(np.int64) & ((1 << 31) - 1)
        e = tab[window & 0xFFF].astype(np.int64)
        l, s = e >> 12, e & 0xFFF
        token = read & (s >= A)
        k = np.where(token, np.minimum(s - A, NTOK - 1), 0)
        m = np.where(token, (np.int64(1) << k) + ((window >> l) & ((np.int64(1) << k) - 1)), m)
        pos = pos + np.where(read, l + k, 0)
        val = np.where(read & ~token, s + int(base), hist[0])
        m = np.maximum(m - 1, 0)
        out[j::run] = val
        hist = hist[1:] + [val]
    return out[:n]


def pack_front(trailer, lengths, base, n, nchunks, stream_words, run=RUN, chunk_runs=CHUNK_RUNS):
    """Header | trailer | lengths: everything of the file in front of the index."""
    return huff.pack_front_of(TZR1, trailer, lengths, base, n, nchunks, stream_words, run, chunk_runs)


def encode_file(payload, table, shape5, warm_up, lengths=None, base=None):
    """The whole entropy.dat of a payload, on the CPU (tests, and the specification of compress.run's output)."""
    payload = np.asarray(payload, np.int16).reshape(-1)
    if base is None:
        base = int(payload.min())
    if lengths is None:
        lengths = code_lengths(token_counts(payload, base, int(payload.max()) - base + 1))
    co, rb, words = encode_body(payload, lengths, base)
    return pack_front(reference_trailer(table, shape5, warm_up), lengths, base, payload.size, co.size, words.size) + pack_body(co, rb, words)


class Parsed:
    """A validated TZR1 entropy.dat: header fields, the reference trailer's content, and views of the sections."""
    coder = "huffr"


def parse(data, key_len=None):
    """Validate a TZR1 entropy.dat (bytes / uint8 array) -> Parsed: huff.parse's checks over A + 8 code lengths."""
    return huff.parse_of(TZR1, Parsed(), check_lengths, data, key_len)


def decode_file(data, key_len=None):
    """-> (payload int16[n], Parsed) on the CPU."""
    p = parse(data, key_len)
    return decode_body(p.chunk_off, p.run_bits, p.words, p.n, p.lengths, p.base), p
