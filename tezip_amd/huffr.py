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

from .huff import (CHUNK_RUNS, HEADER, MAX_LEN, NBINS, RUN, _pad4, body_bytes, canonical_codes, decode_table,  # noqa: F401
                   geometry, kraft_sum, pack_body, parse_trailer, reference_trailer)   # (index | bits are laid out as in TZH1)

MAGIC = b"TZR1"
VERSION = 1
NTOK = 8                # repeat tokens T_0..T_7: stretches of 2^k .. 2^(k+1) - 1 matches
DIST = 3                # the match distance: one pixel of the interleaved (H, W, 3) payload


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


def tokenise(sym, A, run=RUN):
    """sym int64[n] (value - base) -> (tok, extra, nextra), int64[n] each: tok[i] is the symbol coded AT element i -- the
    literal sym[i], A + k at the first element of a stretch, -1 inside a stretch -- followed by nextra[i] raw bits `extra[i]`."""
    sym = np.asarray(sym, np.int64).reshape(-1)
    n = sym.size
    match = np.zeros(n, bool)
    match[DIST:] = sym[DIST:] == sym[:-DIST]
    match &= (np.arange(n) % run) >= DIST                            # (so a stretch never spans a run boundary)
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


def encode_body(payload, lengths, base, run=RUN, chunk_runs=CHUNK_RUNS):
    """int16 payload -> (chunk_off uint32[nchunks], run_bits uint16[nruns], words uint32[stream_words])."""
    sym = np.asarray(payload, np.int64).reshape(-1) - int(base)
    n = sym.size
    ln = np.asarray(lengths, np.int64)
    A = ln.size - NTOK
    if n < 1:
        raise ValueError("huffr: an empty payload cannot be coded")
    if A < 1 or sym.min() < 0 or sym.max() >= A:
        raise ValueError("huffr: the payload holds a value outside the %d literals" % A)
    tok, extra, nextra = tokenise(sym, A, run)
    at = np.nonzero(tok >= 0)[0]                                     # the elements something is coded at
    tl = ln[tok[at]]
    if (tl == 0).any():
        raise ValueError("huffr: the payload needs a literal or a token without a code")
    bits = np.zeros(n, np.int64)
    bits[at] = tl + nextra[at]
    cum = np.concatenate([[0], np.cumsum(bits)])                     # bits in front of element i, chunks unpadded
    nruns, nchunks = geometry(n, run, chunk_runs)
    run_start = np.arange(nruns, dtype=np.int64) * run
    run_bits = cum[np.minimum(run_start + run, n)] - cum[run_start]
    chunk_first = np.arange(nchunks, dtype=np.int64) * run * chunk_runs
    chunk_bits = cum[np.minimum(chunk_first + run * chunk_runs, n)] - cum[chunk_first]
    chunk_off = np.concatenate([[0], np.cumsum((chunk_bits + 31) >> 5)])
    total = int(chunk_off[-1])
    if total >= 1 << 32:
        raise ValueError("huffr: the bit stream needs %d words, the format holds 2^32 - 1" % total)
    ci = at // (run * chunk_runs)
    pos = chunk_off[ci] * 32 + (cum[at] - cum[chunk_first][ci])      # stream bit of every token's first code bit
    code = canonical_codes(ln).astype(np.int64)[tok[at]] | (extra[at] << tl)          # <= 12 + 7 bits
    val = code.astype(np.uint64) << (pos & 31).astype(np.uint64)
    words = np.zeros(total + 1, np.uint64)
    w = pos >> 5                                                     # ascending: codes never overlap, so OR is a sum
    first = np.nonzero(np.concatenate([[True], w[1:] != w[:-1]]))[0]
    words[w[first]] += np.add.reduceat(val & np.uint64(0xFFFFFFFF), first)
    words[w[first] + 1] += np.add.reduceat(val >> np.uint64(32), first)
    return chunk_off[:-1].astype(np.uint32), run_bits.astype(np.uint16), words[:total].astype(np.uint32)


def decode_body(chunk_off, run_bits, words, n, lengths, base, run=RUN, chunk_runs=CHUNK_RUNS):
    """The inverse of encode_body for ANY bits: every run is decoded from its own bit offset, all runs in lockstep as the
    lanes of k_huffr_dec do, one element per step -- a lane inside a stretch copies the element three back, any other lane
    reads a symbol.  Reads past the stream's end see zeros; a stretch ends with its run."""
    nruns, nchunks = geometry(n, run, chunk_runs)
    ln = np.asarray(lengths, np.int64)
    A = ln.size - NTOK
    tab = decode_table(ln)
    rb = np.zeros(nchunks * chunk_runs, np.int64)
    rb[:nruns] = np.asarray(run_bits, np.int64)
    rb = rb.reshape(nchunks, chunk_runs)
    pos = (np.asarray(chunk_off, np.int64)[:, None] * 32 + np.cumsum(rb, 1) - rb).reshape(-1)[:nruns]
    w = np.concatenate([np.asarray(words, np.uint64), np.zeros(2, np.uint64)])
    last = w.size - 2
    out = np.zeros(nruns * run, np.int16)
    h1 = h2 = h3 = np.full(nruns, int(base), np.int64)               # the imaginary history in front of a run
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
        val = np.where(read & ~token, s + int(base), h3)
        m = np.maximum(m - 1, 0)
        out[j::run] = val
        h3, h2, h1 = h2, h1, val
    return out[:n]


def pack_front(trailer, lengths, base, n, nchunks, stream_words, run=RUN, chunk_runs=CHUNK_RUNS):
    """Header | trailer | lengths: everything of the file in front of the index."""
    trailer = np.ascontiguousarray(trailer, "<i2")
    lengths = np.ascontiguousarray(lengths, np.uint8)
    head = HEADER.pack(MAGIC, VERSION, MAX_LEN, int(n), int(base), int(lengths.size) - NTOK, int(run), int(chunk_runs),
                       int(nchunks), int(stream_words), int(trailer.size), 0)
    tb, lb = trailer.tobytes(), lengths.tobytes()
    return head + tb + b"\0" * (_pad4(len(tb)) - len(tb)) + lb + b"\0" * (_pad4(len(lb)) - len(lb))


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
    """Validate a TZR1 entropy.dat (bytes / uint8 array) -> Parsed.  Everything a pointer or a launch will be derived from
    is checked here, on the CPU; a failure is a ValueError that names the field."""
    buf = np.frombuffer(data, np.uint8) if not isinstance(data, np.ndarray) else data.view(np.uint8).reshape(-1)
    if buf.size < HEADER.size:
        raise ValueError("entropy.dat (huffr): file size %d is shorter than the %d-byte header (truncated)" % (buf.size, HEADER.size))
    magic, version, max_len, n, base, A, run, chunk_runs, nchunks, stream_words, trailer_len, _ = HEADER.unpack(buf[:HEADER.size].tobytes())
    if magic != MAGIC:
        raise ValueError("entropy.dat (huffr): magic %r is not %r" % (magic, MAGIC))
    if version != VERSION:
        raise ValueError("entropy.dat (huffr): format version %d, this build reads version %d" % (version, VERSION))
    if max_len != MAX_LEN:
        raise ValueError("entropy.dat (huffr): code length limit L = %d, this build reads L = %d" % (max_len, MAX_LEN))
    if not 1 <= A <= NBINS:
        raise ValueError("entropy.dat (huffr): literal alphabet A = %d outside [1, TZ_NBINS = %d]" % (A, NBINS))
    if base < -32768 or base + A - 1 > 32767:
        raise ValueError("entropy.dat (huffr): symbol base %d with A = %d leaves int16" % (base, A))
    if run != RUN or chunk_runs != CHUNK_RUNS:
        raise ValueError("entropy.dat (huffr): run length R = %d / chunk of %d runs, this build reads R = %d / %d"
                         % (run, chunk_runs, RUN, CHUNK_RUNS))
    if n < 1 or n >= 1 << 40:
        raise ValueError("entropy.dat (huffr): element count n = %d outside [1, 2^40)" % n)
    nruns, want_chunks = geometry(n, run, chunk_runs)
    if nchunks != want_chunks:
        raise ValueError("entropy.dat (huffr): nchunks = %d, n = %d elements make %d chunks" % (nchunks, n, want_chunks))
    if not 7 <= trailer_len <= NBINS + 7:
        raise ValueError("entropy.dat (huffr): trailer length %d outside [7, %d]" % (trailer_len, NBINS + 7))
    o_tr = HEADER.size
    o_len = o_tr + _pad4(trailer_len * 2)
    o_idx = o_len + _pad4(A + NTOK)
    o_runs = o_idx + nchunks * 4
    o_bits = o_runs + _pad4(nruns * 2)
    total = o_bits + stream_words * 4
    if buf.size != total:
        raise ValueError("entropy.dat (huffr): file size %d, the header describes %d bytes (truncated or corrupt file)" % (buf.size, total))
    p = Parsed()
    p.n, p.base, p.A, p.run, p.chunk_runs, p.nchunks, p.nruns, p.stream_words = n, base, A, run, chunk_runs, nchunks, nruns, stream_words
    p.table, p.shape, p.warm_up = parse_trailer(buf[o_tr: o_tr + trailer_len * 2].view("<i2"))
    p.lengths = buf[o_len: o_len + A + NTOK]                         # literals, then T_0..T_7
    check_lengths(p.lengths)
    one, nt, H, W, C = p.shape
    if one != 1 or C != 3 or nt < 1 or H < 1 or W < 1:
        raise ValueError("entropy.dat (huffr): unsupported stack shape %r (expected (1, nt, H, W, 3))" % (tuple(p.shape),))
    if n != nt * H * W * C:
        raise ValueError("entropy.dat (huffr): element count n = %d, the trailer's shape says %d" % (n, nt * H * W * C))
    if key_len is not None and key_len != n:
        raise ValueError("key_frame.dat holds %d bytes, entropy.dat's trailer implies %d" % (key_len, n))
    if not 0 <= p.warm_up < nt:
        raise ValueError("entropy.dat: warm-up count %d outside [0, %d)" % (p.warm_up, nt))
    if p.table is not None and (base != 0 or A > max(len(p.table), 1)):
        raise ValueError("entropy.dat (huffr): alphabet A = %d / base %d does not fit the %d ranks of the table" % (A, base, len(p.table)))
    p.chunk_off = buf[o_idx: o_runs].view("<u4")
    p.run_bits = buf[o_runs: o_runs + nruns * 2].view("<u2")
    p.words = buf[o_bits: total].view("<u4")
    p.body = buf[o_idx: total]                      # index | bits: what tz_huffr_put stages
    co = p.chunk_off.astype(np.int64)
    if co[0] != 0 or (np.diff(co) < 0).any() or co[-1] > stream_words:
        raise ValueError("entropy.dat (huffr): chunk offset table is not ascending inside the %d words of the bit stream" % stream_words)
    rb = p.run_bits.astype(np.int64)
    if (rb > run * MAX_LEN).any():
        raise ValueError("entropy.dat (huffr): a run length of %d bits exceeds R * L = %d" % (int(rb.max()), run * MAX_LEN))
    per_chunk = np.add.reduceat(rb, np.arange(0, nruns, chunk_runs))
    room = (np.concatenate([co[1:], [stream_words]]) - co) * 32
    if (per_chunk > room).any():
        c = int(np.nonzero(per_chunk > room)[0][0])
        raise ValueError("entropy.dat (huffr): the run lengths of chunk %d sum to %d bits, the chunk has %d" % (c, int(per_chunk[c]), int(room[c])))
    return p


def decode_file(data, key_len=None):
    """-> (payload int16[n], Parsed) on the CPU."""
    p = parse(data, key_len)
    return decode_body(p.chunk_off, p.run_bits, p.words, p.n, p.lengths, p.base), p
