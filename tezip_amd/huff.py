"""The Huffman-coded entropy.dat (`--coder huff`; NOT a reference format): container, validation and a plain numpy
encoder / decoder of the stream the GPU kernels write (k_huff_size / k_huff_scan / k_huff_enc / k_huff_dec in
csrc/tz_codec.hip).  The slow pair here is the specification the kernels are tested against (tests/test_huff.py,
tests/test_gpu_huff.py); the product never calls it on the hot path.  DESIGN.md section 9 holds the format as prose.

File layout, little-endian, every section padded with zero bytes to a multiple of 4:
  header   48 bytes: "TZH1" | u16 version = 1 | u16 L = 12 | u64 n | i32 base | u32 A | u32 R | u32 chunk_runs |
           u32 nchunks | u32 stream_words | u32 trailer_len | u32 0
  trailer  trailer_len int16: the reference trailer verbatim (table | T  or  -1, then 1, nt, H, W, 3, then warm_up)
  lengths  A bytes: code length of symbol s (payload value = s + base), 0 = absent, else 1..L; codes are canonical
  index    nchunks u32 word offsets of the chunks in the bit stream, then nruns = ceil(n / R) u16 run sizes in bits
  bits     stream_words u32
A run is R consecutive symbols coded back to back; a chunk is chunk_runs runs and starts on a word boundary.  A code of
length l and canonical value c (MSB first) is stored bit-reversed, first code bit in the lowest free bit of the stream.
"""
import collections
import struct

import numpy as np

MAGIC = b"TZH1"
VERSION = 1
MAX_LEN = 12            # L: a decode table entry is symbol (12 bits) | length (4 bits)
RUN = 256               # R: symbols per run (one lane of the kernels)
CHUNK_RUNS = 64         # runs per chunk (one wave)
NBINS = 2111            # TZ_NBINS: the largest alphabet
HEADER = struct.Struct("<4sHHQiIIIIIII")   # 48 bytes
# What tells the entropy.dat formats apart: the magic, the tag of the messages, and the repeat tokens behind the A literals.
Format = collections.namedtuple("Format", "magic tag ntok")
TZH1 = Format(MAGIC, "huff", 0)


def is_huff(head):
    """The first bytes of an entropy.dat: this project's magic (a zstd frame starts 28 B5 2F FD)."""
    return bytes(head[:4]) == MAGIC


def _pad4(nbytes):
    return (nbytes + 3) & ~3


def code_lengths(counts, max_len=MAX_LEN):
    """tz_huff_lengths (host only): optimal length-limited code lengths from counts; uint8[A], 0 = absent."""
    import ctypes as C
    from . import _lib
    counts = np.ascontiguousarray(counts, np.uint64)
    out = np.zeros(counts.size, np.uint8)
    rc = _lib.load().tz_huff_lengths(counts.ctypes.data, int(counts.size), int(max_len), out.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise ValueError("tz_huff_lengths refused the counts (status %d): no symbol present, more symbols than 2^max_len "
                         "codes, or an alphabet outside [1, %d]" % (rc, NBINS))
    return out


def kraft_sum(lengths, max_len=MAX_LEN):
    """Sum of 2^(max_len - l) over the present symbols: a prefix code has at most 2^max_len."""
    ln = np.asarray(lengths, np.int64)
    ln = ln[ln > 0]
    return int(np.sum(np.int64(1) << (max_len - ln)))


def check_lengths(lengths, max_len=MAX_LEN):
    ln = np.asarray(lengths)
    if ln.ndim != 1 or not 1 <= ln.size <= NBINS:
        raise ValueError("entropy.dat (huff): alphabet size A = %d outside [1, %d]" % (ln.size, NBINS))
    if ln.size and int(ln.max()) > max_len:
        raise ValueError("entropy.dat (huff): code lengths hold %d, the limit L is %d" % (int(ln.max()), max_len))
    if not (ln > 0).any():
        raise ValueError("entropy.dat (huff): code lengths name no symbol")
    if kraft_sum(ln, max_len) > (1 << max_len):
        raise ValueError("entropy.dat (huff): Kraft sum of the code lengths exceeds 1 (not a prefix code)")


def canonical_codes(lengths):
    """-> uint16[A] stored (bit-reversed) codes; canonical order: shorter first, then by symbol."""
    ln = np.asarray(lengths, np.int64)
    order = [s for s in np.lexsort((np.arange(ln.size), ln)) if ln[s] > 0]
    codes = np.zeros(ln.size, np.uint32)
    code, prev = 0, 0
    for s in order:
        code <<= int(ln[s]) - prev
        prev = int(ln[s])
        codes[s] = code
        code += 1
    rev = np.zeros(ln.size, np.uint32)
    for s in order:
        c, l, r = int(codes[s]), int(ln[s]), 0
        for b in range(l):
            r |= ((c >> b) & 1) << (l - 1 - b)
        rev[s] = r
    return rev.astype(np.uint16)


def encode_table(lengths):
    """uint16[A]: stored code | length << 12 (0 for an absent symbol) -- what k_huff_enc holds in LDS."""
    return (canonical_codes(lengths) | (np.asarray(lengths, np.uint16) << 12)).astype(np.uint16)


def decode_table(lengths, max_len=MAX_LEN):
    """uint16[2^L]: symbol | length << 12 for the next L bits of the stream.  Entries no code reaches (a one-symbol
    alphabet) hold the lowest present symbol with length 1, so that a decoder always advances."""
    ln = np.asarray(lengths, np.int64)
    rev = canonical_codes(ln)
    present = np.nonzero(ln > 0)[0]
    tab = np.full(1 << max_len, int(present[0]) | (1 << 12), np.uint16)
    for s in present:
        l = int(ln[s])
        tab[int(rev[s]) + (np.arange(1 << (max_len - l)) << l)] = int(s) | (l << 12)
    return tab


def geometry(n, run=RUN, chunk_runs=CHUNK_RUNS):
    nruns = (n + run - 1) // run
    return nruns, (nruns + chunk_runs - 1) // chunk_runs


def layout(tag, bits, at, run=RUN, chunk_runs=CHUNK_RUNS):
    """bits int64[n]: the bits coded AT every element -> (chunk_off uint32[nchunks], run_bits uint16[nruns], stream_words,
    pos): pos is the stream bit at which the code of each element of `at` starts."""
    n = bits.size
    nruns, nchunks = geometry(n, run, chunk_runs)
    cum = np.concatenate([[0], np.cumsum(bits)])                    # bits in front of element i, chunks unpadded
    run_start = np.arange(nruns, dtype=np.int64) * run
    run_bits = cum[np.minimum(run_start + run, n)] - cum[run_start]
    chunk_first = np.arange(nchunks, dtype=np.int64) * run * chunk_runs
    chunk_bits = cum[np.minimum(chunk_first + run * chunk_runs, n)] - cum[chunk_first]
    chunk_off = np.concatenate([[0], np.cumsum((chunk_bits + 31) >> 5)])
    total = int(chunk_off[-1])
    if total >= 1 << 32:
        raise ValueError("%s: the bit stream needs %d words, the format holds 2^32 - 1" % (tag, total))
    ci = at // (run * chunk_runs)
    pos = chunk_off[ci] * 32 + (cum[at] - cum[chunk_first][ci])
    return chunk_off[:-1].astype(np.uint32), run_bits.astype(np.uint16), total, pos


def scatter(code, pos, total):
    """Codes (fewer than 32 bits each) at ascending, non-overlapping stream bits `pos` -> uint32[total] words."""
    val = code.astype(np.uint64) << (pos & 31).astype(np.uint64)
    words = np.zeros(total + 1, np.uint64)
    w = pos >> 5                                                    # ascending: codes never overlap, so OR is a sum
    first = np.nonzero(np.concatenate([[True], w[1:] != w[:-1]]))[0]
    words[w[first]] += np.add.reduceat(val & np.uint64(0xFFFFFFFF), first)
    words[w[first] + 1] += np.add.reduceat(val >> np.uint64(32), first)
    return words[:total].astype(np.uint32)


def encode_body(payload, lengths, base, run=RUN, chunk_runs=CHUNK_RUNS, tag="huff"):
    """int16 payload -> (chunk_off uint32[nchunks], run_bits uint16[nruns], words uint32[stream_words]); `tag` names the coder
    in the messages."""
    sym = np.asarray(payload, np.int64).reshape(-1) - int(base)
    ln = np.asarray(lengths, np.int64)
    if sym.size < 1:
        raise ValueError("%s: an empty payload cannot be coded" % tag)
    if sym.min() < 0 or sym.max() >= ln.size or (ln[sym] == 0).any():
        raise ValueError("%s: the payload holds a value without a code" % tag)
    chunk_off, run_bits, total, pos = layout(tag, ln[sym], np.arange(sym.size, dtype=np.int64), run, chunk_runs)
    return chunk_off, run_bits, scatter(canonical_codes(ln)[sym], pos, total)


def run_positions(chunk_off, run_bits, words, n, run=RUN, chunk_runs=CHUNK_RUNS):
    """-> (pos int64[nruns]: the stream bit at which every run starts (chunk offset + the run sizes in front of it inside the
    chunk), w: the words as uint64 with two zero words behind them, last: the highest index a 64-bit window may start at)."""
    nruns, nchunks = geometry(n, run, chunk_runs)
    rb = np.zeros(nchunks * chunk_runs, np.int64)
    rb[:nruns] = np.asarray(run_bits, np.int64)
    rb = rb.reshape(nchunks, chunk_runs)
    pos = (np.asarray(chunk_off, np.int64)[:, None] * 32 + np.cumsum(rb, 1) - rb).reshape(-1)[:nruns]
    w = np.concatenate([np.asarray(words, np.uint64), np.zeros(2, np.uint64)])
    return pos, w, w.size - 2


def decode_body(chunk_off, run_bits, words, n, lengths, base, run=RUN, chunk_runs=CHUNK_RUNS):
    """The inverse of encode_body: every run is decoded from its own bit offset, all runs in lockstep as the lanes of
    k_huff_dec do.  Reads past the stream's end see zeros."""
    tab = decode_table(lengths)
    pos, w, last = run_positions(chunk_off, run_bits, words, n, run, chunk_runs)
    out = np.zeros(pos.size * run, np.int16)
    for k in range(run):
        i = np.minimum(pos >> 5, last)
        bits = ((w[i] | (w[i + 1] << np.uint64(32))) >> (pos & 31).astype(np.uint64)) & np.uint64(0xFFF)
        e = tab[bits.astype(np.int64)]
        out[k::run] = (e & 0xFFF).astype(np.int64) + int(base)
        pos = pos + (e >> 12)
    return out[:n]


def reference_trailer(table, shape5, warm_up):
    """compress.py:381-394 without the payload: table | T (or -1) | shape | warm_up as int16."""
    if table is not None:
        tail = np.concatenate([np.asarray(table, np.int64), [len(table)]])
    else:
        tail = np.array([-1], dtype=np.int64)
    return np.concatenate([tail, list(shape5), [warm_up]]).astype("<i2")


def parse_trailer(tr):
    """-> (table | None, shape5, warm_up) of the reference trailer held in the header."""
    tr = np.asarray(tr, np.int16)
    if tr.size < 7:
        raise ValueError("entropy.dat (huff): trailer holds %d values, at least 7 are needed" % tr.size)
    warm_up, shape, tlen = int(tr[-1]), tuple(int(v) for v in tr[-6:-1]), int(tr[-7])
    if tlen == -1:
        if tr.size != 7:
            raise ValueError("entropy.dat (huff): trailer without a table holds %d values, not 7" % tr.size)
        return None, shape, warm_up
    if tlen < 0 or tlen != tr.size - 7:
        raise ValueError("entropy.dat (huff): trailer table length %d does not fit its %d values" % (tlen, tr.size))
    return np.ascontiguousarray(tr[:tlen]), shape, warm_up


def pack_front_of(fmt, trailer, lengths, base, n, nchunks, stream_words, run=RUN, chunk_runs=CHUNK_RUNS):
    """Header | trailer | lengths of the format `fmt`: everything of the file in front of the index."""
    trailer = np.ascontiguousarray(trailer, "<i2")
    lengths = np.ascontiguousarray(lengths, np.uint8)
    head = HEADER.pack(fmt.magic, VERSION, MAX_LEN, int(n), int(base), int(lengths.size) - fmt.ntok, int(run), int(chunk_runs),
                       int(nchunks), int(stream_words), int(trailer.size), 0)
    tb, lb = trailer.tobytes(), lengths.tobytes()
    return head + tb + b"\0" * (_pad4(len(tb)) - len(tb)) + lb + b"\0" * (_pad4(len(lb)) - len(lb))


def pack_front(trailer, lengths, base, n, nchunks, stream_words, run=RUN, chunk_runs=CHUNK_RUNS):
    """Header | trailer | lengths: everything of the file in front of the index."""
    return pack_front_of(TZH1, trailer, lengths, base, n, nchunks, stream_words, run, chunk_runs)


def pack_body(chunk_off, run_bits, words):
    """Index | bits: the part of the file the device writes (tz_huff_encode's stream)."""
    rb = np.ascontiguousarray(run_bits, "<u2").tobytes()
    return (np.ascontiguousarray(chunk_off, "<u4").tobytes() + rb + b"\0" * (_pad4(len(rb)) - len(rb))
            + np.ascontiguousarray(words, "<u4").tobytes())


def body_bytes(n, stream_words, run=RUN, chunk_runs=CHUNK_RUNS):
    nruns, nchunks = geometry(n, run, chunk_runs)
    return nchunks * 4 + _pad4(nruns * 2) + stream_words * 4


def encode_file(payload, table, shape5, warm_up, lengths=None, base=None):
    """The whole entropy.dat of a payload, on the CPU (tests, and the specification of compress.run's output)."""
    payload = np.asarray(payload, np.int16).reshape(-1)
    if base is None:
        base = int(payload.min())
    if lengths is None:
        lengths = code_lengths(np.bincount(payload.astype(np.int64) - base))
    co, rb, words = encode_body(payload, lengths, base)
    return pack_front(reference_trailer(table, shape5, warm_up), lengths, base, payload.size, co.size, words.size) + pack_body(co, rb, words)


class Parsed:
    """A validated Huffman entropy.dat: header fields, the reference trailer's content, and views of the sections."""
    coder = "huff"


def check_index(what, chunk_off, run_bits, stream_words, run=RUN, chunk_runs=CHUNK_RUNS, ascending="ascending"):
    """The index of a stream whose file is `what` (the prefix of the messages): offsets ascending from 0 inside the stream,
    run sizes <= R * L, and the run sizes of a chunk fit the chunk."""
    co = chunk_off.astype(np.int64)
    if co[0] != 0 or (np.diff(co) < 0).any() or co[-1] > stream_words:
        raise ValueError("%s: chunk offset table is not %s inside the %d words of the bit stream" % (what, ascending, stream_words))
    rb = run_bits.astype(np.int64)
    if (rb > run * MAX_LEN).any():
        raise ValueError("%s: a run length of %d bits exceeds R * L = %d" % (what, int(rb.max()), run * MAX_LEN))
    per_chunk = np.add.reduceat(rb, np.arange(0, rb.size, chunk_runs))
    room = (np.concatenate([co[1:], [stream_words]]) - co) * 32
    if (per_chunk > room).any():
        c = int(np.nonzero(per_chunk > room)[0][0])
        raise ValueError("%s: the run lengths of chunk %d sum to %d bits, the chunk has %d" % (what, c, int(per_chunk[c]), int(room[c])))


def as_bytes(data):
    """bytes / any array -> a flat uint8 view"""
    return np.frombuffer(data, np.uint8) if not isinstance(data, np.ndarray) else data.view(np.uint8).reshape(-1)


def parse_of(fmt, p, check, data, key_len=None):
    """Validate an entropy.dat of the format `fmt` (bytes / uint8 array) into the empty Parsed `p`; `check` is the format's
    check_lengths.  Everything a pointer or a launch will be derived from is checked here, on the CPU; a failure is a
    ValueError that names the field."""
    what = "entropy.dat (%s)" % fmt.tag
    buf = as_bytes(data)
    if buf.size < HEADER.size:
        raise ValueError("%s: file size %d is shorter than the %d-byte header (truncated)" % (what, buf.size, HEADER.size))
    magic, version, max_len, n, base, A, run, chunk_runs, nchunks, stream_words, trailer_len, _ = HEADER.unpack(buf[:HEADER.size].tobytes())
    if magic != fmt.magic:
        raise ValueError("%s: magic %r is not %r" % (what, magic, fmt.magic))
    if version != VERSION:
        raise ValueError("%s: format version %d, this build reads version %d" % (what, version, VERSION))
    if max_len != MAX_LEN:
        raise ValueError("%s: code length limit L = %d, this build reads L = %d" % (what, max_len, MAX_LEN))
    if not 1 <= A <= NBINS:
        raise ValueError("%s: %s A = %d outside [1, TZ_NBINS = %d]" % (what, "literal alphabet" if fmt.ntok else "alphabet size", A, NBINS))
    if base < -32768 or base + A - 1 > 32767:
        raise ValueError("%s: symbol base %d with A = %d leaves int16" % (what, base, A))
    if run != RUN or chunk_runs != CHUNK_RUNS:
        raise ValueError("%s: run length R = %d / chunk of %d runs, this build reads R = %d / %d" % (what, run, chunk_runs, RUN, CHUNK_RUNS))
    if n < 1 or n >= 1 << 40:
        raise ValueError("%s: element count n = %d outside [1, 2^40)" % (what, n))
    nruns, want_chunks = geometry(n, run, chunk_runs)
    if nchunks != want_chunks:
        raise ValueError("%s: nchunks = %d, n = %d elements make %d chunks" % (what, nchunks, n, want_chunks))
    if not 7 <= trailer_len <= NBINS + 7:
        raise ValueError("%s: trailer length %d outside [7, %d]" % (what, trailer_len, NBINS + 7))
    o_tr = HEADER.size
    o_len = o_tr + _pad4(trailer_len * 2)
    o_idx = o_len + _pad4(A + fmt.ntok)
    o_runs = o_idx + nchunks * 4
    o_bits = o_runs + _pad4(nruns * 2)
    total = o_bits + stream_words * 4
    if buf.size != total:
        raise ValueError("%s: file size %d, the header describes %d bytes (truncated or corrupt file)" % (what, buf.size, total))
    p.n, p.base, p.A, p.run, p.chunk_runs, p.nchunks, p.nruns, p.stream_words = n, base, A, run, chunk_runs, nchunks, nruns, stream_words
    p.table, p.shape, p.warm_up = parse_trailer(buf[o_tr: o_tr + trailer_len * 2].view("<i2"))
    p.lengths = buf[o_len: o_len + A + fmt.ntok]                     # the literals, then the repeat tokens
    check(p.lengths)
    one, nt, H, W, C = p.shape
    # C: the channels the payload stores per pixel, 3 or -- the opt-in payload of a gray job, tezip_amd/graypayload.py -- 1
    # one: 1, 4 = the spatial delta of a three-channel payload at the channel stride, or 8 = the 2-D spatial delta TZ-SD2 of a payload
    # of three channels or one (tezip_amd/sdelta.py); byte planes (2, 5, 9) are never Huffman-coded
    # each plus 16 (17, 20, 24): the same layout of a closed-loop job (tezip_amd/closedloop.py), which has three channels
    # each plus 48 (49, 52, 56): a closed-loop job with per-tile selection (tezip_amd/predselect.py)
    if one in (17, 20, 24) and C == 3:
        one -= 16
    elif one in (49, 52, 56) and C == 3:
        one -= 48
    elif one in (81, 84, 88) and C == 3:   # each plus 80: a closed-loop job with motion-compensated tiles (tezip_amd/predmotion.py)
        one -= 80
    if one not in (1, 4, 8) or C not in (1, 3) or (one == 4 and C != 3) or nt < 1 or H < 1 or W < 1:
        raise ValueError("%s: unsupported stack shape %r (expected (1, nt, H, W, 3), (1, nt, H, W, 1) for a gray job, "
                         "(4, nt, H, W, 3) for a channel-stride payload or (8, nt, H, W, 3 or 1) for a plane payload; 16 more for a closed-loop job)" % (what, tuple(p.shape)))
    if n != nt * H * W * C:
        raise ValueError("%s: element count n = %d, the trailer's shape says %d" % (what, n, nt * H * W * C))
    if key_len is not None and key_len != nt * H * W * 3:
        raise ValueError("key_frame.dat holds %d bytes, entropy.dat's trailer implies %d" % (key_len, nt * H * W * 3))
    if not 0 <= p.warm_up < nt:
        raise ValueError("entropy.dat: warm-up count %d outside [0, %d)" % (p.warm_up, nt))
    if p.table is not None and (base != 0 or A > max(len(p.table), 1)):
        raise ValueError("%s: alphabet A = %d / base %d does not fit the %d ranks of the table" % (what, A, base, len(p.table)))
    p.chunk_off = buf[o_idx: o_runs].view("<u4")
    p.run_bits = buf[o_runs: o_runs + nruns * 2].view("<u2")
    p.words = buf[o_bits: total].view("<u4")
    p.body = buf[o_idx: total]                      # index | bits: what tz_huff_put / tz_huffr_put stages
    check_index(what, p.chunk_off, p.run_bits, stream_words, run, chunk_runs)
    return p


def parse(data, key_len=None):
    """Validate a Huffman-coded entropy.dat (bytes / uint8 array) -> Parsed."""
    return parse_of(TZH1, Parsed(), check_lengths, data, key_len)


def decode_file(data, key_len=None):
    """-> (payload int16[n], Parsed) on the CPU."""
    p = parse(data, key_len)
    return decode_body(p.chunk_off, p.run_bits, p.words, p.n, p.lengths, p.base), p
