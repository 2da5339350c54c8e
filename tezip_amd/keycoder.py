"""The GPU-coded key_frame.dat (`--key-coder huff`; NOT a reference format): container, validation and a plain numpy
statement of what the kernels k_key_hist / k_key_resid / k_key_unresid_row / k_key_unresid_col (csrc/tz_codec.hip) and the Huffman kernels behind
them write and read.  The slow functions here are the specification the kernels are tested against
(tests/test_keycoder.py, tests/test_gpu_keycoder.py); the product calls only the container, `choose_predictors` and `parse`.
DESIGN.md section 9 holds the format as prose.

A key frame is coded as the residuals of one of four predictors over its own samples, all key frames of a file under ONE
order-0 canonical Huffman code (the TZH1 body of tezip_amd/huff.py with A = 256, base = 0).  The non-key frames of the
reference's zero-except-keys stack are not stored at all.

File layout, little-endian, every section padded with zero bytes to a multiple of 4:
  header   48 bytes: "TZK1" | u16 version = 1 | u16 L = 12 | u32 nt | u32 H | u32 W | u32 C = 3 | u32 nkeys | u32 R = 256 |
           u32 chunk_runs = 64 | u32 nchunks | u32 stream_words | u32 0
  keys     nkeys u32 frame indices, strictly ascending, each < nt
  preds    nkeys bytes: predictor id of each key frame, 0..3
  lengths  256 bytes: code length of residual value s, 0 = absent, else 1..L; canonical codes as in TZH1
  index    nchunks u32 word offsets, then ceil(n / R) u16 run sizes in bits, n = nkeys * H * W * 3   (TZH1 section 4)
  bits     stream_words u32                                                                          (TZH1 section 5)
The symbols are the residuals of the key frames in index order, each frame in (H, W, 3) memory order.

Residual of the sample x at (y, col, ch), neighbours in the same channel: a = left (0 at col 0), b = up (0 at y 0),
c = up-left (0 when either is 0); p = 0 | a | b | a + b - c for predictor 0 | 1 | 2 | 3; r = (x - p) mod 256.
"""
import struct

import numpy as np

from . import huff

MAGIC = b"TZK1"
VERSION = 1
NPRED = 4
HEADER = struct.Struct("<4sHH10I")   # 48 bytes
MAX_FRAMES = 32767                   # tz_frames_begin's limits (the reference's int16 trailer)
MAX_SIDE = 32767


def is_keycoded(head):
    """The first bytes of a key_frame.dat: this project's magic (a zstd frame starts 28 B5 2F FD)."""
    return bytes(head[:4]) == MAGIC


def _pad4(nbytes):
    return (nbytes + 3) & ~3


def residual(frame, pred):
    """uint8 (H, W, 3) frame -> int16[H * W * 3] residuals 0..255 under predictor `pred`."""
    x = np.asarray(frame, np.uint8)
    if x.ndim != 3 or x.shape[2] != 3:
        raise ValueError("a key frame must be a (H, W, 3) uint8 array, got shape %r" % (tuple(x.shape),))
    if not 0 <= int(pred) < NPRED:
        raise ValueError("key_frame.dat (huff): predictor id %d outside [0, 3]" % int(pred))
    x = x.astype(np.int64)
    a, b, c = np.zeros_like(x), np.zeros_like(x), np.zeros_like(x)
    a[:, 1:] = x[:, :-1]
    b[1:] = x[:-1]
    c[1:, 1:] = x[:-1, :-1]
    p = (0, a, b, a + b - c)[int(pred)]
    return ((x - p) & 255).astype(np.int16).reshape(-1)


def unresidual(sym, pred, H, W):
    """The inverse of residual: prefix sums mod 256 along the rows (1), the columns (2) or both (3) -> uint8 (H, W, 3).
    Only the low byte of a symbol counts, as in k_key_unresid_row."""
    if not 0 <= int(pred) < NPRED:
        raise ValueError("key_frame.dat (huff): predictor id %d outside [0, 3]" % int(pred))
    r = (np.asarray(sym, np.int64).reshape(H, W, 3)) & 255
    if int(pred) & 1:
        r = np.cumsum(r, axis=1) & 255
    if int(pred) & 2:
        r = np.cumsum(r, axis=0) & 255
    return r.astype(np.uint8)


def predictor_counts(key_frames):
    """uint8 (k, H, W, 3) -> int64[k][4][256]: how often each residual value occurs in each key frame under each
    predictor (what tz_keys_counts returns)."""
    kf = np.asarray(key_frames, np.uint8)
    out = np.zeros((kf.shape[0], NPRED, 256), np.int64)
    for k in range(kf.shape[0]):
        for p in range(NPRED):
            out[k, p] = np.bincount(residual(kf[k], p), minlength=256)
    return out


def choose_predictors(counts):
    """counts[k][p][256] (exact integers) -> uint8[k]: per key frame the predictor with the lowest order-0 cost
    sum over c > 0 of c * log2(N / c), in float64; ties go to the lowest id.  The product and the slow encoder both call
    this on the same integers, which is what makes their files identical."""
    c = np.asarray(counts).astype(np.float64)
    if c.ndim != 3 or c.shape[1:] != (NPRED, 256):
        raise ValueError("predictor counts must be [nkeys][4][256], got shape %r" % (tuple(c.shape),))
    n = c.sum(axis=2, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        cost = np.where(c > 0, c * np.log2(n / c), 0.0).sum(axis=2)
    return np.argmin(cost, axis=1).astype(np.uint8)   # (argmin returns the first of equal minima)


def chosen_counts(counts, pred):
    """The counts the one code table is made from: those of the chosen predictor of every key frame, summed."""
    c = np.asarray(counts)
    return c[np.arange(c.shape[0]), np.asarray(pred, np.int64)].astype(np.uint64).sum(axis=0)


def pack_front(nt, H, W, idx, pred, lengths, nchunks, stream_words):
    """Header | key indices | predictor ids | lengths: everything of the file in front of the index."""
    idx = np.ascontiguousarray(idx, "<u4")
    pred = np.ascontiguousarray(pred, np.uint8)
    lengths = np.ascontiguousarray(lengths, np.uint8)
    if idx.size < 1 or pred.size != idx.size or lengths.size != 256:
        raise ValueError("key_frame.dat (huff): %d key indices, %d predictor ids, %d code lengths" % (idx.size, pred.size, lengths.size))
    head = HEADER.pack(MAGIC, VERSION, huff.MAX_LEN, int(nt), int(H), int(W), 3, int(idx.size), huff.RUN, huff.CHUNK_RUNS,
                       int(nchunks), int(stream_words), 0)
    pb = pred.tobytes()
    return head + idx.tobytes() + pb + b"\0" * (_pad4(len(pb)) - len(pb)) + lengths.tobytes()


def symbols(key_frames, pred):
    """The int16 symbols of the file's body: the residuals of the key frames, one frame after the other."""
    return np.concatenate([residual(f, p) for f, p in zip(key_frames, pred)])


def key_frames_of(what, stack_or_keyframes, idx, nt):
    """encode_file's arguments -> (uint8 (k, H, W, 3) key frames, int64[k] indices); `what` is the prefix of the messages."""
    x = np.asarray(stack_or_keyframes, np.uint8)
    idx = np.asarray(idx, np.int64).reshape(-1)
    if x.ndim != 4 or x.shape[3] != 3:
        raise ValueError("key frames must be a (k, H, W, 3) uint8 stack, got shape %r" % (tuple(x.shape),))
    if idx.size < 1 or (np.diff(idx) <= 0).any() or idx[0] < 0 or idx[-1] >= nt:
        raise ValueError("%s: key indices must be strictly ascending inside [0, %d)" % (what, nt))
    if x.shape[0] == nt:
        return x[idx], idx
    if x.shape[0] == idx.size:
        return x, idx
    raise ValueError("%d frames given for %d key indices of a %d-frame sequence" % (x.shape[0], idx.size, nt))


def encode_file(stack_or_keyframes, idx, nt):
    """The whole key_frame.dat on the CPU (tests, and the specification of compress.run's output).  The first argument is
    the (nt, H, W, 3) stack, of which the frames `idx` are coded, or the (len(idx), H, W, 3) key frames themselves."""
    kf, idx = key_frames_of("key_frame.dat (huff)", stack_or_keyframes, idx, nt)
    H, W = kf.shape[1:3]
    counts = predictor_counts(kf)
    pred = choose_predictors(counts)
    lengths = huff.code_lengths(chosen_counts(counts, pred))
    co, rb, words = huff.encode_body(symbols(kf, pred), lengths, 0)
    return pack_front(nt, H, W, idx, pred, lengths, co.size, words.size) + huff.pack_body(co, rb, words)


class Parsed:
    """A validated TZK1 key_frame.dat: the stack's shape, the key indices, their predictors, and views of the sections."""


def parse_header(what, magic_want, data):
    """The header of a TZK1 / TZK2 file (`what` is the prefix of the messages) -> (buf, nt, H, W, nkeys, run, chunk_runs,
    nchunks, stream_words, o_pred, o_len, o_co): the fields and where the pred bytes, the lengths and the index start."""
    buf = huff.as_bytes(data)
    if buf.size < HEADER.size:
        raise ValueError("%s: file size %d is shorter than the %d-byte header (truncated)" % (what, buf.size, HEADER.size))
    magic, version, max_len, nt, H, W, C, nkeys, run, chunk_runs, nchunks, stream_words, _ = HEADER.unpack(buf[:HEADER.size].tobytes())
    if magic != magic_want:
        raise ValueError("%s: magic %r is not %r" % (what, magic, magic_want))
    if version != VERSION:
        raise ValueError("%s: format version %d, this build reads version %d" % (what, version, VERSION))
    if max_len != huff.MAX_LEN:
        raise ValueError("%s: code length limit L = %d, this build reads L = %d" % (what, max_len, huff.MAX_LEN))
    if run != huff.RUN or chunk_runs != huff.CHUNK_RUNS:
        raise ValueError("%s: run length R = %d / chunk of %d runs, this build reads R = %d / %d"
                         % (what, run, chunk_runs, huff.RUN, huff.CHUNK_RUNS))
    if C != 3:
        raise ValueError("%s: channel count C = %d, this build reads C = 3" % (what, C))
    if not (1 <= nt <= MAX_FRAMES and 1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
        raise ValueError("%s: stack shape nt = %d, H = %d, W = %d outside [1, %d] x [1, %d]^2" % (what, nt, H, W, MAX_FRAMES, MAX_SIDE))
    if not 1 <= nkeys <= nt:
        raise ValueError("%s: nkeys = %d outside [1, nt = %d]" % (what, nkeys, nt))
    o_pred = HEADER.size + nkeys * 4
    o_len = o_pred + _pad4(nkeys)
    return buf, nt, H, W, nkeys, run, chunk_runs, nchunks, stream_words, o_pred, o_len, o_len + 256


def parse_keys(what, p, buf, nt, nkeys, o_pred):
    """p.idx and p.pred: the key indices, strictly ascending inside [0, nt), and the bytes behind them (not yet checked)."""
    p.idx = buf[HEADER.size: o_pred].view("<u4")
    ix = p.idx.astype(np.int64)
    if (np.diff(ix) <= 0).any() or ix[-1] >= nt:
        raise ValueError("%s: key indices are not strictly ascending inside [0, nt = %d)" % (what, nt))
    p.pred = buf[o_pred: o_pred + nkeys]


def parse_stream(what, p, buf, o_co, n, run, chunk_runs, nchunks, stream_words, frames):
    """Everything that depends on the symbol count n: the chunk count (`frames` words the message), the file's size, the code
    lengths in front of o_co, and the index | bits from there on."""
    nruns, want_chunks = huff.geometry(n, run, chunk_runs)
    if nchunks != want_chunks:
        raise ValueError("%s: nchunks = %d, %s make %d chunks" % (what, nchunks, frames, want_chunks))
    o_runs = o_co + nchunks * 4
    o_bits = o_runs + _pad4(nruns * 2)
    total = o_bits + stream_words * 4
    if buf.size != total:
        raise ValueError("%s: file size %d, the header describes %d bytes (truncated or corrupt file)" % (what, buf.size, total))
    p.n, p.run, p.nchunks, p.nruns, p.stream_words = n, run, nchunks, nruns, stream_words
    p.lengths = buf[o_co - 256: o_co]
    p.chunk_off = buf[o_co: o_runs].view("<u4")
    p.run_bits = buf[o_runs: o_runs + nruns * 2].view("<u2")
    p.words = buf[o_bits: total].view("<u4")
    p.body = buf[o_co: total]                       # index | bits: what tz_keys_put / tz_keysg_put stages


def check_stream(what, p):
    """The code lengths and the index of a parsed file."""
    try:
        huff.check_lengths(p.lengths)
    except ValueError as e:
        raise ValueError(str(e).replace("entropy.dat", "key_frame.dat")) from None
    huff.check_index(what, p.chunk_off, p.run_bits, p.stream_words, p.run, huff.CHUNK_RUNS, "ascending from 0")


def parse(data):
    """Validate a TZK1 key_frame.dat (bytes / uint8 array) -> Parsed.  Everything a pointer or a launch will be derived
    from is checked here, on the CPU; a failure is a ValueError that names the field."""
    what = "key_frame.dat (huff)"
    buf, nt, H, W, nkeys, run, chunk_runs, nchunks, stream_words, o_pred, o_len, o_co = parse_header(what, MAGIC, data)
    p = Parsed()
    p.nt, p.H, p.W, p.nkeys = nt, H, W, nkeys
    parse_stream(what, p, buf, o_co, nkeys * H * W * 3, run, chunk_runs, nchunks, stream_words, "%d key frames of %d x %d" % (nkeys, H, W))
    parse_keys(what, p, buf, nt, nkeys, o_pred)
    if int(p.pred.max()) >= NPRED:
        raise ValueError("%s: predictor id %d outside [0, 3]" % (what, int(p.pred.max())))
    check_stream(what, p)
    return p


def decode_file(data):
    """-> the uint8 (nt, H, W, 3) stack that is zero except at the key frames (what the reference's key_frame.dat holds)."""
    p = parse(data)
    sym = huff.decode_body(p.chunk_off, p.run_bits, p.words, p.n, p.lengths, 0)
    out = np.zeros((p.nt, p.H, p.W, 3), np.uint8)
    fe = p.H * p.W * 3
    for k in range(p.nkeys):
        out[int(p.idx[k])] = unresidual(sym[k * fe: (k + 1) * fe], int(p.pred[k]), p.H, p.W)
    return out
