"""The GPU-coded key_frame.dat that stores a gray key frame once (`--key-coder huffg`; NOT a reference format): container,
validation and a plain numpy statement of what the kernels k_key_gray / k_key_resid / k_key_unresid_* (csrc/tz_codec.hip)
and the Huffman kernels behind them write and read.  The slow functions here are the specification the kernels are tested
against (tests/test_keycoderg.py, tests/test_gpu_keycoderg.py); the product calls only the container, `pred_bytes`,
`chosen_counts` and `parse`.  DESIGN.md section 9 holds the format as prose.

TZK2 is TZK1 (tezip_amd/keycoder.py) with one more bit per key frame.  The reference widens a single-channel source to RGB,
so every key frame of such a job holds each sample three times; a key frame whose three channels are equal at EVERY pixel is
GRAY, contributes the residuals of channel 0 alone, and is replicated to three channels on decode.

File layout, little-endian, every section padded with zero bytes to a multiple of 4 -- TZK1's, section for section:
  header   48 bytes: "TZK2" | u16 version = 1 | u16 L = 12 | u32 nt | u32 H | u32 W | u32 C = 3 (the stack's) | u32 nkeys |
           u32 R = 256 | u32 chunk_runs = 64 | u32 nchunks | u32 stream_words | u32 0
  keys     nkeys u32 frame indices, strictly ascending, each < nt
  preds    nkeys bytes: bits 0-1 the predictor id of the key frame, bit 2 (value 4) GRAY; values above 7 are refused
  lengths  256 bytes: code length of residual value s, 0 = absent, else 1..L; canonical codes as in TZH1
  index    nchunks u32 word offsets, then ceil(n / R) u16 run sizes in bits                              (TZH1 section 4)
  bits     stream_words u32                                                                          (TZH1 section 5)
n is the sum over the key frames of H * W (GRAY) or H * W * 3 (any other frame).  The symbols are the residuals of the key
frames in index order: a GRAY frame's channel 0 in (H, W) order, any other frame in (H, W, 3) memory order as in TZK1.  Frames
are not aligned to runs.  GRAY is a function of the frame (set iff x[y, col, 0] == x[y, col, 1] == x[y, col, 2] everywhere),
not a choice, so the GPU and this module write the same file.

The residual of a GRAY frame is TZK1's over the one channel: neighbours left, up, up-left, each 0 outside the frame.  Its
predictor is chosen by keycoder.choose_predictors from the counts of channel 0, which are formed as the three-channel counts
(tz_keys_counts' result) divided by 3 -- exact, because the three channels of a GRAY frame have identical residuals under every
predictor; `gray_counts` states it, and the product and `encode_file` both go this way.  The one code table is built from the
chosen counts summed over the frames: one-channel counts for GRAY frames, three-channel counts otherwise.
"""
import numpy as np

from . import huff, keycoder

MAGIC = b"TZK2"
VERSION = 1
GRAY = 4                             # bit 2 of a pred byte
HEADER = keycoder.HEADER             # 48 bytes
MAX_FRAMES = keycoder.MAX_FRAMES
MAX_SIDE = keycoder.MAX_SIDE


def is_keycoded(head):
    """The first bytes of a key_frame.dat: this format's magic."""
    return bytes(head[:4]) == MAGIC


_pad4 = keycoder._pad4


def gray_flags(key_frames):
    """uint8 (k, H, W, 3) -> bool[k]: the three channels are equal at every pixel (what tz_keys_gray returns)."""
    kf = np.asarray(key_frames, np.uint8)
    if kf.ndim != 4 or kf.shape[3] != 3:
        raise ValueError("key frames must be a (k, H, W, 3) uint8 stack, got shape %r" % (tuple(kf.shape),))
    return ((kf[..., 0] == kf[..., 1]) & (kf[..., 1] == kf[..., 2])).reshape(kf.shape[0], -1).all(axis=1)


def frame_symbols(gray, H, W):
    """Symbols each key frame contributes -> int64[k]."""
    return np.where(np.asarray(gray, bool), H * W, H * W * 3).astype(np.int64)


def offsets(gray, H, W):
    """(exclusive prefix of frame_symbols as uint64[k], n): where each frame's symbols start, and how many there are."""
    cnt = frame_symbols(gray, H, W)
    return (np.cumsum(cnt) - cnt).astype(np.uint64), int(cnt.sum())


def gray_counts(counts, gray):
    """Three-channel counts[k][4][256] -> the counts the format is defined on: those of a GRAY frame divided by 3 (its
    one-channel counts, exactly), the others as they are."""
    c = np.asarray(counts).astype(np.int64)
    g = np.asarray(gray, bool)
    if (c[g] % 3).any():
        raise ValueError("key_frame.dat (huffg): the residual counts of a gray key frame are not multiples of 3")
    c[g] //= 3
    return c


def pred_bytes(counts, gray):
    """gray_counts' result and the flags -> uint8[k]: predictor id | GRAY."""
    return (keycoder.choose_predictors(counts) | np.where(np.asarray(gray, bool), GRAY, 0)).astype(np.uint8)


def chosen_counts(counts, predg):
    """The counts the one code table is made from (gray_counts' result; the GRAY bit of a pred byte is ignored)."""
    return keycoder.chosen_counts(counts, np.asarray(predg, np.uint8) & 3)


def residual(frame, predg):
    """uint8 (H, W, 3) frame -> its int16 residuals under the pred byte: H * W of channel 0 with GRAY, else TZK1's."""
    x = np.asarray(frame, np.uint8)
    if not 0 <= int(predg) < 2 * GRAY:
        raise ValueError("key_frame.dat (huffg): pred byte %d outside [0, 7]" % int(predg))
    if not int(predg) & GRAY:
        return keycoder.residual(x, int(predg))
    if x.ndim != 3 or x.shape[2] != 3:
        raise ValueError("a key frame must be a (H, W, 3) uint8 array, got shape %r" % (tuple(x.shape),))
    return keycoder.residual(np.repeat(x[:, :, :1], 3, axis=2), int(predg) & 3)[0::3]


def unresidual(sym, predg, H, W):
    """The inverse: prefix sums mod 256 over (H, W) for a GRAY frame, each sample written to all three channels."""
    if not 0 <= int(predg) < 2 * GRAY:
        raise ValueError("key_frame.dat (huffg): pred byte %d outside [0, 7]" % int(predg))
    if not int(predg) & GRAY:
        return keycoder.unresidual(sym, int(predg), H, W)
    r = np.asarray(sym, np.int64).reshape(H, W) & 255
    if int(predg) & 1:
        r = np.cumsum(r, axis=1) & 255
    if int(predg) & 2:
        r = np.cumsum(r, axis=0) & 255
    return np.repeat(r.astype(np.uint8)[:, :, None], 3, axis=2)


def symbols(key_frames, predg):
    """The int16 symbols of the file's body, one frame after the other."""
    return np.concatenate([residual(f, p) for f, p in zip(key_frames, predg)])


def pack_front(nt, H, W, idx, predg, lengths, nchunks, stream_words):
    """Header | key indices | pred bytes | lengths: everything of the file in front of the index."""
    predg = np.ascontiguousarray(predg, np.uint8)
    if predg.size and int(predg.max()) >= 2 * GRAY:
        raise ValueError("key_frame.dat (huffg): pred byte %d outside [0, 7]" % int(predg.max()))
    front = keycoder.pack_front(nt, H, W, idx, predg, lengths, nchunks, stream_words)
    return MAGIC + front[4:]


def encode_file(stack_or_keyframes, idx, nt):
    """The whole key_frame.dat on the CPU (tests, and the specification of compress.run's output).  The first argument is
    the (nt, H, W, 3) stack, of which the frames `idx` are coded, or the (len(idx), H, W, 3) key frames themselves."""
    kf, idx = keycoder.key_frames_of("key_frame.dat (huffg)", stack_or_keyframes, idx, nt)
    H, W = kf.shape[1:3]
    gray = gray_flags(kf)
    counts = gray_counts(keycoder.predictor_counts(kf), gray)
    predg = pred_bytes(counts, gray)
    lengths = huff.code_lengths(chosen_counts(counts, predg))
    co, rb, words = huff.encode_body(symbols(kf, predg), lengths, 0)
    return pack_front(nt, H, W, idx, predg, lengths, co.size, words.size) + huff.pack_body(co, rb, words)


class Parsed:
    """A validated TZK2 key_frame.dat: the stack's shape, the key indices, their pred bytes, and views of the sections."""


def parse(data):
    """Validate a TZK2 key_frame.dat (bytes / uint8 array) -> Parsed.  Everything a pointer or a launch will be derived
    from is checked here, on the CPU; a failure is a ValueError that names the field."""
    what = "key_frame.dat (huffg)"
    buf, nt, H, W, nkeys, run, chunk_runs, nchunks, stream_words, o_pred, o_len, o_co = keycoder.parse_header(what, MAGIC, data)
    # the pred bytes come before anything that depends on n: n is a function of their GRAY bits
    if buf.size < o_co:
        raise ValueError("%s: file size %d is shorter than the %d bytes in front of the index (truncated)" % (what, buf.size, o_co))
    p = Parsed()
    p.nt, p.H, p.W, p.nkeys = nt, H, W, nkeys
    keycoder.parse_keys(what, p, buf, nt, nkeys, o_pred)
    if int(p.pred.max()) >= 2 * GRAY:
        raise ValueError("%s: pred byte %d outside [0, 7]" % (what, int(p.pred.max())))
    p.gray = (p.pred & GRAY) != 0
    p.offsets, n = offsets(p.gray, H, W)
    keycoder.parse_stream(what, p, buf, o_co, n, run, chunk_runs, nchunks, stream_words,
                          "%d key frames of %d x %d (%d of them gray)" % (nkeys, H, W, int(p.gray.sum())))
    keycoder.check_stream(what, p)
    return p


def decode_file(data):
    """-> the uint8 (nt, H, W, 3) stack that is zero except at the key frames (what the reference's key_frame.dat holds)."""
    p = parse(data)
    sym = huff.decode_body(p.chunk_off, p.run_bits, p.words, p.n, p.lengths, 0)
    out = np.zeros((p.nt, p.H, p.W, 3), np.uint8)
    cnt = frame_symbols(p.gray, p.H, p.W)
    for k in range(p.nkeys):
        o = int(p.offsets[k])
        out[int(p.idx[k])] = unresidual(sym[o: o + int(cnt[k])], int(p.pred[k]), p.H, p.W)
    return out
