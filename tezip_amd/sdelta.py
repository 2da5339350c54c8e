"""The spatial delta of the payload at the channel stride (`tezip.py -c --sdelta channel`, tz_set_delta_stride(1)) -- the slow
statement of the format in numpy, the specification the GPU kernels (k_sdelta_s3, k_scan3p, k_undelta_carry_s3) are tested
against.  Not a reference format.

finding_difference (compress.py:73-77) takes out[i] = in[i-1] - in[i] over the flattened (nt, H, W, 3) stack, so the
neighbour of a sample is another CHANNEL of the same pixel.  Here the neighbour is the same channel of the pixel in front:

  encode    out[i] = in[i] for i < S, out[i] = in[i-S] - in[i] (int16 wrap-around) otherwise, S = the payload's channels per
            pixel, over the flattened stack across pixel, row and frame boundaries; then, with the entropy remap, 1600 - x
            and the rank of the symbol in the table (compress.py:348-369) exactly as for the flat delta
  decode    in[i] = in[i-S] - out[i]: S interleaved wrap-around scans, one per class of the element index mod S
  trailer   table | T (or -1) | mark, nt, H, W, 3 | warm_up with mark = 4 (MARK), or 5 (MARK_SHUFFLE) when the payload is
            stored as byte planes; the reference writes 1 there, --shuffle 2, and 3 stays refused.  The mark is written only
            for a payload of three channels: with one channel (--gray on an all-gray job) S = 1, which IS the flat delta,
            and the stream is the --gray stream

The 2-D spatial delta, definition TZ-SD2 (`-c --sdelta plane`, tz_set_delta_plane(1); kernels k_sdelta_plane, k_unplane_cols,
k_unplane_rows), is stated here too.  q[f, y, x, c] is the quantised delta stack, values in [-255, 255], C the payload's
channels (3, or 1 under --gray on an all-gray job); per frame and channel, every neighbour outside the frame taken as 0:

  encode    sd = wrap9(q[y, x-1] + q[y-1, x] - q[y-1, x-1] - q[y, x]), wrap9(v) = ((v + 256) mod 512) - 256 in [-256, 255];
            then 1600 - sd in [1345, 1856] (512 symbols: TZ_NBINS and every coder's alphabet hold) and the rank as above
  decode    q = wrap9(S), S the inclusive 2-D prefix sum of -sd over the frame and channel (mod 2^16 suffices: 512 | 65536)
  trailer   mark = 8 (MARK_PLANE), or 9 (MARK_PLANE_SHUFFLE) with byte planes; the last entry of the shape may be 3 or 1 -- on
            one channel plane is NOT the flat delta, so a --gray plane stream is marked.  3, 6 and 7 stay refused
  example   the 2 x 2 one-channel frame [[255, -255], [-255, 255]] -> sd [[-255, -2], [-2, 4]], symbols [[1855, 1602], [1602, 1596]]

Every frame is coded on its own, so a range decode needs no carry.

Only the lossless back half of the coder changes: a job decodes to exactly the images it decodes to without the flag.

  python -m tezip_amd.sdelta FILE.npy [STRIDE]    sizes of an int16 array under the flat and the strided delta (zstd-9)
"""
import numpy as np

OFFSET = 1600      # compress.py:348
MARK = 4           # first entry of the trailer's stack shape: channel-stride payload
MARK_SHUFFLE = 5   # ... stored as byte planes (--shuffle)
MARKS = (MARK, MARK_SHUFFLE)
MARK_PLANE = 8          # ... 2-D plane payload TZ-SD2 (encode_plane below); the last entry of the shape may be 3 or 1
MARK_PLANE_SHUFFLE = 9  # ... stored as byte planes (--shuffle)
PLANE_MARKS = (MARK_PLANE, MARK_PLANE_SHUFFLE)
MODES = ("flat", "channel", "plane")


def mark(shuffled, plane=False):
    if plane:
        return MARK_PLANE_SHUFFLE if shuffled else MARK_PLANE
    return MARK_SHUFFLE if shuffled else MARK


def is_strided(one):
    """Whether the first entry of a trailer's stack shape says channel stride."""
    return int(one) in MARKS


def is_plane(one):
    """Whether the first entry of a trailer's stack shape says the 2-D plane delta TZ-SD2."""
    return int(one) in PLANE_MARKS


def is_shuffled(one):
    """Whether the first entry of a trailer's stack shape says byte planes (2: flat, 5: channel stride, 9: plane)."""
    return int(one) in (2, MARK_SHUFFLE, MARK_PLANE_SHUFFLE)


def mode_of(one):
    """The --sdelta mode the first entry of a trailer's stack shape states."""
    return "plane" if is_plane(one) else ("channel" if is_strided(one) else "flat")


def _carry(carry, stride):
    c = np.atleast_1d(np.asarray(carry)).astype(np.int16)
    if c.size != stride:
        raise ValueError("the carry holds %d elements, the stride is %d" % (c.size, stride))
    return c


def encode(stack, stride, apply_offset, carry=None):
    """The flattened int16 `stack` -> its spatial delta at `stride`; carry (None, or `stride` elements): the elements in front
    of stack[0].  apply_offset: 1600 - x on top (compress.py:348)."""
    if stride < 1:
        raise ValueError("stride must be positive, not %r" % (stride,))
    x = np.asarray(stack, np.int16).reshape(-1)
    out = x.copy()
    with np.errstate(over="ignore"):
        out[stride:] = x[:-stride] - x[stride:]
        if carry is not None:
            k = min(stride, x.size)
            out[:k] = _carry(carry, stride)[:k] - x[:k]
        if apply_offset:
            out = (np.int16(OFFSET) - out).astype(np.int16)
    return out


def decode(delta, stride, apply_offset, carry=None):
    """The inverse of encode: x[i] = x[i-stride] - s[i], one wrap-around scan per class of i mod stride."""
    if stride < 1:
        raise ValueError("stride must be positive, not %r" % (stride,))
    s = np.asarray(delta, np.int16).reshape(-1).astype(np.int64)
    if apply_offset:
        s = OFFSET - s
    c0 = np.zeros(stride, np.int64) if carry is None else _carry(carry, stride).astype(np.int64)
    if carry is None:
        s[:stride] = -s[:stride]
    out = np.empty(s.size, np.int64)
    for c in range(min(stride, s.size)):
        out[c::stride] = c0[c] - np.cumsum(s[c::stride])
    return (out & 0xFFFF).astype(np.uint16).view(np.int16)


def carry_of(stack, n0, stride):
    """The `stride` elements of the decoded stack in front of element n0 (n0 a positive multiple of stride): what a decoder
    that starts at n0 needs (tz_undelta_carry_stride)."""
    if n0 <= 0 or n0 % stride:
        raise ValueError("n0 = %r is not a positive multiple of the stride %d" % (n0, stride))
    return np.asarray(stack, np.int16).reshape(-1)[n0 - stride:n0].copy()


def wrap9(v):
    """((v + 256) mod 512) - 256, in [-256, 255]."""
    return ((np.asarray(v, np.int64) + 256) % 512) - 256


def encode_plane(stack4d, apply_offset):
    """TZ-SD2: the (nt, H, W, C) int16 quantised delta stack q, values in [-255, 255] -> the flattened int16
    sd = wrap9(q[y, x-1] + q[y-1, x] - q[y-1, x-1] - q[y, x]) per frame and channel, every neighbour outside the frame 0;
    1600 - sd on top when apply_offset.  Every frame is coded on its own."""
    q = np.asarray(stack4d, np.int16)
    if q.ndim != 4:
        raise ValueError("encode_plane takes the (nt, H, W, C) stack, not %d dimensions" % q.ndim)
    q = q.astype(np.int64)
    if q.size and (q.min() < -255 or q.max() > 255):
        raise ValueError("encode_plane takes deltas in [-255, 255]")
    p = np.zeros_like(q)
    p[:, :, 1:] += q[:, :, :-1]
    p[:, 1:, :] += q[:, :-1, :]
    p[:, 1:, 1:] -= q[:, :-1, :-1]
    sd = wrap9(p - q)
    if apply_offset:
        sd = OFFSET - sd
    return sd.astype(np.int16).reshape(-1)


def decode_plane(delta, shape, apply_offset):
    """The inverse of encode_plane -> the flattened stack of `shape` = (nt, H, W, C): q = wrap9(S), S the inclusive 2-D prefix
    sum of -sd over the frame and channel (sums may be taken mod 2^16: 512 divides 65536)."""
    nt, H, W, C = (int(v) for v in shape)
    s = np.asarray(delta, np.int16).reshape(nt, H, W, C).astype(np.int64)
    if apply_offset:
        s = OFFSET - s
    S = np.cumsum(np.cumsum(-s, axis=1), axis=2)
    return wrap9(S).astype(np.int16).reshape(-1)


def build_table(symbols):
    """compress.py:352-361: the symbols present, by count descending, equal counts by ascending symbol."""
    counts = np.bincount(np.asarray(symbols).reshape(-1).astype(np.int64))
    syms = np.nonzero(counts)[0]
    order = np.lexsort((syms, -counts[syms]))   # last key first: count descending, then symbol ascending
    return syms[order].astype(np.int16)


def remap(symbols, table):
    """compress.py:84-90: symbol -> its rank in the table."""
    lut = np.arange(65536, dtype=np.int64) - 32768
    lut[np.asarray(table, np.int64) + 32768] = np.arange(len(table))
    return lut[np.asarray(symbols).astype(np.int64) + 32768].astype(np.int16)


def unmap(ranks, table):
    """decompress.py:31-36: rank -> symbol."""
    t = np.asarray(table, np.int16)
    return t[np.asarray(ranks).astype(np.int64)]


def payload_from_delta(delta_stack, entropy, stride=3, plane=False):
    """The (nt, H, W, C) int16 quantised delta stack -> (payload int16[nt*H*W*C], table | None).  plane: TZ-SD2 in place of
    the delta at `stride`."""
    enc = (lambda off: encode_plane(delta_stack, off)) if plane else (lambda off: encode(delta_stack, stride, off))
    if not entropy:
        return enc(False), None
    y = enc(True)
    table = build_table(y)
    return remap(y, table), table


def delta_from_payload(payload, table, stride=3, plane_shape=None):
    """The inverse of payload_from_delta -> the flattened delta stack.  plane_shape: the (nt, H, W, C) of a TZ-SD2 payload."""
    dec = (lambda s, off: decode_plane(s, plane_shape, off)) if plane_shape is not None else (lambda s, off: decode(s, stride, off))
    if table is None:
        return dec(payload, False)
    return dec(unmap(payload, table), True)


def main(argv=None):
    import sys
    from . import zstd
    argv = sys.argv[1:] if argv is None else argv
    if not 1 <= len(argv) <= 2:
        print(__doc__)
        return 2
    x = np.load(argv[0]).astype(np.int16).reshape(-1)
    stride = int(argv[1]) if len(argv) > 1 else 3
    for name, s in (("flat", 1), ("stride %d" % stride, stride)):
        y = encode(x, s, True)
        print("%-10s zstd-9 %d bytes" % (name, len(zstd.compress(y.tobytes(), 9))))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
