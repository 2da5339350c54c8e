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

Only the lossless back half of the coder changes: a job decodes to exactly the images it decodes to without the flag.

  python -m tezip_amd.sdelta FILE.npy [STRIDE]    sizes of an int16 array under the flat and the strided delta (zstd-9)
"""
import numpy as np

OFFSET = 1600      # compress.py:348
MARK = 4           # first entry of the trailer's stack shape: channel-stride payload
MARK_SHUFFLE = 5   # ... stored as byte planes (--shuffle)
MARKS = (MARK, MARK_SHUFFLE)
MODES = ("flat", "channel")


def mark(shuffled):
    return MARK_SHUFFLE if shuffled else MARK


def is_strided(one):
    """Whether the first entry of a trailer's stack shape says channel stride."""
    return int(one) in MARKS


def is_shuffled(one):
    """Whether the first entry of a trailer's stack shape says byte planes (2: flat, 5: channel stride)."""
    return int(one) in (2, MARK_SHUFFLE)


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


def payload_from_delta(delta_stack, entropy, stride=3):
    """The (nt, H, W, C) int16 quantised delta stack -> (payload int16[nt*H*W*C], table | None)."""
    if not entropy:
        return encode(delta_stack, stride, False), None
    y = encode(delta_stack, stride, True)
    table = build_table(y)
    return remap(y, table), table


def delta_from_payload(payload, table, stride=3):
    """The inverse of payload_from_delta -> the flattened delta stack."""
    if table is None:
        return decode(payload, stride, False)
    return decode(unmap(payload, table), stride, True)


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
