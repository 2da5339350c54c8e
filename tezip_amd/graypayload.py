"""The one-channel payload of a gray job (`tezip.py -c --gray`, tz_set_payload_channels(1)) -- the slow statement of the
format in numpy, the specification the GPU kernels (k_sdelta_gray, k_recon_gray*) are tested against.  Not a reference format.

The reference widens a single-channel source to RGB (compress.py:114), so the payload of such a job carries every delta
three times.  The quantiser runs per frame and per channel (compress.py:316-319) and the decoder's predictions depend on the
key frames alone (decompress.py:143-175): when every frame of a job is gray, channel 0 of the quantised delta stack
reconstructs channel 0 within the bound, and the same sample is right for channels 1 and 2, whose originals equal channel 0.

  payload   nt*H*W int16: finding_difference (compress.py:73-77) over channel 0 of the (nt, H, W, 3) delta stack, then, with
            the entropy remap, 1600 - x and the rank of the symbol in the table (compress.py:348-369)
  table     the symbols of that payload by descending count, ties by ascending symbol (compress.py:352-361)
  trailer   table | T (or -1) | mark, nt, H, W, 1 | warm_up: the stack shape ends in the channel count 1
  decode    the inverse remap and inverse spatial delta over the nt*H*W elements give one delta per pixel;
            sample = clamp(base - delta, 0, 255) with base = the key byte of channel 0 or trunc(pred channel 0 * 255), written
            to all three channels.  key_frame.dat is unchanged: nt*H*W*3 bytes, or TZK1 / TZK2
"""
import numpy as np

OFFSET = 1600   # compress.py:348


def is_gray(frames):
    """True when the three channels of every pixel of the (.., H, W, 3) uint8 stack are equal."""
    f = np.asarray(frames)
    if f.ndim < 3 or f.shape[-1] != 3:
        raise ValueError("frames must end in 3 channels, got shape %r" % (tuple(f.shape),))
    return bool((f[..., 0] == f[..., 1]).all() and (f[..., 1] == f[..., 2]).all())


def spatial_delta(x, carry=None):
    """compress.py:73-77 over the flattened int16 array: out[0] = x[0] (carry - x[0] with a carry), out[i] = x[i-1] - x[i],
    int16 wrap-around."""
    x = np.asarray(x, np.int16).reshape(-1)
    out = x.copy()
    with np.errstate(over="ignore"):
        out[1:] = x[:-1] - x[1:]
        if carry is not None and x.size:
            out[0] = np.int16(carry) - x[0]
    return out


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


def payload_from_delta(delta3, entropy):
    """The (nt, H, W, 3) int16 quantised delta stack of a gray job -> (payload int16[nt*H*W], table | None)."""
    d = np.asarray(delta3, np.int16)
    if d.ndim != 4 or d.shape[3] != 3:
        raise ValueError("delta stack must be (nt, H, W, 3), got shape %r" % (tuple(d.shape),))
    sd = spatial_delta(d[..., 0])
    if not entropy:
        return sd, None
    y = (OFFSET - sd.astype(np.int64)).astype(np.int16)
    table = build_table(y)
    return remap(y, table), table


def reconstruct(base0, delta1):
    """base0: the integer bases of channel 0 (key byte or trunc(pred * 255)), delta1: one int16 delta per pixel, same shape
    (.., H, W) -> uint8 (.., H, W, 3), the sample clamp(base - delta, 0, 255) in all three channels."""
    v = np.clip(np.asarray(base0, np.int64) - np.asarray(delta1, np.int64), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(np.repeat(v[..., None], 3, axis=-1))
