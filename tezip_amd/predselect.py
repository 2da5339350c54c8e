"""Per-tile choice between the network's prediction and the decoded frame in front (`tezip.py -c --loop closed --pred select`,
tz_set_pred_select / tz_pred_modes / tz_put_pred_modes; NOT a reference feature), definition TZ-PS1 -- the slow statement of it
in numpy, the specification the GPU is tested against.

In a closed loop (TZ-CL1, tezip_amd/closedloop.py) encoder and decoder both hold the decoded frame t-1 when frame t is predicted.
That frame is a second predictor, free of charge and agreed on by both sides.  TZ-PS1 is TZ-CL1 except for the value x of a
non-key frame t:

  tiles              16 x 16 pixels over the unpadded H x W frame, TH = ceil(H / 16) by TW = ceil(W / 16); a tile owns all three
                     channels of its pixels, an edge tile only the samples inside the frame
  candidates         x_net = trunc(f32(pred_t * 255)) as in TZ-CL1;  x_prev = dec[t-1]
  cost               cost_c(tile) = sum |Q(x_c - orig_t)| over the tile's samples, Q the job's quantiser exactly as TZ-CL1 applies
                     it (the identity in a lossless job, else TZ-QL1 with E = min(255, floor(|b|))); integers throughout
  mode               m(t, tile) = 1 (the frame in front) iff cost_prev < cost_net: a tie goes to the network.  Key, warm-up and
                     frame-0 tiles have mode 0 and are not evaluated
  reconstruction     x = m ? x_prev : x_net per tile;  q = Q(x - orig);  dec[t] = clamp(x - q, 0, 255).  The network is always
                     fed dec[t-1], whatever modes that frame used; the decoder runs the same loop with the stored modes
  the back half      stays as it is: a tile with m = 1 is EXPRESSED in the prediction stack, pv(v) = (v + 0.5f) / 255.0f for a
                     sample whose dec[t-1] value is v < 255 and 1.0f for v = 255, so that trunc(f32(pv(v) * 255)) == v for all 256
                     values (the unguarded formula exceeds 1.0 only at v = 255); samples outside H x W in the padded stack stay as
                     the network left them.  closedloop.open_loop_q on the patched stack is this statement's q
  stored             a fifth file pred_modes.dat: the magic TZP1, four little-endian u32 (tile edge 16, nt, TH, TW), then
                     ceil(nt * TH * TW / 8) bytes of mode bits, np.packbits(..., bitorder="little") over the frame-major array,
                     pad bits zero
  mark               the first entry of the trailer's stack shape is the closed-loop mark plus 32: 49, 50, 52, 53, 56, 57

Property (lossless jobs): dec = orig, so the network's predictions do not depend on the modes, x_net is TZ-CL1's x, and per tile
sum |q| = min(cost_net, cost_prev) <= cost_net = the tile's sum |q| under TZ-CL1.  This is a statement about the residual's L1
norm, NOT about coded bytes, and it does not hold for a lossy job: there the modes change what is fed back."""
import os
import struct

import numpy as np

from . import closedloop

DEFINITION = "TZ-PS1"
PREDS = ("net", "select")
TILE = 16
MARK_SELECT = 32                         # added to the closed-loop mark of the layout
MARKS = tuple(m + MARK_SELECT for m in closedloop.MARKS)   # 49, 50, 52, 53, 56, 57
FILE = "pred_modes.dat"
MAGIC = b"TZP1"
HEADER = len(MAGIC) + 16

NEEDS_COMPRESS = "--pred is valid with -c (--compress) only (-u recognises the stream by the mark in its trailer)"
NEEDS_CLOSED = ("--pred select chooses between the network and the DECODED frame in front, which only a closed loop holds: "
                "add --loop closed")


def is_select(one):
    """Whether the first entry of a trailer's stack shape says closed loop with per-tile selection."""
    return int(one) in MARKS


def closed_mark(one):
    """The closed-loop mark of the same layout (what closedloop.is_closed reads): one - 32 for a select mark."""
    return int(one) - MARK_SELECT if is_select(one) else int(one)


def stdout_line(modes):
    modes = np.asarray(modes)
    n, k = int(modes.size), int(np.count_nonzero(modes))
    return "pred: select (%s), %d of %d tiles from the frame in front (%.1f %%)" % (DEFINITION, k, n, 100.0 * k / max(n, 1))


def check_flags(pred, loop):
    """The refusals of --pred that tezip.py and a direct caller of compress.run share: None, or the message.  Everything
    --loop closed refuses stays refused by closedloop.check_flags."""
    if pred not in PREDS:
        return "--pred takes one of %s, got %r" % (", ".join(PREDS), pred)
    if pred == "select" and loop != "closed":
        return NEEDS_CLOSED
    return None


# ---------------------------------------------------------------------------------------------------- the slow statement
def tiles_of(h, w):
    return (h + TILE - 1) // TILE, (w + TILE - 1) // TILE


def tile_sums(a):
    """(H, W, 3) integers -> (TH, TW) sums over each tile's samples inside the frame."""
    a = np.asarray(a, np.int64)
    h, w = a.shape[:2]
    th, tw = tiles_of(h, w)
    full = np.zeros((th * TILE, tw * TILE, 3), np.int64)
    full[:h, :w] = a
    return full.reshape(th, TILE, tw, TILE, 3).sum(axis=(1, 3, 4))


def per_sample(modes, h, w):
    """(TH, TW) modes -> (h, w, 1) bool: the mode of every pixel's tile."""
    m = np.repeat(np.repeat(np.asarray(modes, bool), TILE, axis=0), TILE, axis=1)
    return m[:h, :w, None]


def pv(v):
    """The float32 that stands for the u8 value v in the prediction stack: (v + 0.5f) / 255.0f, 1.0f for v = 255."""
    v = np.asarray(v)
    out = (v.astype(np.float32) + np.float32(0.5)) / np.float32(255.0)
    return np.where(v == 255, np.float32(1.0), out).astype(np.float32)


def patch(pred, prev, modes):
    """The prediction (hp, wp, 3) f32 with pv(prev) written into the tiles with mode 1, inside H x W only."""
    h, w = prev.shape[:2]
    out = np.array(pred, np.float32)
    out[:h, :w] = np.where(per_sample(modes, h, w), pv(prev), out[:h, :w])
    return out


def choose(x_net, x_prev, orig, mode, bound, quant):
    """The modes (TH, TW) uint8 of one frame: 1 iff cost_prev < cost_net."""
    cost_net = tile_sums(np.abs(closedloop.quantise(x_net - orig, mode, bound, quant)))
    cost_prev = tile_sums(np.abs(closedloop.quantise(x_prev - orig, mode, bound, quant)))
    return (cost_prev < cost_net).astype(np.uint8)


def encode(frames, p, w, mode, bound, quant, predictor):
    """The encoder's loop, arguments as closedloop.encode.  Returns dict(key, pred: the NETWORK's predictions, patched: the stack
    with every chosen tile expressed in it, q int16, dec uint8, modes uint8 (nt, TH, TW))."""
    frames = np.asarray(frames, np.uint8)
    nt, h, wd, _ = frames.shape
    hp, wp = closedloop.pad8(h), closedloop.pad8(wd)
    key, gfirst = closedloop.key_mask(nt, p, w), closedloop.group_first(nt, p, w)
    c0 = np.asarray(predictor.c0(hp, wp), np.float32)
    pred = np.empty((nt, hp, wp, 3), np.float32)
    q = np.zeros((nt, h, wd, 3), np.int64)
    dec = np.zeros_like(frames)
    modes = np.zeros((nt,) + tiles_of(h, wd), np.uint8)
    for t in range(nt):
        orig = frames[t].astype(np.int64)
        if key[t]:
            pred[t] = c0
            dec[t] = frames[t]
            q[t] = 0 if gfirst[t] else closedloop.x_hat(c0, h, wd) - orig
            continue
        pred[t] = np.asarray(predictor.next(closedloop.u8_to_f32(dec[t - 1], hp, wp)), np.float32)
        x_net, x_prev = closedloop.x_hat(pred[t], h, wd), dec[t - 1].astype(np.int64)
        modes[t] = choose(x_net, x_prev, orig, mode, bound, quant)
        x = np.where(per_sample(modes[t], h, wd), x_prev, x_net)
        q[t] = closedloop.quantise(x - orig, mode, bound, quant)
        dec[t] = np.clip(x - q[t], 0, 255).astype(np.uint8)
    patched = pred.copy()
    for t in np.nonzero(~key)[0]:
        patched[t] = patch(pred[t], dec[t - 1], modes[t])
    return dict(key=key, pred=pred, patched=patched, q=q.astype(np.int16), dec=dec, modes=modes)


def decode(key_frames, p, payload, table, layout, modes, predictor):
    """The decoder's statement: key stack + payload + modes alone -> dict(key, pred, patched, dec)."""
    key_frames = np.asarray(key_frames, np.uint8)
    nt, h, wd, _ = key_frames.shape
    hp, wp = closedloop.pad8(h), closedloop.pad8(wd)
    modes = np.asarray(modes, np.uint8).reshape((nt,) + tiles_of(h, wd))
    q = closedloop.q_of(payload, table, key_frames.shape, layout).astype(np.int64)
    key = key_frames.reshape(nt, -1).any(axis=1)
    if not key[:p + 1].all():
        raise ValueError("key frames do not cover the sequence")
    if modes.max(initial=0) > 1 or modes[key].any():
        raise ValueError("a mode above 1, or a set mode in a key frame")
    c0 = np.asarray(predictor.c0(hp, wp), np.float32)
    pred = np.empty((nt, hp, wp, 3), np.float32)
    patched = np.empty_like(pred)
    dec = np.zeros_like(key_frames)
    for t in range(nt):
        if key[t]:
            pred[t] = patched[t] = c0
            dec[t] = key_frames[t]
            continue
        pred[t] = np.asarray(predictor.next(closedloop.u8_to_f32(dec[t - 1], hp, wp)), np.float32)
        x = np.where(per_sample(modes[t], h, wd), dec[t - 1].astype(np.int64), closedloop.x_hat(pred[t], h, wd))
        dec[t] = np.clip(x - q[t], 0, 255).astype(np.uint8)
        patched[t] = patch(pred[t], dec[t - 1], modes[t])
    return dict(key=key, pred=pred, patched=patched, dec=dec)


# -------------------------------------------------------------------------------------------------------- pred_modes.dat
def pack(modes):
    """modes (nt, TH, TW) of 0 / 1 -> the bytes of pred_modes.dat."""
    modes = np.asarray(modes, np.uint8)
    if modes.ndim != 3 or modes.max(initial=0) > 1:
        raise ValueError("modes: a (nt, TH, TW) array of 0 and 1 wanted")
    nt, th, tw = modes.shape
    return MAGIC + struct.pack("<4I", TILE, nt, th, tw) + np.packbits(modes.reshape(-1), bitorder="little").tobytes()


def unpack(data, nt, h, w):
    """The bytes of pred_modes.dat -> modes (nt, TH, TW) uint8, checked against the trailer's nt, H, W.  ValueError otherwise."""
    data = bytes(data)
    if len(data) < HEADER:
        raise ValueError("%s: truncated (%d bytes, the header alone has %d)" % (FILE, len(data), HEADER))
    if data[:4] != MAGIC:
        raise ValueError("%s: wrong magic %r (expected %r)" % (FILE, data[:4], MAGIC))
    dims = struct.unpack("<4I", data[4:HEADER])
    want = (TILE, nt) + tiles_of(h, w)
    if dims != want:
        raise ValueError("%s: states tile edge, frames and tiles %r, entropy.dat's trailer implies %r" % (FILE, dims, want))
    n = nt * want[2] * want[3]
    nbytes = (n + 7) // 8
    if len(data) != HEADER + nbytes:
        raise ValueError("%s: %s (%d bytes of mode bits, %d expected)" % (FILE, "truncated" if len(data) < HEADER + nbytes else "too long",
                                                                         len(data) - HEADER, nbytes))
    bits = np.unpackbits(np.frombuffer(data, np.uint8, nbytes, HEADER), bitorder="little")
    if bits[n:].any():
        raise ValueError("%s: a pad bit behind the last tile is set" % FILE)
    return np.ascontiguousarray(bits[:n]).reshape(want[1:])


def write(out_dir, modes):
    """pred_modes.dat into out_dir -> its size."""
    data = pack(modes)
    with open(os.path.join(out_dir, FILE), "wb") as f:
        f.write(data)
    return len(data)


def read(data_dir, nt, h, w):
    """pred_modes.dat of data_dir -> modes; ValueError when it is missing or malformed."""
    path = os.path.join(data_dir, FILE)
    if not os.path.isfile(path):
        raise ValueError("%s is missing: a stream with per-tile selection (mark in entropy.dat's trailer) cannot be decoded without it" % FILE)
    with open(path, "rb") as f:
        return unpack(f.read(), nt, h, w)
