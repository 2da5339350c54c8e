"""Motion-compensated tiles in the closed loop (`tezip.py -c --loop closed --pred motion`, tz_set_pred_motion / tz_pred_modes /
tz_pred_vectors / tz_put_pred_modes / tz_put_pred_vectors; NOT a reference feature), definition TZ-PM1 -- the slow statement of it in
numpy, the specification the GPU is tested against.

TZ-PS1 (tezip_amd/predselect.py) lets a 16 x 16 tile of a predicted frame take the decoded frame in front instead of the network's
output.  A frame that has moved is a poor prediction of the next one; TZ-PM1 displaces it per tile by a small vector, as every video
codec does.  TZ-PM1 is TZ-CL1 (tezip_amd/closedloop.py) except for the value x of a non-key frame t:

  tiles              TZ-PS1's: 16 x 16 pixels over the unpadded H x W frame, TH = ceil(H / 16) by TW = ceil(W / 16), all three
                     channels; an edge tile owns only the samples inside the frame
  displaced frame    for a vector (dy, dx), -7 <= dy, dx <= 7:  ref(y, x, c) = dec[t-1][clamp(y + dy, 0, H-1), clamp(x + dx, 0, W-1), c].
                     Coordinates are clamped, the edge is replicated: no vector reads outside the frame
  search             on raw u8 values, independent of the quantiser:  SAD(dy, dx) = sum |ref - orig_t| over the tile's samples.  The
                     tile's vector minimises the integer key  SAD * 4096 + (|dy| + |dx|) * 256 + (dy + 7) * 16 + (dx + 7)  over all
                     225 vectors.  SAD <= 768 * 255 = 195 840, so the key stays below 2^30; no two vectors share a key, so the choice
                     does not depend on the order of any reduction.  Among equal SADs the shorter vector (L1) wins, then the smaller
                     dy, then the smaller dx
  candidates         x_net = trunc(f32(pred_t * 255)) as in TZ-CL1;  x_mc = ref at the chosen vector
  cost and mode      cost_c(tile) = sum |Q(x_c - orig_t)|, Q the job's quantiser exactly as TZ-PS1 applies it.  m = 1 iff
                     cost_mc < cost_net: a tie goes to the network.  Tiles with m = 0, and the tiles of key, warm-up and frame-0
                     frames, carry the vector (0, 0)
  reconstruction     x = m ? x_mc : x_net per tile;  q = Q(x - orig);  dec[t] = clamp(x - q, 0, 255).  The network is always fed
                     dec[t-1]; the decoder runs the same loop with the stored modes and vectors and never searches
  the back half      stays as it is: a tile with m = 1 is expressed in the prediction stack as predselect.pv(ref), which truncates
                     back to ref; samples outside H x W in the padded stack stay as the network left them
  stored             pred_modes.dat: the magic TZP2, five little-endian u32 (tile edge 16, nt, TH, TW, search radius 7), TZ-PS1's
                     mode bits (ceil(nt * TH * TW / 8) bytes, little-endian bit order, pad bits zero), then one byte
                     (dy + 7) * 16 + (dx + 7) for every tile with m = 1 in frame-major tile order (a nibble of 15 is malformed)
  mark               the first entry of the trailer's stack shape is the closed-loop mark plus 64: 81, 82, 84, 85, 88, 89

Property (lossless jobs): dec = orig, so the network's predictions depend on neither modes nor vectors, Q is the identity and
cost_mc = min SAD <= SAD(0, 0) = TZ-PS1's cost_prev (the key orders by SAD first).  Per tile therefore
    sum |q| under TZ-PM1 = min(cost_net, min SAD)  <=  min(cost_net, cost_prev) = sum |q| under TZ-PS1  <=  cost_net = TZ-CL1's.
This is a statement about the residual's L1 norm, NOT about coded bytes, and it does not hold for a lossy job: there modes and
vectors change what is fed back, and the search minimises the raw SAD, not the quantised cost."""
import os
import struct

import numpy as np

from . import closedloop, predselect

DEFINITION = "TZ-PM1"
PREDS = predselect.PREDS + ("motion",)
TILE = predselect.TILE
RADIUS = 7
MARK_MOTION = 64                         # added to the closed-loop mark of the layout
MARKS = tuple(m + MARK_MOTION for m in closedloop.MARKS)   # 81, 82, 84, 85, 88, 89
FILE = predselect.FILE
MAGIC = b"TZP2"
HEADER = len(MAGIC) + 20

NEEDS_CLOSED = ("--pred motion chooses between the network and the displaced DECODED frame in front, which only a closed loop holds: "
                "add --loop closed")


def is_motion(one):
    """Whether the first entry of a trailer's stack shape says closed loop with motion-compensated tiles."""
    return int(one) in MARKS


def select_mark(one):
    """The mark TZ-PS1 gives the same layout (what decompress.check_stream knows): one - 32 for a motion mark."""
    return int(one) - MARK_MOTION + predselect.MARK_SELECT if is_motion(one) else int(one)


def closed_mark(one):
    """The closed-loop mark of the same layout (what closedloop.is_closed reads), for a motion or a select mark."""
    return predselect.closed_mark(select_mark(one))


def pred_of_mark(one):
    """"motion", "select" or "net": what a trailer's mark says about the prediction of a tile."""
    return "motion" if is_motion(one) else "select" if predselect.is_select(one) else "net"


def stdout_line(modes, vectors):
    modes, vectors = np.asarray(modes), np.asarray(vectors)
    n, k = int(modes.size), int(np.count_nonzero(modes))
    j = int(np.count_nonzero((modes != 0) & vectors.reshape(modes.shape + (2,)).any(axis=-1)))
    return "pred: motion (%s), %d of %d tiles from the frame in front (%.1f %%), %d displaced" % (DEFINITION, k, n, 100.0 * k / max(n, 1), j)


def check_flags(pred, loop):
    """predselect.check_flags with the choice `motion`: None, or the message.  The messages for net and select are predselect's."""
    if pred == "motion":
        return None if loop == "closed" else NEEDS_CLOSED
    return predselect.check_flags(pred, loop)


# ---------------------------------------------------------------------------------------------------- the slow statement
def displaced(prev, dy, dx):
    """prev (H, W, 3) read at clamped (y + dy, x + dx); dy, dx scalars or (H, W) integer arrays."""
    h, w = prev.shape[:2]
    yy = np.clip(np.arange(h)[:, None] + dy, 0, h - 1)
    xx = np.clip(np.arange(w)[None, :] + dx, 0, w - 1)
    return prev[yy, xx]


def keys_of(prev, orig):
    """(225, TH, TW) int64: the key of every vector for every tile, vectors in the order dy-major, dx-minor."""
    prev, orig = np.asarray(prev, np.int64), np.asarray(orig, np.int64)
    out = []
    for dy in range(-RADIUS, RADIUS + 1):
        for dx in range(-RADIUS, RADIUS + 1):
            sad = predselect.tile_sums(np.abs(displaced(prev, dy, dx) - orig))
            out.append(sad * 4096 + (abs(dy) + abs(dx)) * 256 + (dy + RADIUS) * 16 + (dx + RADIUS))
    return np.stack(out)


def search(prev, orig):
    """The vectors (TH, TW, 2) int8 of one frame: per tile the (dy, dx) with the smallest key."""
    key = keys_of(prev, orig).min(axis=0)
    return np.stack([((key >> 4) & 15) - RADIUS, (key & 15) - RADIUS], axis=-1).astype(np.int8)


def reference(prev, vectors):
    """x_mc (H, W, 3): every tile's samples of prev displaced by the tile's vector."""
    h, w = prev.shape[:2]
    v = np.repeat(np.repeat(np.asarray(vectors, np.int64), TILE, axis=0), TILE, axis=1)[:h, :w]
    return displaced(prev, v[..., 0], v[..., 1])


def encode(frames, p, w, mode, bound, quant, predictor):
    """The encoder's loop, arguments as closedloop.encode.  Returns dict(key, pred: the NETWORK's predictions, patched: the stack
    with every chosen tile expressed in it, q int16, dec uint8, modes uint8 (nt, TH, TW), vectors int8 (nt, TH, TW, 2))."""
    frames = np.asarray(frames, np.uint8)
    nt, h, wd, _ = frames.shape
    hp, wp = closedloop.pad8(h), closedloop.pad8(wd)
    key, gfirst = closedloop.key_mask(nt, p, w), closedloop.group_first(nt, p, w)
    c0 = np.asarray(predictor.c0(hp, wp), np.float32)
    pred = np.empty((nt, hp, wp, 3), np.float32)
    patched = np.empty_like(pred)
    q = np.zeros((nt, h, wd, 3), np.int64)
    dec = np.zeros_like(frames)
    modes = np.zeros((nt,) + predselect.tiles_of(h, wd), np.uint8)
    vectors = np.zeros(modes.shape + (2,), np.int8)
    for t in range(nt):
        orig = frames[t].astype(np.int64)
        if key[t]:
            pred[t] = patched[t] = c0
            dec[t] = frames[t]
            q[t] = 0 if gfirst[t] else closedloop.x_hat(c0, h, wd) - orig
            continue
        pred[t] = np.asarray(predictor.next(closedloop.u8_to_f32(dec[t - 1], hp, wp)), np.float32)
        found = search(dec[t - 1], frames[t])
        ref = reference(dec[t - 1], found)
        x_net, x_mc = closedloop.x_hat(pred[t], h, wd), ref.astype(np.int64)
        modes[t] = predselect.choose(x_net, x_mc, orig, mode, bound, quant)
        vectors[t] = np.where(modes[t][..., None] != 0, found, 0)
        x = np.where(predselect.per_sample(modes[t], h, wd), x_mc, x_net)
        q[t] = closedloop.quantise(x - orig, mode, bound, quant)
        dec[t] = np.clip(x - q[t], 0, 255).astype(np.uint8)
        patched[t] = predselect.patch(pred[t], ref, modes[t])
    return dict(key=key, pred=pred, patched=patched, q=q.astype(np.int16), dec=dec, modes=modes, vectors=vectors)


def check_vectors(modes, vectors, key=None):
    """modes (nt, TH, TW) and vectors (nt, TH, TW, 2) as a decoder may be given them; ValueError otherwise."""
    modes, vectors = np.asarray(modes), np.asarray(vectors)
    if vectors.shape != modes.shape + (2,):
        raise ValueError("vectors: shape %r wanted for modes of shape %r" % (modes.shape + (2,), modes.shape))
    if modes.max(initial=0) > 1 or (key is not None and modes[key].any()):
        raise ValueError("a mode above 1, or a set mode in a key frame")
    if np.abs(vectors.astype(np.int64)).max(initial=0) > RADIUS:
        raise ValueError("a vector component outside -%d .. %d" % (RADIUS, RADIUS))
    if vectors[modes == 0].any():
        raise ValueError("a non-zero vector on a tile of mode 0")


def decode(key_frames, p, payload, table, layout, modes, vectors, predictor):
    """The decoder's statement: key stack + payload + modes + vectors alone -> dict(key, pred, patched, dec)."""
    key_frames = np.asarray(key_frames, np.uint8)
    nt, h, wd, _ = key_frames.shape
    hp, wp = closedloop.pad8(h), closedloop.pad8(wd)
    modes = np.asarray(modes, np.uint8).reshape((nt,) + predselect.tiles_of(h, wd))
    vectors = np.asarray(vectors, np.int8).reshape(modes.shape + (2,))
    q = closedloop.q_of(payload, table, key_frames.shape, layout).astype(np.int64)
    key = key_frames.reshape(nt, -1).any(axis=1)
    if not key[:p + 1].all():
        raise ValueError("key frames do not cover the sequence")
    check_vectors(modes, vectors, key)
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
        ref = reference(dec[t - 1], vectors[t])
        x = np.where(predselect.per_sample(modes[t], h, wd), ref.astype(np.int64), closedloop.x_hat(pred[t], h, wd))
        dec[t] = np.clip(x - q[t], 0, 255).astype(np.uint8)
        patched[t] = predselect.patch(pred[t], ref, modes[t])
    return dict(key=key, pred=pred, patched=patched, dec=dec)


# -------------------------------------------------------------------------------------------------------- pred_modes.dat
def pack(modes, vectors):
    """modes (nt, TH, TW) of 0 / 1 and vectors (nt, TH, TW, 2) -> the bytes of pred_modes.dat (format TZP2)."""
    modes = np.asarray(modes, np.uint8)
    if modes.ndim != 3 or modes.max(initial=0) > 1:
        raise ValueError("modes: a (nt, TH, TW) array of 0 and 1 wanted")
    vectors = np.asarray(vectors, np.int8)
    check_vectors(modes, vectors)
    nt, th, tw = modes.shape
    v = vectors[modes != 0].astype(np.int64) + RADIUS                      # frame-major tile order
    codes = (v[:, 0] * 16 + v[:, 1]).astype(np.uint8)
    return (MAGIC + struct.pack("<5I", TILE, nt, th, tw, RADIUS) + np.packbits(modes.reshape(-1), bitorder="little").tobytes()
            + codes.tobytes())


def unpack(data, nt, h, w):
    """The bytes of pred_modes.dat -> (modes (nt, TH, TW) uint8, vectors (nt, TH, TW, 2) int8), checked against the trailer's nt,
    H, W.  ValueError otherwise."""
    data = bytes(data)
    if len(data) >= 4 and data[:4] != MAGIC:
        raise ValueError("%s: wrong magic %r (expected %r for a stream with motion-compensated tiles)" % (FILE, data[:4], MAGIC))
    if len(data) < HEADER:
        raise ValueError("%s: truncated (%d bytes, the header alone has %d)" % (FILE, len(data), HEADER))
    dims = struct.unpack("<5I", data[4:HEADER])
    if dims[4] != RADIUS:
        raise ValueError("%s: states the search radius %d, this build reads %d" % (FILE, dims[4], RADIUS))
    want = (TILE, nt) + predselect.tiles_of(h, w) + (RADIUS,)
    if dims != want:
        raise ValueError("%s: states tile edge, frames, tiles and radius %r, entropy.dat's trailer implies %r" % (FILE, dims, want))
    n = nt * want[2] * want[3]
    nbytes = (n + 7) // 8
    if len(data) < HEADER + nbytes:
        raise ValueError("%s: truncated (%d bytes of mode bits, %d expected)" % (FILE, len(data) - HEADER, nbytes))
    bits = np.unpackbits(np.frombuffer(data, np.uint8, nbytes, HEADER), bitorder="little")
    if bits[n:].any():
        raise ValueError("%s: a pad bit behind the last tile is set" % FILE)
    k = int(bits[:n].sum())
    have = len(data) - HEADER - nbytes
    if have != k:
        raise ValueError("%s: %s (%d vector bytes, %d tiles have mode 1)" % (FILE, "truncated" if have < k else "too long", have, k))
    codes = np.frombuffer(data, np.uint8, k, HEADER + nbytes).astype(np.int64)
    if ((codes >> 4) == 15).any() or ((codes & 15) == 15).any():
        raise ValueError("%s: a vector nibble of 15 (components are stored as 0 .. 14)" % FILE)
    modes = np.ascontiguousarray(bits[:n]).reshape(want[1:4])
    vectors = np.zeros(modes.shape + (2,), np.int8)
    vectors[modes != 0] = np.stack([(codes >> 4) - RADIUS, (codes & 15) - RADIUS], axis=-1)
    return modes, vectors


def write(out_dir, modes, vectors):
    """pred_modes.dat into out_dir -> its size."""
    data = pack(modes, vectors)
    with open(os.path.join(out_dir, FILE), "wb") as f:
        f.write(data)
    return len(data)


def read(data_dir, nt, h, w):
    """pred_modes.dat of data_dir -> (modes, vectors); ValueError when it is missing or malformed."""
    path = os.path.join(data_dir, FILE)
    if not os.path.isfile(path):
        raise ValueError("%s is missing: a stream with motion-compensated tiles (mark in entropy.dat's trailer) cannot be decoded without it" % FILE)
    with open(path, "rb") as f:
        return unpack(f.read(), nt, h, w)
