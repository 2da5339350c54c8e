"""compress.run -- same signature, files and messages as the reference's
/root/reference/src/compress.py:93 `run(...)`; everything between "uint8 frame stack" and
"int16 payload + table" runs in libtezip_hip.so on the MI355X (no CPU fallback).

Output directory:
  filename.txt   line 1 "1"|"0" (RGB|L source), then one basename per line  (compress.py:133-136)
  key_frame.dat  zstd-9 of uint8[nt*H*W*3], zero except key frames           (compress.py:271-278)
  entropy.dat    zstd-9 of int16: payload | table | T  (or | -1) | 1,nt,H,W,3 | warm_up
                                                                              (compress.py:381-400)
                 with GRAY (--gray; not a reference format) on a job whose frames are all gray: the payload holds channel 0
                 alone, nt*H*W elements, and the shape in the trailer ends in 1 (tezip_amd/graypayload.py)
                 with SDELTA="channel" (--sdelta channel; not a reference format) on a three-channel payload: the spatial
                 delta of the payload is taken three elements back (the same channel of the pixel in front) and the first
                 entry of the shape in the trailer is 4, or 5 with byte planes (tezip_amd/sdelta.py)
                 with CODER="huff" (--coder huff; not a reference format): "TZH1" header | that trailer | code lengths |
                 index | bit stream, written by the GPU (tezip_amd/huff.py); with CODER="huffr" the
                 same under the magic "TZR1", the code being over literals and period-3 repeat tokens (tezip_amd/huffr.py);
                 with CODER="huffd" under the magic "TZR2", the match distance 0 / 1 / 3 chosen per file (tezip_amd/huffd.py)
  with KEY_CODER="huff" (--key-coder huff; not a reference format) key_frame.dat holds the key frames alone: "TZK1" header |
                 key indices | predictor ids | code lengths | index | bit stream -- per key frame the residuals of the best
                 of four predictors (none, left, up, left + up - upleft), Huffman-coded on the GPU (tezip_amd/keycoder.py,
                 DESIGN.md section 9).  Smaller than zstd-9 on smooth frames, LARGER on sparse ones: hence opt-in
  with KEY_CODER="huffg" (--key-coder huffg) the same under the magic "TZK2": a key frame whose three channels are equal at
                 every pixel (a gray source, widened to RGB) is coded as one channel (tezip_amd/keycoderg.py)
"""
import glob
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import _lib, boundmap, closedframes, closedloop, closedmap, digest, frametarget, huff, huffd, huffr, keycoder, keycoderg, lattice, predmotion, predselect, quality, ratetarget, sdauto, sdelta, sidecar, target, weights, zstd
from . import dist as tzdist
from .data_utils import padding_shape


def io_threads():
    """Threads for PNG decode/encode: the CPUs this process may use, at most 16."""
    try:
        n = len(os.sched_getaffinity(0))
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()
        if q != "max":
            n = min(n, max(1, int(int(q) / int(per))))
    except Exception:
        n = os.cpu_count() or 1
    return max(1, min(16, n))


def load_images(data_dir):
    """compress.py:97-131: sorted(glob), RGB or L only (L is expanded to RGB), all one size."""
    from PIL import Image, UnidentifiedImageError
    file_paths = sorted(glob.glob(os.path.join(data_dir, '*')))
    if len(file_paths) == 0:
        print("ERROR:", data_dir, "is an empty or non-existent directory")
        exit()
    try:
        first = Image.open(file_paths[0])
        image_mode = first.mode
        if all([image_mode != 'RGB', image_mode != 'L']):
            print("ERROR: input image is {0}. Only RGB and grayscale are supported.".format(image_mode))
            exit()
        is_rgb = image_mode == 'RGB'

        def decode(path):
            img = Image.open(path)
            arr = np.array(img if is_rgb else img.convert('RGB'))
            if arr.ndim != 3 or arr.shape[2] != 3:
                raise IndexError(path)
            return arr

        # PIL's codecs release the GIL: decode on a few threads (order is kept by map)
        with ThreadPoolExecutor(max_workers=io_threads()) as pool:
            frames = list(pool.map(decode, file_paths))
        files = [os.path.basename(path) for path in file_paths]
        stack = np.ascontiguousarray(np.stack(frames), dtype=np.uint8)
    except (PermissionError, IndexError, UnidentifiedImageError, IsADirectoryError, ValueError):
        print(data_dir, "contains files or folders that are not images.")
        exit()
    return stack, files, is_rgb


def open_model(weights_dir):
    """compress.py:143-160: same error messages."""
    json_file = os.path.join(weights_dir, weights.JSON_NAME)
    try:
        return weights.load_model(weights_dir)
    except FileNotFoundError:
        print("ERROR: No such file or directory:", json_file)
        exit()
    except OSError as e:
        print("ERROR: No such file or directory:", os.path.join(weights_dir, weights.H5_NAME))
        print(e)
        exit()


def make_context(cfg, wts, hp, wp, max_batch, device=0):
    ctx = _lib.Context(device)
    ctx.load_model(cfg, wts)
    ctx.prepare(hp, wp, max_batch)
    return ctx


SHUFFLE_MARK = 2  # first trailer shape entry of a byte-shuffled stream (the reference always writes 1)


def build_stream(payload, table, shape5, warm_up):
    """compress.py:381-394: payload | table | len(table)  (or | -1) | shape | PREPROCESS, int16.
    shape5[0] is 1 in the reference's format; SHUFFLE_MARK flags the opt-in byte-shuffled payload
    (this build only; `payload` then carries the two byte planes in an int16-typed buffer)."""
    if table is not None:
        tail = np.concatenate([table.astype(np.int64), [len(table)]])
    else:
        tail = np.array([-1], dtype=np.int64)
    trailer = np.concatenate([tail, list(shape5), [warm_up]]).astype(np.int16)
    return np.concatenate([np.asarray(payload, dtype=np.int16).reshape(-1), trailer])


def pack_outputs(frames, key, payload, table, warm_up, shuffled=False):
    """compress.py:271-278 and 375-400: the two zstd-9 frames (key_frame.dat, entropy.dat) as bytes."""
    nt, H, W = frames.shape[:3]
    key_frame = np.zeros_like(frames)
    key_frame[key] = frames[key]
    key_bytes = zstd.compress_array(key_frame, 9, zstd.default_threads())
    stream = build_stream(payload, table, (SHUFFLE_MARK if shuffled else 1, nt, H, W, 3), warm_up)
    return key_bytes, zstd.compress_array(stream, 9, zstd.default_threads())


def write_outputs(out_dir, frames, key, payload, table, warm_up, shuffled=False):
    key_bytes, entropy_bytes = pack_outputs(frames, key, payload, table, warm_up, shuffled)
    with open(os.path.join(out_dir, "key_frame.dat"), mode='wb') as f:
        f.write(key_bytes)
    with open(os.path.join(out_dir, "entropy.dat"), mode='wb') as f:
        f.write(entropy_bytes)
    return len(key_bytes), len(entropy_bytes)


class FrameSource:
    """compress.py:97-131 as a stream: the sorted image files of a directory decoded on a thread pool
    into a small ring of window-sized buffers (the reference appends every image to one growing
    array, compress.py:116-122).  Same acceptance rules and messages as load_images."""

    def __init__(self, data_dir):
        from PIL import Image, UnidentifiedImageError
        self.Image, self.errors = Image, (PermissionError, IndexError, UnidentifiedImageError, IsADirectoryError, ValueError)
        self.data_dir = data_dir
        self.paths = sorted(glob.glob(os.path.join(data_dir, '*')))
        if len(self.paths) == 0:
            print("ERROR:", data_dir, "is an empty or non-existent directory")
            exit()
        try:
            first = Image.open(self.paths[0])
            mode = first.mode
            if all([mode != 'RGB', mode != 'L']):
                print("ERROR: input image is {0}. Only RGB and grayscale are supported.".format(mode))
                exit()
            self.is_rgb = mode == 'RGB'
            self.W, self.H = first.size
        except self.errors:
            self.fail()
        self.nt = len(self.paths)
        self.files = [os.path.basename(p) for p in self.paths]

    def fail(self):
        print(self.data_dir, "contains files or folders that are not images.")
        exit()

    def _decode_into(self, dst, path):
        img = self.Image.open(path)
        arr = np.asarray(img if self.is_rgb else img.convert('RGB'))
        if arr.shape != dst.shape:  # another size or mode: np.array of such a list is not a stack (compress.py:122)
            raise ValueError(path)
        dst[...] = arr

    def chunks(self, per_chunk, pool, ring=3):
        """Yields (first frame index, uint8 (k,H,W,3) view) in order; a yielded buffer is reused
        `ring` chunks later, so the consumer must be done with it when it asks for the next one."""
        bufs = [np.empty((per_chunk, self.H, self.W, 3), np.uint8) for _ in range(ring)]
        starts = list(range(0, self.nt, per_chunk))

        def submit(ci):
            f0 = starts[ci]
            n = min(per_chunk, self.nt - f0)
            buf = bufs[ci % ring]
            return [pool.submit(self._decode_into, buf[j], self.paths[f0 + j]) for j in range(n)], buf[:n], f0

        pending = [submit(ci) for ci in range(min(ring - 1, len(starts)))]
        nxt = len(pending)
        while pending:
            futs, view, f0 = pending.pop(0)
            try:
                for ft in futs:
                    ft.result()
            except self.errors:
                self.fail()
            if nxt < len(starts):  # its buffer was handed out `ring` chunks ago
                pending.append(submit(nxt))
                nxt += 1
            yield f0, view


PAYLOAD_CHUNK = 8 << 20  # int16 elements fetched and fed to zstd at a time
KEY_PREFETCH_BYTES = 256 << 20  # key frames held on the host at once (more than that: streamed one by one)


STAGE_LOG = None   # a list installed by a caller (bench.py's host_pipeline leg): every run appends (run, stage, seconds)


class _Stages:
    """Stage wall times of compress.run / decompress.run: on stderr when TEZIP_TIMING is set (scripts/host_pipeline.py),
    into compress.STAGE_LOG when a caller installed a list there.  `add` records a duration measured elsewhere (a worker
    thread's: such a stage overlaps the ones marked around it)."""

    def __init__(self, run="compress"):
        self.on = bool(os.environ.get("TEZIP_TIMING"))
        self.run = run
        self.t0 = self.last = time.perf_counter()

    def add(self, name, seconds):
        if STAGE_LOG is not None:
            STAGE_LOG.append((self.run, name, float(seconds)))
        if self.on:
            import sys
            print("[tezip timing] %-34s %7.3f s  (overlapped)" % (name, seconds), file=sys.stderr)

    def mark(self, name, ctx=None):
        """ctx: the stage queued device work that may still be running -- when (and only when) stage times are wanted,
        wait for it, so that the time lands on the stage that queued it and not on the next one that synchronises."""
        if self.on or STAGE_LOG is not None:
            if ctx is not None:
                ctx.synchronize()
            now = time.perf_counter()
            if STAGE_LOG is not None:
                STAGE_LOG.append((self.run, name, now - self.last))
            if self.on:
                import sys
                print("[tezip timing] %-34s %7.3f s  (at %.3f s)" % (name, now - self.last, now - self.t0), file=sys.stderr)
            self.last = now


CODERS = ("zstd", "huff", "huffr", "huffd")
HUFF_PIECE = 16 << 20   # bytes of the coded stream fetched and written at a time


def check_coder(coder, shuffle=False, sharded=False):
    """The refusals of --coder, for tezip.py and for a direct caller of run(): None, or the message."""
    if coder not in CODERS:
        return "--coder takes one of %s, got %r" % (", ".join(CODERS), coder)
    if coder != "zstd" and shuffle:
        return "--coder %s cannot be combined with --shuffle (byte planes help zstd; a symbol coder codes whole symbols)" % coder
    if coder != "zstd" and sharded:
        return "--coder %s is not available for a sharded job (WORLD_SIZE > 1): run it on one GPU" % coder
    return None


def check_gray(gray, sharded=False):
    """The refusal of --gray that a direct caller of run() can meet (tezip.py knows the others): None, or the message."""
    if gray and sharded:
        return "--gray is not available for a sharded job (WORLD_SIZE > 1): run it on one GPU"
    return None


QUANT_NOT_SHARDED = "--quant lattice is not available for a sharded job (WORLD_SIZE > 1): run it on one GPU"


def check_quant(quant, sharded=False):
    """The refusals of --quant that a direct caller of run() can meet (tezip.py knows the others): None, or the message."""
    if quant not in lattice.QUANTS:
        return "--quant takes one of %s, got %r" % (", ".join(lattice.QUANTS), quant)
    if quant == "lattice" and sharded:
        return QUANT_NOT_SHARDED
    return None


def check_sdelta(mode, sharded=False):
    """The refusals of --sdelta that a direct caller of run() can meet (tezip.py knows the others): None, or the message."""
    if mode == sdauto.MODE:   # (its own refusals: sdauto.check)
        return None
    if mode not in sdelta.MODES:
        return "--sdelta takes one of %s, got %r" % (", ".join(sdelta.MODES + (sdauto.MODE,)), mode)
    if mode in ("channel", "plane") and sharded:
        return "--sdelta %s is not available for a sharded job (WORLD_SIZE > 1): run it on one GPU" % mode
    return None


PLANE_NO_RATIO = ("--sdelta plane cannot be combined with --target-ratio: the size probe's kernels form flat and channel-stride "
                  "symbols only, so it cannot size a plane payload")


def decide_sdelta(ctx, channels):
    """--sdelta channel once the payload's channel count is known: with three channels the context is set to the channel
    stride and True is returned; a one-channel payload (--gray on an all-gray job) has stride 1, which is the flat delta."""
    if channels == 3:
        ctx.set_delta_stride(1)
        print("sdelta: channel (stride 3)")
        return True
    print("sdelta: channel equals flat on a one-channel payload")
    return False


def decide_plane(ctx):
    """--sdelta plane: the context is set to the 2-D spatial delta TZ-SD2, whatever the payload's channel count (on one channel
    plane is NOT the flat delta)."""
    ctx.set_delta_plane(1)
    print("sdelta: plane (TZ-SD2)")
    return True


def decide_auto(ctx, channels, mode, bound, entropy, coder):
    """--sdelta auto once the bound is known (definition TZ-SDA1, tezip_amd/sdauto.py): one quantiser run sizes the job's
    entropy.dat under every layout the payload has (tz_sdelta_probe), the smallest is taken, and the context is set as
    `--sdelta <chosen>` sets it -- the setters only drop a resident payload, so they may follow the rollout.
    -> (strided, plane)."""
    chosen, sizes = sdauto.choose(ctx.sdelta_probe(mode, bound, entropy, coder), coder)
    print(sdauto.stdout_line(chosen, sizes))
    return chosen == "channel" and decide_sdelta(ctx, channels), chosen == "plane" and decide_plane(ctx)


def decide_gray(ctx, nt, files):
    """--gray after the frames are staged: one read of the resident stack says whether every frame is gray (tz_keys_gray over all
    of them).  Yes: the context is set to the one-channel payload and 1 is returned.  No: 3, and nothing changes -- the flag
    never fails a job and never loses information."""
    gray = ctx.keys_gray(range(nt))
    if gray.all():
        ctx.set_payload_channels(1)
        print("gray: yes, payload stores 1 of 3 channels")
        return 1
    i = int(np.nonzero(~gray)[0][0])
    print("gray: no (frame %d %s has colour), payload keeps three channels" % (i, files[i]))
    return 3


KEY_CODERS = ("zstd", "huff", "huffg")


def check_key_coder(key_coder, sharded=False):
    """The refusals of --key-coder, for tezip.py and for a direct caller of run(): None, or the message."""
    if key_coder not in KEY_CODERS:
        return "--key-coder takes one of %s, got %r" % (", ".join(KEY_CODERS), key_coder)
    if key_coder != "zstd" and sharded:
        return "--key-coder %s is not available for a sharded job (WORLD_SIZE > 1): run it on one GPU" % key_coder
    return None


def _write_coded(path, front, nbytes, get, label, t0):
    """The file of a coder whose stream is resident on the device: `front`, then the nbytes of the stream, fetched by
    get(offset, count, out=) piece by piece into two buffers in turn.  label: what to print the time since t0 under."""
    bufs = [np.empty(min(HUFF_PIECE, nbytes), np.uint8) for _ in range(2)]
    with open(path, mode='wb') as f:
        f.write(front)
        for k, off in enumerate(range(0, nbytes, HUFF_PIECE)):
            cnt = min(HUFF_PIECE, nbytes - off)
            f.write(get(off, cnt, out=bufs[k % 2][:cnt]))
    if label:
        print("{0}:{1}".format(label, time.perf_counter() - t0) + "[sec]")
    return len(front) + nbytes


def _huff_key_file(ctx, path, nt, H, W, key_idx, verbose):
    """key_frame.dat of KEY_CODER="huff": the key frames of the resident stack are counted under the four predictors, the
    predictors and the one code are chosen here (keycoder.choose_predictors, tz_huff_lengths), the device codes them
    (tz_keys_encode) and only the coded stream crosses to the host -- no zero frame, no raw key frame, no zstd."""
    t0 = time.perf_counter()
    counts = ctx.keys_counts(key_idx)
    pred = keycoder.choose_predictors(counts)
    lengths = huff.code_lengths(keycoder.chosen_counts(counts, pred))
    nbytes = ctx.keys_encode(key_idx, pred, lengths)
    n = len(key_idx) * H * W * 3
    nruns, nchunks = huff.geometry(n)
    front = keycoder.pack_front(nt, H, W, key_idx, pred, lengths, nchunks, (nbytes - huff.body_bytes(n, 0)) // 4)
    return _write_coded(path, front, nbytes, ctx.keys_get, "key_coding" if verbose else None, t0)


def _huffg_key_file(ctx, path, nt, H, W, key_idx, verbose):
    """key_frame.dat of KEY_CODER="huffg" (TZK2): as _huff_key_file, and one more read of the key frames says which of them
    are gray (tz_keys_gray); those are counted, coded and stored as one channel (keycoderg.gray_counts: the three-channel
    counts divided by 3, the same integers keycoderg.encode_file uses)."""
    t0 = time.perf_counter()
    gray = ctx.keys_gray(key_idx)
    counts = keycoderg.gray_counts(ctx.keys_counts(key_idx), gray)
    predg = keycoderg.pred_bytes(counts, gray)
    lengths = huff.code_lengths(keycoderg.chosen_counts(counts, predg))
    nbytes = ctx.keysg_encode(key_idx, predg, lengths)
    n = keycoderg.offsets(gray, H, W)[1]
    nruns, nchunks = huff.geometry(n)
    front = keycoderg.pack_front(nt, H, W, key_idx, predg, lengths, nchunks, (nbytes - huff.body_bytes(n, 0)) // 4)
    return _write_coded(path, front, nbytes, ctx.keysg_get, "key_coding" if verbose else None, t0)


class _Done:
    """A finished piece of work where a future is expected."""

    def __init__(self, value):
        self.value = value

    def result(self):
        return self.value


# CODER -> (the format's module, whether the coder chooses a match distance); the name is also the prefix of the Context's methods
_HUFF_CODERS = {"huff": (huff, False), "huffr": (huffr, False), "huffd": (huffd, True)}


def _huff_entropy_file(ctx, path, n, trailer, verbose, coder="huff"):
    """entropy.dat of CODER="huff" / "huffr" / "huffd": the resident payload is coded on the device (tz_huff_encode /
    tz_huffr_encode / tz_huffd_encode) and only the coded stream crosses to the host; the header, the reference trailer and the
    code lengths go in front of it.  huffd: one read of the payload counts it under the three match distances, the distance
    and its code are chosen here from those counts (huffd.choose), and one line says which."""
    t0 = time.perf_counter()
    fmt, has_dist = _HUFF_CODERS[coder]
    counts, base = getattr(ctx, coder + "_counts")()
    if has_dist:
        dist, lengths, costs = fmt.choose(counts)
        print("coder: huffd, match distance %d (bits: none %d, 1: %d, 3: %d)" % ((dist,) + tuple(costs)))
        extra = (dist,)                               # (what encode and pack_front take behind the other coders' arguments)
    else:
        extra, lengths = (), fmt.code_lengths(counts)
    nbytes = getattr(ctx, coder + "_encode")(lengths, base, *extra)
    nruns, nchunks = huff.geometry(n)
    front = fmt.pack_front(trailer, lengths, base, n, nchunks, (nbytes - huff.body_bytes(n, 0)) // 4, *extra)
    # (the three coders leave ONE resident stream: huffr_get and huffd_get are other names of huff_get)
    return _write_coded(path, front, nbytes, ctx.huff_get, "huffman_coding" if verbose else None, t0)


def _key_output(ctx, out_dir, nt, H, W, key, pool, stages=None, verbose=False, key_coder="zstd"):
    """key_frame.dat (compress.py:271-278) from the context-resident frames -> a future of its size.  Nothing of it depends on
    the payload: _stream_outputs starts it in front of entropy.dat, a --target-ratio job in front of its search."""
    n_key = nt * H * W * 3
    key_idx = [int(i) for i in np.nonzero(key)[0]]
    zero = np.zeros((H, W, 3), np.uint8)
    if key_coder in ("huff", "huffg"):
        # few key frames or all of them (-w 1): one path, the stack never leaves the device
        t_k = time.perf_counter()
        key_file_of = _huffg_key_file if key_coder == "huffg" else _huff_key_file
        kf = _Done(key_file_of(ctx, os.path.join(out_dir, "key_frame.dat"), nt, H, W, key_idx, verbose))
        if stages:
            stages.add("key-frame coding + fetch key_frame.dat", time.perf_counter() - t_k)
    elif len(key_idx) * H * W * 3 <= KEY_PREFETCH_BYTES:
        # the usual case, a few key frames: fetched up front, key_frame.dat is compressed by a worker while the
        # payload is fetched and compressed here (the context is not thread-safe: the worker never touches it)
        key_frames = {i: ctx.frames_get(i, 1)[0] for i in key_idx}

        def key_file():
            t0 = time.perf_counter()
            with open(os.path.join(out_dir, "key_frame.dat"), mode='wb') as f:
                sc = zstd.StreamCompressor(f, n_key, 9, max(1, zstd.default_threads() // 4))
                for i in range(nt):
                    sc.write(key_frames.get(i, zero))
                size = sc.close()
            if stages:
                stages.add("zstd-9 key_frame.dat (worker)", time.perf_counter() - t0)
            return size

        kf = pool.submit(key_file)
    else:
        # many key frames (-w 1, DWP with a tiny threshold: up to the whole stack): one at a time through
        # frames_get, written before entropy.dat -- host memory stays independent of the number of frames
        is_key = set(key_idx)
        with open(os.path.join(out_dir, "key_frame.dat"), mode='wb') as f:
            sc = zstd.StreamCompressor(f, n_key, 9, zstd.default_threads())
            for i in range(nt):
                sc.write(ctx.frames_get(i, 1)[0] if i in is_key else zero)
            ksize = sc.close()
        kf = _Done(ksize)
    return kf


def _entropy_output(ctx, out_dir, nt, H, W, table, warm_up, shuffled, stages=None, coder="zstd", verbose=False, channels=3, strided=False,
                    plane=False, closed=False):
    """entropy.dat (compress.py:375-400) from the context-resident payload, piece by piece -> its size.  channels, strided,
    plane, closed: as _stream_outputs'."""
    n = nt * H * W * channels
    if table is not None:
        tail = np.concatenate([table.astype(np.int64), [len(table)]])
    else:
        tail = np.array([-1], dtype=np.int64)
    one = sdelta.mark(shuffled, plane) if strided or plane else (SHUFFLE_MARK if shuffled else 1)
    if closed:   # (2: closed-loop prediction with per-tile selection TZ-PS1, tezip_amd/predselect.py: 32 more; 3: with
        # motion-compensated tiles TZ-PM1, tezip_amd/predmotion.py: 64 more)
        one += closedloop.MARK_CLOSED + (predselect.MARK_SELECT if closed == 2 else predmotion.MARK_MOTION if closed == 3 else 0)
    trailer = np.concatenate([tail, [one, nt, H, W, channels], [warm_up]]).astype(np.int16)
    t_e = time.perf_counter()
    if coder in ("huff", "huffr", "huffd"):
        esize = _huff_entropy_file(ctx, os.path.join(out_dir, "entropy.dat"), n, trailer, verbose, coder)
        if stages:
            stages.add("huffman coding + fetch entropy.dat", time.perf_counter() - t_e)
        return esize
    bufs = [np.empty(min(PAYLOAD_CHUNK, n), np.int16) for _ in range(2)]
    with open(os.path.join(out_dir, "entropy.dat"), mode='wb') as f:
        sc = zstd.StreamCompressor(f, n * 2 + trailer.nbytes, 9, zstd.default_threads())
        for k, off in enumerate(range(0, n, PAYLOAD_CHUNK)):
            cnt = min(PAYLOAD_CHUNK, n - off)
            piece = ctx.payload_get(off, cnt, out=bufs[k % 2][:cnt])
            sc.write(piece)
        sc.write(trailer)
        esize = sc.close()
    if stages:
        stages.add("payload fetch + zstd-9 entropy.dat", time.perf_counter() - t_e)
    return esize


def _stream_outputs(ctx, out_dir, nt, H, W, key, table, warm_up, shuffled, pool, stages=None, coder="zstd", verbose=False,
                    key_coder="zstd", channels=3, strided=False, plane=False, closed=False):
    """key_frame.dat and entropy.dat (compress.py:271-278, 375-400) from the context-resident frames
    and payload, piece by piece: nothing of size nt*H*W lives on the host.  channels: what the resident payload stores per
    pixel (1: a gray job, tezip_amd/graypayload.py); key_frame.dat has three either way.  strided: the payload's spatial delta
    ran at the channel stride, plane: it is the 2-D one, TZ-SD2 (tezip_amd/sdelta.py): the trailer says so in the first entry of
    its shape.  closed: the job ran closed-loop prediction TZ-CL1 (tezip_amd/closedloop.py): that entry is 16 larger; closed == 2:
    with per-tile selection TZ-PS1 (tezip_amd/predselect.py): 48 larger; closed == 3: with motion-compensated tiles TZ-PM1
    (tezip_amd/predmotion.py): 80 larger."""
    kf = _key_output(ctx, out_dir, nt, H, W, key, pool, stages, verbose, key_coder)
    esize = _entropy_output(ctx, out_dir, nt, H, W, table, warm_up, shuffled, stages, coder, verbose, channels, strided, plane, closed)
    return kf.result(), esize


def _accept_job(src, model_shape, warm_up, shuffle, out_dir, levels=1):
    """The checks of a compression job, in this order, each refusal with its message and exit(): the frame size against
    the model's and against its number of levels, the number of frames, --shuffle's multiple of 8.  The accepted job then
    makes out_dir (None: not this process) and writes filename.txt into it: compress.py:133-136 writes it after the images
    are loaded, and a rejected job leaves no directory behind.  Returns the padded frame size."""
    nt, H, W = src.nt, src.H, src.W
    hp, wp = padding_shape(H, W)
    if model_shape is not None and (model_shape[0] != hp or model_shape[1] != wp):
        print("ERROR:Image size is out of scope for this model.")
        print("Compatible sizes for this model are height", model_shape[0] - 7, "to", model_shape[0], "and width",
              model_shape[1] - 7, "to", model_shape[1])
        exit()
    # every level halves the frame: a model of more than four levels needs more than the padding to 8 gives
    # (tz_model_prepare refuses such a size; said here in the reference's words, before anything is written)
    if hp % (1 << (levels - 1)) or wp % (1 << (levels - 1)):
        print("ERROR:Image size is out of scope for this model.")
        print("A model of %d levels needs a padded size that divides by %d: %dx%d does not" % (levels, 1 << (levels - 1), hp, wp))
        exit()
    if nt < warm_up + 2:
        print("ERROR: need at least warm_up+2 images (%d given, warm_up %d)." % (nt, warm_up))
        exit()
    if shuffle and (nt * H * W * 3) % 8:
        print("ERROR: --shuffle needs nt*H*W*3 to be a multiple of 8 (%d x %d x %d x 3 is not)." % (nt, H, W))
        exit()
    if out_dir is not None:
        if not os.path.exists(out_dir):
            os.mkdir(out_dir)
        with open(os.path.join(out_dir, 'filename.txt'), 'w', encoding='UTF-8') as f:
            f.write(f"{int(src.is_rgb)}\n")
            for file_name in src.files:
                f.write("%s\n" % file_name)
    return hp, wp


SSIM_NEEDS_REPORT = "--ssim extends the compression report: add --report"
TARGET_NEEDS_ABS = "--target-psnr finds the abs bound itself: it takes the place of -m and -b"
TARGET_NOT_SHARDED = "--target-psnr is not available for a sharded job (WORLD_SIZE > 1): run it on one GPU"
RATIO_NEEDS_ABS = "--target-ratio finds the abs bound itself: it takes the place of -m, -b and --target-psnr"
RATIO_NOT_SHARDED = "--target-ratio is not available for a sharded job (WORLD_SIZE > 1): run it on one GPU"
RATIO_NEEDS_CODER = ("--target-ratio needs a coder whose file size is an exact function of counts (zstd's is not known without "
                     "running zstd): add --coder huffd")
RATIO_NO_SHUFFLE = "--target-ratio cannot be combined with --shuffle (byte planes are not Huffman-coded)"


def check_ratio(ratio, mode, bound, target_psnr, coder, shuffle, sharded):
    """The refusals of --target-ratio that tezip.py and a direct caller of run() share: None, or the message."""
    return (ratetarget.check_target(ratio) or (RATIO_NEEDS_ABS if mode != "abs" or bound or target_psnr is not None else None)
            or (RATIO_NOT_SHARDED if sharded else None) or (RATIO_NO_SHUFFLE if shuffle else None)
            or (RATIO_NEEDS_CODER if coder not in ratetarget.CODERS else None))


def run(WEIGHTS_DIR, DATA_DIR, OUTPUT_DIR, PREPROCESS, WINDOW_SIZE, THRESHOLD, MODE, BOUND_VALUE, GPU_FLAG, VERBOSE,
        ENTROPY_RUN, device=0, SHUFFLE=False, REPORT=False, CODER="zstd", KEY_CODER="zstd", DIGESTS=False, GRAY=False, SDELTA="flat",
        SSIM=False, TARGET_PSNR=None, TARGET_RATIO=None, PER_FRAME=False, FRAME_BOUNDS=None, QUANT="greedy", BOUND_MAP=None,
        LOOP="open", PRED="net", LOOP_PSNR=None, LOOP_BOUNDS=None, LOOP_MAP=None):
    """SHUFFLE (--shuffle; NOT in the reference): store the payload as byte planes.  Off by default:
    a shuffled entropy.dat is flagged in its trailer and is not readable by the reference.
    REPORT (--report; NOT in the reference): also write quality.json -- per frame and for the sequence the error the
    bound introduced, from the stored payload decoded on the device (tz_encode_quality) -- and print the worst error,
    the PSNR and the compression ratio.  Single-GPU jobs only.
    CODER (--coder; NOT in the reference): "zstd" writes the reference's entropy.dat; "huff" has the GPU Huffman-code the
    payload (tezip_amd/huff.py), "huffr" the same over literals and period-3 repeat tokens (tezip_amd/huffr.py), "huffd" the same
    with the match distance (none, 1 or 3) chosen per file from exact counts (tezip_amd/huffd.py) -- such a
    file is not readable by the reference; `-u` recognises it by its magic.
    Single-GPU jobs only, not with SHUFFLE.
    KEY_CODER (--key-coder; NOT in the reference): "zstd" writes the reference's key_frame.dat; "huff" has the GPU code the
    key frames alone as predictor residuals under a Huffman code (tezip_amd/keycoder.py) -- not readable by the reference,
    `-u` recognises it by its magic; smaller than zstd-9 on smooth frames and larger on sparse ones.  "huffg" is "huff"
    with every gray key frame (three equal channels: a single-channel source) coded as one channel
    (tezip_amd/keycoderg.py).  Independent of CODER and SHUFFLE.  Single-GPU jobs only.
    DIGESTS (--digests; NOT in the reference): also write frame_digests.json (tezip_amd/digest.py) -- per frame the digest
    of what the stored payload decodes to and of the source frame, both taken on the device (tz_encode_digests); `-u`
    verifies its frames against them before it writes an image.  The other files are byte for byte what they are without
    it; the file is written last.  Single-GPU jobs only.
    GRAY (--gray; NOT in the reference): when every frame of the job is gray (three equal channels: a single-channel source
    widened to RGB), entropy.dat stores one payload channel instead of three (tezip_amd/graypayload.py) -- such a file is
    not readable by the reference, `-u` recognises it by the shape in its trailer.  Decided after the frames are staged; a job
    with colour writes exactly the files it writes without the flag.  Works with every CODER, KEY_CODER, SHUFFLE, REPORT and
    DIGESTS.  Single-GPU jobs only.
    SDELTA (--sdelta; NOT in the reference): "flat" (the default: every file, line and launch is what it is without it) or
    "plane": the spatial delta of the payload is the 2-D one, TZ-SD2 (left + up - upleft per frame and channel, wrapped to nine
    bits; tezip_amd/sdelta.py): mark 8 in the trailer, 9 with byte planes, with three channels or one; not with TARGET_RATIO; or
    "auto" (CODER "huff", "huffr" or "huffd", no SHUFFLE, no TARGET_RATIO; definition TZ-SDA1, tezip_amd/sdauto.py): once the bound
    is known, one tz_sdelta_probe on the rollout gives the exact size of entropy.dat under every layout the payload has, and the
    job goes on as the SDELTA of the smallest (a tie: the earlier of flat, channel, plane): every file is that job's; or
    "channel": the spatial delta of a three-channel payload is taken at the channel stride (tezip_amd/sdelta.py); only the
    lossless back half of the coder changes, so the job decodes to exactly the images it decodes to without it.  `-u`
    recognises the stream by the mark in its trailer.  On a one-channel payload (GRAY on an all-gray job) the stride is 1 and
    the files are those of GRAY alone.  Works with every CODER, KEY_CODER, SHUFFLE, REPORT, SSIM and DIGESTS.  Single-GPU jobs only.
    SSIM (--ssim; NOT in the reference; with REPORT only): the report also carries the structural similarity of what the
    stored payload decodes to against the sources (definition TZ-SSIM-1: tezip_amd/ssim.py), from one tz_encode_ssim call on
    the same resident payload; a fourth line is printed.  Every other file is what it is without it.
    TARGET_PSNR (--target-psnr; NOT in the reference; MODE "abs" and an empty BOUND_VALUE): the abs bound is found on the device
    after the rollout (definition TZ-TPSNR-1: tezip_amd/target.py; at most 9 tz_bound_probe calls on the one rollout) and the job
    goes on as `-m abs -b <found>`: every file is what that job writes, one line says what was found, and bound_search.json
    (target, limit, the probes, the result) is written besides.  Works with every other flag above.  Single-GPU jobs only.
    With VERBOSE the quantiser time printed as error_bound includes the probes'.
    TARGET_RATIO (--target-ratio; NOT in the reference; MODE "abs", an empty BOUND_VALUE, no TARGET_PSNR, CODER "huff", "huffr" or
    "huffd", no SHUFFLE): the abs bound is found on the device for "the files may take raw / TARGET_RATIO bytes" (definition
    TZ-TRATIO-1: tezip_amd/ratetarget.py).  key_frame.dat is written in front of the search, whose budget it counts against; at
    most 11 tz_size_probe calls on the one rollout give the exact size of every candidate's entropy.dat; the job goes on as
    `-m abs -b <found>`: every file is what that job writes, one line says what was found, and bound_search.json (target,
    budget, the probes, the result) is written besides.  A target that abs 255 misses: the message, bound_search.json with a
    null result, no entropy.dat, exit status 4.  Works with every KEY_CODER, GRAY, SDELTA, REPORT, SSIM and DIGESTS.
    Single-GPU jobs only.
    PER_FRAME (--per-frame; NOT in the reference; with TARGET_PSNR only): the target holds in EVERY frame that is not stored
    exactly (definition TZ-TPSNR-F1: tezip_amd/frametarget.py): every such frame gets an abs bound of its own from a
    bisection of its own, all of them driven by the same at most 9 tz_bound_probe calls, and the job runs under
    tz_set_frame_bounds.  The files are those of the reference's format (the decoder never sees a bound); bound_search.json
    lists the bounds.  Works with every flag TARGET_PSNR works with.  Single-GPU jobs only.
    FRAME_BOUNDS (--frame-bounds; NOT in the reference; MODE "abs", an empty BOUND_VALUE, no target): the path of a JSON file (a
    list of numbers or an object with a "frame_bounds" list, so that a per-frame search's bound_search.json replays) or a
    sequence: one abs bound per image, finite and >= 0; entries at frame 0, warm-up and key frames are taken as 0.  The
    job runs under tz_set_frame_bounds.  Single-GPU jobs only.
    QUANT (--quant; NOT in the reference): "greedy" (the default: every file, line and launch is what it is without it) is
    the reference's quantiser (compress.py:23-70); "lattice" quantises every delta on its own by definition TZ-QL1
    (tezip_amd/lattice.py) under the same tolerance: one line says so, tezip_amd.json and bound_search.json record it, and the
    files are ordinary ones -- the payload holds the quantised deltas themselves, `-u` needs no flag and does not read the
    record.  Smaller than greedy on data that is not smooth, LARGER on sparse frames at loose bounds (README).  The probes of
    TARGET_PSNR, PER_FRAME and TARGET_RATIO quantise the same way.  Works with every flag above.  Single-GPU jobs only.

    BOUND_MAP (--bound-map; NOT in the reference; MODE "abs", an empty BOUND_VALUE, no target, no FRAME_BOUNDS): the path of a map
    of the images' own size (a .npy with a 2-D uint8 array, or an image with one channel or three equal ones) or such an array:
    one abs bound per pixel, for all three channels in every frame the encoder quantises (definition TZ-BM1:
    tezip_amd/boundmap.py).  The job runs under tz_set_bound_map.  The files are ordinary ones (the decoder never sees a bound);
    one line describes the map, tezip_amd.json records its maximum and its exact pixels (`-u` does not read them), and with
    REPORT quality.json carries the violations per frame (0, or a bug) from tz_encode_map_check on the resident payload: any
    violation is one ERROR line per frame and exit status 3.  Works with every QUANT, CODER, KEY_CODER, SHUFFLE, GRAY, SDELTA,
    REPORT, SSIM and DIGESTS.  Single-GPU jobs only.

    LOOP (--loop; NOT in the reference): "open" (the default: every file, line and launch is what it is without it) feeds the
    predictor its own last prediction inside a window (compress.py:230); "closed" feeds it the DECODED frame in front, definition
    TZ-CL1 (tezip_amd/closedloop.py): the rollout is tz_rollout_closed under the job's mode, bound and quantiser, every prediction
    is a one-step prediction, and the unchanged back half stores the loop's quantised deltas.  One line says so, tezip_amd.json
    records it, and the first entry of the trailer's shape is 16 larger; `-u` recognises the stream by that mark.  WINDOW_SIZE
    only (no THRESHOLD), MODE "abs", lossless or with QUANT "lattice"; not with GRAY, TARGET_PSNR, TARGET_RATIO, PER_FRAME,
    FRAME_BOUNDS or BOUND_MAP (a target's probes assume predictions that do not depend on the bound).  Works with every SDELTA,
    CODER, KEY_CODER, SHUFFLE, REPORT, SSIM and DIGESTS.  VERBOSE prints no per-step MSE lines.  Single-GPU jobs only.

    LOOP_PSNR (--loop-psnr; NOT in the reference; LOOP "closed", QUANT "lattice", MODE "abs", an empty BOUND_VALUE): a PSNR in dB
    that every frame not stored exactly must reach, definition TZ-CLF1 (tezip_amd/closedframes.py): the ONE closed-loop rollout
    (tz_rollout_closed_frames) finds every frame's abs bound when the loop stands at that frame, by a bisection that stays on the
    device.  One line says so, bound_search.json holds the search, and the job then runs under tz_set_frame_bounds with the bounds
    found; `-u` takes no flag.  LOOP_BOUNDS (--loop-bounds): the bounds given instead -- a path or a sequence as FRAME_BOUNDS
    takes them (a bound_search.json replays).  Not with PRED "select" / "motion", nor with anything LOOP "closed" refuses.

    LOOP_MAP (--loop-map; NOT in the reference; LOOP "closed", QUANT "lattice", MODE "abs", an empty BOUND_VALUE): one abs bound per
    pixel for the closed loop, definition TZ-CLM1 (tezip_amd/closedmap.py) -- a path as BOUND_MAP takes it, or a 2-D uint8 array of
    the images' own size.  The closed-loop rollout (tz_rollout_closed_map) decodes every pixel under its own tolerance, with PRED
    "select" the tiles are chosen under the map, and the job then runs under tz_set_bound_map with that map; `-u` takes no flag.
    tezip_amd.json is the closed job's plus BOUND_MAP's informational "bound_map"; with REPORT quality.json gains BOUND_MAP's
    object and the per-frame violations.  Not with PRED "motion", BOUND_MAP, LOOP_PSNR or LOOP_BOUNDS, nor with anything LOOP
    "closed" refuses.

    PRED (--pred; NOT in the reference): "net" (the default: every file, line and launch is what it is without it) or, with LOOP
    "closed", "select": every 16 x 16 tile of a predicted frame takes whichever of the network's prediction and the decoded frame
    in front leaves the smaller quantised residual, definition TZ-PS1 (tezip_amd/predselect.py).  One line says how many tiles
    took the frame in front, a fifth file pred_modes.dat holds one bit per tile, tezip_amd.json records it, and the first entry of
    the trailer's shape is 48 larger than the open-loop mark; `-u` recognises the stream by that mark.  REPORT counts the file in
    `ratio:` and adds "pred_select" to quality.json.  Everything LOOP "closed" refuses stays refused.  Or "motion": the frame in
    front is displaced per tile by a vector of up to 7 pixels found by a full search, definition TZ-PM1 (tezip_amd/predmotion.py);
    the line also counts the displaced tiles, pred_modes.dat (format TZP2) also holds one byte per chosen tile, the mark is 80
    larger than the open-loop one and quality.json gains "pred_motion".

    One process: the images stream through a ring of window buffers into HBM while the model loads,
    and key_frame.dat / entropy.dat are written from context-resident data in pieces, so host memory
    does not grow with the number of frames.  Under torch.distributed.run the windows are sharded
    over the ranks (tezip_amd/dist.py) from a stack that every rank loads."""
    if not GPU_FLAG:
        print("ERROR: this build runs the compression path on an AMD MI355X only (no CPU path).")
        exit()
    if TARGET_RATIO is not None:   # (tezip.py refuses this before any GPU is touched; a caller of run() gets the same answer)
        problem = check_ratio(TARGET_RATIO, MODE, BOUND_VALUE, TARGET_PSNR, CODER, SHUFFLE, tzdist.active() is not None)
        if problem:
            print("ERROR:", problem)
            sys.exit(2)
    problem = (check_coder(CODER, SHUFFLE, tzdist.active() is not None) or check_key_coder(KEY_CODER, tzdist.active() is not None)
               or check_gray(GRAY, tzdist.active() is not None) or check_sdelta(SDELTA, tzdist.active() is not None))
    if problem:   # (tezip.py refuses this before any GPU is touched; a caller of run() gets the same answer)
        print("ERROR:", problem)
        sys.exit(2)
    if SDELTA == "plane" and TARGET_RATIO is not None:   # likewise
        print("ERROR:", PLANE_NO_RATIO)
        sys.exit(2)
    if SDELTA == sdauto.MODE:   # likewise
        problem = sdauto.check(CODER, SHUFFLE, tzdist.active() is not None, TARGET_RATIO)
        if problem:
            print("ERROR:", problem)
            sys.exit(2)
    if SSIM and not REPORT:   # (tezip.py refuses this before any GPU is touched; a caller of run() gets the same answer)
        print("ERROR:", SSIM_NEEDS_REPORT)
        sys.exit(2)
    problem = check_quant(QUANT, tzdist.active() is not None)
    if problem:   # likewise
        print("ERROR:", problem)
        sys.exit(2)
    loop_map = None
    if LOOP_MAP is not None:   # likewise (in front of every other check: a refusal of this job names the flag that defines it)
        problem = closedmap.check_flags(LOOP_MAP, LOOP, QUANT, MODE, BOUND_VALUE, PRED, True, False, tzdist.active() is not None, GRAY,
                                        THRESHOLD, TARGET_PSNR, TARGET_RATIO, PER_FRAME, FRAME_BOUNDS, BOUND_MAP, LOOP_PSNR, LOOP_BOUNDS)
        if not problem:
            try:
                loop_map = closedmap.load(LOOP_MAP)
            except ValueError as e:
                problem = str(e)
        if problem:
            print("ERROR:", problem)
            sys.exit(2)
    loop_frames = LOOP_PSNR is not None or LOOP_BOUNDS is not None
    loop_bounds = None
    if loop_frames:   # likewise (in front of --loop's check: a refusal of this job names the flag that defines it)
        problem = closedframes.check_flags(LOOP_PSNR, LOOP_BOUNDS, LOOP, QUANT, None if LOOP_PSNR is not None and MODE == "abs" else MODE,
                                           BOUND_VALUE, PRED, True, False, tzdist.active() is not None, GRAY, THRESHOLD, TARGET_PSNR,
                                           TARGET_RATIO, PER_FRAME, FRAME_BOUNDS, BOUND_MAP)
        if not problem and LOOP_BOUNDS is not None:
            try:
                loop_bounds = closedframes.load(LOOP_BOUNDS)
            except ValueError as e:
                problem = str(e)
        if problem:
            print("ERROR:", problem)
            sys.exit(2)
    problem = closedloop.check_flags(LOOP, MODE, BOUND_VALUE, QUANT, THRESHOLD, False, tzdist.active() is not None, GRAY, TARGET_PSNR,
                                     TARGET_RATIO, PER_FRAME, FRAME_BOUNDS, BOUND_MAP)
    if problem:   # likewise
        print("ERROR:", problem)
        sys.exit(2)
    problem = predmotion.check_flags(PRED, LOOP)
    if problem:   # likewise
        print("ERROR:", problem)
        sys.exit(2)
    closed = LOOP == "closed"
    select = PRED == "select"
    motion = PRED == "motion"
    if TARGET_PSNR is not None:   # (tezip.py refuses this before any GPU is touched; a caller of run() gets the same answer)
        problem = (target.check_target(TARGET_PSNR) or (TARGET_NEEDS_ABS if MODE != "abs" or BOUND_VALUE else None)
                   or (TARGET_NOT_SHARDED if tzdist.active() is not None else None))
        if problem:
            print("ERROR:", problem)
            sys.exit(2)
    frame_bounds = None
    if PER_FRAME or FRAME_BOUNDS is not None:   # (tezip.py refuses this before any GPU is touched; a caller of run() gets the same answer)
        problem = frametarget.check(PER_FRAME, FRAME_BOUNDS, MODE, BOUND_VALUE, TARGET_PSNR, TARGET_RATIO, tzdist.active() is not None)
        if not problem and FRAME_BOUNDS is not None:
            try:
                frame_bounds = frametarget.load(FRAME_BOUNDS)
            except ValueError as e:
                problem = str(e)
        if problem:
            print("ERROR:", problem)
            sys.exit(2)
    bound_map = None
    if BOUND_MAP is not None:   # (tezip.py refuses this before any GPU is touched; a caller of run() gets the same answer)
        problem = boundmap.check_flags(BOUND_MAP, MODE, BOUND_VALUE, TARGET_PSNR, TARGET_RATIO, PER_FRAME, FRAME_BOUNDS,
                                       tzdist.active() is not None)
        if not problem:
            try:
                bound_map = boundmap.load(BOUND_MAP) if isinstance(BOUND_MAP, (str, os.PathLike)) else np.ascontiguousarray(BOUND_MAP)
                if bound_map.dtype != np.uint8 or bound_map.ndim != 2:
                    raise ValueError("bound map BOUND_MAP is a %s array of shape %s: a map is a 2-D uint8 array" % (bound_map.dtype, bound_map.shape))
            except ValueError as e:
                problem = str(e)
        if problem:
            print("ERROR:", problem)
            sys.exit(2)
    if tzdist.active() is not None:
        if REPORT:   # (tezip.py refuses this before any GPU is touched; a caller of run() gets the same answer)
            print("ERROR: --report is not available for a sharded job (WORLD_SIZE > 1): run it on one GPU")
            sys.exit(2)
        if DIGESTS:  # likewise
            print("ERROR: --digests is not available for a sharded job (WORLD_SIZE > 1): run it on one GPU")
            sys.exit(2)
        return _run_sharded(WEIGHTS_DIR, DATA_DIR, OUTPUT_DIR, PREPROCESS, WINDOW_SIZE, THRESHOLD, MODE, BOUND_VALUE,
                            VERBOSE, ENTROPY_RUN, device, SHUFFLE, CODER)
    stages = _Stages()
    src = FrameSource(DATA_DIR)
    nt, H, W = src.nt, src.H, src.W
    if frame_bounds is not None:   # known once the directory is listed: before the model, the context and the rollout
        problem = frametarget.check_length(frame_bounds, nt, FRAME_BOUNDS)
        if problem:
            print("ERROR:", problem)
            sys.exit(2)
    if loop_bounds is not None:   # likewise
        problem = closedframes.check_length(loop_bounds, nt, LOOP_BOUNDS)
        if problem:
            print("ERROR:", problem)
            sys.exit(2)
    if loop_map is not None:   # likewise
        problem = closedmap.check_size(loop_map, H, W, LOOP_MAP if isinstance(LOOP_MAP, (str, os.PathLike)) else "LOOP_MAP")
        if problem:
            print("ERROR:", problem)
            sys.exit(2)
    if bound_map is not None:   # likewise
        problem = boundmap.check_size(bound_map, H, W, BOUND_MAP if isinstance(BOUND_MAP, (str, os.PathLike)) else "BOUND_MAP")
        if problem:
            print("ERROR:", problem)
            sys.exit(2)
    per_chunk = max(1, min(WINDOW_SIZE or 16, 64))
    with ThreadPoolExecutor(max_workers=io_threads() + 1) as pool:
        chunks = src.chunks(per_chunk, pool)   # decoding starts with the first next(); model + HIP start-up overlap it
        stages.mark("list + probe")
        head = next(chunks)
        stages.mark("first window decoded")
        cfg, wts, model_shape = open_model(WEIGHTS_DIR)
        stages.mark("model directory read")
        hp, wp = _accept_job(src, model_shape, PREPROCESS, SHUFFLE, OUTPUT_DIR, cfg.nb_layers)
        nwin = 1 if WINDOW_SIZE is None else max(1, (nt - PREPROCESS + WINDOW_SIZE - 1) // WINDOW_SIZE)
        ctx = make_context(cfg, wts, hp, wp, min(nwin, 64), device)
        stages.mark("context + model prepare")
        try:
            ctx.frames_begin(nt, H, W)
            ctx.frames_put(*head)
            for f0, view in chunks:
                ctx.frames_put(f0, view)   # pageable ring buffer: free again when the call returns
            stages.mark("remaining windows decoded + staged", ctx)
            channels = 3
            if GRAY:
                channels = decide_gray(ctx, nt, src.files)
                stages.mark("gray check (device)")
            strided = SDELTA == "channel" and decide_sdelta(ctx, channels)
            plane = SDELTA == "plane" and decide_plane(ctx)
            sd_mode = "plane" if plane else ("channel" if strided else "flat")
            if QUANT == "lattice":   # the probes of the searches below and the job itself quantise by TZ-QL1
                ctx.set_quantiser("lattice")
                print(lattice.STDOUT_LINE)
            if VERBOSE:
                ctx.prof_enable(True)
            t0 = time.time()
            if closed and loop_frames:   # TZ-CLF1: TZ-CL1 under one abs bound per frame, given or found inside the one rollout
                print(closedloop.STDOUT_LINE)
                if LOOP_PSNR is not None:
                    limit = target.sse_limit(LOOP_PSNR, H * W * 3)
                    key = (ctx.rollout_closed_frames(None, PREPROCESS, WINDOW_SIZE, sse_limit=limit) if limit > 0 else
                           ctx.rollout_closed_frames(None, PREPROCESS, WINDOW_SIZE, bounds=[0.0] * nt))   # (the lossless job: no probe)
                    found, found_sse = ctx.loop_frame_bounds()
                    search_doc = closedframes.make(LOOP_PSNR, H * W * 3, limit, frametarget.fixed_frames(key, PREPROCESS), src.files, found,
                                                   found_sse, ctx.loop_search_trace() if limit > 0 else [])
                    search_doc["quant"] = "lattice"
                    frame_bounds = search_doc["frame_bounds"]
                    print(closedframes.stdout_line(search_doc))
                else:
                    key = ctx.rollout_closed_frames(None, PREPROCESS, WINDOW_SIZE, bounds=loop_bounds)
                    frame_bounds = [float(b) for b in ctx.loop_frame_bounds()[0]]   # (0 at the frames stored exactly)
                    print(closedframes.explicit_line(frame_bounds))
            elif closed and loop_map is not None:   # TZ-CLM1: TZ-CL1 under one abs bound per pixel; the job below runs under the same map
                print(closedloop.STDOUT_LINE)
                ctx.set_bound_map(loop_map)
                print(closedmap.stdout_line(loop_map))
                if select:
                    ctx.set_pred_select(True)
                key = ctx.rollout_closed_map(None, PREPROCESS, WINDOW_SIZE)
                if select:
                    modes = ctx.pred_modes()
                    print(predselect.stdout_line(modes[~key]))
                bound_map, BOUND_MAP, BOUND_VALUE = loop_map, LOOP_MAP, [0.0]   # (what the report and the sidecar say about a map)
            elif closed:   # TZ-CL1: the decoded frame is fed back, under the job's own bound and quantiser (no window MSE exists)
                print(closedloop.STDOUT_LINE)
                if select:   # TZ-PS1: per tile, the network or the decoded frame in front
                    ctx.set_pred_select(True)
                elif motion:   # TZ-PM1: per tile, the network or the decoded frame in front displaced by the tile's vector
                    ctx.set_pred_motion(predmotion.RADIUS)
                key = ctx.rollout_closed(None, PREPROCESS, WINDOW_SIZE, MODE, BOUND_VALUE)
                if select:
                    modes = ctx.pred_modes()
                    print(predselect.stdout_line(modes[~key]))
                elif motion:
                    modes, vectors = ctx.pred_modes(), ctx.pred_vectors()
                    print(predmotion.stdout_line(modes[~key], vectors[~key]))
            else:
                key, mse = ctx.rollout(None, PREPROCESS, WINDOW_SIZE, THRESHOLD, want_mse=bool(VERBOSE))
            if VERBOSE:
                for i in range(PREPROCESS + 1, nt) if not closed else ():
                    print("MSE:", mse[i])
                    if key[i] and i > PREPROCESS:
                        print("move key point")
                print("predict:{0}".format(time.time() - t0) + "[sec]")
            stages.mark("rollout", ctx)
            if PER_FRAME:   # one rollout and one probe serve every frame's candidate: a frame's quantiser sees its own bound alone
                fixed = frametarget.fixed_frames(key, PREPROCESS)
                limit = target.sse_limit(TARGET_PSNR, H * W * 3)

                def probe(cand):
                    ctx.set_frame_bounds([target.bound_of(c) for c in cand])
                    return ctx.bound_probe("abs", [0.0])["sse"]

                ks, sse, trace = frametarget.search(probe, limit, fixed)
                search_doc = frametarget.make(TARGET_PSNR, H * W * 3, limit, fixed, src.files, ks, sse, trace)
                frame_bounds = search_doc["frame_bounds"]
                print(frametarget.stdout_line(search_doc))
                stages.mark("per-frame bound search (device)")
            elif frame_bounds is not None and not loop_frames:
                frame_bounds = [0.0 if fx else b for fx, b in zip(frametarget.fixed_frames(key, PREPROCESS), frame_bounds)]
                print(frametarget.explicit_line(frame_bounds))
            if bound_map is not None and loop_map is None:   # the job: abs, pixel p under bound_map[p] in every frame (BOUND_VALUE is not read)
                ctx.set_bound_map(bound_map)
                print(boundmap.stdout_line(bound_map))
                BOUND_VALUE = [0.0]
            if frame_bounds is not None:   # the job: abs, frame f under frame_bounds[f]
                ctx.set_frame_bounds(frame_bounds)
            elif TARGET_PSNR is not None:   # one rollout serves every candidate: the predictions do not depend on the bound
                # (a probe describes the job in the payload layout decide_gray left in force: the one-channel job's own SSE)
                limit = target.sse_limit(TARGET_PSNR, nt * H * W * 3)
                k, trace = target.search(lambda c: int(ctx.bound_probe("abs", [target.bound_of(c)])["sse"].sum()), limit)
                search_doc = target.make(TARGET_PSNR, nt * H * W * 3, limit, trace, k)
                BOUND_VALUE = [target.bound_of(k)]
                print(target.stdout_line(search_doc))
                stages.mark("bound search (device)")
            if TARGET_RATIO is not None:   # likewise; the budget counts the files that do not depend on the bound, so they come first
                _key_output(ctx, OUTPUT_DIR, nt, H, W, key, pool, stages, VERBOSE, KEY_CODER).result()
                fixed = sum(os.path.getsize(os.path.join(OUTPUT_DIR, f)) for f in ("filename.txt", "key_frame.dat"))
                raw = nt * H * W * 3
                limit = ratetarget.budget(raw, TARGET_RATIO)
                k, trace = ratetarget.search(lambda c: ratetarget.file_bytes(
                    ctx.size_probe("abs", [ratetarget.bound_of(c)], ENTROPY_RUN, CODER), CODER), fixed, limit)
                search_doc = ratetarget.make(TARGET_RATIO, raw, limit, fixed, trace, k)
                stages.mark("key_frame.dat + bound search (device)")
                if k is None:
                    if QUANT == "lattice":
                        search_doc["quant"] = "lattice"
                    print(ratetarget.unreachable_line(search_doc))
                    ratetarget.write(OUTPUT_DIR, search_doc)
                    sys.exit(ratetarget.EXIT_UNREACHABLE)
                BOUND_VALUE = [ratetarget.bound_of(k)]
                print(ratetarget.stdout_line(search_doc))
            if SDELTA == sdauto.MODE:   # the bound is known: size the layouts on the one rollout, then go on as the chosen job
                strided, plane = decide_auto(ctx, channels, MODE, BOUND_VALUE if frame_bounds is None else [0.0], ENTROPY_RUN, CODER)
                sd_mode = "plane" if plane else ("channel" if strided else "flat")
                stages.mark("sdelta probe (device)")
            # (under frame bounds the bound of encode() is not read)
            _, table, _ = ctx.encode(MODE, BOUND_VALUE if frame_bounds is None else [0.0], ENTROPY_RUN, payload="resident", shuffle=SHUFFLE)
            stages.mark("encode (payload resident)", ctx)
            if REPORT:   # stream-ordered before _stream_outputs fetches the payload; changes nothing it reads
                t0 = time.time()
                stats = ctx.encode_quality("resident", table if ENTROPY_RUN else None, shuffle=SHUFFLE)
                if VERBOSE:
                    print("quality:{0}".format(time.time() - t0) + "[sec]")
                stages.mark("quality report (device)")
                if bound_map is not None:   # likewise: the decoded stack against the originals under the map
                    map_rec = ctx.encode_map_check("resident", table if ENTROPY_RUN else None, shuffle=SHUFFLE)
                    stages.mark("bound map check (device)")
                if SSIM:   # likewise, on the same resident payload
                    t0 = time.time()
                    ssim_rec = ctx.encode_ssim("resident", table if ENTROPY_RUN else None, shuffle=SHUFFLE)
                    if VERBOSE:
                        print("ssim:{0}".format(time.time() - t0) + "[sec]")
                    stages.mark("ssim (device)")
            if DIGESTS:  # likewise: the decoder's tail into scratch, one pass over what it yields and one over the originals
                t0 = time.time()
                dig = ctx.encode_digests("resident", table if ENTROPY_RUN else None, shuffle=SHUFFLE)
                if VERBOSE:
                    print("digests:{0}".format(time.time() - t0) + "[sec]")
                stages.mark("frame digests (device)")
            if VERBOSE:
                prof = ctx.prof_get()
                print("error_bound:{0}".format(prof["quant"][0] / 1e3) + "[sec]")
                print("finding_difference:{0}".format(prof["spatial_delta_hist"][0] / 1e3) + "[sec]")
                if ENTROPY_RUN:
                    # compress.py:351-365 times 1600 - x, bincount and the table sort; the first two are fused into
                    # the spatial-delta kernel here (timed above), what is left is the host-side sort
                    print("table_create:{0}".format(prof["table_create"][0] / 1e3) + "[sec]")
                    print("replacing_based_on_frequency:{0}".format(prof["lut_remap"][0] / 1e3) + "[sec]")
            if TARGET_RATIO is not None:   # (key_frame.dat is there already)
                _entropy_output(ctx, OUTPUT_DIR, nt, H, W, table if ENTROPY_RUN else None, PREPROCESS, SHUFFLE, stages, coder=CODER,
                                verbose=VERBOSE, channels=channels, strided=strided, plane=plane)
            else:
                _stream_outputs(ctx, OUTPUT_DIR, nt, H, W, key, table if ENTROPY_RUN else None, PREPROCESS, SHUFFLE, pool, stages,
                                coder=CODER, verbose=VERBOSE, key_coder=KEY_CODER, channels=channels, strided=strided, plane=plane,
                                **({"closed": 3 if motion else 2 if select else True} if closed else {}))
            if select:
                modes_size = predselect.write(OUTPUT_DIR, modes)
            elif motion:
                modes_size = predmotion.write(OUTPUT_DIR, modes, vectors)
            if closed:
                doc = sidecar.write(OUTPUT_DIR, ctx.rollout_contract(), wts, hp, wp, (nt, H, W, PREPROCESS),
                                    payload_channels=channels, sdelta=sd_mode, quant=QUANT, loop="closed",
                                    **({"bound_map": boundmap.stats(loop_map)} if loop_map is not None else {}),
                                    **({"pred": "select"} if select else {"pred": "motion"} if motion else {}))
            elif bound_map is not None:
                doc = sidecar.write(OUTPUT_DIR, ctx.rollout_contract(), wts, hp, wp, (nt, H, W, PREPROCESS),
                                    payload_channels=channels, sdelta=sd_mode, quant=QUANT, bound_map=boundmap.stats(bound_map))
            elif QUANT == "lattice":
                doc = sidecar.write(OUTPUT_DIR, ctx.rollout_contract(), wts, hp, wp, (nt, H, W, PREPROCESS),
                                    payload_channels=channels, sdelta=sd_mode, quant="lattice")
            else:
                doc = sidecar.write(OUTPUT_DIR, ctx.rollout_contract(), wts, hp, wp, (nt, H, W, PREPROCESS),   # the contract the predictions were made under
                                    payload_channels=channels, sdelta=sd_mode)
            if VERBOSE:
                print("arithmetic contract:", doc["arithmetic_contract"])
            stages.mark("key_frame.dat + entropy.dat")
            if REPORT:   # the three files exist: the ratio is known
                report = quality.summarize(stats, src.files, H, W, MODE, [] if bound_map is not None else BOUND_VALUE, quality.file_sizes(OUTPUT_DIR),
                                           window=WINDOW_SIZE, threshold=THRESHOLD, warm_up=PREPROCESS,
                                           **({"ssim": ssim_rec} if SSIM else {}))
                if select:   # pred_modes.dat is part of the stream
                    report["stored_bytes"] += modes_size
                    report["ratio"] = float(report["raw_bytes"]) / float(report["stored_bytes"])
                    report["pred_select"] = {"tiles": int(modes[~key].size), "prev_tiles": int(np.count_nonzero(modes))}
                elif motion:   # likewise
                    report["stored_bytes"] += modes_size
                    report["ratio"] = float(report["raw_bytes"]) / float(report["stored_bytes"])
                    report["pred_motion"] = {"tiles": int(modes[~key].size), "prev_tiles": int(np.count_nonzero(modes)),
                                             "displaced_tiles": int(np.count_nonzero(vectors.any(axis=-1)))}
                if frame_bounds is not None:
                    report["frame_bounds"] = [float(b) for b in frame_bounds]
                if bound_map is not None:
                    report["bound_map"] = {"file": os.fspath(BOUND_MAP) if isinstance(BOUND_MAP, (str, os.PathLike)) else None,
                                           "max": int(bound_map.max()), "violations": int(map_rec["violations"].sum()),
                                           "max_excess": int(map_rec["max_excess"].max()) if nt else 0}
                    for entry, r in zip(report["per_frame"], map_rec):
                        entry["violations"] = int(r["violations"])
                quality.write(OUTPUT_DIR, report)
                for line in quality.stdout_lines(report):
                    print(line)
                if bound_map is not None:
                    broken = [i for i in range(nt) if map_rec["violations"][i]]
                    for i in broken:   # a bug, not a property of the data
                        print(boundmap.broken_line(i, src.files[i], int(map_rec["violations"][i])))
                    if broken:
                        sys.exit(boundmap.EXIT_BROKEN)
                    print(boundmap.HELD_LINE)
            if QUANT == "lattice" and (TARGET_PSNR is not None or TARGET_RATIO is not None):
                search_doc["quant"] = "lattice"
            if PER_FRAME:
                frametarget.write(OUTPUT_DIR, search_doc)
            elif LOOP_PSNR is not None:
                closedframes.write(OUTPUT_DIR, search_doc)
            elif TARGET_PSNR is not None:
                target.write(OUTPUT_DIR, search_doc)
            if TARGET_RATIO is not None:
                ratetarget.write(OUTPUT_DIR, search_doc)
            if DIGESTS:  # last: every other file is what it is without the flag
                digest.write(OUTPUT_DIR, digest.make(dig[0], dig[1], (H, W, 3)))
        finally:
            ctx.close()


class _NotImages(Exception):
    """A rank met a file that is not an image of the stack's size and mode (the reference's message, compress.py:124-131)."""


def _decode_list(src, indices, pool):
    """The frames `indices` of a FrameSource as one uint8 (len, H, W, 3) array, decoded on `pool`."""
    indices = list(indices)
    out = np.empty((len(indices), src.H, src.W, 3), np.uint8)
    futs = [pool.submit(src._decode_into, out[j], src.paths[i]) for j, i in enumerate(indices)]
    try:
        for ft in futs:
            ft.result()
    except src.errors:
        raise _NotImages(src.data_dir)
    return out


def pack_outputs_from_keys(nt, H, W, key, key_frames, payload, table, warm_up, shuffled=False):
    """pack_outputs for a caller that holds only the key frames: `key_frames` maps frame index -> uint8 (H, W, 3)."""
    stack = np.zeros((nt, H, W, 3), np.uint8)
    for i in np.nonzero(key)[0]:
        stack[i] = key_frames[int(i)]
    key_bytes = zstd.compress_array(stack, 9, zstd.default_threads())
    stream = build_stream(payload, table, (SHUFFLE_MARK if shuffled else 1, nt, H, W, 3), warm_up)
    return key_bytes, zstd.compress_array(stream, 9, zstd.default_threads())


def _run_sharded(WEIGHTS_DIR, DATA_DIR, OUTPUT_DIR, PREPROCESS, WINDOW_SIZE, THRESHOLD, MODE, BOUND_VALUE, VERBOSE,
                 ENTROPY_RUN, device, SHUFFLE, CODER="zstd"):
    """Under torch.distributed.run.  SWP: the windows are sharded over the ranks and so is the image I/O -- every rank
    lists the directory (names only) and decodes the files of ITS frame range, nothing else (compress.py:97-122 decodes
    every file in one loop); rank 0 additionally reads the few key frames key_frame.dat needs and writes the files.
    DWP does not shard (its windows are found sequentially): rank 0 runs it alone."""
    problem = check_coder(CODER, SHUFFLE, sharded=True)
    if problem:
        print("ERROR:", problem)
        sys.exit(2)
    job = tzdist.active()
    rank0 = job[0] == 0
    src = FrameSource(DATA_DIR)          # lists, probes the first image (mode, size): same messages as load_images
    nt, H, W = src.nt, src.H, src.W
    cfg, wts, model_shape = open_model(WEIGHTS_DIR)
    hp, wp = _accept_job(src, model_shape, PREPROCESS, SHUFFLE, OUTPUT_DIR if rank0 else None, cfg.nb_layers)
    if WINDOW_SIZE is None:
        if rank0:
            print("NOTE: DWP (-t) finds its windows sequentially and does not shard: running on rank 0 only.")
        else:
            return
        job = None
    if job:
        device = tzdist.init_from_env()
        nt_local = max(b - a for a, b in tzdist.plan_shards(nt, PREPROCESS, WINDOW_SIZE, job[1]))
        nwin = max(1, (nt_local + WINDOW_SIZE - 1) // WINDOW_SIZE)
    else:
        nwin = 1
    ctx = make_context(cfg, wts, hp, wp, min(nwin, 64), device)
    decoded = []          # (f0, f1) ranges this rank decoded: tests read it through TEZIP_IO_LOG
    try:
        with ThreadPoolExecutor(max_workers=io_threads()) as pool:
            own = {}

            def fetch(f0, f1):
                decoded.append((f0, f1))
                own["f0"], own["frames"] = f0, _decode_list(src, range(f0, f1), pool)
                return own["frames"]

            try:
                if job:
                    res = tzdist.compress_sharded(tzdist.HipEngine(ctx, device), fetch, PREPROCESS, WINDOW_SIZE, MODE,
                                                  BOUND_VALUE, ENTROPY_RUN, nt=nt)
                else:
                    frames = fetch(0, nt)
                    key, _ = ctx.rollout(frames, PREPROCESS, None, THRESHOLD)
                    payload, table, _ = ctx.encode(MODE, BOUND_VALUE, ENTROPY_RUN, shuffle=SHUFFLE)
                    res = (payload, table, key)
            except _NotImages:
                src.fail()
            if res is None:
                return
            payload, table, key = res
            if job and SHUFFLE:
                payload = ctx.byte_shuffle(np.ascontiguousarray(payload)).view(np.int16)
            # key_frame.dat (compress.py:271-278): the key frames of rank 0's own range are in memory, the others -- one
            # per window -- are read from their files here
            f0 = own.get("f0", 0)
            have = own.get("frames")
            key_frames = {}
            missing = []
            for i in (int(v) for v in np.nonzero(key)[0]):
                if have is not None and f0 <= i < f0 + len(have):
                    key_frames[i] = have[i - f0]
                else:
                    missing.append(i)
            try:
                for i, arr in zip(missing, _decode_list(src, missing, pool)):
                    key_frames[i] = arr
                decoded.extend((i, i + 1) for i in missing)
            except _NotImages:
                src.fail()
        key_bytes, entropy_bytes = pack_outputs_from_keys(nt, H, W, key, key_frames, payload, table if ENTROPY_RUN else None,
                                                          PREPROCESS, SHUFFLE)
        with open(os.path.join(OUTPUT_DIR, "key_frame.dat"), mode='wb') as f:
            f.write(key_bytes)
        with open(os.path.join(OUTPUT_DIR, "entropy.dat"), mode='wb') as f:
            f.write(entropy_bytes)
        doc = sidecar.write(OUTPUT_DIR, ctx.get_contract(), wts, hp, wp, (nt, H, W, PREPROCESS))   # every rank runs under the same TEZIP_PA / frame size
        if VERBOSE:
            print("arithmetic contract:", doc["arithmetic_contract"])
    finally:
        _log_io("compress", job, decoded)
        ctx.close()


def _log_io(what, job, ranges):
    """TEZIP_IO_LOG=<dir>: every rank leaves `<what>.rank<r>` with the frame ranges it decoded / encoded (tests assert
    that a rank of a sharded job touches the files of its own windows only)."""
    d = os.environ.get("TEZIP_IO_LOG")
    if d:
        rank = job[0] if job else 0
        try:   # (a diagnostic: it must never be what a job fails on, least of all from a `finally`)
            with open(os.path.join(d, "%s.rank%d" % (what, rank)), "w") as f:
                f.write(" ".join("%d:%d" % r for r in ranges) + "\n")
        except OSError:
            pass
