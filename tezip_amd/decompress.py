"""decompress.run -- same signature, inputs and outputs as the reference's
/root/reference/src/decompress.py:39 `run(...)`; the rollout replay, inverse remap, inverse
spatial delta (a prefix scan on the GPU instead of the reference's Python loop) and the
reconstruction run in libtezip_hip.so."""
import functools
import os
import sys
import time

import numpy as np

from . import _lib, closedloop, digest, huff, huffd, huffr, keycoder, keycoderg, predmotion, predselect, sidecar, zstd
from . import dist as tzdist
from . import sdelta
from .compress import SHUFFLE_MARK, make_context, open_model
from .data_utils import padding_shape


def parse_stream(data):
    """decompress.py:105-113, 203-221: -> (payload, table|None, shape5, warm_up)."""
    s = np.frombuffer(data, dtype='<i2')
    if s.size < 8:
        raise ValueError("entropy.dat is too short")
    warm_up = int(s[-1])
    shape = tuple(int(v) for v in s[-6:-1])
    tlen = int(s[-7])
    if tlen == -1:
        return s[:-7], None, shape, warm_up
    if tlen < 0 or tlen > s.size - 7:
        raise ValueError("corrupt table length %d" % tlen)
    return s[: -7 - tlen], s[-7 - tlen: -7], shape, warm_up


def check_stream(shape, warm_up, payload_len, key_len):
    """The trailer is data from a file: cross-check it before any pointer derived from it reaches
    the native library.  The reference fails with a ValueError at its reshapes
    (decompress.py:115,240) for the same inconsistencies."""
    one, nt, H, W, C = shape
    # C: the channels the PAYLOAD stores per pixel -- 3, or 1 for this build's opt-in payload of a gray job (--gray,
    # tezip_amd/graypayload.py); the frames and key_frame.dat have three channels either way
    # one: 1 in the reference, SHUFFLE_MARK for byte planes; sdelta.MARK / MARK_SHUFFLE (4 / 5) say the same of a payload whose
    # spatial delta ran at the channel stride (--sdelta channel, tezip_amd/sdelta.py), which has three channels;
    # sdelta.MARK_PLANE / MARK_PLANE_SHUFFLE (8 / 9) of a payload under the 2-D spatial delta TZ-SD2 (--sdelta plane), which has
    # three channels or one.  3, 6 and 7 mean nothing.  Each of the six plus 16 (17, 18, 20, 21, 24, 25): the same layout of a
    # closed-loop job (--loop closed, tezip_amd/closedloop.py), which has three channels
    # Each of those plus 32 (49, 50, 52, 53, 56, 57): a closed-loop job with per-tile selection (--pred select, tezip_amd/predselect.py)
    if closedloop.is_closed(predselect.closed_mark(one)) and C != 3:
        raise ValueError("entropy.dat: a closed-loop stream (mark %d) has a three-channel payload, the trailer says %d" % (one, C))
    one = closedloop.open_mark(predselect.closed_mark(one))
    if (one not in (1, SHUFFLE_MARK) + sdelta.MARKS + sdelta.PLANE_MARKS or C not in (1, 3) or (one in sdelta.MARKS and C != 3)
            or nt < 1 or H < 1 or W < 1):
        raise ValueError("entropy.dat: unsupported stack shape %r (expected (1, nt, H, W, 3), (1, nt, H, W, 1) for a gray job, "
                         "(4, nt, H, W, 3) for a channel-stride payload or (8, nt, H, W, 3 or 1) for a plane payload)" % (tuple(shape),))
    n = nt * H * W * C
    if payload_len != n:
        raise ValueError("entropy.dat: payload holds %d elements, the trailer says %d (truncated or corrupt file)"
                         % (payload_len, n))
    if key_len != nt * H * W * 3:
        raise ValueError("key_frame.dat holds %d bytes, the stack shape %r of entropy.dat's trailer implies %d"
                         % (key_len, tuple(shape), nt * H * W * 3))
    if not 0 <= warm_up < nt:
        raise ValueError("entropy.dat: warm-up count %d outside [0, %d)" % (warm_up, nt))


def check_channels(data_dir, C):
    """The payload channels entropy.dat's trailer states (3, or 1 for a --gray job) against tezip_amd.json, which records 1
    and says nothing for 3.  The trailer is authoritative; a sidecar that contradicts it belongs to another stream."""
    want = sidecar.channels_of(sidecar.read(data_dir))
    if want is not None and want != C:
        raise ValueError("tezip_amd.json describes the payload as %d-channel, entropy.dat's trailer as %d-channel" % (want, C))


def check_sdelta(data_dir, one):
    """The stride of the payload's spatial delta that entropy.dat's trailer states (mark 4 / 5: channel) against tezip_amd.json,
    which records "channel" and says nothing for flat.  The trailer is authoritative; a sidecar that contradicts it belongs to
    another stream.  Marks 8 / 9 (plane, TZ-SD2) likewise against "plane".  Returns the mode for set_sdelta: 0 flat, 1 channel,
    2 plane."""
    have = sdelta.mode_of(one)
    want = sidecar.sdelta_of(sidecar.read(data_dir))
    if want is not None and want != have:
        raise ValueError("tezip_amd.json describes the payload's spatial delta as %s, entropy.dat's trailer as %s" % (want, have))
    return sdelta.MODES.index(have)


def check_loop(data_dir, one):
    """The prediction loop that entropy.dat's trailer states (the open-loop mark plus 16: closed, TZ-CL1) against tezip_amd.json,
    which records "closed" and says nothing for open.  The trailer is authoritative; a sidecar that contradicts it belongs to
    another stream.  Returns whether the stream is a closed-loop one."""
    have = "closed" if closedloop.is_closed(one) else "open"
    want = sidecar.loop_of(sidecar.read(data_dir))
    if want is not None and want != have:
        raise ValueError("tezip_amd.json describes the prediction loop as %s, entropy.dat's trailer as %s" % (want, have))
    return have == "closed"


def early_pred_modes(data_dir):
    """pred_modes.dat of a stream whose sidecar states per-tile selection (TZ-PS1, tezip_amd/predselect.py) and the stack, read
    and validated against that stack before a GPU is touched -> the modes, or None when the sidecar says nothing of it (the
    trailer's mark decides then, in stream_pred).  ValueError for a missing or malformed file.  A sidecar that states
    motion-compensated tiles (TZ-PM1, tezip_amd/predmotion.py): likewise with that definition's format TZP2."""
    doc = sidecar.read(data_dir)
    stack = sidecar.stack_of(doc)
    pred = sidecar.pred_of(doc)
    if pred not in ("select", "motion") or stack is None:
        return None
    if pred == "motion":
        return predmotion.read(data_dir, stack[0], stack[1], stack[2])[0]
    return predselect.read(data_dir, stack[0], stack[1], stack[2])


def stream_pred(data_dir, one, nt, H, W):
    """What entropy.dat's trailer states about the prediction of a tile -- the closed-loop mark plus 32: per-tile selection
    (TZ-PS1), plus 64: motion-compensated tiles (TZ-PM1, tezip_amd/predmotion.py) -- against tezip_amd.json, which records "select"
    or "motion" and says nothing otherwise.  The trailer is authoritative; a sidecar that contradicts it belongs to another
    stream.  Returns (kind, modes, vectors): kind "net", "select" or "motion"; the modes of pred_modes.dat, validated against the
    trailer's stack, None for "net"; the vectors for "motion" alone, else None."""
    have = predmotion.pred_of_mark(one)
    want = sidecar.pred_of(sidecar.read(data_dir))
    if want is not None and want != have:
        raise ValueError("tezip_amd.json describes the prediction as %s, entropy.dat's trailer as %s" % (want, have))
    if have == "motion":
        return (have,) + tuple(predmotion.read(data_dir, nt, H, W))
    return have, (predselect.read(data_dir, nt, H, W) if have == "select" else None), None


def check_pred(data_dir, one, nt, H, W):
    """stream_pred's modes alone: None for a stream whose tiles all come from the network."""
    return stream_pred(data_dir, one, nt, H, W)[1]


def stream_pred_or_exit(data_dir, one, nt, H, W):
    """stream_pred with a refusal as one ERROR line and exit status 2 (the error class of adopt_contract: nothing was written)."""
    try:
        return stream_pred(data_dir, one, nt, H, W)
    except ValueError as e:
        print("ERROR:", e)
        sys.exit(2)


def pred_modes_or_exit(data_dir, one, nt, H, W):
    """stream_pred_or_exit's modes alone."""
    return stream_pred_or_exit(data_dir, one, nt, H, W)[1]


def put_pred(ctx, kind, modes, vectors):
    """What stream_pred returned, in front of ctx.rollout_decode_closed: nothing for "net", TZ-PS1's modes for "select", TZ-PM1's
    modes and vectors for "motion"."""
    if kind == "motion":
        ctx.set_pred_motion(predmotion.RADIUS)
        ctx.put_pred_modes(modes)
        ctx.put_pred_vectors(vectors)
    elif kind == "select":
        ctx.set_pred_select(True)
        ctx.put_pred_modes(modes)


def refuse_closed_range(frames):
    """A frame range of a closed-loop stream: exit status 2 (the error class of adopt_contract: nothing was written)."""
    if frames is not None:
        print("ERROR:", closedloop.NO_FRAMES)
        sys.exit(2)


def set_sdelta(ctx, mode):
    """check_sdelta's mode on the context: tz_set_delta_stride for flat and channel, tz_set_delta_plane for plane."""
    if mode == 2:
        ctx.set_delta_plane(1)
    else:
        ctx.set_delta_stride(mode)


TAIL_ELEMS = _lib.TZ_NBINS + 8  # the longest trailer: table (<= 2111 symbols) + T + shape(5) + warm_up
# piece sizes of the streaming paths, read when a run starts (tests/test_gpu_pieces.py shrinks them to make every loop iterate)
PUT_PIECE = 16 << 20            # bytes of a coded body (TZH1 / TZR1 / TZR2 / TZK1 / TZK2) staged per huff_put / huffr_put / keys_put
FETCH_WINDOW_BYTES = 16 << 20   # a fetch window holds the frames that fit in this many bytes (at least one)
PREFETCH_PIECE_BYTES = 16 << 20  # _Prefetch: bytes of entropy.dat decompressed per piece
PREFETCH_DEPTH = 8              # _Prefetch: pieces queued ahead of the consumer


def coded_format(head):
    """The module of this build's opt-in entropy.dat formats the first bytes of a file name (huff: TZH1, huffr: TZR1,
    huffd: TZR2), or None for the reference's zstd frame."""
    for fmt in (huff, huffr, huffd):
        if bytes(head[:4]) == fmt.MAGIC:
            return fmt
    return None


def coded_calls(ctx, coded):
    """(begin, put, decode) of the context for a parsed TZH1 / TZR1 / TZR2 file; begin takes (bytes, n, lengths, base, run=)."""
    begin, put, decode = (getattr(ctx, "%s_%s" % (coded.coder, op)) for op in ("begin", "put", "decode"))
    if coded.coder == "huffd":                   # (the file's match distance goes with its lengths)
        begin = functools.partial(begin, dist=coded.dist)
    return begin, put, decode


def parse_coded_keys(head, path):
    """The key_frame.dat at `path`, of which `head` holds the first bytes: this build's opt-in formats (TZK1, TZK2) validated
    whole on the CPU -> keycoder.Parsed / keycoderg.Parsed; None for the reference's zstd frame."""
    for fmt in (keycoder, keycoderg):
        if fmt.is_keycoded(head):
            return fmt.parse(np.fromfile(path, np.uint8))
    return None


def stage_coded_keys(ctx, keys, stack):
    """A parsed TZK1 / TZK2 key_frame.dat -> the context's frame stack, as frames_begin + frames_put of the zero-except-keys
    stack leave it (tz_keys_begin / tz_keys_put / tz_keys_decode, or their tz_keysg_* forms).  stack: the (nt, H, W)
    entropy.dat describes."""
    if (keys.nt, keys.H, keys.W) != tuple(stack):
        raise ValueError("key_frame.dat describes the stack as %r (frames, height, width), entropy.dat's trailer as %r"
                         % ((keys.nt, keys.H, keys.W), tuple(stack)))
    begin, put, decode = ((ctx.keysg_begin, ctx.keysg_put, ctx.keysg_decode) if isinstance(keys, keycoderg.Parsed) else
                          (ctx.keys_begin, ctx.keys_put, ctx.keys_decode))
    begin(keys.body.size, keys.nt, keys.H, keys.W, keys.idx, keys.pred, keys.lengths)
    piece = PUT_PIECE
    for off in range(0, keys.body.size, piece):
        put(off, keys.body[off: off + piece])                               # pageable: the piece is free again on return
    decode()


def adopt_contract(DATA_DIR, wts, VERBOSE):
    """The arithmetic contract this directory must be decoded under (tezip_amd/sidecar.py): the one tezip_amd.json
    records; without that file --pa / TEZIP_PA, else None = by frame size.  A contradiction (a --pa that disagrees with the
    sidecar, another model's weights, a damaged tezip_amd.json) ends the run with a message and EXIT STATUS 2: this error
    class has no counterpart in the reference, so its `print` + `exit()` habit (status 0) is not mirrored -- a launcher
    must not see success when no frame was written."""
    try:
        contract = sidecar.resolve(sidecar.read(DATA_DIR), wts)
    except sidecar.SidecarMismatch as e:
        print("ERROR:", e)
        sys.exit(2)
    if VERBOSE and contract:
        print("arithmetic contract: TZ-PA%d" % contract)
    return contract


VERIFY_MODES = ("auto", "require", "off")


def check_verify(mode, data_dir, sharded=False):
    """The refusals of --verify that need no GPU, for tezip.py and for a direct caller of run(): None, or the message."""
    if mode not in VERIFY_MODES:
        return "--verify takes one of %s, got %r" % (", ".join(VERIFY_MODES), mode)
    if mode == "require" and sharded:
        return "--verify require is not available for a sharded job (WORLD_SIZE > 1), which does not verify: run it on one GPU"
    if mode == "require" and not digest.present(data_dir):
        return "--verify require: %s holds no %s (compress with --digests)" % (data_dir, digest.NAME)
    return None


def check_records(records, nt, H, W):
    """frame_digests.json against the stack the stream describes; a contradiction ends the run with EXIT STATUS 2 (the error
    class of adopt_contract: nothing was written)."""
    try:
        digest.validate(records, nt, (H, W, 3))
    except ValueError as e:
        print("ERROR:", e)
        sys.exit(2)


def verify_frames(records, got, first, file_names):
    """The digests `got` of the decoded frames first, first + 1, ... against the recorded ones, before any image is written:
    a mismatch names the frames (ten at the most, the rest counted) and ends the run with EXIT STATUS 3."""
    bad = digest.mismatches(records, got, first)
    if bad:
        for line in digest.mismatch_lines(bad, file_names):
            print(line)
        sys.exit(3)
    print("verified: %d frames" % len(got))


class _Prefetch:
    """zstd.stream_decompress of one file on a worker thread (libzstd releases the GIL), its pieces copied into a ring of
    host buffers and handed over through a bounded queue: the caller -- the only thread that touches the context -- can
    queue the decoder's rollout first and collect the payload afterwards.  At most `depth` + 2 pieces exist at a time,
    whatever the length of the stream.  An error on the worker is raised where the caller iterates."""

    def __init__(self, path, piece_bytes=None, depth=None):
        import queue
        import threading
        piece_bytes = PREFETCH_PIECE_BYTES if piece_bytes is None else piece_bytes    # (None: the module constant now)
        depth = PREFETCH_DEPTH if depth is None else depth
        self.path, self.piece_bytes = path, piece_bytes
        self.q = queue.Queue(maxsize=depth)
        self.nbuf = depth + 2     # `depth` queued + the one the caller holds + the one being filled
        self.stop = False
        self.t = threading.Thread(target=self._run, daemon=True)
        self.t.start()

    def _put(self, item):
        import queue
        while not self.stop:
            try:
                self.q.put(item, timeout=0.1)
                return True
            except queue.Full:
                pass
        return False

    def _run(self):
        try:
            bufs = []
            with open(self.path, "rb") as f:
                for k, (size, piece) in enumerate(zstd.stream_decompress(f, piece_bytes=self.piece_bytes)):
                    if len(bufs) < self.nbuf:
                        bufs.append(np.empty(self.piece_bytes, np.uint8))
                    buf = bufs[k % self.nbuf]
                    buf[:piece.size] = piece
                    if not self._put((size, buf[:piece.size])):
                        return
            self._put(None)
        except BaseException as e:   # handed to the consumer
            self._put(e)

    def __iter__(self):
        while True:
            item = self.q.get()
            if item is None:
                return
            if isinstance(item, BaseException):
                raise item
            yield item

    def close(self):
        self.stop = True
        self.t.join(timeout=5.0)


def _run_streaming(DATA_DIR, OUTPUT_DIR, file_names, isRGB, cfg, wts, model_shape, VERBOSE, device, contract=None, stack=None,
                   frames=None, records=None):
    """decompress.py:87-279 with nothing of size nt*H*W on the host: entropy.dat is decompressed
    piece by piece straight into HBM (the trailer is read from the last piece), key_frame.dat
    likewise, the decoded frames come back window by window and are PNG-encoded on a thread pool
    while the next window is fetched.  Returns False when the stream needs the whole-array path
    (this build's opt-in byte-shuffled payload).
    `stack` = (nt, H, W) from tezip_amd.json (round 6), or None: the reference keeps the shape in the LAST values of
    entropy.dat (compress.py:390-394), so without it nothing can start before the whole payload is decompressed; with it
    the key frames are staged and the decoder's rollout is queued FIRST, entropy.dat being decompressed on a worker
    thread meanwhile, and the trailer is checked against it when it arrives.
    `frames` = (A, B): only frames [A, B) are rolled out, decoded and written (tz_rollout_decode_range / tz_decode_range);
    the whole stream is still staged, because its trailer holds the table and the shape.
    `records` = the validated frame_digests.json, or None: the decoded frames are checked against it where they lie in HBM
    (tz_decoded_digests), before the first of them is fetched."""
    from concurrent.futures import ThreadPoolExecutor
    from PIL import Image
    from .compress import _Stages, io_threads
    stages = _Stages("decompress")
    paths = {n: os.path.join(DATA_DIR, n) for n in ("key_frame.dat", "entropy.dat")}
    for n in ("key_frame.dat", "entropy.dat"):
        if not os.path.exists(paths[n]):
            print("ERROR: No such file or directory:", paths[n])
            exit()
    ctx = _lib.Context(device)
    try:
        ctx.load_model(cfg, wts)
        if contract:
            ctx.set_contract(contract)
        stages.mark("context + model load")
        with open(paths["key_frame.dat"], "rb") as f:
            head = f.read(64)
        # this build's opt-in key-frame file (TZK1 / TZK2): validated whole on the CPU; the length the zero-except-keys stack
        # would have stands in its header, so the cross-checks below see what they see for the reference's file
        keys = parse_coded_keys(head, paths["key_frame.dat"])
        key_len = keys.nt * keys.H * keys.W * 3 if keys is not None else zstd.content_size(head)

        def checks(nt, H, W):
            hp, wp = padding_shape(H, W)
            if model_shape is not None and (model_shape[0] != hp or model_shape[1] != wp):
                print("ERROR:keyframe size and model size do not match.")
                print("model size: height ", model_shape[0] - 7, "～", model_shape[0], " width ", model_shape[1] - 7, "～", model_shape[1])
                print("key frame size: height ", H, " width ", W)
                exit()
            if len(file_names) != nt:
                print("ERROR：The lengths of filename.txt and images do not match.")
                print("filename.txt：", len(file_names))
                print("number of images", nt)
                exit()
            return hp, wp

        def stage_keys(nt, H, W, hp, wp):
            """key_frame.dat into HBM (decompress.py:97-103); returns frames per fetch window"""
            ctx.prepare(hp, wp, 64 if nt > 64 else max(1, nt))
            stages.mark("model prepare")
            fb = H * W * 3
            per = max(1, FETCH_WINDOW_BYTES // fb)
            if keys is not None:
                stage_coded_keys(ctx, keys, (nt, H, W))
                stages.mark("stage key_frame.dat + key-frame decode", ctx)
                return per
            ctx.frames_begin(nt, H, W)
            first = 0
            with open(paths["key_frame.dat"], "rb") as f:
                for _, piece in zstd.stream_decompress(f, piece_bytes=per * fb):
                    k = piece.size // fb
                    ctx.frames_put(first, piece[: k * fb].reshape(k, H, W, 3))
                    first += k
            if first != nt:
                raise ValueError("key_frame.dat: truncated stream")
            stages.mark("zstd-d key_frame.dat + stage to HBM", ctx)
            return per

        def rollout(nt, warm_up):
            if VERBOSE:
                ctx.prof_enable(True)
            t0 = time.time()
            lo, hi = frames or (0, nt)
            ctx.rollout_decode_range(None, warm_up, lo, hi - lo)   # (key discovery, then the predictor launches are queued)
            if VERBOSE:
                print("predict:{0}".format(time.time() - t0) + "[sec]")

        # a closed-loop stream (TZ-CL1, tezip_amd/closedloop.py) has no rollout ahead of its payload: every step of
        # tz_rollout_decode_closed reads the quantised deltas.  The sidecar says so up front; the trailer's mark has the last word
        sidecar_closed = sidecar.loop_of(sidecar.read(DATA_DIR)) == "closed"

        with open(paths["entropy.dat"], "rb") as f:
            ent_head = f.read(64)
        fmt = coded_format(ent_head)
        if fmt is not None:
            # this build's opt-in Huffman file: everything the decoder needs stands in FRONT of the bit stream, so the
            # whole file is validated on the CPU (huff.parse / huffr.parse / huffd.parse) before anything is staged, and the
            # rollout is queued first
            coded = fmt.parse(np.fromfile(paths["entropy.dat"], np.uint8), key_len)
            table, warm_up = coded.table, coded.warm_up
            one, nt, H, W, C = coded.shape
            tile_pred = stream_pred_or_exit(DATA_DIR, one, nt, H, W)
            one = predmotion.closed_mark(one)
            closed = check_loop(DATA_DIR, one)
            one = closedloop.open_mark(one)
            if closed:
                refuse_closed_range(frames)
            if stack is not None and key_len == stack[0] * stack[1] * stack[2] * 3 and len(file_names) == stack[0] \
                    and (nt, H, W, warm_up) != tuple(stack):
                raise ValueError("tezip_amd.json describes the stack as %r (frames, height, width, warm-up), entropy.dat's trailer as %r"
                                 % (tuple(stack), (nt, H, W, warm_up)))
            if frames is not None:
                check_frames(frames, nt)
            hp, wp = checks(nt, H, W)
            begin, put, expand = coded_calls(ctx, coded)
            begin(coded.body.size, coded.n, coded.lengths, coded.base, run=coded.run)
            per = stage_keys(nt, H, W, hp, wp)
            if not closed:
                rollout(nt, warm_up)
                stages.mark("rollout (decoder) queued")
            piece = PUT_PIECE
            for off in range(0, coded.body.size, piece):
                put(off, coded.body[off: off + piece])                  # pageable: the piece is free again on return
            expand()                                                    # -> the payload buffer, as payload_put leaves it
            stages.mark("stage entropy.dat + huffman decode", ctx)
        else:
            with open(paths["entropy.dat"], "rb") as f:
                ent_size = zstd.content_size(f.read(64))
            if ent_size % 2 or ent_size < 16:
                raise ValueError("entropy.dat is too short")
            total = ent_size // 2
            # the stack is known up front only from this build's sidecar -- a HINT: it is used when it agrees with everything
            # that can be checked now (key_frame.dat's size, the model's frame size, filename.txt), and the trailer has the last
            # word; a hint that does not fit is dropped and the late path below reports whatever is really wrong
            early = None
            if stack is not None and key_len == stack[0] * stack[1] * stack[2] * 3 and len(file_names) == stack[0]:
                hp_e, wp_e = padding_shape(stack[1], stack[2])
                if (model_shape is None or (model_shape[0] == hp_e and model_shape[1] == wp_e)) and not sidecar_closed:
                    early = stack
            pre = _Prefetch(paths["entropy.dat"])      # entropy.dat is being decompressed from here on
            try:
                per = None
                ctx.payload_begin(total)               # (in front of the rollout: the copy stream need not wait for it)
                if early is not None:
                    nt, H, W, warm_early = early
                    hp, wp = checks(nt, H, W)
                    per = stage_keys(nt, H, W, hp, wp)
                    rollout(nt, warm_early)
                    stages.mark("rollout (decoder) queued")
                tail = np.zeros(0, np.int16)
                off = 0
                for size, piece in pre:
                    if size != ent_size or piece.size % 2 or off * 2 + piece.size > ent_size:
                        raise ValueError("entropy.dat: inconsistent stream")
                    p16 = piece.view(np.int16)
                    ctx.payload_put(off, p16)       # staged on the copy stream; the piece buffer is free on return
                    off += p16.size
                    tail = np.concatenate([tail, p16[-TAIL_ELEMS:]])[-TAIL_ELEMS:]
            finally:
                pre.close()
            if off != total:
                raise ValueError("entropy.dat: truncated stream")
            stages.mark("zstd-d entropy.dat + stage to HBM", ctx)
            warm_up, shape, tlen = int(tail[-1]), tuple(int(v) for v in tail[-6:-1]), int(tail[-7])
            if tlen < -1 or tlen > tail.size - 7:
                raise ValueError("corrupt table length %d" % tlen)
            table = None if tlen == -1 else np.ascontiguousarray(tail[tail.size - 7 - tlen: tail.size - 7])
            payload_len = total - 7 - max(tlen, 0)
            check_stream((predmotion.select_mark(shape[0]),) + shape[1:], warm_up, payload_len, key_len)   # (a motion mark: as its layout's select mark)
            tile_pred = stream_pred_or_exit(DATA_DIR, *shape[:4])
            shape = (predmotion.closed_mark(shape[0]),) + shape[1:]
            closed = check_loop(DATA_DIR, shape[0])   # (a rollout that ran early on a closed-loop stream: the sidecar is another stream's)
            if closed:
                refuse_closed_range(frames)
            shape = (closedloop.open_mark(shape[0]),) + shape[1:]
            if sdelta.is_shuffled(shape[0]):
                return False
            one, nt, H, W, C = shape
            if early is not None and (nt, H, W, warm_up) != tuple(early):
                raise ValueError("tezip_amd.json describes the stack as %r (frames, height, width, warm-up), entropy.dat's trailer as %r"
                                 % (tuple(early), (nt, H, W, warm_up)))
            if frames is not None:
                check_frames(frames, nt)
            if early is None:
                hp, wp = checks(nt, H, W)
                per = stage_keys(nt, H, W, hp, wp)
                if not closed:
                    rollout(nt, warm_up)
        check_channels(DATA_DIR, C)
        ctx.set_payload_channels(C)         # 1: the one-channel payload of a gray job; the frames keep three channels
        set_sdelta(ctx, check_sdelta(DATA_DIR, one))   # 1: the payload's spatial delta ran at the channel stride, 2: plane
        if records is not None:
            check_records(records, nt, H, W)
        stages.mark("rollout (decoder)", ctx)
        lo, hi = frames or (0, nt)
        if closed:   # the staged payload becomes the quantised deltas, then predict and reconstruct step by step
            if VERBOSE:
                ctx.prof_enable(True)
            t0 = time.time()
            put_pred(ctx, *tile_pred)   # TZ-PS1 / TZ-PM1: the stored modes (and vectors) pick every tile's prediction
            ctx.rollout_decode_closed(None, warm_up, None, table)
            if VERBOSE:
                print("predict:{0}".format(time.time() - t0) + "[sec]")
        else:
            ctx.decode_range(None, table, lo, hi - lo, out="resident")
        stages.mark("decode tail (frames resident)", ctx)
        if records is not None:
            verify_frames(records, ctx.decoded_digests(lo, hi - lo), lo, file_names)
            stages.mark("verify frame digests")
        if VERBOSE:
            prof = ctx.prof_get()
            if table is not None:
                print("replacing_based_on_frequency:{0}".format(prof["lut_remap"][0] / 1e3) + "[sec]")
            print("finding_difference:{0}".format(prof["undelta_scan"][0] / 1e3) + "[sec]")
        print("save as RGB" if isRGB else "save as gray")
        ring = [np.empty((per, H, W, 3), np.uint8) for _ in range(3)]
        busy = [[], [], []]

        def save(buf, j, name):
            # decompress.py:272-278: the grayscale save is overwritten by an unconditional RGB save
            Image.fromarray(buf[j]).save(os.path.join(OUTPUT_DIR, name))

        with ThreadPoolExecutor(max_workers=io_threads()) as pool:  # PIL's encoder releases the GIL
            for ci, f0 in enumerate(range(lo, hi, per)):
                k = min(per, hi - f0)
                slot = ci % 3
                for ft in busy[slot]:
                    ft.result()           # the encoders of the window that used this buffer are done
                ctx.decoded_get(f0, k, out=ring[slot][:k])
                busy[slot] = [pool.submit(save, ring[slot], j, file_names[f0 + j]) for j in range(k)]
            for fs in busy:
                for ft in fs:
                    ft.result()
        stages.mark("frames fetch + PNG encode")
    finally:
        ctx.close()
    return True


def check_frames(frames, nt):
    """A frame range (A, B) must satisfy 0 <= A < B <= nt (filename.txt's length, then entropy.dat's trailer)."""
    a, b = frames
    if not 0 <= a < b <= nt:
        raise ValueError("frame range %d:%d is outside the %d frames of this sequence (0 <= A < B <= %d)" % (a, b, nt, nt))


def run(WEIGHTS_DIR, DATA_DIR, OUTPUT_DIR, GPU_FLAG, VERBOSE, device=0, frames=None, verify="auto"):
    """frames: None = every frame (the reference's behaviour), or (A, B) = write file_names[A:B] only, byte-identical to
    what a whole decode writes for those names (B None = to the end).  Not in the reference.
    verify (--verify; not in the reference): "auto" = when the directory holds frame_digests.json (`-c --digests`,
    tezip_amd/digest.py) the decoded frames -- those of `frames` only -- are checked against it on the device before an
    image is written: a mismatch names the frames, writes nothing and exits with status 3, a match prints
    "verified: <count> frames"; a directory without the file decodes as ever.  "require" = the same, and a missing file
    is exit status 2 before a GPU is touched.  "off" = never check: the way to salvage a damaged directory.  A sharded
    job does not verify (auto: rank 0 says so; require: refused)."""
    if not GPU_FLAG:
        print("ERROR: this build runs the decompression path on an AMD MI355X only (no CPU path).")
        exit()
    job = tzdist.active()
    if frames is not None and job is not None:
        # same error class as adopt_contract: a launcher must not see success when no frame was written
        print("ERROR: a frame range (--frames) cannot be decoded by a sharded job (WORLD_SIZE > 1): run it on one GPU")
        sys.exit(2)
    rank0 = job is None or job[0] == 0
    problem = check_verify(verify, DATA_DIR, job is not None)
    if problem:   # (tezip.py refuses this before any GPU is touched; a caller of run() gets the same answer)
        print("ERROR:", problem)
        sys.exit(2)
    # every rank of a sharded job writes the images of its own windows: each makes the directory (on one node they race for
    # the same one, hence exist_ok; on node-local paths each node gets its share -- INTEGRATION.md section 3)
    os.makedirs(OUTPUT_DIR, exist_ok=True)
    isRGB = True
    try:
        with open(os.path.join(DATA_DIR, 'filename.txt'), 'r', encoding='UTF-8') as f:
            file_names = [s.strip() for s in f.readlines()]
    except FileNotFoundError:
        print("ERROR:No such file or directory:", os.path.join(DATA_DIR, 'filename.txt'))
        exit()
    # decompress.py:55: `isdigit` is not called there, so any 1-character first line is the flag
    if file_names and len(file_names[0]) == 1:
        isRGB = bool(int(file_names.pop(0)))
    if frames is not None:
        frames = (int(frames[0]), len(file_names) if frames[1] is None else int(frames[1]))
        try:
            check_frames(frames, len(file_names))
        except ValueError as e:
            print("ERROR:", e)
            sys.exit(2)

    records = None
    if verify != "off" and digest.present(DATA_DIR):
        if job is not None:
            if rank0:
                print("NOTE: a sharded job (WORLD_SIZE > 1) does not verify %s: run -u on one GPU to check the frames" % digest.NAME)
        else:
            try:   # a damaged file is an error, not 'absent': same class and exit status as adopt_contract's
                records = digest.read(DATA_DIR, frames=len(file_names))
            except ValueError as e:
                print("ERROR:", e)
                sys.exit(2)

    cfg, wts, model_shape = open_model(WEIGHTS_DIR)
    contract = adopt_contract(DATA_DIR, wts, VERBOSE)
    try:   # a stream with per-tile selection (tezip_amd/predselect.py): its fifth file is read and validated before a GPU is touched
        early_pred_modes(DATA_DIR)
    except ValueError as e:
        print("ERROR:", e)
        sys.exit(2)
    if job is None and not os.environ.get("TEZIP_NO_STREAMING"):
        # (the sidecar passed adopt_contract: it is readable or absent)
        stack = None if os.environ.get("TEZIP_NO_EARLY_ROLLOUT") else sidecar.stack_of(sidecar.read(DATA_DIR))
        if records is not None:
            done = _run_streaming(DATA_DIR, OUTPUT_DIR, file_names, isRGB, cfg, wts, model_shape, VERBOSE, device, contract, stack,
                                  frames, records)
        else:
            done = _run_streaming(DATA_DIR, OUTPUT_DIR, file_names, isRGB, cfg, wts, model_shape, VERBOSE, device, contract, stack,
                                  frames)
        if done:
            return

    def read(name):
        try:
            with open(os.path.join(DATA_DIR, name), mode='rb') as f:
                return zstd.decompress(f.read())
        except FileNotFoundError:
            print("ERROR: No such file or directory:", os.path.join(DATA_DIR, name))
            exit()

    keys = None
    try:
        with open(os.path.join(DATA_DIR, "key_frame.dat"), mode='rb') as f:
            # this build's opt-in key-frame file: validated here, expanded on the device below
            keys = parse_coded_keys(f.read(4), os.path.join(DATA_DIR, "key_frame.dat"))
    except FileNotFoundError:
        pass   # (read() below prints the reference's message)
    if keys is not None and job is not None:
        print("ERROR: a GPU-coded key_frame.dat (--key-coder huff / huffg) cannot be decoded by a sharded job (WORLD_SIZE > 1): run it on one GPU")
        sys.exit(2)
    key_bytes = None if keys is not None else read("key_frame.dat")
    key_len = keys.nt * keys.H * keys.W * 3 if keys is not None else len(key_bytes)   # (the zero-except-keys stack's size)
    coded = None
    try:
        with open(os.path.join(DATA_DIR, "entropy.dat"), mode='rb') as f:
            fmt = coded_format(f.read(4))
            if fmt is not None:           # this build's opt-in Huffman file: validated here, expanded on the device below
                coded = fmt.parse(np.fromfile(os.path.join(DATA_DIR, "entropy.dat"), np.uint8), key_len)
    except FileNotFoundError:
        pass   # (read() below prints the reference's message)
    if coded is not None:
        if job is not None:
            print("ERROR: a Huffman-coded entropy.dat cannot be decoded by a sharded job (WORLD_SIZE > 1): run it on one GPU")
            sys.exit(2)
        payload, table, shape, warm_up = None, coded.table, coded.shape, coded.warm_up
    else:
        payload, table, shape, warm_up = parse_stream(read("entropy.dat"))
        check_stream((predmotion.select_mark(shape[0]),) + tuple(shape[1:]), warm_up, payload.size, key_len)   # (a motion mark: as its layout's select mark)
    tile_pred = stream_pred_or_exit(DATA_DIR, *shape[:4])
    shape = (predmotion.closed_mark(shape[0]),) + tuple(shape[1:])
    closed = check_loop(DATA_DIR, shape[0])
    shape = (closedloop.open_mark(shape[0]),) + tuple(shape[1:])
    if closed and job is not None:
        print("ERROR:", closedloop.NO_SHARDED_DECODE)
        sys.exit(2)
    if closed:
        refuse_closed_range(frames)
    _, nt, H, W, C = shape
    check_channels(DATA_DIR, C)
    if C == 1 and job is not None:
        print("ERROR: a one-channel payload (--gray) cannot be decoded by a sharded job (WORLD_SIZE > 1): run it on one GPU")
        sys.exit(2)
    stride_mode = check_sdelta(DATA_DIR, shape[0])
    if stride_mode and job is not None:
        print("ERROR: a %s payload (--sdelta %s) cannot be decoded by a sharded job (WORLD_SIZE > 1): run it on one GPU"
              % (("channel-stride", "channel") if stride_mode == 1 else ("plane", "plane")))
        sys.exit(2)
    key_frames = None if keys is not None else np.frombuffer(key_bytes, dtype=np.uint8).reshape(nt, H, W, 3)
    hp, wp = padding_shape(H, W)
    if model_shape is not None and (model_shape[0] != hp or model_shape[1] != wp):
        print("ERROR:keyframe size and model size do not match.")
        print("model size: height ", model_shape[0] - 7, "～", model_shape[0], " width ", model_shape[1] - 7, "～", model_shape[1])
        print("key frame size: height ", H, " width ", W)
        exit()
    if len(file_names) != nt:
        print("ERROR：The lengths of filename.txt and images do not match.")
        print("filename.txt：", len(file_names))
        print("number of images", nt)
        exit()
    if frames is not None:
        check_frames(frames, nt)
    if records is not None:
        check_records(records, nt, H, W)

    if job:
        device = tzdist.init_from_env()
    ctx = make_context(cfg, wts, hp, wp, 64 if nt > 64 else max(1, nt), device)
    first = 0           # index of frames[0] in the sequence: a rank of a sharded job holds (and saves) its own windows only
    try:
        if contract:
            ctx.set_contract(contract)
        ctx.set_payload_channels(C)
        set_sdelta(ctx, stride_mode)
        if sdelta.is_shuffled(shape[0]):  # this build's opt-in byte planes -> the int16 payload
            payload = ctx.byte_unshuffle(np.ascontiguousarray(payload).view(np.uint8))
        if job:
            # key intervals sharded over the ranks (tezip_amd/dist.py); no frame travels: each rank saves its own
            first, _, frames = tzdist.decompress_sharded(tzdist.HipEngine(ctx, device), key_frames, payload, table, warm_up,
                                                         gather=False)
        else:
            if VERBOSE:
                ctx.prof_enable(True)
            t0 = time.time()
            tb = None if table is None else np.ascontiguousarray(table)
            first, end = frames or (0, nt)
            if keys is not None:    # the same C calls as the streaming path; the stack stays on the device
                stage_coded_keys(ctx, keys, (nt, H, W))
            kf = None if keys is not None else np.ascontiguousarray(key_frames)
            if not closed:   # (tz_rollout_decode_closed reads the payload in every step: it runs once that is staged)
                ctx.rollout_decode_range(kf, warm_up, first, end - first)
                if VERBOSE:
                    print("predict:{0}".format(time.time() - t0) + "[sec]")
            if coded is not None:
                begin, put, expand = coded_calls(ctx, coded)
                begin(coded.body.size, coded.n, coded.lengths, coded.base, run=coded.run)
                put(0, np.ascontiguousarray(coded.body))
                expand()
            if closed:   # TZ-PS1 / TZ-PM1: the stored modes (and vectors) pick every tile's prediction
                put_pred(ctx, *tile_pred)
            if closed:
                ctx.rollout_decode_closed(kf, warm_up, None if coded is not None else np.ascontiguousarray(payload), tb)
                if VERBOSE:
                    print("predict:{0}".format(time.time() - t0) + "[sec]")
                frames = ctx.decoded_get(0, nt)
            else:
                frames = ctx.decode_range(None if coded is not None else np.ascontiguousarray(payload), tb, first, end - first)
            if VERBOSE:
                prof = ctx.prof_get()
                if table is not None:
                    print("replacing_based_on_frequency:{0}".format(prof["lut_remap"][0] / 1e3) + "[sec]")
                print("finding_difference:{0}".format(prof["undelta_scan"][0] / 1e3) + "[sec]")
            if records is not None:   # the whole-array path: the digests of what it decoded (tz_frame_digests), before any image
                verify_frames(records, ctx.frame_digests(frames), first, file_names)
    finally:
        ctx.close()

    from concurrent.futures import ThreadPoolExecutor
    from PIL import Image
    from .compress import _log_io, io_threads
    if rank0:
        print("save as RGB" if isRGB else "save as gray")

    def save(j):
        # decompress.py:272-278: the grayscale save is overwritten by an unconditional RGB save
        Image.fromarray(frames[j]).save(os.path.join(OUTPUT_DIR, file_names[first + j]))

    if job:
        # the ranks meet once more so that none returns (and the launcher none reports success) before every file is
        # written -- or learns that a rank could not
        import torch.distributed as dist
        err = None
        try:
            with ThreadPoolExecutor(max_workers=io_threads()) as pool:
                list(pool.map(save, range(len(frames))))
        except Exception as e:
            err = e
        _log_io("decompress", job, [(first, first + len(frames))])
        try:
            tzdist._all_ok(err is None, dist, "writing the decoded images")
        except RuntimeError:
            if err is not None:
                raise err
            raise
        return
    with ThreadPoolExecutor(max_workers=io_threads()) as pool:  # PIL's encoder releases the GIL
        list(pool.map(save, range(len(frames))))
