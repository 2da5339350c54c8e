"""TEZIP command line for the MI355X build.

Behaviourally equivalent to the reference CLI (/root/reference/src/tezip.py:10-100): same
flags, same validation order and the same messages on stdout, process exit code 0 on
validation errors.  The structure is this build's own: flags come from a table, validation is a
list of (predicate, message key) rules evaluated in the reference's order, and the device probe
asks the HIP library instead of TensorFlow.  `-l` trains with tezip_amd/train.py (PyTorch
autograd) on .npy stacks written by tezip_amd/train_data_create.py.
"""
import argparse
import os
import sys

if __package__ in (None, ""):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    __package__ = "tezip_amd"

from . import boundmap, closedframes, closedloop, closedmap, compress, decompress, frametarget, predmotion, predselect, sdauto, target, train  # noqa: E402

# (short, long, argparse keywords) -- tezip.py:88-99
FLAG_TABLE = (
    ("-l", "--learn", dict(type=str, nargs=2, metavar=("model", "dir"), dest="learn")),
    ("-c", "--compress", dict(type=str, nargs=3, metavar=("model", "dir", "file"), dest="compress")),
    ("-u", "--uncompress", dict(type=str, nargs=3, metavar=("model", "file", "dir"), dest="uncompress")),
    ("-p", "--preprocess", dict(type=int, nargs=1, metavar="warm_up_num", dest="preprocess")),
    ("-w", "--window", dict(type=int, nargs=1, metavar="window_size", dest="window")),
    ("-t", "--threshold", dict(type=float, nargs=1, metavar="MSE_threshold", dest="threshold")),
    ("-m", "--mode", dict(type=str, nargs=1, metavar="mode", dest="mode")),
    ("-b", "--bound", dict(type=float, nargs="*", metavar="value", dest="bound", default=None)),
    ("-f", "--force", dict(action="store_true")),
    ("-v", "--verbose", dict(action="store_true")),
    ("-n", "--no_entropy", dict(action="store_false")),  # store_false: entropy remap is on by default
    # not in the reference: compress once per candidate -w and keep the smallest output (BASELINE.json configs[4];
    # tezip_amd/sweep.py).  No value = 5 10 15 20 25 30 35 40.  Takes the place of -w / -t.
    # not in the reference: byte-shuffled payload (flagged in the trailer; the reference cannot read such a file)
    (None, "--shuffle", dict(action="store_true")),
    (None, "--sweep", dict(type=int, nargs="*", metavar="window_size", dest="sweep", default=None)),
    # not in the reference: the predictor's arithmetic contract.  0 / absent = by frame size (TZ-PA2 from
    # 256x256 pixels on), 1 = TZ-PA1 (what files compressed by builds before round 4 need for -u), 2 = TZ-PA2.  The same
    # value must be given to -c and -u: the reference's file format has no field for it.
    (None, "--pa", dict(type=int, choices=(0, 1, 2), default=None, dest="pa")),
    # not in the reference: with -u, write only frames A:B (half-open, either end may be omitted) or the one frame N of
    # the sequence, decoded without rolling out, scanning and saving the others (decompress.run(frames=...))
    (None, "--frames", dict(type=str, default=None, metavar="A:B", dest="frames")),
    # not in the reference: with -c, also write quality.json (the error the bound introduced, per frame and for the
    # sequence, from the stored payload decoded on the GPU) and print max_abs_err / PSNR / ratio (compress.run(REPORT=...))
    (None, "--report", dict(action="store_true", dest="report")),
    # not in the reference: with -c --report, the report also carries the structural similarity (SSIM, definition TZ-SSIM-1 in
    # tezip_amd/ssim.py) of what the stored payload decodes to against the sources, per frame and for the sequence, computed on
    # the GPU (compress.run(SSIM=True)); `python -m tezip_amd.ssim IMAGES RESTORED` gives the same figures after a -u
    (None, "--ssim", dict(action="store_true", dest="ssim")),
    # not in the reference: with -c, the coder of entropy.dat.  zstd = the reference's file; huff = canonical Huffman codes
    # written by the GPU (tezip_amd/huff.py; the reference cannot read such a file, -u recognises it by its magic); huffr = the
    # same with repeat tokens for the payload's period-3 runs (tezip_amd/huffr.py), a smaller file under an error bound; huffd =
    # one coder over both: it counts the payload at match distance none / 1 / 3 and codes at the cheapest (tezip_amd/huffd.py)
    (None, "--coder", dict(type=str, choices=("zstd", "huff", "huffr", "huffd"), default="zstd", dest="coder")),
    # not in the reference: with -c, the coder of key_frame.dat.  zstd = the reference's file; huff = the key frames alone, as
    # predictor residuals Huffman-coded by the GPU (tezip_amd/keycoder.py; the reference cannot read such a file, -u recognises
    # it by its magic).  Much smaller on smooth frames, LARGER than zstd on sparse ones (README): check with --report's ratio.
    # huffg = huff with every gray key frame (a single-channel source, widened to RGB) coded as one channel (tezip_amd/keycoderg.py)
    (None, "--key-coder", dict(type=str, choices=("zstd", "huff", "huffg"), default="zstd", dest="key_coder")),
    # not in the reference: with -c, also write frame_digests.json (tezip_amd/digest.py): per frame the digest of what the stored
    # payload decodes to and of the source frame, taken on the GPU (compress.run(DIGESTS=True)).  The other files do not change
    (None, "--digests", dict(action="store_true", dest="digests")),
    # not in the reference: with -c, store ONE payload channel in entropy.dat when every frame of the job is gray (a
    # single-channel source, widened to RGB: tezip_amd/graypayload.py; the reference cannot read such a file, -u recognises it by
    # the shape in its trailer).  A job with colour writes exactly the files it writes without the flag
    (None, "--gray", dict(action="store_true", dest="gray")),
    # not in the reference: with -u, what to do about frame_digests.json.  auto (also when the flag is absent) = when the file
    # is there, the decoded frames are checked against it on the GPU before an image is written (a mismatch: exit status 3, no
    # image); require = the same, and a directory without the file is refused; off = never check (salvage a damaged directory)
    (None, "--verify", dict(type=str, choices=decompress.VERIFY_MODES, default=None, dest="verify")),
    # not in the reference: with -c, the stride of the payload's spatial delta.  flat (also when the flag is absent) = the
    # reference's finding_difference, whose neighbour of a sample is another channel of the same pixel; channel = the same channel
    # of the pixel in front (tezip_amd/sdelta.py; smaller on colour jobs, LARGER on a gray source stored with three channels: use
    # --gray there; the reference cannot read such a file, -u recognises it by the mark in its trailer); plane = the 2-D predictor
    # left + up - upleft per frame and channel, TZ-SD2 (smaller on smooth colour data lossless and under --quant lattice, LARGER
    # under the greedy quantiser from abs 6 on and on sparse or gray sources: README; not with --sweep, --target-ratio or a
    # sharded job); auto (with --coder huff / huffr / huffd) = the one of the three under which this job's entropy.dat is
    # smallest, known exactly from one more pass over the quantised deltas (definition TZ-SDA1 in tezip_amd/sdauto.py; every file
    # is what `--sdelta <chosen>` writes; not with --shuffle, --sweep, --target-ratio or a sharded job)
    (None, "--sdelta", dict(type=str, choices=("flat", "channel", "plane", "auto"), default=None, dest="sdelta")),
    # not in the reference: with -c, IN PLACE of -m and -b: the job is `-m abs -b E` with the E (a multiple of 0.5) that a
    # bisection over the GPU's exact error sums finds for a sequence PSNR of at least DB (definition TZ-TPSNR-1 in
    # tezip_amd/target.py: one rollout, at most 9 probes; a boundary, not necessarily the largest such bound).  Also writes
    # bound_search.json (compress.run(TARGET_PSNR=...))
    (None, "--target-psnr", dict(type=float, default=None, metavar="DB", dest="target_psnr")),
    # not in the reference: with -c and --coder huff / huffr / huffd, IN PLACE of -m and -b: the job is `-m abs -b E` with the E (a
    # multiple of 0.5) at which the files first fit into 1/R of the frames' bytes, found by a bisection over the exact size the
    # GPU computes for a candidate's entropy.dat without writing it (definition TZ-TRATIO-1 in tezip_amd/ratetarget.py: one
    # rollout, at most 11 probes; a boundary, not necessarily the smallest such bound).  Also writes bound_search.json; a
    # target that abs 255 misses ends the job with exit status 4 (compress.run(TARGET_RATIO=...))
    (None, "--target-ratio", dict(type=float, default=None, metavar="R", dest="target_ratio")),
    # not in the reference: with -c --target-psnr DB: the target holds in EVERY frame that is not stored exactly (frame 0, warm-up
    # and key frames are).  Each such frame gets an abs bound of its own (a multiple of 0.5) from a bisection of its own, all
    # driven by the same at most 9 probes (definition TZ-TPSNR-F1 in tezip_amd/frametarget.py; per frame a boundary, not
    # necessarily the largest such bound).  The files are ordinary ones: -u needs no flag (compress.run(PER_FRAME=True))
    (None, "--per-frame", dict(action="store_true", dest="per_frame")),
    # not in the reference: with -c -m abs, IN PLACE of -b: one abs bound per image from a JSON file, a list of numbers or an
    # object with a "frame_bounds" list (the bound_search.json of a --per-frame job replays); 0 keeps a frame lossless; entries
    # at frames that are stored exactly are taken as 0 (compress.run(FRAME_BOUNDS=FILE))
    (None, "--frame-bounds", dict(type=str, default=None, metavar="FILE", dest="frame_bounds")),
    # not in the reference: with -c -m abs, IN PLACE of -b: one abs bound per PIXEL from a map of the images' own size -- a .npy
    # holding a 2-D uint8 array, or an image with one channel (or three equal ones); 0 keeps a pixel exact in every frame
    # (definition TZ-BM1 in tezip_amd/boundmap.py).  The files are ordinary ones: -u needs no flag (compress.run(BOUND_MAP=FILE))
    (None, "--bound-map", dict(type=str, default=None, metavar="FILE", dest="bound_map")),
    # not in the reference: with -c, the quantiser of a lossy job.  greedy (also when the flag is absent) = the reference's
    # error_bound, which merges runs of neighbouring deltas; lattice = every delta on its own to the nearest multiple of
    # 2 floor(E) + 1 under the same tolerance E (definition TZ-QL1 in tezip_amd/lattice.py; smaller on data that is not smooth,
    # LARGER on sparse frames at loose bounds, and at tight bounds about 2 dB less PSNR for the same worst-case error: README).
    # The files are ordinary ones: -u needs no flag (compress.run(QUANT=...))
    (None, "--quant", dict(type=str, choices=("greedy", "lattice"), default=None, dest="quant")),
    # not in the reference: with -c, what the predictor is fed inside a window.  open (also when the flag is absent) = its own last
    # prediction (compress.py:230); closed = the DECODED frame in front, which the decoder holds anyway: every prediction is a
    # one-step prediction (definition TZ-CL1 in tezip_amd/closedloop.py; smaller files with a trained model, README).  With -w and
    # -m abs, lossless or with --quant lattice; not with -t, --sweep, --gray, a target, --per-frame, --frame-bounds, --bound-map
    # or a sharded job.  -u recognises the stream by the mark in its trailer (compress.run(LOOP=...))
    (None, "--loop", dict(type=str, choices=("open", "closed"), default=None, dest="loop")),
    # not in the reference: with -c --loop closed, what a 16 x 16 tile of a predicted frame is predicted from.  net (also when the
    # flag is absent) = the network, today's job byte for byte; select = whichever of the network and the decoded frame in front
    # leaves the smaller quantised residual, one bit per tile in a fifth file pred_modes.dat (definition TZ-PS1 in
    # tezip_amd/predselect.py; in a lossless job no tile's residual grows in L1 norm, which promises nothing about bytes: README).
    # motion = select with the frame in front displaced per tile by a vector of up to 7 pixels found by a full search; the file also
    # holds one byte per chosen tile (definition TZ-PM1 in tezip_amd/predmotion.py).
    # -u recognises the stream by the mark in its trailer (compress.run(PRED=...))
    (None, "--pred", dict(type=str, choices=("net", "select", "motion"), default=None, dest="pred")),
    # not in the reference: with -c --loop closed --quant lattice, IN PLACE of -m and -b: every frame that is not stored exactly
    # reaches DB dB.  The ONE closed-loop rollout finds each frame's abs bound (a multiple of 0.5) when the loop stands at that
    # frame, where its prediction no longer depends on anything undecided (definition TZ-CLF1 in tezip_amd/closedframes.py; per
    # frame a boundary, greedy in time).  bound_search.json holds the search; -u needs no flag (compress.run(LOOP_PSNR=DB))
    (None, "--loop-psnr", dict(type=float, default=None, metavar="DB", dest="loop_psnr")),
    # not in the reference: with -c --loop closed --quant lattice -m abs, IN PLACE of -b: one abs bound per image for the closed
    # loop, from a JSON file as --frame-bounds reads it (the bound_search.json of a --loop-psnr job replays); entries at frames that
    # are stored exactly are taken as 0 (compress.run(LOOP_BOUNDS=FILE))
    (None, "--loop-bounds", dict(type=str, default=None, metavar="FILE", dest="loop_bounds")),
    # not in the reference: with -c --loop closed --quant lattice -m abs, IN PLACE of -b: one abs bound per pixel for the closed
    # loop, from what --bound-map reads (a .npy holding a 2-D uint8 array, or a single-channel image of the images' own size); with
    # --pred select the tiles are chosen under that map (definition TZ-CLM1 in tezip_amd/closedmap.py).  -u needs no flag
    # (compress.run(LOOP_MAP=FILE))
    (None, "--loop-map", dict(type=str, default=None, metavar="FILE", dest="loop_map")),
)

TEXT = {
    "several": ("Please select only one of learn or compress or uncompress.",
                "Command to check the options is -h or --help"),
    "nothing": ("Please mode select!", "learn or compress or uncompress.",
                "Command to check the options is -h or --help"),
    "no_p": ("Please specify the -p or --preprocess option!", "warm up num."),
    "no_window": ("Please specify the window size(-w or --window) or MSE threshold(-t or --threshold) option!",
                  "Select window size for SWP and MSE threshold for DWP."),
    "two_windows": ("Please select only one of window size(-w or --window) or MSE threshold(-t or --threshold)!",
                    "Select window size for SWP and MSE threshold for DWP."),
    "bad_mode": ("Please specify the -m or --mode correctly!", "'abs' or 'rel' or 'absrel' or 'pwrel'."),
    "no_bound": ("Please specify the -b or --bound option!", "error bound value."),
    "bound_count": ("If the -m or --mode is 'abs' or 'rel' or 'pwrel', enter one for -b or --bound. : value",
                    "If the -m or --mode is 'absrel', enter two in -b or --bound. : abs_value rel_value"),
}
BOUNDS_WANTED = {"abs": 1, "rel": 1, "pwrel": 1, "absrel": 2}


def build_parser():
    parser = argparse.ArgumentParser(prog="TEZIP", formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    for short, long_, kw in FLAG_TABLE:
        parser.add_argument(*([short, long_] if short else [long_]), **kw)
    return parser


def parse_frames(spec):
    """--frames SPEC -> (A, B) with B None for "to the end"; "N" is N:N+1.  Raises ValueError for a malformed spec or
    negative indices (the bound against the sequence length is checked once filename.txt is read)."""
    spec = spec.strip()
    try:
        if ":" in spec:
            a, b = spec.split(":")
            a = int(a) if a.strip() else 0
            b = int(b) if b.strip() else None
        else:
            a = int(spec)
            b = a + 1
    except ValueError:
        raise ValueError("--frames takes A:B (either end may be omitted) or N, got %r" % spec) from None
    if a < 0 or (b is not None and b < 0):
        raise ValueError("--frames indices must be non-negative, got %r" % spec)
    if b is not None and b <= a:
        raise ValueError("--frames %r is an empty range" % spec)
    return a, b


def check_frames_flag(arg):
    """--frames is valid with -u only.  Returns (frames, None), or (None, message) for a refusal."""
    spec = getattr(arg, "frames", None)
    if spec is None:
        return None, None
    if arg.uncompress is None or arg.learn is not None or arg.compress is not None:
        return None, "--frames is valid with -u (--uncompress) only"
    try:
        return parse_frames(spec), None
    except ValueError as e:
        return None, str(e)


def check_report_flag(arg):
    """--report is valid with -c of one single-GPU job only.  Returns None, or the message of a refusal."""
    if not getattr(arg, "report", False):
        return None
    if arg.compress is None or arg.uncompress is not None or arg.learn is not None:
        return "--report is valid with -c (--compress) only"
    if getattr(arg, "sweep", None) is not None:
        return "--report cannot be combined with --sweep"
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        return "--report is not available for a sharded job (WORLD_SIZE > 1): run it on one GPU"
    return None


def check_coder_flag(arg):
    """--coder huff / huffr / huffd is valid with -c of one single-GPU job, without --shuffle and --sweep.  Returns None, or the message
    of a refusal."""
    if getattr(arg, "coder", "zstd") == "zstd":
        return None
    if arg.compress is None or arg.uncompress is not None or arg.learn is not None:
        return "--coder is valid with -c (--compress) only (-u recognises the coder of a file by itself)"
    if getattr(arg, "sweep", None) is not None:
        return "--coder %s cannot be combined with --sweep" % arg.coder
    return compress.check_coder(arg.coder, arg.shuffle, int(os.environ.get("WORLD_SIZE", "1")) > 1)


def check_key_coder_flag(arg):
    """--key-coder huff / huffg is valid with -c of one single-GPU job, without --sweep.  Returns None, or the message of a refusal."""
    if getattr(arg, "key_coder", "zstd") == "zstd":
        return None
    if arg.compress is None or arg.uncompress is not None or arg.learn is not None:
        return "--key-coder is valid with -c (--compress) only (-u recognises the coder of a file by itself)"
    if getattr(arg, "sweep", None) is not None:
        return "--key-coder %s cannot be combined with --sweep" % arg.key_coder
    return compress.check_key_coder(arg.key_coder, int(os.environ.get("WORLD_SIZE", "1")) > 1)


def check_digests_flag(arg):
    """--digests is valid with -c of one single-GPU job, without --sweep.  Returns None, or the message of a refusal."""
    if not getattr(arg, "digests", False):
        return None
    if arg.compress is None or arg.uncompress is not None or arg.learn is not None:
        return "--digests is valid with -c (--compress) only"
    if getattr(arg, "sweep", None) is not None:
        return "--digests cannot be combined with --sweep"
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        return "--digests is not available for a sharded job (WORLD_SIZE > 1): run it on one GPU"
    return None


def check_ssim_flag(arg):
    """--ssim is valid with -c --report of one single-GPU job only.  Returns None, or the message of a refusal."""
    if not getattr(arg, "ssim", False):
        return None
    if arg.compress is None or arg.uncompress is not None or arg.learn is not None:
        return "--ssim is valid with -c (--compress) --report only"
    if getattr(arg, "sweep", None) is not None:
        return "--ssim cannot be combined with --sweep"
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        return "--ssim is not available for a sharded job (WORLD_SIZE > 1): run it on one GPU"
    if not getattr(arg, "report", False):
        return compress.SSIM_NEEDS_REPORT
    return None


def check_gray_flag(arg):
    """--gray is valid with -c of one single-GPU job, without --sweep.  Returns None, or the message of a refusal."""
    if not getattr(arg, "gray", False):
        return None
    if arg.compress is None or arg.uncompress is not None or arg.learn is not None:
        return "--gray is valid with -c (--compress) only (-u recognises a one-channel payload by itself)"
    if getattr(arg, "sweep", None) is not None:
        return "--gray cannot be combined with --sweep"
    return compress.check_gray(True, int(os.environ.get("WORLD_SIZE", "1")) > 1)


def check_sdelta_flag(arg):
    """--sdelta is valid with -c only; `channel`, `plane` and `auto` need one single-GPU job without --sweep, `plane` and `auto`
    one without --target-ratio, `auto` a GPU coder and no --shuffle.  Returns None, or the message of a refusal."""
    mode = getattr(arg, "sdelta", None)
    if mode is None:
        return None
    if arg.compress is None or arg.uncompress is not None or arg.learn is not None:
        return "--sdelta is valid with -c (--compress) only (-u recognises a channel-stride payload by itself)"
    if mode == sdauto.MODE:   # the size of the job's own entropy.dat decides: a GPU coder, one job, one GPU, a given bound
        if getattr(arg, "sweep", None) is not None:
            return "--sdelta auto cannot be combined with --sweep: run the job you want with -w or -t"
        return sdauto.check(getattr(arg, "coder", "zstd"), arg.shuffle, int(os.environ.get("WORLD_SIZE", "1")) > 1,
                            getattr(arg, "target_ratio", None))
    if mode in ("channel", "plane") and getattr(arg, "sweep", None) is not None:
        return "--sdelta %s cannot be combined with --sweep" % mode
    if mode == "plane" and getattr(arg, "target_ratio", None) is not None:
        return compress.PLANE_NO_RATIO
    return compress.check_sdelta(mode, int(os.environ.get("WORLD_SIZE", "1")) > 1)


def check_quant_flag(arg):
    """--quant is valid with -c only; `lattice` needs one single-GPU job without --sweep.  Returns None, or the message of a
    refusal."""
    quant = getattr(arg, "quant", None)
    if quant is None:
        return None
    if arg.compress is None or arg.uncompress is not None or arg.learn is not None:
        return "--quant is valid with -c (--compress) only (-u decodes such a job without a flag)"
    if quant == "lattice" and getattr(arg, "sweep", None) is not None:
        return "--quant lattice cannot be combined with --sweep"
    return compress.check_quant(quant, int(os.environ.get("WORLD_SIZE", "1")) > 1)


def check_loop_flag(arg):
    """--loop is valid with -c only; `closed` needs one single-GPU SWP job under one abs bound (lossless, or --quant lattice).
    Returns None, or the message of a refusal."""
    loop = getattr(arg, "loop", None)
    if loop is None:
        return None
    if arg.compress is None or arg.uncompress is not None or arg.learn is not None:
        return closedloop.NEEDS_COMPRESS
    return closedloop.check_flags(loop, arg.mode[0] if arg.mode else None, arg.bound or [], getattr(arg, "quant", None),
                                  arg.threshold[0] if arg.threshold is not None else None, getattr(arg, "sweep", None) is not None,
                                  int(os.environ.get("WORLD_SIZE", "1")) > 1, bool(getattr(arg, "gray", False)),
                                  getattr(arg, "target_psnr", None), getattr(arg, "target_ratio", None),
                                  bool(getattr(arg, "per_frame", False)), getattr(arg, "frame_bounds", None),
                                  getattr(arg, "bound_map", None))


def check_closedframes_flags(arg):
    """--loop-psnr and --loop-bounds go with -c --loop closed --quant lattice of one single-GPU job, in place of -b (and of -m for
    --loop-psnr).  The file of --loop-bounds is read here (its length is checked once the images are listed).  Returns None, or
    the message of a refusal."""
    db, path = getattr(arg, "loop_psnr", None), getattr(arg, "loop_bounds", None)
    if db is None and path is None:
        return None
    problem = closedframes.check_flags(
        db, path, getattr(arg, "loop", None), getattr(arg, "quant", None), arg.mode[0] if arg.mode else None, arg.bound or [],
        getattr(arg, "pred", None), arg.compress is not None and arg.uncompress is None and arg.learn is None,
        getattr(arg, "sweep", None) is not None, int(os.environ.get("WORLD_SIZE", "1")) > 1, bool(getattr(arg, "gray", False)),
        arg.threshold[0] if arg.threshold is not None else None, getattr(arg, "target_psnr", None), getattr(arg, "target_ratio", None),
        bool(getattr(arg, "per_frame", False)), getattr(arg, "frame_bounds", None), getattr(arg, "bound_map", None))
    if problem or path is None:
        return problem
    try:
        closedframes.load(path)
    except ValueError as e:
        return str(e)
    return None


def check_closedmap_flag(arg):
    """--loop-map goes with -c --loop closed --quant lattice -m abs of one single-GPU job, in place of -b.  The file is read here
    (its size is checked once the images are listed).  Returns None, or the message of a refusal."""
    path = getattr(arg, "loop_map", None)
    if path is None:
        return None
    problem = closedmap.check_flags(
        path, getattr(arg, "loop", None), getattr(arg, "quant", None), arg.mode[0] if arg.mode else None, arg.bound or [],
        getattr(arg, "pred", None), arg.compress is not None and arg.uncompress is None and arg.learn is None,
        getattr(arg, "sweep", None) is not None, int(os.environ.get("WORLD_SIZE", "1")) > 1, bool(getattr(arg, "gray", False)),
        arg.threshold[0] if arg.threshold is not None else None, getattr(arg, "target_psnr", None), getattr(arg, "target_ratio", None),
        bool(getattr(arg, "per_frame", False)), getattr(arg, "frame_bounds", None), getattr(arg, "bound_map", None),
        getattr(arg, "loop_psnr", None), getattr(arg, "loop_bounds", None))
    if problem:
        return problem
    try:
        closedmap.load(path)
    except ValueError as e:
        return str(e)
    return None


def check_pred_flag(arg):
    """--pred is valid with -c only; `select` and `motion` need --loop closed.  Returns None, or the message of a refusal."""
    pred = getattr(arg, "pred", None)
    if pred is None:
        return None
    if arg.compress is None or arg.uncompress is not None or arg.learn is not None:
        return predselect.NEEDS_COMPRESS
    return predmotion.check_flags(pred, getattr(arg, "loop", None) or "open")


def check_target_flag(arg):
    """--target-psnr is valid with -c of one single-GPU job, in place of -m and -b, without --sweep.  Returns None, or the
    message of a refusal."""
    db = getattr(arg, "target_psnr", None)
    if db is None:
        return None
    if arg.compress is None or arg.uncompress is not None or arg.learn is not None:
        return "--target-psnr is valid with -c (--compress) only"
    if getattr(arg, "sweep", None) is not None:
        return "--target-psnr cannot be combined with --sweep"
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        return compress.TARGET_NOT_SHARDED
    if arg.mode is not None or arg.bound is not None:
        return compress.TARGET_NEEDS_ABS
    return target.check_target(db)


def check_ratio_flag(arg):
    """--target-ratio is valid with -c of one single-GPU job with a GPU coder, in place of -m, -b and --target-psnr, without
    --sweep and --shuffle.  Returns None, or the message of a refusal."""
    ratio = getattr(arg, "target_ratio", None)
    if ratio is None:
        return None
    if arg.compress is None or arg.uncompress is not None or arg.learn is not None:
        return "--target-ratio is valid with -c (--compress) only"
    if getattr(arg, "sweep", None) is not None:
        return "--target-ratio cannot be combined with --sweep"
    return compress.check_ratio(ratio, "abs" if arg.mode is None else None, arg.bound, getattr(arg, "target_psnr", None),
                                getattr(arg, "coder", "zstd"), arg.shuffle, int(os.environ.get("WORLD_SIZE", "1")) > 1)


def check_frame_bounds_flags(arg):
    """--per-frame goes with -c --target-psnr, --frame-bounds with -c -m abs in place of -b; both need one single-GPU job without
    --sweep.  The file of --frame-bounds is read here (its length is checked once the images are listed).  Returns None, or the
    message of a refusal."""
    per_frame, path = bool(getattr(arg, "per_frame", False)), getattr(arg, "frame_bounds", None)
    if not per_frame and path is None:
        return None
    flag = "--per-frame" if per_frame else "--frame-bounds"
    if arg.compress is None or arg.uncompress is not None or arg.learn is not None:
        return "%s is valid with -c (--compress) only (-u decodes such a job without a flag)" % flag
    if getattr(arg, "sweep", None) is not None:
        return "%s cannot be combined with --sweep" % flag
    problem = frametarget.check(per_frame, path, "abs" if per_frame and arg.mode is None else (arg.mode[0] if arg.mode else None),
                                arg.bound, getattr(arg, "target_psnr", None), getattr(arg, "target_ratio", None),
                                int(os.environ.get("WORLD_SIZE", "1")) > 1)
    if problem or path is None:
        return problem
    try:
        frametarget.load(path)
    except ValueError as e:
        return str(e)
    return None


def check_bound_map_flag(arg):
    """--bound-map goes with -c -m abs in place of -b and of every way to find a bound; one single-GPU job without --sweep.  The
    file is read here (its size is checked once the images are listed).  Returns None, or the message of a refusal."""
    path = getattr(arg, "bound_map", None)
    if path is None:
        return None
    if arg.compress is None or arg.uncompress is not None or arg.learn is not None:
        return boundmap.NEEDS_COMPRESS
    if getattr(arg, "sweep", None) is not None:
        return boundmap.NO_SWEEP
    problem = boundmap.check_flags(path, arg.mode[0] if arg.mode else None, arg.bound, getattr(arg, "target_psnr", None),
                                   getattr(arg, "target_ratio", None), bool(getattr(arg, "per_frame", False)),
                                   getattr(arg, "frame_bounds", None), int(os.environ.get("WORLD_SIZE", "1")) > 1)
    if problem:
        return problem
    try:
        boundmap.load(path)
    except ValueError as e:
        return str(e)
    return None


def check_verify_flag(arg):
    """--verify is valid with -u only; `require` needs frame_digests.json in the directory and one GPU.  Returns None, or the
    message of a refusal."""
    mode = getattr(arg, "verify", None)
    if mode is None:
        return None
    if arg.uncompress is None or arg.learn is not None or arg.compress is not None:
        return "--verify is valid with -u (--uncompress) only"
    return decompress.check_verify(mode, arg.uncompress[1], int(os.environ.get("WORLD_SIZE", "1")) > 1)


def probe_gpu(force_cpu):
    """tezip.py:12-21 asked TensorFlow for a GPU; here a context on device 0 must open."""
    if force_cpu:
        return False
    try:
        from . import _lib
        _lib.Context(0).close()
        return True
    except Exception:
        return False


def complain(key):
    print("ERROR")
    for line in TEXT[key]:
        print(line)


def check_compress(arg):
    """Reference order (tezip.py:40-84).  Returns None when the request is complete, else the key
    of the message to print; prints the mode name where the reference does."""
    if arg.preprocess is None:
        return "no_p"
    have_sweep = getattr(arg, "sweep", None) is not None
    have_w, have_t = arg.window is not None or have_sweep, arg.threshold is not None
    if not have_w and not have_t:
        return "no_window"
    if (have_w and have_t) or (have_sweep and arg.window is not None):  # --sweep takes the place of -w / -t: not beside them
        return "two_windows"
    if arg.mode is None:  # the reference raises a TypeError here; report it as a bad mode instead
        return "bad_mode"
    print(arg.mode[0])
    if arg.mode[0] not in BOUNDS_WANTED:
        return "bad_mode"
    if not arg.bound:
        return "no_bound"
    if len(arg.bound) != BOUNDS_WANTED[arg.mode[0]]:
        return "bound_count"
    return None


def _main(arg):
    frames, problem = check_frames_flag(arg)
    if problem:   # exit status 2, as decompress.adopt_contract's errors: nothing was written
        print("ERROR:", problem)
        sys.exit(2)
    problem = check_closedmap_flag(arg)
    if problem:   # likewise (in front of every other check: a refusal of this job names the flag that defines it)
        print("ERROR:", problem)
        sys.exit(2)
    problem = check_closedframes_flags(arg)
    if problem:   # likewise (in front of --loop's check: a refusal of this job names the flag that defines it)
        print("ERROR:", problem)
        sys.exit(2)
    problem = check_loop_flag(arg)
    if problem:   # likewise (in front of the other flags' checks: a refusal of this job names the flag that defines it)
        print("ERROR:", problem)
        sys.exit(2)
    problem = check_pred_flag(arg)
    if problem:   # likewise (behind --loop's check: everything the closed loop refuses stays refused in its own words)
        print("ERROR:", problem)
        sys.exit(2)
    problem = check_bound_map_flag(arg)
    if problem:   # likewise (in front of the other flags' checks: a refusal of this job names the flag that defines it)
        print("ERROR:", problem)
        sys.exit(2)
    problem = check_frame_bounds_flags(arg)
    if problem:   # likewise (in front of the other flags' checks: a refusal of this job names the flag that defines it)
        print("ERROR:", problem)
        sys.exit(2)
    problem = check_ratio_flag(arg)
    if problem:   # likewise (in front of the other flags' checks: a refusal of this job names the flag that defines it)
        print("ERROR:", problem)
        sys.exit(2)
    problem = check_report_flag(arg)
    if problem:   # likewise, before any GPU is touched
        print("ERROR:", problem)
        sys.exit(2)
    problem = check_coder_flag(arg)
    if problem:   # likewise
        print("ERROR:", problem)
        sys.exit(2)
    problem = check_key_coder_flag(arg)
    if problem:   # likewise
        print("ERROR:", problem)
        sys.exit(2)
    problem = check_digests_flag(arg)
    if problem:   # likewise
        print("ERROR:", problem)
        sys.exit(2)
    problem = check_ssim_flag(arg)
    if problem:   # likewise
        print("ERROR:", problem)
        sys.exit(2)
    problem = check_verify_flag(arg)
    if problem:   # likewise
        print("ERROR:", problem)
        sys.exit(2)
    problem = check_gray_flag(arg)
    if problem:   # likewise
        print("ERROR:", problem)
        sys.exit(2)
    problem = check_sdelta_flag(arg)
    if problem:   # likewise
        print("ERROR:", problem)
        sys.exit(2)
    problem = check_target_flag(arg)
    if problem:   # likewise
        print("ERROR:", problem)
        sys.exit(2)
    problem = check_quant_flag(arg)
    if problem:   # likewise
        print("ERROR:", problem)
        sys.exit(2)
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:  # launched by torch.distributed.run: one rank per GPU
        from . import dist as tzdist
        tzdist.init_from_env()
    gpu = probe_gpu(arg.force)
    print("GPU MODE" if gpu else "CPU MODE")
    chosen = [name for name in ("learn", "compress", "uncompress") if getattr(arg, name) is not None]
    if len(chosen) > 1:
        return complain("several")
    if not chosen:
        return complain("nothing")
    if chosen[0] == "learn":
        print("train mode")
        return train.run(arg.learn[0], arg.learn[1], arg.verbose)
    if chosen[0] == "uncompress":
        print("uncompress mode")
        model, src, dst = arg.uncompress
        if getattr(arg, "verify", None) is not None:
            return decompress.run(model, src, dst, gpu, arg.verbose, frames=frames, verify=arg.verify)
        if frames is not None:
            return decompress.run(model, src, dst, gpu, arg.verbose, frames=frames)
        return decompress.run(model, src, dst, gpu, arg.verbose)
    print("compress mode")
    db, ratio = getattr(arg, "target_psnr", None), getattr(arg, "target_ratio", None)
    per_frame, bounds_file = bool(getattr(arg, "per_frame", False)), getattr(arg, "frame_bounds", None)
    map_file = getattr(arg, "bound_map", None)
    loop_db, loop_file = getattr(arg, "loop_psnr", None), getattr(arg, "loop_bounds", None)
    if loop_db is not None:   # an `abs` job whose bounds the closed loop finds: the same checks, and `abs` is printed
        problem = check_compress(argparse.Namespace(**dict(vars(arg), mode=["abs"], bound=[0.0])))
    elif loop_file is not None or getattr(arg, "loop_map", None) is not None:   # an `abs` job whose bounds come from the file
        problem = check_compress(argparse.Namespace(**dict(vars(arg), bound=[0.0])))
    elif bounds_file is not None or map_file is not None:   # an `abs` job whose bounds come from the file: the same checks with a bound in -b's place
        problem = check_compress(argparse.Namespace(**dict(vars(arg), bound=[0.0])))
    elif db is not None or ratio is not None:   # the job is an `abs` job whose bound is still to be found: the same checks, and `abs` is printed
        problem = check_compress(argparse.Namespace(**dict(vars(arg), mode=["abs"], bound=[0.0])))
    else:
        problem = check_compress(arg)
    if problem:
        return complain(problem)
    model, src, dst = arg.compress
    if arg.sweep is not None and arg.window is None:
        from . import sweep
        return sweep.run(model, src, dst, arg.preprocess[0], arg.sweep or None, arg.mode[0], arg.bound, arg.verbose,
                         arg.no_entropy)
    window = arg.window[0] if arg.window is not None else None
    threshold = arg.threshold[0] if arg.threshold is not None else None
    if loop_db is not None or loop_file is not None:   # TZ-CLF1 (every other flag travels with it; the jobs without it are the calls below)
        return compress.run(model, src, dst, arg.preprocess[0], window, threshold, "abs", [], gpu, arg.verbose,
                            arg.no_entropy, SHUFFLE=arg.shuffle, REPORT=bool(getattr(arg, "report", False)),
                            CODER=getattr(arg, "coder", "zstd"), KEY_CODER=getattr(arg, "key_coder", "zstd"),
                            DIGESTS=bool(getattr(arg, "digests", False)), SDELTA=getattr(arg, "sdelta", None) or "flat",
                            SSIM=bool(getattr(arg, "ssim", False)), QUANT="lattice", LOOP="closed",
                            **({"LOOP_PSNR": loop_db} if loop_db is not None else {"LOOP_BOUNDS": loop_file}))
    if getattr(arg, "loop_map", None) is not None:   # TZ-CLM1 (likewise)
        return compress.run(model, src, dst, arg.preprocess[0], window, threshold, "abs", [], gpu, arg.verbose,
                            arg.no_entropy, SHUFFLE=arg.shuffle, REPORT=bool(getattr(arg, "report", False)),
                            CODER=getattr(arg, "coder", "zstd"), KEY_CODER=getattr(arg, "key_coder", "zstd"),
                            DIGESTS=bool(getattr(arg, "digests", False)), SDELTA=getattr(arg, "sdelta", None) or "flat",
                            SSIM=bool(getattr(arg, "ssim", False)), QUANT="lattice", LOOP="closed", LOOP_MAP=arg.loop_map,
                            **({"PRED": "select"} if getattr(arg, "pred", None) == "select" else {}))
    if getattr(arg, "loop", None) == "closed":   # (open is the job without the flag: the calls below; every other flag travels with it)
        return compress.run(model, src, dst, arg.preprocess[0], window, threshold, arg.mode[0], arg.bound, gpu, arg.verbose,
                            arg.no_entropy, SHUFFLE=arg.shuffle, REPORT=bool(getattr(arg, "report", False)),
                            CODER=getattr(arg, "coder", "zstd"), KEY_CODER=getattr(arg, "key_coder", "zstd"),
                            DIGESTS=bool(getattr(arg, "digests", False)), SDELTA=getattr(arg, "sdelta", None) or "flat",
                            SSIM=bool(getattr(arg, "ssim", False)), QUANT=getattr(arg, "quant", None) or "greedy", LOOP="closed",
                            **({"PRED": arg.pred} if getattr(arg, "pred", None) in ("select", "motion") else {}))
    if map_file is not None:   # (every other flag travels with it; the jobs without it are the calls below)
        return compress.run(model, src, dst, arg.preprocess[0], window, threshold, "abs", [], gpu,
                            arg.verbose, arg.no_entropy, SHUFFLE=arg.shuffle, REPORT=bool(getattr(arg, "report", False)),
                            CODER=getattr(arg, "coder", "zstd"), KEY_CODER=getattr(arg, "key_coder", "zstd"),
                            DIGESTS=bool(getattr(arg, "digests", False)), GRAY=bool(getattr(arg, "gray", False)),
                            SDELTA=getattr(arg, "sdelta", None) or "flat", SSIM=bool(getattr(arg, "ssim", False)),
                            QUANT=getattr(arg, "quant", None) or "greedy", BOUND_MAP=map_file)
    if getattr(arg, "quant", None) == "lattice":   # (greedy is the job without the flag: the calls below; every other flag travels with it)
        searched = db is not None or ratio is not None or bounds_file is not None
        return compress.run(model, src, dst, arg.preprocess[0], window, threshold, "abs" if searched else arg.mode[0],
                            [] if searched else arg.bound, gpu, arg.verbose, arg.no_entropy, SHUFFLE=arg.shuffle,
                            REPORT=bool(getattr(arg, "report", False)), CODER=getattr(arg, "coder", "zstd"),
                            KEY_CODER=getattr(arg, "key_coder", "zstd"), DIGESTS=bool(getattr(arg, "digests", False)),
                            GRAY=bool(getattr(arg, "gray", False)), SDELTA=getattr(arg, "sdelta", None) or "flat",
                            SSIM=bool(getattr(arg, "ssim", False)), TARGET_PSNR=db, TARGET_RATIO=ratio, PER_FRAME=per_frame,
                            FRAME_BOUNDS=bounds_file, QUANT="lattice")
    if per_frame or bounds_file is not None:   # (every other flag travels with it; the jobs without it are the calls below)
        return compress.run(model, src, dst, arg.preprocess[0], window, threshold, "abs", [], gpu,
                            arg.verbose, arg.no_entropy, SHUFFLE=arg.shuffle, REPORT=bool(getattr(arg, "report", False)),
                            CODER=getattr(arg, "coder", "zstd"), KEY_CODER=getattr(arg, "key_coder", "zstd"),
                            DIGESTS=bool(getattr(arg, "digests", False)), GRAY=bool(getattr(arg, "gray", False)),
                            SDELTA=getattr(arg, "sdelta", None) or "flat", SSIM=bool(getattr(arg, "ssim", False)), TARGET_PSNR=db,
                            PER_FRAME=per_frame, FRAME_BOUNDS=bounds_file)
    if ratio is not None:   # (every other flag travels with it; the jobs without it are the calls below)
        return compress.run(model, src, dst, arg.preprocess[0], window, threshold, "abs", [], gpu,
                            arg.verbose, arg.no_entropy, SHUFFLE=arg.shuffle, REPORT=bool(getattr(arg, "report", False)),
                            CODER=getattr(arg, "coder", "zstd"), KEY_CODER=getattr(arg, "key_coder", "zstd"),
                            DIGESTS=bool(getattr(arg, "digests", False)), GRAY=bool(getattr(arg, "gray", False)),
                            SDELTA=getattr(arg, "sdelta", None) or "flat", SSIM=bool(getattr(arg, "ssim", False)), TARGET_RATIO=ratio)
    if db is not None:   # (every other flag travels with it; the jobs without it are the calls below)
        return compress.run(model, src, dst, arg.preprocess[0], window, threshold, "abs", [], gpu,
                            arg.verbose, arg.no_entropy, SHUFFLE=arg.shuffle, REPORT=bool(getattr(arg, "report", False)),
                            CODER=getattr(arg, "coder", "zstd"), KEY_CODER=getattr(arg, "key_coder", "zstd"),
                            DIGESTS=bool(getattr(arg, "digests", False)), GRAY=bool(getattr(arg, "gray", False)),
                            SDELTA=getattr(arg, "sdelta", None) or "flat", SSIM=bool(getattr(arg, "ssim", False)), TARGET_PSNR=db)
    if getattr(arg, "sdelta", None) in ("channel", "plane", "auto"):   # (flat is the job without the flag: the calls below)
        return compress.run(model, src, dst, arg.preprocess[0], window, threshold, arg.mode[0], arg.bound, gpu,
                            arg.verbose, arg.no_entropy, SHUFFLE=arg.shuffle, REPORT=bool(getattr(arg, "report", False)),
                            CODER=getattr(arg, "coder", "zstd"), KEY_CODER=getattr(arg, "key_coder", "zstd"),
                            DIGESTS=bool(getattr(arg, "digests", False)), GRAY=bool(getattr(arg, "gray", False)),
                            SSIM=bool(getattr(arg, "ssim", False)), SDELTA=arg.sdelta)
    if getattr(arg, "ssim", False):
        return compress.run(model, src, dst, arg.preprocess[0], window, threshold, arg.mode[0], arg.bound, gpu,
                            arg.verbose, arg.no_entropy, SHUFFLE=arg.shuffle, REPORT=True,
                            CODER=getattr(arg, "coder", "zstd"), KEY_CODER=getattr(arg, "key_coder", "zstd"),
                            DIGESTS=bool(getattr(arg, "digests", False)), GRAY=bool(getattr(arg, "gray", False)), SSIM=True)
    if getattr(arg, "gray", False):
        return compress.run(model, src, dst, arg.preprocess[0], window, threshold, arg.mode[0], arg.bound, gpu,
                            arg.verbose, arg.no_entropy, SHUFFLE=arg.shuffle, REPORT=bool(getattr(arg, "report", False)),
                            CODER=getattr(arg, "coder", "zstd"), KEY_CODER=getattr(arg, "key_coder", "zstd"),
                            DIGESTS=bool(getattr(arg, "digests", False)), GRAY=True)
    if getattr(arg, "digests", False):
        return compress.run(model, src, dst, arg.preprocess[0], window, threshold, arg.mode[0], arg.bound, gpu,
                            arg.verbose, arg.no_entropy, SHUFFLE=arg.shuffle, REPORT=bool(getattr(arg, "report", False)),
                            CODER=getattr(arg, "coder", "zstd"), KEY_CODER=getattr(arg, "key_coder", "zstd"), DIGESTS=True)
    if getattr(arg, "key_coder", "zstd") != "zstd":
        return compress.run(model, src, dst, arg.preprocess[0], window, threshold, arg.mode[0], arg.bound, gpu,
                            arg.verbose, arg.no_entropy, SHUFFLE=arg.shuffle, REPORT=bool(getattr(arg, "report", False)),
                            CODER=getattr(arg, "coder", "zstd"), KEY_CODER=arg.key_coder)
    if getattr(arg, "coder", "zstd") != "zstd":
        return compress.run(model, src, dst, arg.preprocess[0], window, threshold, arg.mode[0], arg.bound, gpu,
                            arg.verbose, arg.no_entropy, SHUFFLE=arg.shuffle, REPORT=bool(getattr(arg, "report", False)),
                            CODER=arg.coder)
    if getattr(arg, "report", False):
        return compress.run(model, src, dst, arg.preprocess[0], window, threshold, arg.mode[0], arg.bound, gpu,
                            arg.verbose, arg.no_entropy, SHUFFLE=arg.shuffle, REPORT=True)
    return compress.run(model, src, dst, arg.preprocess[0], window, threshold, arg.mode[0], arg.bound, gpu,
                        arg.verbose, arg.no_entropy, SHUFFLE=arg.shuffle)


def main(arg):
    """--pa travels to the library as TEZIP_PA (every context made during this run starts with it: tz_ctx_create); the
    variable is put back when the run ends, so that a caller that drives main() in-process is left as it was."""
    if getattr(arg, "pa", None) is None:
        return _main(arg)
    before = os.environ.get("TEZIP_PA")
    os.environ["TEZIP_PA"] = str(arg.pa)
    try:
        return _main(arg)
    finally:
        if before is None:
            os.environ.pop("TEZIP_PA", None)
        else:
            os.environ["TEZIP_PA"] = before


if __name__ == "__main__":
    main(build_parser().parse_args())
