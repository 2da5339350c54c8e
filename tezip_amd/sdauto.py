"""The payload's spatial delta chosen by exact size (`tezip.py -c ... --sdelta auto --coder huff|huffr|huffd`; not in the
reference).

Definition TZ-SDA1 (also DESIGN.md section 9 and include/tezip_hip.h).  The payload has three spatial deltas -- flat (the
reference's), channel and plane (TZ-SD2: tezip_amd/sdelta.py) -- and each wins somewhere.  The quantised deltas do not depend on
the layout, and with a GPU coder the size of entropy.dat is an exact function of integer counts (TZ-TRATIO-1,
tezip_amd/ratetarget.py), so one rollout and one quantiser run size all three (tz_sdelta_probe):

  candidates  flat, channel, plane, in this order.  On a one-channel payload (--gray on an all-gray job) channel IS flat, so it
              is no candidate there.
  E(layout)   ratetarget.file_bytes(record, coder), record the tz_size_record of the stream that the job's own tz_encode ->
              tz_<coder>_counts -> host code choice -> tz_<coder>_encode would write under that layout.  The bound, -m, --quant,
              frame bounds, -n, --gray and --coder are the job's own.  The front of the file differs per layout (A, table_len),
              so whole files are compared, not stream words.
  choice      the smallest E; a tie goes to the earlier candidate.
  guarantee   every file the job writes is byte for byte what `-c --sdelta <chosen>` writes with the same other flags; the size
              of its entropy.dat is the chosen E, and no larger than the entropy.dat of either other explicit job.

zstd's size cannot be known without running zstd: the flag belongs to the GPU coders.  This module is pure numpy; the records
come from the library (tezip_amd/_lib.py Context.sdelta_probe).  plane_symbols, count_of_plane and bits_of_plane are the slow
statement of the plane layouts of k_size_count / k_size_bits (csrc/tz_codec.hip): the symbols IN FRONT of the rank remap, as
ratetarget.count_of / bits_of are for the flat, gray and channel-stride layouts."""
import numpy as np

from . import ratetarget, sdelta

DEFINITION = "TZ-SDA1"
MODE = "auto"
CANDIDATES = sdelta.MODES          # flat, channel, plane: the order of tz_sdelta_probe's records and of a tie
CODERS = tuple(ratetarget.CODERS)  # the coders whose file size is a function of counts

NEEDS_GPU_CODER = ("--sdelta auto needs a GPU coder: zstd's size cannot be known without running zstd, add --coder huffd "
                   "(or huff, huffr)")
NO_SHUFFLE = "--sdelta auto cannot be combined with --shuffle: byte planes are not Huffman-coded; drop --shuffle"
NO_RATIO = ("--sdelta auto cannot be combined with --target-ratio: the bound search sizes one layout; run --target-ratio with "
            "--sdelta flat or channel")
NOT_SHARDED = "--sdelta auto is not available for a sharded job (WORLD_SIZE > 1): run it on one GPU"


def check(coder, shuffle, sharded, target_ratio):
    """None, or why a job cannot run --sdelta auto (the refusal of tezip.py and compress.run)."""
    if sharded:
        return NOT_SHARDED
    if shuffle:
        return NO_SHUFFLE
    if coder not in CODERS:
        return NEEDS_GPU_CODER
    if target_ratio is not None:
        return NO_RATIO
    return None


# ---- the slow statement of the plane layouts of k_size_count and k_size_bits
def plane_symbols(q, channels=3, offset=True):
    """The plane payload symbols (TZ-SD2) of the quantised delta stack q, int16 (nt, H, W, 3) with values in [-255, 255], in
    front of the rank remap; channels 3: every element, 1: channel 0 alone.  sdelta.encode_plane at every index."""
    q = np.asarray(q, np.int16)
    if q.ndim != 4 or q.shape[3] != 3:
        raise ValueError("plane_symbols takes the (nt, H, W, 3) stack, not shape %r" % (q.shape,))
    if channels not in (1, 3):
        raise ValueError("a payload has 3 channels or 1, not %r" % (channels,))
    return sdelta.encode_plane(q if channels == 3 else q[..., :1], offset)


def count_of_plane(q, channels=3, offset=True):
    """k_size_count over the plane symbols: ratetarget.count_of's result."""
    return ratetarget.count_of_symbols(plane_symbols(q, channels, offset))


def bits_of_plane(q, lens, dist, channels=3, offset=True):
    """k_size_bits over the plane symbols: ratetarget.bits_of's result."""
    return ratetarget.bits_of_symbols(plane_symbols(q, channels, offset), lens, dist)


# ---- the choice and the printed line
def sizes_of(records, coder):
    """The three records of tz_sdelta_probe (n == 0, or None: no candidate) -> [E or None] in the order of CANDIDATES."""
    if len(records) != len(CANDIDATES):
        raise ValueError("%d records, one per candidate %s wanted" % (len(records), ", ".join(CANDIDATES)))
    return [None if r is None or int(r["n"]) == 0 else int(ratetarget.file_bytes(r, coder)) for r in records]


def choose(records, coder):
    """-> (mode, sizes): the candidate of the smallest E, a tie to the earlier one; sizes as sizes_of gives them."""
    sizes = sizes_of(records, coder)
    best = None
    for i, e in enumerate(sizes):
        if e is not None and (best is None or e < sizes[best]):
            best = i
    if best is None:
        raise ValueError("no layout is a candidate")
    return CANDIDATES[best], sizes


def stdout_line(mode, sizes):
    return "sdelta: auto -> %s (bytes: %s)" % (mode, ", ".join("%s %s" % (name, "-" if e is None else "%d" % e)
                                                                 for name, e in zip(CANDIDATES, sizes)))
