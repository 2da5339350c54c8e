"""frame_digests.json -- per-frame digests of a compressed directory (`-c --digests`, `-u --verify`).

None of the stored formats carries a checksum, and a lossless decode depends on the decoder's predictions being the
encoder's bit for bit; the sidecar (tezip_amd.json) guards the contract and the weights, nothing guards the RESULT.  `-c`
knows exactly which bytes `-u` must produce: it runs the decoder's tail over the stored payload (tz_encode_digests) and
records one digest per frame; `-u` takes the digests of the decoded frames on the device (tz_decoded_digests /
tz_frame_digests) before the first image is written and compares.  The reference opens exactly its three files, so a fifth
file is invisible to it.

The digest, TZD64 version 1 (this module is its slow statement in numpy; the device's is k_digest in csrc/tz_codec.hip).
For a frame of n bytes x[0..n) in (H, W, 3) memory order, all arithmetic mod 2^64:

    key(i)  = 256 * i + x[i]
    mix(k)  : z = k + 0x9E3779B97F4A7C15
              z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9
              z = (z ^ (z >> 27)) * 0x94D049BB133111EB
              return z ^ (z >> 31)                         (splitmix64's output function)
    digest  = sum over i of mix(key(i))

mix is a bijection and the keys of a frame are distinct, so a change of one sample changes the digest with certainty; the
sum is commutative, so a GPU may cut a frame over lanes, waves and workgroups in any way.  It is an ERROR-DETECTION code,
not a cryptographic hash: it guards against damage and against decoders that stopped agreeing with the encoder, not against
someone who constructs a collision on purpose.

The file:

    {"format": 1, "algorithm": "TZD64-1", "frames": nt, "shape": [H, W, 3],
     "decoded":  [16 lower-case hex digits per frame, filename.txt order],   what the stored payload decodes to
     "original": [the same for the source frames]}                           equal to "decoded" where the job lost nothing

`python -m tezip_amd.digest --check COMPRESSED_DIR IMAGE_DIR` compares the images a `-u` wrote (or any copy of them) with
the "decoded" digests on the CPU: one line per mismatch, exit status 0, or 3 on a mismatch (2: the records are unusable)."""
import json
import os
import re
import sys

import numpy as np

NAME = "frame_digests.json"
FORMAT = 1
ALGORITHM = "TZD64-1"
MAX_REPORTED = 10          # mismatching frames named one by one; the rest are counted

_PIECE = 1 << 20           # bytes mixed at a time (8 B of key per byte)
_HEX = re.compile(r"^[0-9a-f]{16}$")


def _mix(k):
    z = k + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def frame_digest(x):
    """TZD64 of one frame: any uint8 array, read in C order.  A Python int in [0, 2^64)."""
    x = np.ascontiguousarray(x)
    if x.dtype != np.uint8:
        raise TypeError("a frame is uint8, got %s" % x.dtype)
    x = x.reshape(-1)
    total = np.uint64(0)
    with np.errstate(over="ignore"):
        for lo in range(0, x.size, _PIECE):
            piece = x[lo: lo + _PIECE]
            key = np.arange(lo, lo + piece.size, dtype=np.uint64) * np.uint64(256) + piece
            total = total + _mix(key).sum(dtype=np.uint64)
    return int(total)


def stack_digests(stack):
    """TZD64 of every frame stack[f]: uint64[len(stack)]."""
    return np.array([frame_digest(f) for f in stack], np.uint64)


def to_hex(digests):
    return ["%016x" % int(d) for d in digests]


def from_hex(words):
    return np.array([int(w, 16) for w in words], np.uint64)


def make(decoded, original, shape):
    """The document for uint64 digests `decoded` and `original` of frames of `shape` = (H, W, 3)."""
    doc = {"format": FORMAT, "algorithm": ALGORITHM, "frames": len(decoded), "shape": [int(v) for v in shape],
           "decoded": to_hex(decoded), "original": to_hex(original)}
    validate(doc)
    return doc


def validate(doc, frames=None, shape=None):
    """Raises ValueError naming the field that is wrong.  frames / shape: what the stream says (None: not compared)."""
    def bad(field, why):
        return ValueError("%s: field %r %s" % (NAME, field, why))

    if not isinstance(doc, dict):
        raise ValueError("%s: not a JSON object" % NAME)
    if doc.get("format") != FORMAT:
        raise bad("format", "is %r, this build reads %r" % (doc.get("format"), FORMAT))
    if doc.get("algorithm") != ALGORITHM:
        raise bad("algorithm", "is %r, this build reads %r" % (doc.get("algorithm"), ALGORITHM))
    nt = doc.get("frames")
    if not isinstance(nt, int) or isinstance(nt, bool) or nt < 1:
        raise bad("frames", "is %r, expected a positive integer" % (nt,))
    sh = doc.get("shape")
    if (not isinstance(sh, list) or len(sh) != 3 or not all(isinstance(v, int) and not isinstance(v, bool) for v in sh)
            or sh[0] < 1 or sh[1] < 1 or sh[2] != 3):
        raise bad("shape", "is %r, expected [H, W, 3]" % (sh,))
    for field in ("decoded", "original"):
        words = doc.get(field)
        if not isinstance(words, list):
            raise bad(field, "is missing or not a list")
        if len(words) != nt:
            raise bad(field, "holds %d digests, 'frames' says %d" % (len(words), nt))
        for i, w in enumerate(words):
            if not isinstance(w, str) or not _HEX.match(w):
                raise bad(field, "entry %d is %r, expected 16 lower-case hex digits" % (i, w))
    if frames is not None and nt != frames:
        raise bad("frames", "is %d, the stream holds %d frames" % (nt, frames))
    if shape is not None and list(sh) != [int(v) for v in shape]:
        raise bad("shape", "is %r, the stream holds %d frames of %r" % (sh, nt, [int(v) for v in shape]))
    return doc


def write(out_dir, doc):
    with open(os.path.join(out_dir, NAME), "w", encoding="UTF-8") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return doc


def present(data_dir):
    return os.path.exists(os.path.join(data_dir, NAME))


def read(data_dir, frames=None, shape=None):
    """The validated records of a compressed directory, or None when it has none.  A file that is there but damaged is a
    ValueError, not 'absent'."""
    path = os.path.join(data_dir, NAME)
    if not os.path.exists(path):
        return None
    try:
        with open(path, "r", encoding="UTF-8") as f:
            doc = json.load(f)
    except OSError as e:
        raise ValueError("%s cannot be read (%s)" % (path, e))
    except ValueError as e:
        raise ValueError("%s is damaged: not JSON (%s)" % (path, e))
    return validate(doc, frames, shape)


def mismatches(doc, got, first=0, field="decoded"):
    """Sequence indices of the frames whose digests `got` (uint64, frames first, first + 1, ...) differ from the records."""
    want = from_hex(doc[field][first: first + len(got)])
    return [first + int(j) for j in np.nonzero(want != np.asarray(got, np.uint64))[0]]


def mismatch_lines(bad, names):
    lines = ["ERROR: frame %d (%s) does not match its recorded digest" % (i, names[i]) for i in bad[:MAX_REPORTED]]
    if len(bad) > MAX_REPORTED:
        lines.append("ERROR: ... and %d more frames do not match" % (len(bad) - MAX_REPORTED))
    return lines


def read_names(data_dir):
    """filename.txt's image names (its first line, the RGB flag, dropped as decompress.run drops it)."""
    with open(os.path.join(data_dir, "filename.txt"), "r", encoding="UTF-8") as f:
        names = [s.strip() for s in f.readlines()]
    if names and len(names[0]) == 1:
        names.pop(0)
    return names


def check_images(data_dir, image_dir):
    """Compare the images of image_dir named in data_dir's filename.txt with the recorded `decoded` digests, on the CPU.
    Returns the lines to print, one per frame that is missing, of another size or of other content."""
    from PIL import Image
    names = read_names(data_dir)
    doc = read(data_dir, frames=len(names))
    if doc is None:
        raise ValueError("%s holds no %s (compress with --digests)" % (data_dir, NAME))
    lines = []
    for i, name in enumerate(names):
        path = os.path.join(image_dir, name)
        try:
            with Image.open(path) as img:
                arr = np.asarray(img.convert("RGB"))
        except (OSError, ValueError) as e:
            lines.append("frame %d (%s): cannot be read (%s)" % (i, name, e))
            continue
        if list(arr.shape) != doc["shape"]:
            lines.append("frame %d (%s): shape %r, recorded %r" % (i, name, list(arr.shape), doc["shape"]))
        elif "%016x" % frame_digest(arr) != doc["decoded"][i]:
            lines.append("frame %d (%s): does not match its recorded digest" % (i, name))
    return lines


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m tezip_amd.digest", description="check decoded images against frame_digests.json (no GPU)")
    ap.add_argument("--check", nargs=2, metavar=("COMPRESSED_DIR", "IMAGE_DIR"), required=True)
    arg = ap.parse_args(argv)
    try:
        lines = check_images(*arg.check)
    except (OSError, ValueError) as e:
        print("ERROR:", e)
        return 2
    for line in lines:
        print(line)
    if lines:
        return 3
    print("verified: %d frames" % len(read_names(arg.check[0])))
    return 0


if __name__ == "__main__":
    sys.exit(main())
