"""tezip_amd.json -- what the reference's three files cannot say about a compressed directory.

A lossless decode needs the decoder's predictions bit-identical to the encoder's
(/root/reference/src/decompress.py:252-253: `X_hat * 255 - difference`).  The reference leaves the
predictor's float32 arithmetic to Keras/TensorFlow/cuDNN; this build fixes it as an arithmetic
CONTRACT (TZ-PA1 direct chains / TZ-PA2 Winograd chains, include/tezip_hip.h tz_set_contract), and
which one encoded a stream is not derivable from the stream.  The reference's decoder opens exactly
filename.txt, key_frame.dat and entropy.dat (decompress.py:48-103), so a fourth file is invisible to
it; `-c` writes this one, `-u` adopts it:

  {"format": 1, "arithmetic_contract": "TZ-PA2", "contract": 2, "tz_version": 101,
   "arch": "gfx950", "padded_frame": [512, 512], "weights_sha256": "...", "stack": [80, 512, 512, 0]}

`payload_channels` = 1 (optional): the payload of entropy.dat stores one channel per pixel (`-c --gray` on a job whose frames
are all gray, tezip_amd/graypayload.py); a job with the three-channel payload has no such key.  The trailer of entropy.dat
states the same and is authoritative: a sidecar that contradicts it is an error.

`sdelta` = "channel" (optional): the spatial delta of the payload was taken at the channel stride (`-c --sdelta channel` on a
three-channel payload, tezip_amd/sdelta.py), or "plane": it is the 2-D one, TZ-SD2 (`-c --sdelta plane`, three channels or one);
every other job has no such key.  The trailer of entropy.dat states the same (mark 4 or 5, 8 or 9) and is authoritative: a sidecar
that contradicts it is an error.

`quant` = "lattice" (optional): the job's deltas were quantised by the lattice quantiser TZ-QL1 (`-c --quant lattice`,
tezip_amd/lattice.py); every other job has no such key.  Informational: the payload holds the quantised deltas themselves, a
decoder never sees a bound, and `-u` does not read the key.

`loop` = "closed" (optional): the job ran closed-loop prediction TZ-CL1 (`-c --loop closed`, tezip_amd/closedloop.py); every other
job has no such key.  The mark in entropy.dat's trailer is authoritative (the open-loop mark plus 16); a sidecar that contradicts
it is an error.  A decoder that reads "closed" here does not queue its rollout ahead of the payload: the loop needs it.

`pred` = "select" (optional): the job chose per 16 x 16 tile between the network and the decoded frame in front, TZ-PS1
(`-c --loop closed --pred select`, tezip_amd/predselect.py); every other job has no such key.  The mark in entropy.dat's trailer is
authoritative (the closed-loop mark plus 32); a sidecar that contradicts it is an error.  `pred` = "motion": the frame in front was
displaced per tile, TZ-PM1 (`--pred motion`, tezip_amd/predmotion.py); the mark is the closed-loop mark plus 64.

`stack` = [frames, height, width, warm_up] (round 6, optional): the reference stores these in the LAST seven
values of entropy.dat (compress.py:390-394), so a decoder learns it only when the whole payload is decompressed; with
it here the decoder runs its rollout WHILE entropy.dat is being decompressed (decompress._run_streaming) and checks the
trailer against it afterwards.

  * sidecar present: the decoder runs under its contract; a --pa / TEZIP_PA that contradicts it is an
    error (the output would be off by one grey level on a fraction of 'lossless' samples, silently);
    a model whose weights hash differs is an error too (the output would be noise);
  * sidecar absent (a directory written by the reference, or by a build before round 5): the rule of
    rounds 1-4 -- --pa / TEZIP_PA if given, else by padded frame size.
"""
import hashlib
import json
import os

NAME = "tezip_amd.json"
FORMAT = 1


class SidecarMismatch(ValueError):
    pass


def weights_sha256(wts):
    h = hashlib.sha256()
    for w in wts:
        h.update(memoryview(w if w.flags["C_CONTIGUOUS"] else w.copy()).cast("B"))
    return h.hexdigest()


def requested_contract():
    """What the command line (--pa, exported as TEZIP_PA by tezip.py) asked for: 1, 2 or None."""
    v = os.environ.get("TEZIP_PA", "").strip()
    return int(v) if v in ("1", "2") else None


def write(out_dir, contract, wts, hp, wp, stack=None, payload_channels=3, sdelta="flat", quant="greedy", bound_map=None, loop="open",
          pred="net"):
    from . import _lib
    if contract not in (1, 2):
        raise ValueError("contract must be 1 or 2, not %r" % (contract,))
    doc = {"format": FORMAT, "arithmetic_contract": "TZ-PA%d" % contract, "contract": int(contract),
           "tz_version": int(_lib.load().tz_version()), "arch": "gfx950", "padded_frame": [int(hp), int(wp)],
           "weights_sha256": weights_sha256(wts)}
    if stack is not None:
        doc["stack"] = [int(v) for v in stack]
    if payload_channels == 1:   # a --gray job; every other job has no such key
        doc["payload_channels"] = 1
    if sdelta in ("channel", "plane"):   # a --sdelta channel job with a three-channel payload, or a --sdelta plane job; every
        doc["sdelta"] = sdelta           # other job has no such key
    if quant == "lattice":      # a --quant lattice job; every other job has no such key
        doc["quant"] = "lattice"
    if bound_map is not None:   # a --bound-map job: {"max", "exact_pixels"}, informational (`-u` does not read it); else no such key
        doc["bound_map"] = {"max": int(bound_map["max"]), "exact_pixels": int(bound_map["exact_pixels"])}
    if loop == "closed":        # a --loop closed job (tezip_amd/closedloop.py); every other job has no such key
        doc["loop"] = "closed"
    if pred in ("select", "motion"):   # a --pred select job (tezip_amd/predselect.py) or a --pred motion job (tezip_amd/predmotion.py);
        doc["pred"] = pred             # every other job has no such key
    with open(os.path.join(out_dir, NAME), "w", encoding="UTF-8") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return doc


def read(data_dir):
    """The sidecar of a compressed directory, or None when there is none.  A file that is there but unreadable is an
    error, not 'absent': falling back to a guess is exactly the silent failure this file exists to prevent."""
    path = os.path.join(data_dir, NAME)
    if not os.path.exists(path):
        return None
    try:
        with open(path, "r", encoding="UTF-8") as f:
            doc = json.load(f)
        if doc.get("format") != FORMAT or doc.get("contract") not in (1, 2):
            raise ValueError("format %r, contract %r" % (doc.get("format"), doc.get("contract")))
    except (OSError, ValueError) as e:
        raise SidecarMismatch("%s is damaged (%s); remove it only if you know which --pa the directory was compressed "
                              "with" % (path, e))
    return doc


def stack_of(doc):
    """(nt, H, W, warm_up) when the sidecar records a plausible stack, else None (older sidecars, the reference's directories)."""
    st = doc.get("stack") if doc else None
    if (isinstance(st, list) and len(st) == 4 and all(isinstance(v, int) for v in st) and all(1 <= v <= 32767 for v in st[:3])
            and 0 <= st[3] < st[0]):
        return tuple(st)
    return None


def channels_of(doc):
    """The payload channels the sidecar states: 1 for a --gray job (tezip_amd/graypayload.py), 3 for a sidecar without the key,
    None without a sidecar.  Anything else in the key is a damaged file."""
    if doc is None:
        return None
    ch = doc.get("payload_channels", 3)
    if ch not in (1, 3) or isinstance(ch, bool):
        raise SidecarMismatch("%s states payload_channels %r (1 is the only value ever written)" % (NAME, ch))
    return ch


def sdelta_of(doc):
    """The mode of the payload's spatial delta the sidecar states: "channel" for a --sdelta channel job, "plane" for a --sdelta
    plane job (tezip_amd/sdelta.py), "flat" for a sidecar without the key, None without a sidecar.  Anything else is a damaged
    file."""
    if doc is None:
        return None
    mode = doc.get("sdelta", "flat")
    if mode not in ("flat", "channel", "plane") or ("sdelta" in doc and mode == "flat"):
        raise SidecarMismatch("%s states sdelta %r (\"channel\" and \"plane\" are the only values ever written)" % (NAME, mode))
    return mode


def loop_of(doc):
    """The prediction loop the sidecar states: "closed" for a --loop closed job (tezip_amd/closedloop.py), "open" for a sidecar
    without the key, None without a sidecar.  Anything else is a damaged file."""
    if doc is None:
        return None
    loop = doc.get("loop", "open")
    if loop not in ("open", "closed") or ("loop" in doc and loop == "open"):
        raise SidecarMismatch("%s states loop %r (\"closed\" is the only value ever written)" % (NAME, loop))
    return loop


def pred_of(doc):
    """What the sidecar states about per-tile selection: "select" for a --pred select job (tezip_amd/predselect.py), "motion" for a
    --pred motion job (tezip_amd/predmotion.py), "net" for a sidecar without the key, None without a sidecar.  Anything else is a
    damaged file."""
    if doc is None:
        return None
    pred = doc.get("pred", "net")
    if pred not in ("net", "select", "motion") or ("pred" in doc and pred == "net"):
        raise SidecarMismatch("%s states pred %r (\"select\" and \"motion\" are the only values ever written)" % (NAME, pred))
    return pred


def resolve(doc, wts=None):
    """The contract a decoder must run under given the sidecar `doc` (may be None) and the command line.  Returns 1, 2 or
    None (= no sidecar and nothing asked for: by frame size).  Raises SidecarMismatch on a contradiction."""
    asked = requested_contract()
    if doc is None:
        return asked
    if asked is not None and asked != doc["contract"]:
        raise SidecarMismatch("this directory was compressed under %s (%s), --pa / TEZIP_PA asks for TZ-PA%d: a decode under "
                              "another arithmetic contract is silently off by one grey level on part of the samples.  Drop "
                              "--pa (the recorded contract is adopted)." % (doc["arithmetic_contract"], NAME, asked))
    if wts is not None and doc.get("weights_sha256") and doc["weights_sha256"] != weights_sha256(wts):
        raise SidecarMismatch("the model given to -u is not the model this directory was compressed with (%s records "
                              "another weights_sha256): the decoder's predictions would not be the encoder's." % NAME)
    return doc["contract"]
