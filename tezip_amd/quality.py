"""Reconstruction-error report of a compression job (`tezip.py -c ... --report`; not in the reference).

The per-frame records come from the library (tz_encode_quality: the stored payload decoded by the decoder's tail on
the device and compared with the originals, exact integers); this module only turns them into the figures a user of an
error-bounded compressor reads -- worst error, MSE, PSNR, compression ratio -- and writes them as quality.json next to
the reference's three files.  Pure numpy: no GPU is needed here."""
import json
import math
import os

import numpy as np

FILE_NAME = "quality.json"
REFERENCE_FILES = ("filename.txt", "key_frame.dat", "entropy.dat")   # what -c writes in the reference (compress.py)


def _records(stats):
    """(nt, 3) int64 of (sse, max_abs, n_changed) from a tz_frame_quality record array or anything shaped (nt, 3)."""
    a = np.asarray(stats)
    if a.dtype.names:
        return np.stack([a["sse"].astype(np.int64), a["max_abs"].astype(np.int64), a["n_changed"].astype(np.int64)], axis=1)
    a = np.asarray(a, dtype=np.int64)
    if a.ndim != 2 or a.shape[1] != 3:
        raise ValueError("quality records must be (nt, 3) (sse, max_abs, n_changed), got shape %r" % (a.shape,))
    return a


def psnr_db(sse, elements):
    """10 log10(255^2 / MSE) in float64 with MSE = sse / elements; None (JSON null) when nothing changed."""
    if sse == 0:
        return None
    return 10.0 * math.log10(255.0 ** 2 / (float(sse) / float(elements)))


def _sizes(sizes):
    if isinstance(sizes, dict):
        return [int(sizes[n]) for n in REFERENCE_FILES]
    sizes = [int(v) for v in sizes]
    if len(sizes) != 3:
        raise ValueError("sizes: the byte sizes of %s" % ", ".join(REFERENCE_FILES))
    return sizes


def summarize(stats, names, H, W, mode, bound, sizes, window=None, threshold=None, warm_up=None, ssim=None):
    """The report of one job as a JSON-ready dict.
    stats: the per-frame records in frame order; names: the frames' file names (filename.txt order); sizes: the byte
    sizes of filename.txt, key_frame.dat and entropy.dat (a dict by name or a sequence in that order).  PSNR per frame
    uses the frame's H*W*3 samples, the sequence's PSNR the sum of sse over all nt*H*W*3 samples (not a mean of frame
    PSNRs).  ratio = nt*H*W*3 / (sum of the three sizes).
    ssim (--ssim): the per-frame tz_frame_ssim records (tezip_amd/ssim.py) -- the document then gains "ssim" and "ssim_min" (the
    worst window of the job) at the top and in every per_frame entry, null where a frame has no window; None: exactly the
    document without them."""
    rec = _records(stats)
    nt = len(rec)
    if len(names) != nt:
        raise ValueError("%d names for %d frames" % (len(names), nt))
    fe = int(H) * int(W) * 3
    total = nt * fe
    sse = int(rec[:, 0].sum())
    stored = sum(_sizes(sizes))
    per_frame = [{"name": str(n), "max_abs_err": int(r[1]), "sse": int(r[0]), "n_changed": int(r[2]),
                  "psnr_db": psnr_db(int(r[0]), fe)} for n, r in zip(names, rec)]
    doc = {
        "mode": mode,
        "bound": [float(b) for b in bound],
        "window": None if window is None else int(window),
        "threshold": None if threshold is None else float(threshold),
        "warm_up": None if warm_up is None else int(warm_up),
        "frames": nt,
        "height": int(H),
        "width": int(W),
        "lossless": sse == 0,
        "max_abs_err": int(rec[:, 1].max()) if nt else 0,
        "mse": float(sse) / float(total) if total else 0.0,
        "psnr_db": psnr_db(sse, total),
        "n_changed": int(rec[:, 2].sum()),
        "raw_bytes": total,
        "stored_bytes": stored,
        "ratio": float(total) / float(stored) if stored else None,
        "per_frame": per_frame,
    }
    if ssim is not None:
        from . import ssim as tzssim
        fig = tzssim.figures(ssim)
        if len(fig["per_frame"]) != nt:
            raise ValueError("%d ssim records for %d frames" % (len(fig["per_frame"]), nt))
        doc["ssim"], doc["ssim_min"] = fig["ssim"], fig["ssim_min"]
        for entry, f in zip(per_frame, fig["per_frame"]):
            entry["ssim"], entry["ssim_min"] = f["ssim"], f["ssim_min"]
    return doc


def file_sizes(out_dir):
    """Byte sizes of the reference's three files in a -c output directory."""
    return {n: os.path.getsize(os.path.join(out_dir, n)) for n in REFERENCE_FILES}


def write(out_dir, doc):
    path = os.path.join(out_dir, FILE_NAME)
    with open(path, "w", encoding="UTF-8") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return path


def stdout_lines(doc):
    """The three lines -c --report prints, and the SSIM line behind them when the document has the key (--ssim)."""
    psnr = "inf" if doc["psnr_db"] is None else "%.4f" % doc["psnr_db"]
    lines = ["max_abs_err: %d" % doc["max_abs_err"], "PSNR: %s [dB]" % psnr, "ratio: %.4f" % doc["ratio"]]
    if "ssim" in doc:
        from . import ssim as tzssim
        lines.append(tzssim.stdout_line(doc["ssim"], doc["ssim_min"]))
    return lines
