"""CPU checks of the compression report (`tezip.py -c ... --report`): the summary arithmetic of tezip_amd/quality.py, the
refusals of the flag outside a single-GPU -c job, and the record layout shared by the header and the binding."""
import ctypes
import json
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT


def _stats(rows):
    from tezip_amd import _lib
    a = np.zeros(len(rows), _lib.QUALITY_DTYPE)
    for i, (s, m, c) in enumerate(rows):
        a[i] = (s, m, c)
    return a


# ------------------------------------------------------------------------------------------------------ summarize
def test_psnr_of_known_values():
    from tezip_amd import quality
    H, W = 4, 5
    fe = H * W * 3
    # MSE 1 -> 20 log10(255) = 48.1308 dB; MSE 4 -> 6.0206 dB less; MSE 255^2 -> 0 dB
    doc = quality.summarize(_stats([(fe, 1, fe), (4 * fe, 2, fe), (255 ** 2 * fe, 255, fe)]), ["a", "b", "c"], H, W, "abs",
                            [2.0], (10, 20, 30))
    p = [f["psnr_db"] for f in doc["per_frame"]]
    assert p[0] == pytest.approx(20 * math.log10(255), abs=1e-12)
    assert p[0] - p[1] == pytest.approx(10 * math.log10(4), abs=1e-12)
    assert p[2] == pytest.approx(0.0, abs=1e-12)
    assert doc["max_abs_err"] == 255 and doc["n_changed"] == 3 * fe
    assert doc["lossless"] is False


def test_sequence_psnr_is_from_the_summed_sse_not_a_mean_of_frame_psnrs():
    from tezip_amd import quality
    H, W = 8, 8
    fe = H * W * 3
    rows = [(0, 0, 0), (fe * 100, 30, 17), (fe * 1, 1, fe), (3, 1, 3)]
    doc = quality.summarize(_stats(rows), list("wxyz"), H, W, "abs", [2.0], (1, 1, 1))
    sse = sum(r[0] for r in rows)
    assert doc["mse"] == sse / (4 * fe)
    assert doc["psnr_db"] == pytest.approx(10 * math.log10(255 ** 2 / (sse / (4 * fe))), abs=1e-12)
    frame_mean = np.mean([f["psnr_db"] for f in doc["per_frame"] if f["psnr_db"] is not None])
    assert abs(doc["psnr_db"] - frame_mean) > 1.0
    assert doc["per_frame"][0]["psnr_db"] is None      # an unchanged frame has no finite PSNR
    assert doc["max_abs_err"] == 30 and doc["n_changed"] == 17 + fe + 3


def test_lossless_is_null_psnr_and_json_has_no_infinity(tmp_path):
    from tezip_amd import quality
    doc = quality.summarize(np.zeros((3, 3), np.int64), ["1.png", "2.png", "3.png"], 2, 3, "abs", [0.0], (5, 6, 7))
    assert doc["lossless"] is True and doc["psnr_db"] is None and doc["mse"] == 0.0 and doc["max_abs_err"] == 0
    assert all(f["psnr_db"] is None for f in doc["per_frame"])
    path = quality.write(str(tmp_path), doc)
    assert os.path.basename(path) == "quality.json"
    text = open(path).read()
    assert "Infinity" not in text and "NaN" not in text
    assert json.loads(text) == doc
    assert quality.stdout_lines(doc)[1].startswith("PSNR: inf")


def test_ratio_names_and_parameters():
    from tezip_amd import quality
    H, W, nt = 6, 7, 3
    names = ["f_010.png", "f_002.png", "f_100.png"]   # kept as given (filename.txt order)
    sizes = {"filename.txt": 31, "key_frame.dat": 400, "entropy.dat": 569}
    doc = quality.summarize([[1, 1, 1], [0, 0, 0], [8, 2, 2]], names, H, W, "absrel", [3.0, 0.01], sizes, window=None,
                            threshold=0.25, warm_up=2)
    assert [f["name"] for f in doc["per_frame"]] == names
    assert doc["ratio"] == nt * H * W * 3 / 1000 and doc["stored_bytes"] == 1000 and doc["raw_bytes"] == nt * H * W * 3
    assert doc["mode"] == "absrel" and doc["bound"] == [3.0, 0.01]
    assert doc["window"] is None and doc["threshold"] == 0.25 and doc["warm_up"] == 2
    assert [f["sse"] for f in doc["per_frame"]] == [1, 0, 8] and [f["n_changed"] for f in doc["per_frame"]] == [1, 0, 2]
    assert doc == quality.summarize(_stats([(1, 1, 1), (0, 0, 0), (8, 2, 2)]), names, H, W, "absrel", [3.0, 0.01],
                                    (31, 400, 569), threshold=0.25, warm_up=2)
    lines = quality.stdout_lines(doc)
    assert [ln.split(":")[0] for ln in lines] == ["max_abs_err", "PSNR", "ratio"]
    with pytest.raises(ValueError):
        quality.summarize([[1, 1, 1]], ["a", "b"], H, W, "abs", [1.0], (1, 1, 1))


# ---------------------------------------------------------------------------------------------------- record layout
def test_record_layout_of_binding_and_header():
    from tezip_amd import _lib
    assert ctypes.sizeof(_lib.FrameQuality) == 16 and _lib.QUALITY_DTYPE.itemsize == 16
    assert [f[0] for f in _lib.FrameQuality._fields_] == list(_lib.QUALITY_DTYPE.names) == ["sse", "max_abs", "n_changed"]
    text = open(os.path.join(ROOT, "include", "tezip_hip.h")).read()
    assert re.search(r"int\s+tz_encode_quality\s*\(", text)
    assert re.search(r"unsigned long long sse;\s*(/\*.*?\*/)?\s*unsigned max_abs;\s*(/\*.*?\*/)?\s*unsigned n_changed;", text,
                     flags=re.S)
    assert "tz_encode_quality" in _lib.EXPORTS


# ------------------------------------------------------------------------------------------------------ CLI refusals
def _cli(args, env_extra=None):
    env = dict(os.environ)
    env.update(env_extra or {})
    return subprocess.run([sys.executable, "-m", "tezip_amd.tezip"] + args, cwd=ROOT, env=env, capture_output=True, text=True,
                          timeout=120)


@pytest.mark.parametrize("args,env", [
    (["-u", "M", "SRC", "{out}", "--report"], {}),
    (["-l", "M", "SRC", "--report"], {}),
    (["-c", "M", "SRC", "{out}", "-p", "0", "--sweep", "5", "10", "-m", "abs", "-b", "2", "--report"], {}),
    (["-c", "M", "SRC", "{out}", "-p", "0", "-w", "5", "-m", "abs", "-b", "2", "--report"],
     {"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"}),
])
def test_report_refusals_exit_2_and_write_nothing(tmp_path, args, env):
    out = tmp_path / "out"
    r = _cli([a.replace("{out}", str(out)) for a in args], env)
    assert r.returncode == 2, r.stdout + r.stderr
    assert r.stdout.startswith("ERROR:") and "--report" in r.stdout
    assert "GPU MODE" not in r.stdout and "CPU MODE" not in r.stdout      # refused before the device probe
    assert not out.exists()


def test_report_is_not_in_the_refusals_of_other_flags():
    from tezip_amd import tezip
    p = tezip.build_parser()
    assert tezip.check_report_flag(p.parse_args(["-c", "m", "d", "o", "-p", "0", "-w", "5", "-m", "abs", "-b", "2"])) is None
    assert tezip.check_report_flag(p.parse_args(["-u", "m", "d", "o", "--frames", "1:2"])) is None
    assert tezip.check_report_flag(p.parse_args(["-c", "m", "d", "o", "-p", "0", "-w", "5", "-m", "abs", "-b", "2",
                                                 "--report"])) is None
    frames, problem = tezip.check_frames_flag(p.parse_args(["-c", "m", "d", "o", "--frames", "1:2", "--report"]))
    assert frames is None and "--report" not in problem
    r = _cli(["-u", "M", "SRC", "OUT", "--frames", "x"])
    assert r.returncode == 2 and "--report" not in r.stdout
