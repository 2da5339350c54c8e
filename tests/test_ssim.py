"""TZ-SSIM-1 without a GPU (tezip_amd/ssim.py; `-c --report --ssim`): the numpy statement against a brute-force loop over
windows in exact arithmetic, the window geometry, the properties an SSIM must have, the report's new keys, the refusals of
the flag and the image-directory CLI."""
import contextlib
import io
import json
from fractions import Fraction

import numpy as np
import pytest

from tezip_amd import quality, ssim

ONE = 1 << 32


def _tezip(args):
    """tezip.py's main in this process -> (exit status, stdout)."""
    from tezip_amd import tezip
    buf = io.StringIO()
    code = 0
    with contextlib.redirect_stdout(buf):
        try:
            tezip.main(tezip.build_parser().parse_args([str(a) for a in args]))
        except SystemExit as e:
            code = 0 if e.code is None else e.code
    return code, buf.getvalue()


# --------------------------------------------------------------------------------------------- against exact arithmetic
def _round_half_even(x):
    """Fraction -> int, ties to even."""
    fl = x.numerator // x.denominator
    rest = x - fl
    if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and fl % 2):
        return fl + 1
    return fl


def _tie_distance(x):
    """How far the Fraction x lies from the nearest half-integer."""
    return abs(x % 1 - Fraction(1, 2))


def _brute(a, b):
    """Per window of two (H, W, 3) frames, in window order (y, x, channel): (Q from the exact r rounded half to even, the
    distance of the exact r * 2^32 from the nearest half-integer)."""
    H, W = a.shape[:2]
    out = []
    for y in range(0, H - 7, 4):
        for x in range(0, W - 7, 4):
            for c in range(3):
                s1 = s2 = sa = sb = s12 = 0
                for dy in range(8):
                    for dx in range(8):
                        u, v = int(a[y + dy, x + dx, c]), int(b[y + dy, x + dx, c])
                        s1, s2, sa, sb, s12 = s1 + u, s2 + v, sa + u * u, sb + v * v, s12 + u * v
                n1 = 200 * s1 * s2 + 2663424
                n2 = 200 * (64 * s12 - s1 * s2) + 23970816
                d1 = 100 * (s1 * s1 + s2 * s2) + 2663424
                d2 = 100 * (64 * (sa + sb) - s1 * s1 - s2 * s2) + 23970816
                assert d1 > 0 and d2 > 0 and max(abs(n1), abs(n2), d1, d2) < 1 << 53
                exact = Fraction(n1 * n2, d1 * d2) * ONE
                out.append((_round_half_even(exact), _tie_distance(exact)))
    return out


def _pairs():
    rng = np.random.default_rng(20261018)
    h, w = 13, 21
    noise = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    other = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    smooth = np.stack([120 + 60 * np.sin(xx / 3.0), 90 + 40 * np.cos(yy / 2.0), 10.0 * yy + xx], -1).clip(0, 255).astype(np.uint8)
    near = np.clip(smooth.astype(int) + rng.integers(-2, 3, smooth.shape), 0, 255).astype(np.uint8)
    flat0, flat255 = np.zeros((h, w, 3), np.uint8), np.full((h, w, 3), 255, np.uint8)
    return [(noise, other), (smooth, near), (smooth, noise), (flat0, flat255), (flat255, noise)]


def test_frame_records_equal_a_brute_force_loop_in_exact_arithmetic():
    """The float64 route (two rounded products, one rounded quotient) may land on the other side of a tie only where the exact
    r * 2^32 lies next to a half-integer; the seeds are chosen so that no such window occurs, and then every Q must be equal."""
    for a, b in _pairs():
        want = _brute(a, b)
        got = ssim.window_q(a, b).reshape(-1)
        assert len(want) == got.size == ssim.window_count(*a.shape[:2])
        assert all(dist > Fraction(1, 1000) for _, dist in want), "a window of this seed lies within 1e-3 of a tie"
        assert [int(q) for q in got] == [q for q, _ in want]
        rec = ssim.frame_records(a, b)[0]
        assert int(rec["sum_q32"]) == sum(q for q, _ in want) and int(rec["min_q32"]) == min(q for q, _ in want)
        assert int(rec["windows"]) == len(want) and int(rec["reserved"]) == 0


def test_the_brute_force_distance_is_a_distance_to_a_tie():
    assert _round_half_even(Fraction(5, 2)) == 2 and _round_half_even(Fraction(7, 2)) == 4 and _round_half_even(Fraction(-5, 2)) == -2
    assert _round_half_even(Fraction(-7, 3)) == -2 and _round_half_even(Fraction(8, 3)) == 3
    for exact, dist in ((Fraction(5, 2), 0), (Fraction(3), Fraction(1, 2)), (Fraction(-9, 4), Fraction(1, 4)), (Fraction(26, 10), Fraction(1, 10))):
        assert _tie_distance(exact) == dist


# ------------------------------------------------------------------------------------------------------------ geometry
@pytest.mark.parametrize("H", [7, 8, 11, 12, 13])
@pytest.mark.parametrize("W", [7, 8, 11, 12, 13])
def test_window_counts(H, W):
    per_side = {7: 0, 8: 1, 11: 1, 12: 2, 13: 2}
    want = 3 * per_side[H] * per_side[W]
    assert ssim.window_count(H, W) == want
    rng = np.random.default_rng(H * 100 + W)
    a = rng.integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    b = rng.integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    rec = ssim.frame_records(a, b)
    assert rec.dtype == ssim.SSIM_DTYPE and rec.dtype.itemsize == 24
    assert (rec["windows"] == want).all() and (rec["reserved"] == 0).all()
    if want == 0:
        assert (rec["sum_q32"] == 0).all() and (rec["min_q32"] == 0).all()
        fig = ssim.figures(rec)
        assert fig["ssim"] is None and fig["ssim_min"] is None and fig["per_frame"][0] == {"ssim": None, "ssim_min": None}
    else:   # the uncovered edge is not compared
        b2 = b.copy()
        b2[:, (H - 8) // 4 * 4 + 8:] ^= 0xFF
        b2[:, :, (W - 8) // 4 * 4 + 8:] ^= 0xFF
        np.testing.assert_array_equal(ssim.frame_records(a, b2), rec)


# ---------------------------------------------------------------------------------------------------------- properties
def test_identical_frames_give_one_for_every_window():
    rng = np.random.default_rng(3)
    a = rng.integers(0, 256, (2, 20, 17, 3), dtype=np.uint8)
    a[1] = 0
    assert (ssim.window_q(a[0], a[0]) == ONE).all() and (ssim.window_q(a[1], a[1]) == ONE).all()
    rec = ssim.frame_records(a, a)
    assert (rec["sum_q32"] == rec["windows"].astype(np.int64) * ONE).all() and (rec["min_q32"] == ONE).all()
    fig = ssim.figures(rec)
    assert fig["ssim"] == 1.0 and fig["ssim_min"] == 1.0


def test_an_inverted_checkerboard_gives_a_negative_sum():
    yy, xx = np.meshgrid(np.arange(16), np.arange(24), indexing="ij")
    a = np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[..., None], 3, axis=2)
    rec = ssim.frame_records(a, 255 - a)[0]
    assert int(rec["sum_q32"]) < 0 and int(rec["min_q32"]) < 0
    assert ssim.figures(rec.reshape(1))["ssim"] < -0.9


def test_symmetry():
    for a, b in _pairs():
        np.testing.assert_array_equal(ssim.frame_records(a, b), ssim.frame_records(b, a))


def test_sequence_figures_weigh_windows_not_frames():
    rec = np.zeros(3, ssim.SSIM_DTYPE)
    rec["sum_q32"], rec["min_q32"], rec["windows"] = [3 * ONE, 0, ONE // 2], [ONE, 0, ONE // 4], [3, 0, 1]
    fig = ssim.figures(rec)
    assert fig["ssim"] == 3.5 / 4 and fig["ssim_min"] == 0.25          # (the frame without a window does not count)
    assert fig["per_frame"] == [{"ssim": 1.0, "ssim_min": 1.0}, {"ssim": None, "ssim_min": None}, {"ssim": 0.5, "ssim_min": 0.25}]


# --------------------------------------------------------------------------------------------------------- the report
def test_summarize_without_ssim_is_todays_document_and_with_it_gains_four_keys():
    stats = np.array([[0, 0, 0], [40, 2, 17]], np.int64)
    names = ["a.png", "b.png"]
    args = (stats, names, 16, 24, "abs", [2.0], {"filename.txt": 10, "key_frame.dat": 100, "entropy.dat": 200})
    base = quality.summarize(*args, window=5, warm_up=1)
    assert list(base) == ["mode", "bound", "window", "threshold", "warm_up", "frames", "height", "width", "lossless", "max_abs_err",
                          "mse", "psnr_db", "n_changed", "raw_bytes", "stored_bytes", "ratio", "per_frame"]
    assert list(base["per_frame"][1]) == ["name", "max_abs_err", "sse", "n_changed", "psnr_db"]
    assert quality.summarize(*args, window=5, warm_up=1, ssim=None) == base
    assert len(quality.stdout_lines(base)) == 3
    rng = np.random.default_rng(8)
    a = rng.integers(0, 256, (2, 16, 24, 3), dtype=np.uint8)
    b = a.copy()
    b[1, 3:9, 5:11] ^= 0x10
    rec = ssim.frame_records(a, b)
    doc = quality.summarize(*args, window=5, warm_up=1, ssim=rec)
    fig = ssim.figures(rec)
    assert {k: v for k, v in doc.items() if k not in ("ssim", "ssim_min", "per_frame")} == {k: v for k, v in base.items() if k != "per_frame"}
    assert doc["ssim"] == fig["ssim"] < 1.0 and doc["ssim_min"] == fig["ssim_min"] == fig["per_frame"][1]["ssim_min"]
    for entry, before, f in zip(doc["per_frame"], base["per_frame"], fig["per_frame"]):
        assert {k: v for k, v in entry.items() if k not in ("ssim", "ssim_min")} == before
        assert entry["ssim"] == f["ssim"] and entry["ssim_min"] == f["ssim_min"]
    assert doc["per_frame"][0]["ssim"] == 1.0
    lines = quality.stdout_lines(doc)
    assert lines[:3] == quality.stdout_lines(base)
    assert lines[3:] == ["SSIM: %.6f (worst window %.6f)" % (doc["ssim"], doc["ssim_min"])]
    assert json.loads(json.dumps(doc)) == doc
    small = quality.summarize(stats, names, 7, 24, "abs", [2.0], [10, 100, 200], ssim=ssim.frame_records(a[:, :7], b[:, :7]))
    assert small["ssim"] is None and small["per_frame"][0]["ssim_min"] is None
    assert quality.stdout_lines(small)[3:] == ["SSIM: n/a"]
    with pytest.raises(ValueError):
        quality.summarize(*args, ssim=rec[:1])


# ------------------------------------------------------------------------------------------------------------ the flag
JOB = ["-p", "0", "-w", "5", "-m", "abs", "-b", "2"]


@pytest.mark.parametrize("args,env,needle", [
    (["-c", "M", "SRC", "{out}"] + JOB + ["--ssim"], {}, "add --report"),
    (["-u", "M", "SRC", "{out}", "--ssim"], {}, "--ssim"),
    (["-l", "M", "SRC", "--ssim"], {}, "--ssim"),
    (["-c", "M", "SRC", "{out}", "-p", "0", "--sweep", "5", "10", "-m", "abs", "-b", "2", "--ssim"], {}, "--sweep"),
    (["-c", "M", "SRC", "{out}", "-p", "0", "--sweep", "5", "10", "-m", "abs", "-b", "2", "--report", "--ssim"], {}, "--sweep"),
    (["-c", "M", "SRC", "{out}"] + JOB + ["--ssim"], {"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"}, "WORLD_SIZE"),
    (["-c", "M", "SRC", "{out}"] + JOB + ["--report", "--ssim"], {"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"}, "WORLD_SIZE"),
])
def test_ssim_refusals_exit_2_before_a_gpu_is_touched(tmp_path, monkeypatch, args, env, needle):
    from tezip_amd import tezip
    out = tmp_path / "out"
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setattr(tezip, "probe_gpu", lambda force: pytest.fail("the device was probed"))
    code, text = _tezip([a.replace("{out}", str(out)) for a in args])
    assert code == 2, text
    assert text.startswith("ERROR:") and needle in text
    assert "GPU MODE" not in text and "CPU MODE" not in text
    assert not out.exists()


def test_the_flag_alone_changes_no_other_check():
    from tezip_amd import tezip
    p = tezip.build_parser()
    assert tezip.check_ssim_flag(p.parse_args(["-c", "m", "d", "o"] + JOB)) is None
    ok = p.parse_args(["-c", "m", "d", "o"] + JOB + ["--report", "--ssim", "--shuffle", "--digests", "--gray", "--coder", "huff",
                                                      "--key-coder", "huffg"])
    assert tezip.check_ssim_flag(ok) is None and tezip.check_report_flag(ok) is None
    assert "--report" in tezip.check_ssim_flag(p.parse_args(["-c", "m", "d", "o"] + JOB + ["--ssim"]))


def test_run_refuses_ssim_without_report(capsys):
    from tezip_amd import compress
    with pytest.raises(SystemExit) as e:
        compress.run("M", "SRC", "OUT", 0, 5, None, "abs", [2.0], True, False, True, SSIM=True)
    assert e.value.code == 2 and "add --report" in capsys.readouterr().out


def test_the_abi_is_bound():
    from tezip_amd import _lib
    assert "tz_ssim_frames" in _lib.EXPORTS and "tz_encode_ssim" in _lib.EXPORTS
    assert _lib.SSIM_DTYPE is ssim.SSIM_DTYPE


# ------------------------------------------------------------------------------------------------- the directory CLI
def _write_dir(path, frames, mode="RGB"):
    from PIL import Image
    path.mkdir()
    for t, f in enumerate(frames):
        Image.fromarray(f if mode == "RGB" else f[..., 0], mode).save(path / ("f_%03d.png" % t))


def test_directory_cli(tmp_path, capsys):
    rng = np.random.default_rng(5)
    gray = np.repeat(rng.integers(0, 256, (3, 12, 17, 1), dtype=np.uint8), 3, axis=3)
    other = gray.copy()
    other[1, 2:7, 3:9] //= 2
    _write_dir(tmp_path / "a", gray, "L")          # single-channel files are widened
    _write_dir(tmp_path / "b", other)
    assert ssim.main([str(tmp_path / "a"), str(tmp_path / "b")]) == 0
    lines = capsys.readouterr().out.splitlines()
    fig = ssim.figures(ssim.frame_records(gray, other))
    assert len(lines) == 5
    for t in (0, 1, 2):
        f = fig["per_frame"][t]
        assert lines[t] == "f_%03d.png: SSIM %.6f (worst window %.6f)" % (t, f["ssim"], f["ssim_min"])
    assert lines[0] == "f_000.png: SSIM 1.000000 (worst window 1.000000)" and fig["per_frame"][1]["ssim"] < 1.0
    assert lines[3] == "SSIM: %.6f" % fig["ssim"] and lines[4] == "SSIM_min: %.6f" % fig["ssim_min"]
    names, rec = ssim.compare_dirs(str(tmp_path / "a"), str(tmp_path / "b"))
    assert names == ["f_000.png", "f_001.png", "f_002.png"]
    np.testing.assert_array_equal(rec, ssim.frame_records(gray, other))
    _write_dir(tmp_path / "fewer", other[:2])
    assert ssim.main([str(tmp_path / "a"), str(tmp_path / "fewer")]) == 2
    assert capsys.readouterr().out.startswith("ERROR:")
    _write_dir(tmp_path / "narrow", other[:, :, :16])
    assert ssim.main([str(tmp_path / "a"), str(tmp_path / "narrow")]) == 2
    assert ssim.main([str(tmp_path / "a"), str(tmp_path / "missing")]) == 2
    capsys.readouterr()
    _write_dir(tmp_path / "tiny_a", gray[:, :7])
    _write_dir(tmp_path / "tiny_b", other[:, :7])
    assert ssim.main([str(tmp_path / "tiny_a"), str(tmp_path / "tiny_b")]) == 0
    assert capsys.readouterr().out.splitlines()[-2:] == ["SSIM: n/a", "SSIM_min: n/a"]
