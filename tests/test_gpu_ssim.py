"""TZ-SSIM-1 on a MI355X (k_ssim; tz_ssim_frames, tz_encode_ssim, `-c --report --ssim`): the kernel's records against the numpy
statement of tezip_amd/ssim.py, every field equal as integers -- no tolerance: the definition has one floating-point
division, and a different Q would be a finding about it --, at the shapes where its tiles, aprons and row alignments can go
wrong, whatever the number of workgroups and whatever device memory held before; the records of an encode against the frames
the context's own decoder makes of the payload; and the report against the images `-u` writes."""
import contextlib
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

SMALL_STACKS = (3, 16, 32)
ONE = 1 << 32
NT = 3
# the tile is 15 x 15 window origins = 64 x 64 pixels, apron included: 64 x 64 and 130 x 67 fill it exactly in one direction or
# both, 70 x 150 and 130 x 67 straddle it
SHAPES = [(7, 9), (8, 8), (9, 13), (12, 12), (61, 90), (64, 64), (70, 150), (130, 67)]
CONTENTS = ["random", "equal", "one_sample", "0_vs_255", "scene"]
_CASES = {}


def _pair(h, w, content):
    from tezip_amd import ssim, synth
    rng = np.random.default_rng(1000 * h + w)
    a = rng.integers(0, 256, (NT, h, w, 3), dtype=np.uint8)
    if content == "random":
        b = rng.integers(0, 256, (NT, h, w, 3), dtype=np.uint8)
    elif content == "equal":
        b = a.copy()
    elif content == "one_sample":    # the last sample a window covers (the last sample of the frame where there is none)
        ny, nx = ssim.window_grid(h, w)
        y, x = (4 * ny + 3, 4 * nx + 3) if ny else (h - 1, w - 1)
        b = a.copy()
        b[:, y, x, 2] ^= 0x80
    elif content == "0_vs_255":
        a, b = np.zeros_like(a), np.full_like(a, 255)
    else:                            # a smooth pair one frame apart
        f = synth.translating_scene(NT + 1, h, w, seed=7)
        a, b = np.ascontiguousarray(f[:-1]), np.ascontiguousarray(f[1:])
    return a, b


def _case(h, w, content):
    """(a, b, numpy records): computed once, shared, never written to."""
    key = (h, w, content)
    if key not in _CASES:
        from tezip_amd import ssim
        a, b = _pair(h, w, content)
        want = ssim.frame_records(a, b)
        for x in (a, b, want):
            x.setflags(write=False)
        _CASES[key] = (a, b, want)
    return _CASES[key]


def _same(got, want, msg=""):
    for field in ("sum_q32", "min_q32", "windows", "reserved"):
        np.testing.assert_array_equal(got[field], want[field], err_msg="%s %s" % (field, msg))


@pytest.fixture(scope="module")
def ctx():
    from tezip_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------------------------------------ kernel against numpy
@pytest.mark.parametrize("h,w", SHAPES)
def test_kernel_equals_numpy(ctx, h, w):
    from tezip_amd import ssim
    for content in CONTENTS:
        a, b, want = _case(h, w, content)
        got = ctx.ssim_frames(np.ascontiguousarray(a), np.ascontiguousarray(b))
        assert got.dtype == ssim.SSIM_DTYPE
        _same(got, want, "%dx%d %s" % (h, w, content))
        assert (got["windows"] == ssim.window_count(h, w)).all()
        if (h, w) == (7, 9):
            assert not got["windows"].any() and not got["min_q32"].any() and not got["sum_q32"].any()
        elif content == "equal":
            assert (got["min_q32"] == ONE).all() and (got["sum_q32"] == got["windows"].astype(np.int64) * ONE).all()
        elif content == "one_sample":   # seen by exactly one window of one channel
            assert (got["min_q32"] < ONE).all() and (got["sum_q32"] > (got["windows"].astype(np.int64) - 1) * ONE).all()
    assert ssim.window_count(8, 8) == 3


@pytest.mark.parametrize("offset", [1, 2, 3])
def test_unaligned_device_stacks(ctx, offset):
    """Device views that start 1..3 bytes behind a dword boundary, each stack at its own offset: the rows at both ends of a
    stack take the byte loads."""
    import torch
    for (h, w) in ((9, 13), (61, 90), (64, 64)):
        a, b, want = _case(h, w, "random")
        views = []
        for x, off in ((a, offset), (b, (offset + 1) % 4)):
            flat = torch.from_numpy(np.ascontiguousarray(x).reshape(-1).copy())
            buf = torch.full((flat.numel() + 32,), 0xEE, dtype=torch.uint8, device="cuda")
            base = (-buf.data_ptr()) % 16
            view = buf[base + off: base + off + flat.numel()]
            view.copy_(flat)
            views.append((buf, view.view(NT, h, w, 3)))
        torch.cuda.synchronize()
        _same(ctx.ssim_frames(views[0][1], views[1][1]), want, "%dx%d offset %d" % (h, w, offset))


CHILD = r'''
import sys
import numpy as np
sys.path.insert(0, %r)
from tezip_amd import _lib
src = np.load(sys.argv[1])
ctx = _lib.Context(0)
out = {}
for rep in range(2):   # the second pass runs on recycled pool blocks
    for name in sorted(k[2:] for k in src.files if k.startswith("a_")):
        out[name] = ctx.ssim_frames(src["a_" + name], src["b_" + name])
ctx.close()
np.savez(sys.argv[2], **out)
print("child ok")
'''


@pytest.mark.parametrize("env", [{"TEZIP_SSIM_GRID": "1"}, {"TEZIP_SSIM_GRID": "3"}, {}, {"TEZIP_POISON": "165"}],
                         ids=["grid1", "grid3", "default", "poison0xA5"])
def test_records_do_not_depend_on_the_grid_or_on_stale_memory(tmp_path, env):
    """Both switches are read once per process: each setting runs in a fresh child (TEZIP_POISON takes a decimal byte: 165 = 0xA5)."""
    stacks, wants = {}, {}
    for (h, w) in SHAPES:
        for content in ("random", "scene", "one_sample"):
            name = "%dx%d_%s" % (h, w, content)
            a, b, wants[name] = _case(h, w, content)
            stacks["a_" + name], stacks["b_" + name] = a, b
    np.savez(tmp_path / "in.npz", **stacks)
    e = dict(os.environ)
    for k in ("TEZIP_SSIM_GRID", "TEZIP_POISON"):
        e.pop(k, None)
    e.update(env)
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-c", CHILD % ROOT, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")],
                       env=e, capture_output=True, text=True, timeout=150)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout + r.stderr[-2000:]
    got = np.load(tmp_path / "out.npz")
    assert sorted(got.files) == sorted(wants)
    for name, want in wants.items():
        _same(got[name], want, name)


def test_argument_errors():
    from tezip_amd import _lib
    c = _lib.Context(0)
    try:
        c.prof_enable(True)
        x = np.zeros(8 * 8 * 3, np.uint8)
        out = np.full(2, 7, _lib.SSIM_DTYPE)
        p, o = x.ctypes.data, out.ctypes.data
        assert c.lib.tz_ssim_frames(c.h, p, p, -1, 8, 8, o) == -1
        assert c.lib.tz_ssim_frames(c.h, p, p, 1, 0, 8, o) == -1
        assert c.lib.tz_ssim_frames(c.h, p, p, 1, 8, -3, o) == -1
        assert c.lib.tz_ssim_frames(c.h, p, p, 1, 1 << 15, 1 << 16, o) == -1      # a frame of 3 * 2^31 bytes
        assert c.lib.tz_ssim_frames(c.h, None, p, 1, 8, 8, o) == -1
        assert c.lib.tz_ssim_frames(c.h, p, p, 1, 8, 8, None) == -1
        assert c.lib.tz_ssim_frames(c.h, p, p, 0, 8, 8, o) == 0                   # launches nothing
        assert c.prof_get()["quality"][1] == 0 and (out["windows"] == 7).all()
        assert c.lib.tz_ssim_frames(c.h, p, p, 1, 8, 8, o) == 0
        assert c.prof_get()["quality"][1] > 0                                     # counted where k_quality is counted
        assert tuple(out[0]) == (3 * ONE, ONE, 3, 0) and int(out["windows"][1]) == 7
        assert c.lib.tz_encode_ssim(c.h, None, 0, None, -1, 0, o) == -4           # no rollout
    finally:
        c.close()


# ----------------------------------------------------------------------------------------------------------- encodes
def _model(seed=4):
    from tezip_amd.prednet import PredNetConfig
    cfg = PredNetConfig(stack_sizes=SMALL_STACKS)
    return cfg, cfg.init_weights(seed=seed, bias_scale=0.2)


def _frames(scene):
    from tezip_amd import synth
    return synth.moving_blobs(12, 64, 64, seed=1) if scene == "blobs" else synth.translating_scene(12, 61, 90, seed=5)


@pytest.mark.parametrize("scene,bound,shuffle,channels", [
    ("blobs", 0.0, False, 3), ("scene", 0.0, False, 3), ("blobs", 2.0, False, 3), ("scene", 2.0, False, 3),
    ("scene", 2.0, True, 3), ("blobs", 2.0, False, 1)])
def test_encode_ssim_describes_what_the_decoder_makes_of_the_payload(scene, bound, shuffle, channels):
    from tezip_amd import _lib, ssim
    frames = _frames(scene)
    nt, h, w, _ = frames.shape
    p = 1
    cfg, wts = _model()
    c = _lib.Context(0)
    try:
        c.load_model(cfg, wts)
        c.prepare(_lib.pad8(h), _lib.pad8(w), max_batch=4)
        c.set_payload_channels(channels)
        key, _ = c.rollout(frames, p, 5)
        payload, table, _ = c.encode("abs", [bound], True, shuffle=shuffle)
        payload = np.array(payload, copy=True)
        assert payload.size == nt * h * w * channels
        got = c.encode_ssim(payload, table, shuffle=shuffle)
        q = c.encode_quality(payload, table, shuffle=shuffle)
        c.encode("abs", [bound], True, payload="resident", shuffle=shuffle)          # ... and on the resident payload
        _same(c.encode_ssim("resident", table, shuffle=shuffle), got, "resident")
        np.testing.assert_array_equal(c.payload_get(0, payload.size), payload)       # nothing of the context changed
        assert (got["windows"] == ssim.window_count(h, w)).all() and (got["reserved"] == 0).all()
        if bound == 0:
            assert (got["min_q32"] == ONE).all() and (got["sum_q32"] == got["windows"].astype(np.int64) * ONE).all()
        plain = c.byte_unshuffle(payload.view(np.uint8)) if shuffle else payload
        c.rollout_decode(np.where(key[:, None, None, None], frames, 0).astype(np.uint8), p)
        dec = c.decode(plain, table).copy()
        want = ssim.frame_records(dec, frames)
        _same(got, want, "%s abs %g" % (scene, bound))
        if bound > 0:
            assert (got["min_q32"] < ONE).any() and (q["max_abs"] <= 2).all()
        with pytest.raises(_lib.TezipError) as e:                                    # a decoder rollout is not an encode
            c.encode_ssim(payload, table, shuffle=shuffle)
        assert e.value.status == -4
    finally:
        c.close()


# --------------------------------------------------------------------------------------------------------------- CLI
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


def test_cli_report_with_ssim_end_to_end(tmp_path):
    from PIL import Image
    from tezip_amd import _lib, ssim, weights
    frames = _frames("scene")
    nt, h, w, _ = frames.shape
    cfg, wts = _model()
    mdir = str(tmp_path / "model")
    weights.save_model(mdir, cfg, wts, _lib.pad8(h), _lib.pad8(w))
    ddir = tmp_path / "data"
    ddir.mkdir()
    names = ["f_%03d.png" % t for t in range(nt)]
    for t in range(nt):
        Image.fromarray(frames[t]).save(ddir / names[t])
    job = ["-p", "1", "-w", "5", "-m", "abs", "-b", "2", "--report"]
    with_s, without = str(tmp_path / "comp_s"), str(tmp_path / "comp")
    code, out_s = _tezip(["-c", mdir, ddir, with_s] + job + ["--ssim"])
    assert code == 0, out_s
    code, out = _tezip(["-c", mdir, ddir, without] + job)
    assert code == 0, out
    # without the flag: today's document and today's three lines
    report_lines = [ln for ln in out.splitlines() if ln.startswith(("max_abs_err:", "PSNR:", "ratio:", "SSIM"))]
    assert [ln.split(":")[0] for ln in report_lines] == ["max_abs_err", "PSNR", "ratio"]
    base = json.load(open(os.path.join(without, "quality.json")))
    assert "ssim" not in base and "ssim_min" not in base and all("ssim" not in f and "ssim_min" not in f for f in base["per_frame"])
    # with it: four lines, four keys, nothing else differs
    doc = json.load(open(os.path.join(with_s, "quality.json")))
    lines_s = [ln for ln in out_s.splitlines() if ln.startswith(("max_abs_err:", "PSNR:", "ratio:", "SSIM"))]
    assert lines_s == report_lines + ["SSIM: %.6f (worst window %.6f)" % (doc["ssim"], doc["ssim_min"])]
    assert sorted(os.listdir(with_s)) == sorted(os.listdir(without))
    for n in os.listdir(without):
        if n != "quality.json":
            assert open(os.path.join(with_s, n), "rb").read() == open(os.path.join(without, n), "rb").read(), n
    assert {k: v for k, v in doc.items() if k not in ("ssim", "ssim_min", "per_frame")} == {k: v for k, v in base.items() if k != "per_frame"}
    assert [{k: v for k, v in f.items() if k not in ("ssim", "ssim_min")} for f in doc["per_frame"]] == base["per_frame"]
    # -u, then the directory CLI on the sources and the restored images: the same figures, exactly
    udir = str(tmp_path / "dec")
    code, out_u = _tezip(["-u", mdir, with_s, udir])
    assert code == 0, out_u
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        assert ssim.main([str(ddir), udir]) == 0
    cli_lines = buf.getvalue().splitlines()
    got_names, rec = ssim.compare_dirs(str(ddir), udir)
    fig = ssim.figures(rec)
    assert got_names == names == [f["name"] for f in doc["per_frame"]]
    assert [(f["ssim"], f["ssim_min"]) for f in doc["per_frame"]] == [(f["ssim"], f["ssim_min"]) for f in fig["per_frame"]]
    assert (doc["ssim"], doc["ssim_min"]) == (fig["ssim"], fig["ssim_min"])
    assert cli_lines[:nt] == ["%s: SSIM %.6f (worst window %.6f)" % (f["name"], f["ssim"], f["ssim_min"]) for f in doc["per_frame"]]
    assert cli_lines[nt:] == ["SSIM: %.6f" % doc["ssim"], "SSIM_min: %.6f" % doc["ssim_min"]]
    assert doc["ssim_min"] <= doc["ssim"] < 1.0 and doc["max_abs_err"] == 2
    assert doc["per_frame"][0]["ssim"] == 1.0                                    # (frame 0 is a key frame: stored as it is)
