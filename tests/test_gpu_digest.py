"""Per-frame digests on a MI355X (k_digest; `-c --digests`, `-u --verify`): the kernel against the numpy statement of
tezip_amd/digest.py at the shapes where its cutting can go wrong, whatever the alignment of the stack and the number of
workgroups; the records `-c` writes against the images `-u` writes and the inputs; and detection -- of a changed record and
of a stream that is valid in every field but decodes one frame differently -- before an image is written."""
import contextlib
import io
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

SMALL_STACKS = (3, 16, 32)


def _rule(n):
    return ((7 * np.arange(n, dtype=np.int64)) % 251).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ kernel against numpy
def _stack(name):
    rng = np.random.default_rng(11)
    if name == "700x1x1":      # a lane's 16 bytes span six frames
        return rng.integers(0, 256, (700, 1, 1, 3), dtype=np.uint8)
    if name == "9x8x8":
        return rng.integers(0, 256, (9, 8, 8, 3), dtype=np.uint8)
    if name == "5x61x90":      # 16 470 bytes = 6 mod 16: every frame starts at another alignment
        return rng.integers(0, 256, (5, 61, 90, 3), dtype=np.uint8)
    if name == "4x64x64":      # three tiles per frame: a frame is shared by several workgroups
        return rng.integers(0, 256, (4, 64, 64, 3), dtype=np.uint8)
    if name == "1x8x700000":   # positions from 2^24 on
        return _rule(8 * 700000 * 3).reshape(1, 8, 700000, 3)
    raise KeyError(name)


SHAPES = ["700x1x1", "9x8x8", "5x61x90", "4x64x64", "1x8x700000"]
_CASES = {}


def _case(name):
    """(stack, numpy digests): computed once, shared, never written to."""
    if name not in _CASES:
        from tezip_amd import digest
        x = _stack(name)
        x.setflags(write=False)
        want = digest.stack_digests(x)
        want.setflags(write=False)
        _CASES[name] = (x, want)
    return _CASES[name]


@pytest.fixture(scope="module")
def ctx():
    from tezip_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _device_view(x, offset):
    """The bytes of x in device memory, starting `offset` bytes behind a 16-byte boundary."""
    import torch
    flat = torch.from_numpy(np.ascontiguousarray(x).reshape(-1).copy())
    buf = torch.zeros(flat.numel() + 32, dtype=torch.uint8, device="cuda")
    base = (-buf.data_ptr()) % 16
    view = buf[base + offset: base + offset + flat.numel()]
    view.copy_(flat)
    torch.cuda.synchronize()
    assert view.data_ptr() % 16 == offset and view.is_contiguous()
    return buf, view


@pytest.mark.parametrize("name", SHAPES)
def test_kernel_equals_numpy_from_host_and_device(ctx, name):
    import torch
    x, want = _case(name)
    nf, fb = x.shape[0], x[0].size
    if name == "1x8x700000":
        assert "%016x" % int(want[0]) == "61f0594597e474b8"      # the known answer of the format
    np.testing.assert_array_equal(ctx.frame_digests(np.ascontiguousarray(x)), want)
    _, view = _device_view(x, 0)
    np.testing.assert_array_equal(ctx.frame_digests(view, nf, fb), want)
    out = torch.full((nf,), -1, dtype=torch.int64, device="cuda")    # device words: the same 64 bits
    torch.cuda.synchronize()
    ctx.frame_digests(view, nf, fb, out=out)
    np.testing.assert_array_equal(out.cpu().numpy().view(np.uint64), want)


@pytest.mark.parametrize("offset", [1, 5, 15])
def test_unaligned_device_views(ctx, offset):
    x, want = _case("5x61x90")
    _, view = _device_view(x, offset)
    np.testing.assert_array_equal(ctx.frame_digests(view, 5, 61 * 90 * 3), want)
    y, want_y = _case("700x1x1")
    _, view = _device_view(y, offset)
    np.testing.assert_array_equal(ctx.frame_digests(view, 700, 3), want_y)


@pytest.mark.parametrize("grid", ["1", "2", "7", "1000"])
def test_digests_do_not_depend_on_the_grid(grid):
    from tezip_amd import _lib
    before = os.environ.get("TEZIP_DIGEST_GRID")
    os.environ["TEZIP_DIGEST_GRID"] = grid        # read when a context is made
    try:
        c = _lib.Context(0)
        try:
            for name in ("5x61x90", "700x1x1", "9x8x8", "4x64x64"):
                x, want = _case(name)
                np.testing.assert_array_equal(c.frame_digests(np.ascontiguousarray(x)), want, err_msg=name)
            x, want = _case("5x61x90")
            for offset in (0, 1, 5, 15):
                _, view = _device_view(x, offset)
                np.testing.assert_array_equal(c.frame_digests(view, 5, 61 * 90 * 3), want, err_msg="offset %d" % offset)
        finally:
            c.close()
    finally:
        if before is None:
            os.environ.pop("TEZIP_DIGEST_GRID", None)
        else:
            os.environ["TEZIP_DIGEST_GRID"] = before


def test_argument_and_state_errors():
    from tezip_amd import _lib
    c = _lib.Context(0)
    try:
        c.prof_enable(True)
        x = np.zeros(64, np.uint8)
        out = np.full(4, 7, np.uint64)
        # frames of 2^32 bytes and more are refused before anything is staged or launched
        assert c.lib.tz_frame_digests(c.h, x.ctypes.data, 1, 1 << 32, out.ctypes.data) == -1
        assert c.lib.tz_frame_digests(c.h, x.ctypes.data, -1, 16, out.ctypes.data) == -1
        assert c.lib.tz_frame_digests(c.h, None, 1, 16, out.ctypes.data) == -1
        assert c.lib.tz_frame_digests(c.h, x.ctypes.data, 1, 16, None) == -1
        assert c.prof_get()["digest"][1] == 0
        assert c.lib.tz_frame_digests(c.h, x.ctypes.data, 0, 16, out.ctypes.data) == 0 and (out == 7).all()
        assert c.lib.tz_frame_digests(c.h, x.ctypes.data, 4, 0, out.ctypes.data) == 0 and (out == 0).all()   # empty frames
        assert c.lib.tz_decoded_digests(c.h, 0, 1, out.ctypes.data) == -4        # no decoded frames in the context
        assert c.lib.tz_encode_digests(c.h, None, 0, None, -1, 0, out.ctypes.data, None) == -4   # no rollout
    finally:
        c.close()


def test_decoded_and_encode_digests_through_the_abi():
    """tz_encode_digests on an encode, tz_decoded_digests on a fresh context's resident decode of the same payload and
    tz_frame_digests of the frames it fetches: one answer; the range rule is tz_decoded_get's."""
    from tezip_amd import _lib, digest, synth
    from tezip_amd.prednet import PredNetConfig
    cfg = PredNetConfig(stack_sizes=SMALL_STACKS)
    wts = cfg.init_weights(seed=1, bias_scale=0.2)
    nt, h, w, p = 12, 61, 90, 1
    frames = synth.translating_scene(nt, h, w, seed=1)
    enc, dec = _lib.Context(0), _lib.Context(0)
    try:
        for c in (enc, dec):
            c.load_model(cfg, wts)
            c.prepare(_lib.pad8(h), _lib.pad8(w), max_batch=4)
        key, _ = enc.rollout(frames, p, 4)
        payload, table, _ = enc.encode("abs", [2.0], True)
        payload = np.array(payload, copy=True)
        d_dec, d_org = enc.encode_digests(payload, table)
        np.testing.assert_array_equal(d_org, digest.stack_digests(frames))
        q = enc.encode_quality(payload, table)
        np.testing.assert_array_equal(d_dec != d_org, q["n_changed"] > 0)
        only_dec, none = enc.encode_digests(payload, table, original=False)
        assert none is None
        np.testing.assert_array_equal(only_dec, d_dec)
        again, t2, _ = enc.encode("abs", [2.0], True)      # a following encode behaves as it would have
        np.testing.assert_array_equal(again, payload)
        keys = np.where(key[:, None, None, None], frames, 0).astype(np.uint8)
        dec.rollout_decode(keys, p)
        dec.decode(payload, table, out="resident")
        np.testing.assert_array_equal(dec.decoded_digests(0, nt), d_dec)
        np.testing.assert_array_equal(dec.decoded_digests(3, 4), d_dec[3:7])
        np.testing.assert_array_equal(digest.stack_digests(dec.decoded_get(0, nt)), d_dec)
        out = np.zeros(nt + 1, np.uint64)
        assert dec.lib.tz_decoded_digests(dec.h, 0, nt + 1, out.ctypes.data) == -1
        assert dec.lib.tz_decoded_digests(dec.h, -1, 2, out.ctypes.data) == -1
        dec.rollout_decode_range(keys, p, 5, 4)             # a range decode: sequence indices inside [5, 9)
        dec.decode_range(payload, table, 5, 4, out="resident")
        np.testing.assert_array_equal(dec.decoded_digests(6, 3), d_dec[6:9])
        assert dec.lib.tz_decoded_digests(dec.h, 4, 2, out.ctypes.data) == -1
        assert dec.lib.tz_decoded_digests(dec.h, 8, 2, out.ctypes.data) == -1
    finally:
        enc.close()
        dec.close()


# ------------------------------------------------------------------------------------------------------- end to end
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


def _read_images(d, names):
    from PIL import Image
    return np.stack([np.asarray(Image.open(os.path.join(d, n)).convert("RGB")) for n in names])


JOBS = {   # scene, size, bound, extra flags of -c
    "lossless": ("blobs", (64, 64), "0", []),
    "abs2": ("blobs", (64, 64), "2", []),
    "lossless_gpu_coders": ("blobs", (64, 64), "0", ["--coder", "huffr", "--key-coder", "huff"]),
    "abs2_gpu_coders": ("blobs", (64, 64), "2", ["--coder", "huffr", "--key-coder", "huff"]),
    "abs2_shuffle_61x90": ("scene", (61, 90), "2", ["--shuffle"]),     # -u takes the whole-array path
}
NT = 12
_RUNS = {}


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("digest_e2e")


def _job(workdir, name):
    """The job's model, inputs and two compressed directories (with --digests --report / without either flag) and the
    images `-u` writes from the first: made once per module."""
    if name in _RUNS:
        return _RUNS[name]
    from PIL import Image
    from tezip_amd import _lib, synth, weights
    from tezip_amd.prednet import PredNetConfig
    scene, (h, w), bound, extra = JOBS[name]
    base = workdir / name
    base.mkdir()
    cfg = PredNetConfig(stack_sizes=SMALL_STACKS)
    wts = cfg.init_weights(seed=4, bias_scale=0.2)
    mdir = str(base / "model")
    weights.save_model(mdir, cfg, wts, _lib.pad8(h), _lib.pad8(w))
    frames = synth.moving_blobs(NT, h, w, seed=1) if scene == "blobs" else synth.translating_scene(NT, h, w, seed=5)
    ddir = base / "data"
    ddir.mkdir()
    names = ["f_%03d.png" % t for t in range(NT)]
    for t in range(NT):
        Image.fromarray(frames[t]).save(ddir / names[t])
    job = ["-p", "1", "-w", "5", "-m", "abs", "-b", bound] + extra
    with_d, without = str(base / "comp_d"), str(base / "comp")
    code, out_d = _tezip(["-c", mdir, ddir, with_d] + job + ["--digests", "--report"])
    assert code == 0, out_d
    code, out = _tezip(["-c", mdir, ddir, without] + job)
    assert code == 0, out
    udir = str(base / "dec_d")
    code, out_u = _tezip(["-u", mdir, with_d, udir])
    assert code == 0, out_u
    _RUNS[name] = dict(mdir=mdir, frames=frames, names=names, with_d=with_d, without=without, udir=udir, out_u=out_u,
                       base=base, lossless=bound == "0")
    return _RUNS[name]


@pytest.mark.parametrize("name", list(JOBS))
def test_records_describe_what_u_writes(workdir, name):
    from tezip_amd import digest
    r = _job(workdir, name)
    four = ["entropy.dat", "filename.txt", "key_frame.dat", "tezip_amd.json"]
    assert sorted(os.listdir(r["without"])) == four
    assert sorted(os.listdir(r["with_d"])) == sorted(four + ["frame_digests.json", "quality.json"])
    for n in four:   # the flag changes nothing that -c writes otherwise
        assert open(os.path.join(r["with_d"], n), "rb").read() == open(os.path.join(r["without"], n), "rb").read(), n
    h, w = r["frames"].shape[1:3]
    doc = digest.read(r["with_d"], frames=NT, shape=(h, w, 3))
    assert sorted(os.listdir(r["udir"])) == r["names"]
    dec = _read_images(r["udir"], r["names"])
    assert doc["decoded"] == digest.to_hex(digest.stack_digests(dec))
    assert doc["original"] == digest.to_hex(digest.stack_digests(r["frames"]))
    report = json.load(open(os.path.join(r["with_d"], "quality.json")))
    changed = [f["n_changed"] > 0 for f in report["per_frame"]]
    assert [a != b for a, b in zip(doc["decoded"], doc["original"])] == changed
    if r["lossless"]:
        assert not any(changed) and (dec == r["frames"]).all()
    else:
        assert any(changed) and not all(changed)       # (key frames carry no error)
    assert r["out_u"].splitlines().count("verified: %d frames" % NT) == 1
    part = str(r["base"] / "dec_part")
    code, out = _tezip(["-u", r["mdir"], r["with_d"], part, "--frames", "3:7"])
    assert code == 0, out
    assert out.splitlines().count("verified: 4 frames") == 1
    assert sorted(os.listdir(part)) == r["names"][3:7]
    code, out = _tezip(["-u", r["mdir"], r["with_d"], str(r["base"] / "dec_req"), "--verify", "require"])
    assert code == 0 and "verified: %d frames" % NT in out, out


def test_whole_array_path_verifies_too(workdir, monkeypatch):
    r = _job(workdir, "abs2")
    monkeypatch.setenv("TEZIP_NO_STREAMING", "1")
    udir = str(r["base"] / "dec_whole")
    code, out = _tezip(["-u", r["mdir"], r["with_d"], udir])
    assert code == 0 and out.splitlines().count("verified: %d frames" % NT) == 1, out
    assert (_read_images(udir, r["names"]) == _read_images(r["udir"], r["names"])).all()
    code, out = _tezip(["-u", r["mdir"], r["with_d"], str(r["base"] / "dec_whole_part"), "--frames", "3:7"])
    assert code == 0 and out.splitlines().count("verified: 4 frames") == 1, out


# -------------------------------------------------------------------------------------------------------- detection
def _files(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d))}


@pytest.mark.parametrize("name", ["abs2", "abs2_shuffle_61x90"])
def test_a_changed_record_is_detected_before_an_image_is_written(workdir, name):
    from tezip_amd import digest
    r = _job(workdir, name)
    bad_dir = str(r["base"] / "comp_bad_record")
    shutil.copytree(r["with_d"], bad_dir)
    doc = json.load(open(os.path.join(bad_dir, digest.NAME)))
    word = doc["decoded"][7]
    doc["decoded"][7] = word[:5] + ("0" if word[5] != "0" else "1") + word[6:]     # one hex digit
    digest.write(bad_dir, doc)
    out_dir = str(r["base"] / "dec_bad_record")
    code, out = _tezip(["-u", r["mdir"], bad_dir, out_dir])
    assert code == 3, out
    errors = [ln for ln in out.splitlines() if ln.startswith("ERROR")]
    assert errors == ["ERROR: frame 7 (%s) does not match its recorded digest" % r["names"][7]]
    assert "verified" not in out
    assert not os.path.exists(out_dir) or os.listdir(out_dir) == []          # no image
    code, out = _tezip(["-u", r["mdir"], bad_dir, str(r["base"] / "dec_bad_record_0_7"), "--frames", "0:7"])
    assert code == 0 and "verified: 7 frames" in out, out
    off_dir = str(r["base"] / "dec_bad_record_off")
    code, out = _tezip(["-u", r["mdir"], bad_dir, off_dir, "--verify", "off"])
    assert code == 0 and "verified" not in out and "ERROR" not in out, out
    assert _files(off_dir) == _files(r["udir"])                                # the images of before the change
    if name == "abs2":   # the status is the process's exit status
        p = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m", "tezip_amd.tezip", "-u", r["mdir"], bad_dir,
                            str(r["base"] / "dec_bad_record_cli")], cwd=ROOT, capture_output=True, text=True, timeout=330)
        assert p.returncode == 3, p.stdout + p.stderr
        assert "ERROR: frame 7 (%s) does not match its recorded digest" % r["names"][7] in p.stdout


def test_a_valid_stream_that_decodes_one_frame_differently_is_detected(workdir):
    """Two ADJACENT unequal payload elements of a non-key frame k exchanged: the multiset of symbols and every prefix sum
    behind the pair are what they were, so the stream is valid in every field and only frame k decodes differently."""
    from tezip_amd import zstd
    from tezip_amd.decompress import parse_stream
    r = _job(workdir, "abs2")
    h, w = r["frames"].shape[1:3]
    fe = h * w * 3
    keys = np.frombuffer(zstd.decompress(open(os.path.join(r["with_d"], "key_frame.dat"), "rb").read()), np.uint8)
    is_key = keys.reshape(NT, fe).any(axis=1)
    warm_up = 1
    k = next(i for i in range(NT // 2, NT) if not is_key[i] and i > warm_up)
    stream = np.frombuffer(zstd.decompress(open(os.path.join(r["with_d"], "entropy.dat"), "rb").read()), "<i2").copy()
    payload, table, shape, p = parse_stream(stream)
    assert tuple(shape) == (1, NT, h, w, 3) and p == warm_up and payload.size == NT * fe
    clean = _files(r["udir"])
    seg = payload[k * fe: (k + 1) * fe]
    pairs = k * fe + np.nonzero(seg[:-1] != seg[1:])[0]
    assert pairs.size > 0
    bad_dir = str(r["base"] / "comp_bad_stream")
    shutil.copytree(r["with_d"], bad_dir)
    found = None
    for n, i in enumerate(pairs[:8]):
        bad = stream.copy()                     # (the trailer is untouched)
        bad[i], bad[i + 1] = stream[i + 1], stream[i]
        with open(os.path.join(bad_dir, "entropy.dat"), "wb") as f:
            f.write(zstd.compress_array(bad, 9))
        off_dir = str(r["base"] / ("dec_bad_stream_off_%d" % n))
        code, out = _tezip(["-u", r["mdir"], bad_dir, off_dir, "--verify", "off"])
        assert code == 0, out
        got = _files(off_dir)
        if got != clean:
            found = i
            assert [nm for nm in r["names"] if got[nm] != clean[nm]] == [r["names"][k]]    # only frame k
            break
    assert found is not None, "no exchange among the first 8 pairs of frame %d changed an image" % k
    out_dir = str(r["base"] / "dec_bad_stream")
    code, out = _tezip(["-u", r["mdir"], bad_dir, out_dir])
    assert code == 3, out
    errors = [ln for ln in out.splitlines() if ln.startswith("ERROR")]
    assert errors == ["ERROR: frame %d (%s) does not match its recorded digest" % (k, r["names"][k])]
    assert not os.path.exists(out_dir) or os.listdir(out_dir) == []
    code, out = _tezip(["-u", r["mdir"], bad_dir, str(r["base"] / "dec_bad_stream_0_k"), "--frames", "0:%d" % k])
    assert code == 0 and "verified: %d frames" % k in out, out


# ------------------------------------------------------------------------------------- a directory without the file
@pytest.mark.parametrize("name,env", [("abs2", {}), ("abs2", {"TEZIP_NO_STREAMING": "1"}), ("abs2_gpu_coders", {}),
                                      ("abs2_shuffle_61x90", {})])
def test_a_directory_without_records_decodes_as_ever(workdir, monkeypatch, name, env):
    from tezip_amd import _lib
    r = _job(workdir, name)
    launches = []

    class Spy(_lib.Context):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            self.prof_enable(True)

        def close(self):
            if getattr(self, "h", None):
                launches.append(self.prof_get()["digest"][1])
            super().close()

    for key, value in env.items():
        monkeypatch.setenv(key, value)
    monkeypatch.setattr(_lib, "Context", Spy)
    tag = "_".join(["dec_plain"] + sorted(env))
    code, out = _tezip(["-u", r["mdir"], r["without"], str(r["base"] / tag)])
    assert code == 0, out
    assert launches and not any(launches)                        # contexts were watched; none launched k_digest
    assert "verified" not in out and "digest" not in out
    assert _files(str(r["base"] / tag)) == _files(r["udir"])      # the bytes -u writes from the recorded twin
    launches.clear()
    code, out_v = _tezip(["-u", r["mdir"], r["with_d"], str(r["base"] / (tag + "_recorded"))])
    assert code == 0 and sum(launches) == 1, out_v                # (the watch sees the launch where there is one)
    assert [ln for ln in out_v.splitlines() if not ln.startswith("verified:")] == out.splitlines()
