"""The lattice quantiser TZ-QL1 on a MI355X (tz_set_quantiser, tz_lattice_bound, tz_lattice_bound_frames; `-c --quant lattice`):
the seams and the encoder's entry points against the slow statement (tezip_amd/lattice.py) followed by each layout's slow
reference, the probes against the job they describe, and the command line end to end.  Integers and bytes throughout."""
import json
import os

import numpy as np
import pytest

import test_gpu_ratetarget as TR
import test_gpu_target as TT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from tezip_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _reset(ctx):
    ctx.prof_enable(False)
    ctx.set_quantiser(0)
    ctx.set_frame_bounds(None)
    ctx.set_payload_channels(3)
    ctx.set_delta_stride(0)


# ------------------------------------------------------------------------------------------------------ 1. the seams
SEAM_SIZES = [(21, 30), (61, 90), (64, 64)]     # HW % 8 != 0; several blocks and a frame boundary inside a vector group; whole groups
SEAM_CASES = [("abs", [b]) for b in (0.5, 1.0, 2.0, 2.5, 127.0, 255.0, 300.0)] + [("rel", [0.02]), ("absrel", [3.0, 0.05]), ("pwrel", [0.05])]
SEAM_SKIP = np.array([0, 0, 1, 0, 0, 0, 0], np.uint8)
SEAM_BOUNDS = [0.0, 0.5, 9.0, 1.0, 2.5, 127.0, 300.0]


def _seam_stacks(h, w):
    rng = np.random.default_rng(h * 1000 + w)
    diff = rng.integers(-255, 256, (7, h, w, 3)).astype(np.int16)
    diff[:, 0, 0] = [-255, 255, -254]           # the extremes, in every frame and channel
    diff[:, -1, -1] = [255, -255, 254]
    orig = rng.integers(0, 256, diff.shape).astype(np.uint8)
    orig[3] = np.clip(orig[3], 100, 140)        # a narrow slab: rel tolerances below 1
    orig[4, :, :, 1] = 77                       # a constant slab: rel tolerance 0
    return orig, diff


@pytest.fixture(scope="module")
def seam_want():
    from tezip_amd import lattice
    memo = {}

    def get(h, w):
        if (h, w) not in memo:
            orig, diff = _seam_stacks(h, w)
            want = {(m, tuple(v)): lattice.quantise_stack(orig, diff, m, v, SEAM_SKIP) for m, v in SEAM_CASES}
            want["frames"] = lattice.quantise_stack(orig, diff, "abs", [0.0], SEAM_SKIP, bounds=SEAM_BOUNDS)
            memo[h, w] = (orig, diff, want)
        return memo[h, w]
    return get


def _on_device(stack, off, dtype):
    import torch
    t = torch.zeros(stack.size + 16, dtype=dtype, device="cuda")
    t[off: off + stack.size] = torch.from_numpy(stack.reshape(-1)).cuda()
    return t, t[off: off + stack.size].view(stack.shape)


@pytest.mark.parametrize("h,w", SEAM_SIZES)
def test_seams_equal_the_slow_statement(ctx, seam_want, h, w):
    import torch
    orig, diff, want = seam_want(h, w)
    changed = 0
    for mode, value in SEAM_CASES:
        key = (mode, tuple(value))
        got = ctx.lattice_bound(orig, diff.copy(), mode, value, SEAM_SKIP)
        np.testing.assert_array_equal(got, want[key], err_msg="host, %s %r" % key)
        np.testing.assert_array_equal(got[2], diff[2])                       # the skipped frame
        changed += int((got != diff).any())
        if mode == "abs" and value[0] < 1:
            np.testing.assert_array_equal(got, diff)
        if mode == "abs" and value[0] >= 255:
            assert not np.delete(got, 2, axis=0).any()
    assert changed == len(SEAM_CASES) - 1                                    # every case but abs 0.5 bites
    got = ctx.lattice_bound_frames(orig, diff.copy(), SEAM_BOUNDS, SEAM_SKIP)
    np.testing.assert_array_equal(got, want["frames"])
    for f in (0, 1, 2):                                                      # bound 0, bound 0.5 and the skipped frame
        np.testing.assert_array_equal(got[f], diff[f])
    # device stacks: on the allocation's alignment, and off every wider one
    for off_o, off_d in ((0, 0), (1, 1), (3, 5)):
        for key in [(m, tuple(v)) for m, v in SEAM_CASES[2:4] + SEAM_CASES[7:]] + ["frames"]:
            _, to = _on_device(orig, off_o, torch.uint8)
            whole, td = _on_device(diff, off_d, torch.int16)
            torch.cuda.synchronize()
            if key == "frames":
                ctx.lattice_bound_frames(to, td, SEAM_BOUNDS, SEAM_SKIP)
            else:
                ctx.lattice_bound(to, td, key[0], list(key[1]), SEAM_SKIP)
            ctx.synchronize()                    # (device outputs are stream-ordered, not complete on return)
            np.testing.assert_array_equal(td.cpu().numpy(), want[key], err_msg="device, offsets %d %d, %r" % (off_o, off_d, key))
            assert not whole[:off_d].any().item() and not whole[off_d + diff.size:].any().item()


def test_seam_arguments(ctx, seam_want):
    orig, diff, want = seam_want(21, 30)
    d = diff.copy()
    call = lambda mode, b0, b1, n=len(diff): ctx.lib.tz_lattice_bound(ctx.h, orig.ctypes.data, d.ctypes.data, None, n, 21, 30, mode, b0, b1)  # noqa: E731
    for mode, b0, b1 in ((0, float("nan"), 0.0), (1, -0.01, 0.0), (3, -0.01, 0.0), (2, 2.0, -0.01), (2, 2.0, float("nan")), (4, 2.0, 0.0), (-1, 2.0, 0.0)):
        assert call(mode, b0, b1) == -1, (mode, b0, b1)                      # where tz_error_bound refuses
        np.testing.assert_array_equal(d, diff)
    for mode, b0, b1 in ((0, 0.0, 0.0), (1, 0.0, 0.0), (2, 2.0, 0.0), (3, 0.0, 0.0)):
        assert call(mode, b0, b1) == 0                                       # no tolerance: nothing changes
        np.testing.assert_array_equal(d, diff)
    assert call(0, 2.0, 0.0, 0) == 0 and call(0, 2.0, 0.0, -1) == -1
    np.testing.assert_array_equal(d, diff)
    b = np.array(SEAM_BOUNDS)
    fcall = lambda bounds, n=len(diff): ctx.lib.tz_lattice_bound_frames(ctx.h, orig.ctypes.data, d.ctypes.data, None, n, 21, 30,  # noqa: E731
                                                                      None if bounds is None else bounds.ctypes.data)
    for bad in (float("nan"), -1.0, float("inf")):
        bb = b.copy()
        bb[3] = bad
        assert fcall(bb) == -1
        np.testing.assert_array_equal(d, diff)
        with pytest.raises(Exception, match="frame 3"):
            ctx.lattice_bound_frames(orig, d, bb)
    assert fcall(None) == -1 and fcall(b, -1) == -1 and fcall(b, 0) == 0 and fcall(np.full(len(diff), 0.75)) == 0
    np.testing.assert_array_equal(d, diff)
    # the seams are independent of the context's own settings, and the greedy seam of the lattice setting
    from oracle import coracle
    try:
        ctx.set_frame_bounds([9.0] * 3)
        ctx.set_quantiser(1)
        np.testing.assert_array_equal(ctx.lattice_bound(orig, diff.copy(), "abs", [2.0], SEAM_SKIP), want["abs", (2.0,)])
        np.testing.assert_array_equal(ctx.lattice_bound_frames(orig, diff.copy(), SEAM_BOUNDS, SEAM_SKIP), want["frames"])
        np.testing.assert_array_equal(ctx.error_bound(orig[3:4], diff[3:4].copy(), "abs", [2.0])[0],
                                      coracle.error_bound_frame(orig[3], diff[3], "abs", [2.0]))
    finally:
        _reset(ctx)


def test_setter(ctx):
    assert ctx.get_quantiser() == 0
    for bad in (-1, 2, 7):
        assert ctx.lib.tz_set_quantiser(ctx.h, bad) == -1 and ctx.get_quantiser() == 0
    with pytest.raises(Exception, match="quantiser"):
        ctx.set_quantiser(2)
    assert ctx.lib.tz_set_quantiser(None, 1) == -1 and ctx.lib.tz_get_quantiser(None) == -1
    ctx.set_quantiser("lattice")
    assert ctx.get_quantiser() == 1
    ctx.set_quantiser("greedy")
    assert ctx.get_quantiser() == 0


# ------------------------------------------------------------------------------------------------------- 2. the job
def _scene64():
    from tezip_amd import synth
    return synth.translating_scene(7, 64, 64)            # unpadded, HW % 8 == 0: the fused front applies in every layout


def _scene_padded():
    from tezip_amd import synth
    return synth.translating_scene(7, 61, 90)            # padded to 64 x 96: the unfused kernels


def _blobs64():
    from tezip_amd import synth
    return synth.moving_blobs(7, 64, 64)                 # gray


def _blobs_padded():
    from tezip_amd import synth
    return np.ascontiguousarray(synth.moving_blobs(7, 32, 32)[:, :21, :30])


JOBS = {   # frames, warm_up, window, threshold, payload channels, delta stride
    "scene64_flat": (_scene64, 1, 3, None, 3, 0),
    "scene64_channel": (_scene64, 1, 3, None, 3, 1),
    "blobs64_gray": (_blobs64, 1, 3, None, 1, 0),
    "padded_flat": (_scene_padded, 1, 3, None, 3, 0),
    "padded_channel": (_scene_padded, 1, 3, None, 3, 1),
    "padded_gray": (_blobs_padded, 1, 3, None, 1, 0),
    "padded_flat_dwp": (_scene_padded, 0, None, "auto", 3, 0),
}
BOUNDS = [("abs", [2.0]), ("abs", [6.5]), ("abs", [300.0]), ("rel", [0.02]), ("absrel", [4.0, 0.5]), ("pwrel", [0.05])]
CYCLE = [2.0, 7.5, 0.0, 3.5, 63.5, 0.3]


def _slow_payload(q, channels, stride, entropy):
    """the layout's slow reference on a quantised delta stack -> (payload, table | None)"""
    from oracle import oracle as O
    from tezip_amd import graypayload, sdelta
    if channels == 1:
        return graypayload.payload_from_delta(q, entropy)
    if stride:
        return sdelta.payload_from_delta(q, entropy, 3)
    sd = O.finding_difference_enc(q).reshape(-1)
    if not entropy:
        return sd, None
    y = (O.OFFSET - sd.astype(np.int64)).astype(np.int16)
    table = O.build_table(y)
    return O.remap_enc(y, table), table


def _launches(ctx, call):
    ctx.prof_enable(True)
    ctx.prof_reset()
    out = call()
    n = {k: v[1] for k, v in ctx.prof_get().items()}
    ctx.prof_enable(False)
    return out, n


@pytest.mark.parametrize("job", sorted(JOBS))
def test_encode_under_the_lattice_quantiser(ctx, job):
    from tezip_amd import frametarget, lattice
    make, p, window, thr, channels, stride = JOBS[job]
    frames = make()
    nt, h, w, _ = frames.shape
    fused = h % 8 == 0 and w % 8 == 0
    try:
        key = TT._rollout(ctx, frames, p, window, thr)
        if channels == 3:
            TT._nontrivial(ctx, frames, key)
        skip = np.array(frametarget.fixed_frames(key, p), np.uint8)
        delta = ctx.encode_delta("abs", [0.0]).copy()                  # the job's deltas, unquantised
        turn = iter(CYCLE * nt)
        fbounds = [9.0 if fx else next(turn) for fx in skip]
        ctx.set_payload_channels(channels)
        ctx.set_delta_stride(stride)
        lossless = {e: [np.array(a, copy=True) if a is not None else None for a in ctx.encode("abs", [0.0], e)[:2]] for e in (True, False)}
        greedy = np.array(ctx.encode("abs", [2.0], True)[0], copy=True)
        ctx.set_quantiser(1)
        for mode, value, bounds in [(m, v, None) for m, v in BOUNDS] + [("abs", [99.0], fbounds)]:
            ctx.set_frame_bounds(bounds)
            q = lattice.quantise_stack(frames, delta, mode, value, skip, bounds=bounds)
            lossy = [f for f in range(nt) if (q[f] != delta[f]).any()]
            assert len(lossy) >= 2 and not any(skip[f] for f in lossy), "%s %r bites in several predicted frames" % (mode, value)
            for entropy in (True, False):
                want_p, want_t = _slow_payload(q, channels, stride, entropy)
                (payload, table, _), n = _launches(ctx, lambda: ctx.encode(mode, value, entropy))
                what = "%s %r bounds %r entropy %s" % (mode, value, bounds is not None, entropy)
                np.testing.assert_array_equal(np.asarray(payload).reshape(-1), want_p, err_msg=what)
                if entropy:
                    np.testing.assert_array_equal(table, want_t, err_msg=what)
                else:
                    assert table is None
                # the route: one fused pass over pred / orig where the frames allow it, else delta, k_lattice, spatial delta
                assert (n["delta"], n["spatial_delta_hist"], n["quant_serial_chains"]) == ((1, 0, 0) if fused else (1, 1, 0)), (what, n)
                if channels == 3:    # the delta tap is the quantised stack, and the payload beside it the same payload
                    p2, t2, tap = ctx.encode(mode, value, entropy, want_delta=True)
                    np.testing.assert_array_equal(tap, q, err_msg=what)
                    np.testing.assert_array_equal(np.asarray(p2).reshape(-1), want_p, err_msg=what)
                if entropy and (nt * h * w * channels) % 8 == 0:      # --shuffle: the byte planes of the same payload
                    planes, t3, _ = ctx.encode(mode, value, True, shuffle=True)
                    np.testing.assert_array_equal(ctx.byte_unshuffle(np.asarray(planes).view(np.uint8).reshape(-1)).reshape(-1), want_p)
                    np.testing.assert_array_equal(t3, want_t)
            if channels == 3 and stride == 0:                           # tz_encode_delta (flat layout only, as under greedy)
                np.testing.assert_array_equal(ctx.encode_delta(mode, value), q)
            # a resident payload decodes within the tolerance: tz_encode_quality is the decoder's tail
            _, table, _ = ctx.encode(mode, value, True, payload="resident")
            rec = TT._records(ctx.encode_quality("resident", table))
            if mode == "abs":
                lim = [0 if skip[f] else int(bounds[f] if bounds else min(255.0, value[0])) for f in range(nt)]
                assert all(rec[f, 1] <= lim[f] for f in range(nt)) and rec[:, 0].sum() > 0
        ctx.set_frame_bounds(None)
        assert (np.asarray(ctx.encode("abs", [2.0], True)[0]).reshape(-1) != greedy.reshape(-1)).any()    # not the greedy job's payload
        # tolerances below 1 are the lossless job, byte for byte, on the lossless kernels
        for mode, value, bounds in (("abs", [0.5], None), ("abs", [0.999], None), ("rel", [0.0039], None), ("pwrel", [0.0039], None),
                                    ("absrel", [0.9, 7.0], None), ("abs", [7.0], [0.0, 0.5, 0.999, 0.0, 0.25, 0.75, 0.0])):
            ctx.set_frame_bounds(bounds)
            for entropy in (True, False):
                (payload, table, _), n = _launches(ctx, lambda: ctx.encode(mode, value, entropy))
                np.testing.assert_array_equal(payload, lossless[entropy][0], err_msg="%s %r" % (mode, value))
                if entropy:
                    np.testing.assert_array_equal(table, lossless[entropy][1])
                assert n["quant"] == 0, n
            assert not TT._records(ctx.bound_probe(mode, value)).any()
        ctx.set_frame_bounds(None)
        # the refusals are the greedy quantiser's; the sharded entry points are out of scope
        for mode, value in (("rel", [-0.01]), ("pwrel", [-0.01]), ("absrel", [2.0, -0.01]), ("abs", [float("nan")])):
            with pytest.raises(Exception):
                ctx.encode(mode, value, True)
            with pytest.raises(Exception):
                ctx.bound_probe(mode, value)
        if channels == 3 and stride == 0:
            from tezip_amd import _lib
            hist, edge = np.zeros(_lib.TZ_NBINS, np.uint64), np.zeros(2, np.int16)
            assert ctx.lib.tz_encode_begin(ctx.h, 0, 2.0, 0.0, 1, hist.ctypes.data, edge.ctypes.data) == -6       # TZ_ERR_UNSUPPORTED
            with pytest.raises(Exception, match="lattice"):
                ctx.encode_begin("abs", [2.0])
            assert ctx.lib.tz_encode_finish(ctx.h, 0, 0, None, -1, None) == -6
        # back to the default: today's bytes and today's launches
        ctx.set_quantiser(0)
        again, n = _launches(ctx, lambda: ctx.encode("abs", [2.0], True))
        np.testing.assert_array_equal(again[0], greedy)
    finally:
        _reset(ctx)


# ---------------------------------------------------------------------------------------------------- 3. the probes
@pytest.mark.parametrize("job", ["scene64_flat", "scene64_channel", "padded_gray", "padded_flat_dwp"])
def test_probes_describe_the_lattice_job(ctx, job):
    make, p, window, thr, channels, stride = JOBS[job]
    frames = make()
    try:
        TT._rollout(ctx, frames, p, window, thr)
        ctx.set_payload_channels(channels)
        ctx.set_delta_stride(stride)
        greedy = TT._records(ctx.bound_probe("abs", [6.5]))
        ctx.set_quantiser(1)
        some = 0
        for mode, bound in [("abs", [k / 2]) for k in (0, 1, 2, 5, 13, 64, 510)] + [("rel", [0.02]), ("absrel", [3.0, 0.5]), ("pwrel", [0.1])]:
            got = TT._records(ctx.bound_probe(mode, bound))
            payload, table, _ = ctx.encode(mode, bound, True)
            np.testing.assert_array_equal(got, TT._records(ctx.encode_quality(payload, table)), err_msg="%s %r" % (mode, bound))
            some += int(got[:, 0].sum() > 0)
        assert some >= 7
        assert (TT._records(ctx.bound_probe("abs", [6.5])) != greedy).any()           # (not the greedy job's records)
        for coder in ("huff", "huffr", "huffd"):
            for bound in (0.0, 2.0, 6.5, 255.0):
                for entropy in (True, False):
                    want, _ = TR._real(ctx, coder, bound, entropy)
                    rec = ctx.size_probe("abs", [bound], entropy, coder)
                    assert (int(rec["bytes"]), int(rec["table_len"])) == (want["bytes"], want["table_len"]), (coder, bound, entropy)
        ctx.set_frame_bounds([0.0, 9.0, 2.0, 0.5, 6.5, 3.0, 127.0][:len(frames)])
        got = TT._records(ctx.bound_probe("abs", [0.0]))
        payload, table, _ = ctx.encode("abs", [0.0], True)
        np.testing.assert_array_equal(got, TT._records(ctx.encode_quality(payload, table)))
        want, _ = TR._real(ctx, "huffd", 0.0, True)
        assert int(ctx.size_probe("abs", [0.0], True, "huffd")["bytes"]) == want["bytes"]
    finally:
        _reset(ctx)


def test_a_default_job_after_a_lattice_job_is_the_oracles_greedy_payload(ctx):
    from oracle import coracle
    from tezip_amd import frametarget
    frames = _scene_padded()
    try:
        key = TT._rollout(ctx, frames, 1, 3)
        skip = frametarget.fixed_frames(key, 1)
        delta = ctx.encode_delta("abs", [0.0]).copy()
        ctx.set_quantiser(1)
        _, table, _ = ctx.encode("abs", [2.0], True, payload="resident")
        ctx.set_quantiser(0)
        with pytest.raises(Exception):                     # the change dropped the resident payload
            ctx.encode_quality("resident", table)
        q = delta.copy()
        for f in range(len(frames)):
            if not skip[f]:
                q[f] = coracle.error_bound_frame(frames[f], delta[f], "abs", [2.0])
        for entropy in (True, False):
            payload, table, _ = ctx.encode("abs", [2.0], entropy)
            want_p, want_t = _slow_payload(q, 3, 0, entropy)
            np.testing.assert_array_equal(np.asarray(payload).reshape(-1), want_p)
            if entropy:
                np.testing.assert_array_equal(table, want_t)
    finally:
        _reset(ctx)


# ---------------------------------------------------------------------------------------------------------- 4. CLI
@pytest.fixture(scope="module")
def jobs(tmp_path_factory):
    """{name: (model directory, image directory, names, frames)} on disk once for the CLI tests"""
    from PIL import Image
    from tezip_amd import _lib, weights
    root = tmp_path_factory.mktemp("lattice_cli")
    cfg, wts = TT._model()
    out = {}
    for name, frames in (("scene", _scene_padded()), ("scene64", _scene64()), ("blobs", _blobs_padded())):
        mdir, ddir = str(root / (name + "_model")), root / (name + "_data")
        weights.save_model(mdir, cfg, wts, _lib.pad8(frames.shape[1]), _lib.pad8(frames.shape[2]))
        ddir.mkdir()
        names = ["f_%03d.png" % t for t in range(len(frames))]
        for t, n in enumerate(names):
            Image.fromarray(frames[t]).save(ddir / n)
        out[name] = (mdir, str(ddir), names, frames)
    return out


JOB = ["-p", "1", "-w", "3"]
CLI_CASES = {
    "scene": ("scene", JOB, []),
    "scene64_huffd_channel": ("scene64", JOB, ["--coder", "huffd", "--sdelta", "channel", "--key-coder", "huff"]),
    "blobs_gray_huffr": ("blobs", JOB, ["--gray", "--coder", "huffr"]),
    "scene64_dwp_shuffle": ("scene64", ["-p", "0", "-t", "1.0"], ["--shuffle"]),      # (a threshold no window reaches: one DWP window)
}


@pytest.mark.parametrize("case", sorted(CLI_CASES))
def test_cli_lattice_job_and_its_decode(tmp_path, capsys, jobs, case):
    from tezip_amd import lattice
    job, window, flags = CLI_CASES[case]
    mdir, ddir, names, frames = jobs[job]
    nt = len(frames)
    comp, plain, udir = str(tmp_path / "comp"), str(tmp_path / "plain"), str(tmp_path / "dec")
    code, out = TR._main(["-c", mdir, ddir, comp] + window + ["-m", "abs", "-b", "2", "--quant", "lattice", "--report", "--digests"] + flags, capsys)
    assert code == 0, out
    assert out.splitlines().count(lattice.STDOUT_LINE) == 1 and lattice.STDOUT_LINE == "quant: lattice (TZ-QL1)"
    assert json.load(open(os.path.join(comp, "tezip_amd.json")))["quant"] == "lattice"
    quality = json.load(open(os.path.join(comp, "quality.json")))
    assert 0 < quality["max_abs_err"] <= 2 and "max_abs_err: %d" % quality["max_abs_err"] in out.splitlines()
    code, out = TR._main(["-u", mdir, comp, udir, "--verify", "require"], capsys)            # no flag for the new content
    assert code == 0 and "verified: %d frames" % nt in out, out
    dec = TR._images(udir, names).astype(np.int64)
    err = np.abs(dec - frames).reshape(nt, -1).max(axis=1)
    assert err.max() <= 2 and err.max() == quality["max_abs_err"] and err.tolist() == [fr["max_abs_err"] for fr in quality["per_frame"]]
    # --quant greedy is the job without the flag: every file, and no line about a quantiser
    code, out_g = TR._main(["-c", mdir, ddir, str(tmp_path / "greedy")] + window + ["-m", "abs", "-b", "2", "--quant", "greedy"] + flags, capsys)
    code2, out_p = TR._main(["-c", mdir, ddir, plain] + window + ["-m", "abs", "-b", "2"] + flags, capsys)
    assert code == 0 and code2 == 0 and "quant:" not in out_g and "quant:" not in out_p
    assert sorted(os.listdir(plain)) == sorted(os.listdir(str(tmp_path / "greedy")))
    for name in os.listdir(plain):
        assert open(os.path.join(plain, name), "rb").read() == open(os.path.join(str(tmp_path / "greedy"), name), "rb").read(), name
    assert "quant" not in json.load(open(os.path.join(plain, "tezip_amd.json")))
    assert open(os.path.join(plain, "entropy.dat"), "rb").read() != open(os.path.join(comp, "entropy.dat"), "rb").read()


@pytest.mark.parametrize("case", ["scene", "blobs_gray_huffr"])
def test_cli_target_psnr_under_the_lattice_is_the_abs_job_it_finds(tmp_path, capsys, jobs, case):
    job, window, flags = CLI_CASES[case]
    mdir, ddir, names, frames = jobs[job]
    flags = flags + ["--quant", "lattice", "--report", "--digests"]
    found, plain = str(tmp_path / "comp_t"), str(tmp_path / "comp")
    code, out = TR._main(["-c", mdir, ddir, found] + window + ["--target-psnr", "40"] + flags, capsys)
    assert code == 0 and "quant: lattice (TZ-QL1)" in out.splitlines(), out
    doc = json.load(open(os.path.join(found, "bound_search.json")))
    bound = doc["result"]["bound"]
    assert doc["quant"] == "lattice" and 0 < bound < 255 and doc["probes"] <= 9
    quality = json.load(open(os.path.join(found, "quality.json")))
    assert quality["psnr_db"] >= 40.0 and quality["bound"] == [bound] and not quality["lossless"]
    code, out = TR._main(["-c", mdir, ddir, plain] + window + ["-m", "abs", "-b", repr(bound)] + flags, capsys)
    assert code == 0, out
    assert sorted(os.listdir(found)) == sorted(os.listdir(plain) + ["bound_search.json"])
    for name in os.listdir(plain):
        assert open(os.path.join(found, name), "rb").read() == open(os.path.join(plain, name), "rb").read(), name


def test_cli_per_frame_and_ratio_searches_run_under_the_lattice(tmp_path, capsys, jobs):
    mdir, ddir, names, frames = jobs["scene"]
    nt = len(frames)
    a, b, udir = str(tmp_path / "a"), str(tmp_path / "b"), str(tmp_path / "dec")
    code, out = TR._main(["-c", mdir, ddir, a] + JOB + ["--target-psnr", "38", "--per-frame", "--quant", "lattice", "--report"], capsys)
    assert code == 0, out
    doc = json.load(open(os.path.join(a, "bound_search.json")))
    assert doc["quant"] == "lattice" and len(doc["frame_bounds"]) == nt
    quality = json.load(open(os.path.join(a, "quality.json")))
    assert all(fr["psnr_db"] is None or fr["psnr_db"] >= 38.0 for fr in quality["per_frame"]) and not quality["lossless"]
    code, out = TR._main(["-u", mdir, a, udir], capsys)
    assert code == 0, out
    dec = TR._images(udir, names).astype(np.int64)
    assert ((dec - frames) ** 2).reshape(nt, -1).sum(axis=1).tolist() == [fr["sse"] for fr in quality["per_frame"]]
    sizes = {}
    for bound in ("0", "255"):
        code, out = TR._main(["-c", mdir, ddir, str(tmp_path / ("p" + bound))] + JOB + ["-m", "abs", "-b", bound, "--coder", "huffd", "--quant", "lattice"], capsys)
        assert code == 0, out
        sizes[bound] = sum(os.path.getsize(os.path.join(str(tmp_path / ("p" + bound)), n)) for n in ("filename.txt", "key_frame.dat", "entropy.dat"))
    R = frames.size / ((sizes["0"] + sizes["255"]) / 2.0)
    code, out = TR._main(["-c", mdir, ddir, b] + JOB + ["--target-ratio", repr(R), "--coder", "huffd", "--quant", "lattice"], capsys)
    assert code == 0, out
    doc = json.load(open(os.path.join(b, "bound_search.json")))
    assert doc["quant"] == "lattice"
    from tezip_amd import ratetarget
    assert TR._total(b) <= ratetarget.budget(frames.size, R) and 0 < doc["result"]["bound"] < 255
