"""One abs bound per frame on a MI355X (tz_set_frame_bounds, tz_error_bound_frames; definition TZ-TPSNR-F1,
tezip_amd/frametarget.py): the seam against the uniform quantiser and the C oracle frame by frame, the four entry points under
frame bounds against the stitching of uniform jobs and the unfused chain, the refusals, the per-frame search against the
same search over uniform probes, and the command line end to end.  Integers and bytes throughout."""
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
    c.set_frame_bounds(None)
    c.close()


# ------------------------------------------------------------------------------------------------------ 1. the seam
SEAM_BOUNDS = [0.0, 0.3, 0.5, 2.0, 5.0, 7.5, 63.5, 255.0]
SEAM_SKIP = np.array([0, 0, 0, 0, 1, 0, 0, 0], np.uint8)     # (frame 4 is skipped whatever its bound says)


def _seam_stacks(h, w):
    """int16 deltas in [-255, 255]: slow triangle ramps without a jump (what keeps two greedy chains out of step and sends a
    chain to k_q_serial where it spans tiles), the same with jitter, and plain jitter"""
    n = h * w
    i = np.arange(n)
    rng = np.random.default_rng(h * 1000 + w)
    frames = []
    for f, (period, step) in enumerate(((10, 1), (7, 1), (23, 2), (3, 1), (64, 1), (50, 3), (5, 1), (9, 2))):
        tri = np.abs(((i // period) * step % 400) - 200) - 100
        jit = rng.integers(-4, 5, n)
        wide = rng.integers(-255, 256, n)
        frames.append(np.stack([tri, np.clip(2 * tri + jit, -255, 255), wide if f % 2 else -tri], axis=-1).reshape(h, w, 3))
    diff = np.stack(frames).astype(np.int16)
    orig = rng.integers(0, 256, diff.shape).astype(np.uint8)
    return orig, diff


@pytest.fixture(scope="module")
def seam_want():
    """(h, w) -> orig, diff and what every frame must become: the C oracle's abs quantiser at the frame's own bound"""
    from oracle import coracle
    memo = {}

    def get(h, w):
        if (h, w) not in memo:
            orig, diff = _seam_stacks(h, w)
            want = diff.copy()
            for f, b in enumerate(SEAM_BOUNDS):
                if b != 0.0 and not SEAM_SKIP[f]:
                    want[f] = coracle.error_bound_frame(orig[f], diff[f], "abs", [b])
            assert sum((want[f] != diff[f]).any() for f in range(len(diff))) == 5     # 2, 7.5, 63.5, 255 and 0.5 change their frames
            memo[h, w] = (orig, diff, want)
        return memo[h, w]
    return get


SEAM_SIZES = [(21, 30), (64, 64), (72, 88)]   # HW % 4 != 0 (ungrouped staging); exactly one 4096-element tile; two tiles


@pytest.mark.parametrize("h,w", SEAM_SIZES)
def test_seam_is_the_uniform_quantiser_frame_by_frame(ctx, seam_want, h, w):
    import torch
    orig, diff, want = seam_want(h, w)
    ctx.prof_enable(True)
    ctx.prof_reset()
    got = ctx.error_bound_frames(orig, diff.copy(), SEAM_BOUNDS, SEAM_SKIP)
    print("%dx%d: %d chains took k_q_serial" % (h, w, ctx.prof_get()["quant_serial_chains"][1]))
    ctx.prof_enable(False)
    for f, b in enumerate(SEAM_BOUNDS):
        np.testing.assert_array_equal(got[f], want[f], err_msg="host, frame %d at abs %g" % (f, b))
        if not SEAM_SKIP[f]:    # the uniform call on that frame alone
            np.testing.assert_array_equal(ctx.error_bound(orig[f:f + 1], diff[f:f + 1].copy(), "abs", [b])[0], got[f], err_msg="frame %d" % f)
    np.testing.assert_array_equal(got[4], diff[4])                       # the skipped frame is untouched
    np.testing.assert_array_equal(got[0], diff[0])                       # and so is the frame at bound 0
    # device stacks: on the allocation's alignment, and off every wider one (the ungrouped staging at any frame size)
    n = diff.size
    for off_o, off_d in ((0, 0), (1, 1)):
        to = torch.zeros(n + 16, dtype=torch.uint8, device="cuda")
        td = torch.zeros(n + 16, dtype=torch.int16, device="cuda")
        to[off_o: off_o + n] = torch.from_numpy(orig.reshape(-1)).cuda()
        td[off_d: off_d + n] = torch.from_numpy(diff.reshape(-1)).cuda()
        torch.cuda.synchronize()
        ctx.error_bound_frames(to[off_o: off_o + n].view(orig.shape), td[off_d: off_d + n].view(diff.shape), SEAM_BOUNDS, SEAM_SKIP)
        ctx.synchronize()                # (device outputs are stream-ordered, not complete on return)
        np.testing.assert_array_equal(td[off_d: off_d + n].cpu().numpy().reshape(diff.shape), want, err_msg="device, offsets %d %d" % (off_o, off_d))
        assert not td[:off_d].any().item() and not td[off_d + n:].any().item()


def test_seam_arguments(ctx, seam_want):
    from oracle import coracle
    orig, diff, want = seam_want(21, 30)
    d = diff.copy()
    b = np.array(SEAM_BOUNDS)
    call = lambda bounds, n=len(diff): ctx.lib.tz_error_bound_frames(ctx.h, orig.ctypes.data, d.ctypes.data, None, n, 21, 30,  # noqa: E731
                                                                     None if bounds is None else bounds.ctypes.data)
    for bad in (float("nan"), -1.0, float("inf")):
        bb = b.copy()
        bb[3] = bad
        assert call(bb) == -1
        np.testing.assert_array_equal(d, diff)                           # nothing was touched
        with pytest.raises(Exception, match="frame 3"):
            ctx.error_bound_frames(orig, d, bb)
    assert call(None) == -1 and call(b, -1) == -1
    assert call(b, 0) == 0
    np.testing.assert_array_equal(d, diff)
    assert call(np.zeros(len(diff))) == 0                                # every bound 0: nothing runs
    np.testing.assert_array_equal(d, diff)
    ctx.set_frame_bounds([9.0] * 3)                                      # the context's own setting does not reach the seams
    try:
        np.testing.assert_array_equal(ctx.error_bound_frames(orig, diff.copy(), SEAM_BOUNDS, SEAM_SKIP), want)
        np.testing.assert_array_equal(ctx.error_bound(orig[3:4], diff[3:4].copy(), "abs", [2.0])[0], want[3])
        np.testing.assert_array_equal(ctx.error_bound(orig[3:4], diff[3:4].copy(), "rel", [0.01])[0],
                                      coracle.error_bound_frame(orig[3], diff[3], "rel", [0.01]))
    finally:
        ctx.set_frame_bounds(None)


# ------------------------------------------------------------------------------------------------------- 2. the job
def _scene64():
    from tezip_amd import synth
    return synth.translating_scene(8, 64, 80)            # unpadded, HW % 8 == 0: the fused fronts apply


def _scene_padded():
    from tezip_amd import synth
    return synth.translating_scene(8, 61, 90)            # padded to 64 x 96: the unfused kernels


JOBS = {   # frames, warm_up, window, threshold, payload channels, delta stride
    "scene64_p0_w4": (_scene64, 0, 4, None, 3, 0),
    "scene64_p1_w4": (_scene64, 1, 4, None, 3, 0),
    "padded_p0_w4": (_scene_padded, 0, 4, None, 3, 0),
    "padded_p0_dwp": (TT._scene, 0, None, "auto", 3, 0),
    "blobs_one_channel": TT.PROBE_JOBS["blobs_one_channel"],
    "scene_channel_stride": TT.PROBE_JOBS["scene_channel_stride"],
    "scene64_channel_stride": (_scene64, 0, 4, None, 3, 1),
}
CYCLE = [2.0, 7.5, 0.0, 3.5, 63.5, 0.3, 12.0, 0.5]


def _job_bounds(key, p):
    """the predicted frames take CYCLE's bounds in turn; the frames the encoder never quantises an entry that must not matter"""
    from tezip_amd import frametarget
    turn = iter(CYCLE * len(key))
    return [9.0 if fx else next(turn) for fx in frametarget.fixed_frames(key, p)]


def _stitched(ctx, bounds):
    """the delta stack of the job, frame f from the uniform tz_encode_delta at bounds[f] (flat three-channel layout)"""
    per_bound = {b: ctx.encode_delta("abs", [b]).copy() for b in sorted(set(bounds))}
    return np.stack([per_bound[b][f] for f, b in enumerate(bounds)])


def _unfused(sd, stack, channels, stride, entropy):
    """tz_encode_delta's stack, then the layout's spatial delta, table and remap (the numpy statement: tezip_amd/sdelta.py)"""
    x = stack[..., 0] if channels == 1 else stack
    return sd.payload_from_delta(np.ascontiguousarray(x), entropy, 3 if stride else 1)


@pytest.mark.parametrize("job", sorted(JOBS))
def test_entry_points_under_frame_bounds(ctx, job):
    from tezip_amd import sdelta as sd
    make, p, window, thr, channels, stride = JOBS[job]
    frames = make()
    nt = len(frames)
    try:
        key = TT._rollout(ctx, frames, p, window, thr)
        TT._nontrivial(ctx, frames, key)
        bounds = _job_bounds(key, p)
        # uniform jobs first, nothing set: the stitching, the uniform probes and what a plain encode gives
        assert ctx.get_frame_bounds() == 0
        stitched = _stitched(ctx, bounds)
        lossless = ctx.encode_delta("abs", [0.0]).copy()
        lossy = [f for f in range(nt) if (stitched[f] != lossless[f]).any()]
        assert len(lossy) >= 2 and all(bounds[f] >= 0.5 for f in lossy), "the bounds of this job bite in several frames"
        ctx.set_payload_channels(channels)
        ctx.set_delta_stride(stride)
        uniform_probe = {b: TT._records(ctx.bound_probe("abs", [b])) for b in sorted(set(bounds))}
        plain = {e: [np.array(a, copy=True) if a is not None else None for a in ctx.encode("abs", [2.0], e)[:2]] for e in (True, False)}
        ctx.prof_enable(True)
        ctx.prof_reset()
        ctx.encode("abs", [2.0], True)
        launches_before = {k: v[1] for k, v in ctx.prof_get().items()}
        ctx.prof_enable(False)

        ctx.set_frame_bounds(bounds)
        assert ctx.get_frame_bounds() == nt
        # tz_encode_delta (flat layout only, as without bounds): the stitching, bit for bit
        ctx.set_payload_channels(3)
        ctx.set_delta_stride(0)
        np.testing.assert_array_equal(ctx.encode_delta("abs", [99.0]), stitched)         # (b0 is not read)
        ctx.set_payload_channels(channels)
        ctx.set_delta_stride(stride)
        # tz_encode: payload and table of the unfused chain on that stack
        for entropy in (True, False):
            payload, table, _ = ctx.encode("abs", [0.0], entropy)
            want_p, want_t = _unfused(sd, stitched, channels, stride, entropy)
            np.testing.assert_array_equal(np.asarray(payload).reshape(-1), want_p, err_msg="payload, entropy %s" % entropy)
            if entropy:
                np.testing.assert_array_equal(table, want_t)
            else:
                assert table is None
            if channels == 3:    # the delta tap is the same stack, and the payload beside it the same payload
                p2, t2, tap = ctx.encode("abs", [0.0], entropy, want_delta=True)
                np.testing.assert_array_equal(tap, stitched)
                np.testing.assert_array_equal(np.asarray(p2).reshape(-1), want_p)
        ctx.prof_enable(True)
        ctx.prof_reset()
        payload, table, _ = ctx.encode("abs", [0.0], True)
        launches = {k: v[1] for k, v in ctx.prof_get().items()}
        ctx.prof_enable(False)
        # the route: the fused lossy front where the uniform job takes it (no delta stack is made), else the unfused kernels
        fused = channels == 3 and stride == 0 and frames.shape[1] % 8 == 0 and frames.shape[2] % 8 == 0
        assert (launches["delta"] == 0) == fused == (launches_before["delta"] == 0), (launches, launches_before)
        # tz_bound_probe: record f is the uniform probe's at bounds[f]; it is what the stored payload decodes to
        got = TT._records(ctx.bound_probe("abs", [0.0]))
        for f, b in enumerate(bounds):
            np.testing.assert_array_equal(got[f], uniform_probe[b][f], err_msg="frame %d at abs %g" % (f, b))
        quality = TT._records(ctx.encode_quality(payload, table))
        np.testing.assert_array_equal(got, quality)
        assert all(quality[f, 1] <= int(np.ceil(bounds[f])) for f in range(nt)) and quality[:, 0].sum() > 0
        # tz_encode_ssim and tz_encode_digests work on the stored payload
        assert len(ctx.encode_ssim(payload, table)) == nt
        dig = ctx.encode_digests(payload, table)
        exact = [f for f in range(nt) if quality[f, 0] == 0]
        assert all(dig[0][f] == dig[1][f] for f in exact) and any(dig[0][f] != dig[1][f] for f in range(nt))
        # tz_size_probe: the size of the stream tz_encode plus the coder then write
        for entropy in (True, False):
            want, _ = TR._real(ctx, "huffd", 0.0, entropy)
            rec = ctx.size_probe("abs", [0.0], entropy, "huffd")
            assert (int(rec["bytes"]), int(rec["dist"]), int(rec["table_len"])) == (want["bytes"], want["dist"], want["table_len"])
        # --shuffle: the byte planes of the same payload
        if (nt * frames.shape[1] * frames.shape[2] * channels) % 8 == 0:
            planes, t3, _ = ctx.encode("abs", [0.0], True, shuffle=True)
            np.testing.assert_array_equal(ctx.byte_unshuffle(np.asarray(planes).view(np.uint8).reshape(-1)).reshape(-1), np.asarray(payload).reshape(-1))
        # cleared: a uniform encode gives the bytes and makes the launches it made before
        ctx.set_frame_bounds(None)
        assert ctx.get_frame_bounds() == 0
        for e in (True, False):
            again = ctx.encode("abs", [2.0], e)
            np.testing.assert_array_equal(again[0], plain[e][0])
            if e:
                np.testing.assert_array_equal(again[1], plain[e][1])
        ctx.prof_enable(True)
        ctx.prof_reset()
        ctx.encode("abs", [2.0], True)
        assert {k: v[1] for k, v in ctx.prof_get().items()} == launches_before
        ctx.prof_enable(False)
    finally:
        ctx.prof_enable(False)
        ctx.set_frame_bounds(None)
        ctx.set_payload_channels(3)
        ctx.set_delta_stride(0)


def test_lossless_and_identity_bounds_are_the_lossless_job(ctx):
    frames = _scene64()
    TT._rollout(ctx, frames, 0, 4)
    want = [np.array(a, copy=True) for a in ctx.encode("abs", [0.0], True)[:2]]
    try:
        for bounds in ([0.0] * 8, [0.0, 0.3, 0.499, 0.0, 0.25, 0.1, 0.0, 0.499]):
            ctx.set_frame_bounds(bounds)
            payload, table, _ = ctx.encode("abs", [7.0], True)
            np.testing.assert_array_equal(payload, want[0])
            np.testing.assert_array_equal(table, want[1])
            assert not TT._records(ctx.bound_probe("abs", [7.0])).any()
    finally:
        ctx.set_frame_bounds(None)


# ------------------------------------------------------------------------------------------------- 3. the refusals
def test_refusals_while_bounds_are_set():
    from tezip_amd import _lib
    c = _lib.Context(0)
    try:
        frames = _scene64()
        nt = len(frames)
        key = TT._rollout(c, frames, 0, 4)
        out = np.zeros(nt, _lib.QUALITY_DTYPE)
        stack = np.zeros(frames.shape, np.int16)
        good = np.array(_job_bounds(key, 0))
        assert c.lib.tz_set_frame_bounds(c.h, good.ctypes.data, nt) == 0 and c.get_frame_bounds() == nt
        want = c.encode_delta("abs", [0.0]).copy()
        for bad in (float("nan"), -1.0, float("inf")):            # refused, and the previous setting survives
            b = good.copy()
            b[5] = bad
            assert c.lib.tz_set_frame_bounds(c.h, b.ctypes.data, nt) == -1
            assert c.get_frame_bounds() == nt
            np.testing.assert_array_equal(c.encode_delta("abs", [0.0]), want)
        assert c.lib.tz_set_frame_bounds(c.h, good.ctypes.data, -1) == -1 and c.get_frame_bounds() == nt
        with pytest.raises(Exception, match="frame 5"):
            c.set_frame_bounds([1.0] * 5 + [-2.0])
        for mode in (1, 2, 3):                                       # rel, absrel, pwrel
            assert c.lib.tz_encode_delta(c.h, mode, 0.01, 0.01, stack.ctypes.data) == -1
            assert c.lib.tz_bound_probe(c.h, mode, 0.01, 0.01, out.ctypes.data) == -1
        with pytest.raises(Exception, match="abs"):
            c.encode("rel", [0.01], True)
        with pytest.raises(Exception, match="abs"):
            c.size_probe("rel", [0.01], True, "huffd")
        hist, edge = np.zeros(_lib.TZ_NBINS, np.uint64), np.zeros(2, np.int16)
        assert c.lib.tz_encode_begin(c.h, 0, 2.0, 0.0, 1, hist.ctypes.data, edge.ctypes.data) == -6       # TZ_ERR_UNSUPPORTED
        with pytest.raises(Exception, match="per-frame"):
            c.encode_begin("abs", [2.0])
        c.set_frame_bounds(good[:-1])                                # n != nt
        assert c.lib.tz_encode_delta(c.h, 0, 2.0, 0.0, stack.ctypes.data) == -1
        assert c.lib.tz_bound_probe(c.h, 0, 2.0, 0.0, out.ctypes.data) == -1
        with pytest.raises(Exception, match="%d frames" % (nt - 1)):
            c.encode("abs", [2.0], True)
        with pytest.raises(Exception, match="%d frames" % (nt - 1)):
            c.size_probe("abs", [2.0], True, "huffd")
        c.set_frame_bounds(good)                                     # a refused call leaves the context usable
        np.testing.assert_array_equal(c.encode_delta("abs", [0.0]), want)
        assert c.lib.tz_set_frame_bounds(c.h, None, 0) == 0 and c.get_frame_bounds() == 0
        assert c.lib.tz_encode_begin(c.h, 0, 2.0, 0.0, 1, hist.ctypes.data, edge.ctypes.data) == 0
        assert c.lib.tz_get_frame_bounds(None) == -1 and c.lib.tz_set_frame_bounds(None, None, 0) == -1
    finally:
        c.close()


# --------------------------------------------------------------------------------------------------- 4. the search
@pytest.mark.parametrize("job", ["scene64_p0_w4", "padded_p0_w4", "blobs_one_channel"])
def test_search_on_the_device_equals_the_search_over_uniform_probes(ctx, job):
    from tezip_amd import frametarget as ft
    from tezip_amd import target
    make, p, window, thr, channels, stride = JOBS[job]
    frames = make()
    nt = len(frames)
    try:
        ctx.set_payload_channels(channels)
        key = TT._rollout(ctx, frames, p, window, thr)
        fixed = ft.fixed_frames(key, p)
        memo = {}

        def uniform(cand):        # frame f of the uniform job -m abs -b k/2
            ctx.set_frame_bounds(None)
            for k in set(cand):
                if k not in memo:
                    memo[k] = ctx.bound_probe("abs", [k / 2])["sse"].astype(np.int64)
            return [int(memo[k][f]) for f, k in enumerate(cand)]

        def device(cand):
            ctx.set_frame_bounds([k / 2 for k in cand])
            return ctx.bound_probe("abs", [0.0])["sse"]

        n = frames.shape[1] * frames.shape[2] * 3
        searched_some = False
        for T in (30, 35, 40):
            limit = target.sse_limit(T, n)
            got = ft.search(device, limit, fixed)
            want = ft.search(uniform, limit, fixed)
            assert got == want and len(got[2]) <= 9
            ks, sse, trace = got
            print(job, "T=%d" % T, "k", ks)
            at_k, above = device(ks), device([0 if fx else min(k + 1, 510) for k, fx in zip(ks, fixed)])     # two more probes
            for f in range(nt):
                if fixed[f]:
                    assert ks[f] == 0 and at_k[f] == 0
                    continue
                assert at_k[f] == sse[f] <= limit and (ks[f] == 510 or above[f] > limit)
                searched_some = searched_some or 1 <= ks[f] <= 509
        assert searched_some, "no target of these met a frame between lossless and abs 255: the case shows nothing"
    finally:
        ctx.set_frame_bounds(None)
        ctx.set_payload_channels(3)


# ---------------------------------------------------------------------------------------------------------- 5. CLI
@pytest.fixture(scope="module")
def jobs(tmp_path_factory):
    """{name: (model directory, image directory, names, frames)} on disk once for the CLI tests"""
    from PIL import Image
    from tezip_amd import _lib, synth, weights
    root = tmp_path_factory.mktemp("frame_bounds_cli")
    cfg, wts = TT._model()
    out = {}
    for name, frames in (("scene", _scene_padded()), ("blobs", np.ascontiguousarray(synth.moving_blobs(8, 32, 32)[:, :21, :30]))):
        mdir, ddir = str(root / (name + "_model")), root / (name + "_data")
        weights.save_model(mdir, cfg, wts, _lib.pad8(frames.shape[1]), _lib.pad8(frames.shape[2]))
        ddir.mkdir()
        names = ["f_%03d.png" % t for t in range(len(frames))]
        for t, n in enumerate(names):
            Image.fromarray(frames[t]).save(ddir / n)
        out[name] = (mdir, str(ddir), names, frames)
    return out


JOB = ["-p", "0", "-w", "4"]
CLI_CASES = {
    "scene": ("scene", []),
    "scene_huffd_channel": ("scene", ["--coder", "huffd", "--sdelta", "channel"]),
    "blobs_gray": ("blobs", ["--gray"]),
}


@pytest.mark.parametrize("case", sorted(CLI_CASES))
def test_cli_per_frame_target_and_its_replay(tmp_path, capsys, jobs, case):
    from tezip_amd import frametarget as ft
    from tezip_amd import target
    job, flags = CLI_CASES[case]
    mdir, ddir, names, frames = jobs[job]
    nt = len(frames)
    flags = flags + ["--report", "--digests"]
    found, replay, udir = str(tmp_path / "comp_t"), str(tmp_path / "comp_r"), str(tmp_path / "dec")
    code, out = TR._main(["-c", mdir, ddir, found] + JOB + ["--target-psnr", "35", "--per-frame"] + flags, capsys)
    assert code == 0, out
    doc = json.load(open(os.path.join(found, "bound_search.json")))
    assert [ln for ln in out.splitlines() if ln.startswith("target: ")] == [ft.stdout_line(doc)] and "abs" in out.splitlines()
    n = frames.shape[1] * frames.shape[2] * 3
    limit = target.sse_limit(35, n)
    fixed = [f % 4 == 0 for f in range(nt)]
    assert (doc["definition"], doc["target_psnr_db"], doc["frame_samples"], doc["sse_limit"]) == ("TZ-TPSNR-F1", 35.0, n, limit)
    assert [fr["fixed"] for fr in doc["frames"]] == fixed and [fr["name"] for fr in doc["frames"]] == names
    assert doc["probes"] == len(doc["trace"]) <= 9 and doc["frame_bounds"] == [0.0 if fx else fr["k"] / 2 for fx, fr in zip(fixed, doc["frames"])]
    assert any(1 <= fr["k"] <= 509 for fr in doc["frames"] if not fr["fixed"])
    quality = json.load(open(os.path.join(found, "quality.json")))
    assert quality["mode"] == "abs" and quality["bound"] == [] and quality["frame_bounds"] == doc["frame_bounds"]
    assert [fr["sse"] for fr in quality["per_frame"]] == [fr["sse"] for fr in doc["frames"]]
    assert all(fr["max_abs_err"] <= int(np.ceil(b)) for fr, b in zip(quality["per_frame"], doc["frame_bounds"]))
    code, out = TR._main(["-u", mdir, found, udir, "--verify", "require"], capsys)      # no flag for the new content
    assert code == 0 and "verified: %d frames" % nt in out, out
    dec = TR._images(udir, names).astype(np.int64)
    sse = ((dec - frames) ** 2).reshape(nt, -1).sum(axis=1)
    print(case, "k", [fr["k"] for fr in doc["frames"]], "sse", sse.tolist(), "limit", limit)
    assert sse.tolist() == [fr["sse"] for fr in doc["frames"]]
    for f in range(nt):
        if fixed[f]:
            assert sse[f] == 0
        else:     # the floor, from the images themselves
            assert sse[f] == 0 or 10.0 * np.log10(n * 65025.0 / sse[f]) >= 35.0
    # the search's file replays as explicit bounds: every other file byte for byte
    code, out = TR._main(["-c", mdir, ddir, replay] + JOB + ["-m", "abs", "--frame-bounds", os.path.join(found, "bound_search.json")] + flags, capsys)
    assert code == 0, out
    assert ft.explicit_line(doc["frame_bounds"]) in out.splitlines() and "abs" in out.splitlines()
    assert sorted(os.listdir(found)) == sorted(os.listdir(replay) + ["bound_search.json"])
    for name in os.listdir(replay):
        assert open(os.path.join(found, name), "rb").read() == open(os.path.join(replay, name), "rb").read(), name
    sidecar = json.load(open(os.path.join(found, "tezip_amd.json")))
    assert "frame_bounds" not in json.dumps(sidecar)


def test_cli_explicit_zero_bounds_keep_those_frames_lossless(tmp_path, capsys, jobs):
    mdir, ddir, names, frames = jobs["scene"]
    nt = len(frames)
    bounds = [8.0] * nt
    bounds[2] = bounds[3] = 0.0
    path = str(tmp_path / "bounds.json")
    json.dump(bounds, open(path, "w"))
    comp, udir = str(tmp_path / "comp"), str(tmp_path / "dec")
    code, out = TR._main(["-c", mdir, ddir, comp] + JOB + ["-m", "abs", "--frame-bounds", path, "--shuffle"], capsys)
    assert code == 0, out
    assert "frame bounds: %d frames, abs 0..8" % nt in out.splitlines()
    assert sorted(os.listdir(comp)) == ["entropy.dat", "filename.txt", "key_frame.dat", "tezip_amd.json"]
    code, out = TR._main(["-u", mdir, comp, udir, "--frames", "1:6"], capsys)             # a streamed range
    assert code == 0, out
    dec = TR._images(udir, names[1:6]).astype(np.int64)
    err = np.abs(dec - frames[1:6]).reshape(5, -1).max(axis=1)
    assert err[1] == 0 and err[2] == 0 and err[3] == 0                   # frames 2, 3 restored, 4 is a key frame
    assert 0 < err[0] <= 8 and 0 < err[4] <= 8                           # frames 1 and 5 are the lossy job's
