"""One abs bound per pixel on a MI355X (tz_set_bound_map and its seams; definition TZ-BM1, tezip_amd/boundmap.py): the greedy
seam against the C oracle's pwrel walk with the map in place of the originals, the lattice seam against the numpy statement,
tz_encode under a map against the unfused chain in every layout and under both quantisers, the decoded frames and the check
kernel, the probes, the refusals, and the command line end to end.  Integers and bytes throughout."""
import json
import os

import numpy as np
import pytest

import test_gpu_frame_bounds as TF
import test_gpu_ratetarget as TR
import test_gpu_sdauto as SA
import test_gpu_target as TT

pytestmark = pytest.mark.gpu

SIZES = [(21, 30), (64, 64), (72, 88)]   # HW % 4 != 0 (ungrouped staging); exactly one 4096-element tile; two tiles, a run across the stitch
SKIP = np.array([0, 0, 0, 0, 1, 0, 0, 0], np.uint8)
MAPS = ("uniform2", "roi", "random", "wide")


def make_map(name, h, w):
    if name == "uniform2":
        return np.full((h, w), 2, np.uint8)
    if name == "roi":       # a rectangle of zeros in a field of 6: its edges sit off every 4-pixel group and 64-element chunk
        m = np.full((h, w), 6, np.uint8)
        m[5:18, 3:23] = 0
        return m
    if name == "random":
        return np.random.default_rng(h * 100 + w).integers(0, 9, (h, w)).astype(np.uint8)
    m = np.full((h, w), 255, np.uint8)   # "wide": a field of 255 with a column of zeros
    m[:, w // 3] = 0
    return m


@pytest.fixture(scope="module")
def ctx():
    from tezip_amd import _lib
    c = _lib.Context(0)
    yield c
    c.set_bound_map(None)
    c.close()


@pytest.fixture(scope="module")
def seam_want():
    """(h, w, map) -> diff, M and what every frame must become: the C oracle's pwrel walk at b0 = 1 over the map"""
    from oracle import coracle
    memo = {}

    def get(h, w, name):
        if (h, w, name) not in memo:
            _, diff = TF._seam_stacks(h, w)
            M = make_map(name, h, w)
            T3 = np.ascontiguousarray(np.repeat(M[..., None], 3, axis=-1))
            want = diff.copy()
            for f in range(len(diff)):
                if not SKIP[f]:
                    want[f] = coracle.error_bound_frame(T3, diff[f], "pwrel", [1.0])
            want.setflags(write=False)
            memo[h, w, name] = (diff, M, want)
        return memo[h, w, name]
    return get


# --------------------------------------------------------------------------------------------------- 1. the greedy seam
@pytest.mark.parametrize("h,w", SIZES)
def test_greedy_seam_is_the_oracles_walk_over_the_map(ctx, seam_want, h, w):
    import torch
    shape = (8, h, w)
    for name in MAPS:
        diff, M, want = seam_want(h, w, name)
        ctx.prof_enable(True)
        ctx.prof_reset()
        got = ctx.error_bound_map(diff.copy(), M, shape, SKIP)
        print("%dx%d %s: %d chains took k_q_serial" % (h, w, name, ctx.prof_get()["quant_serial_chains"][1]))
        ctx.prof_enable(False)
        for f in range(8):
            np.testing.assert_array_equal(got[f], want[f], err_msg="host, %s frame %d" % (name, f))
        np.testing.assert_array_equal(got[4], diff[4])                        # the skipped frame is untouched
        assert (got != diff).any()
        if name == "uniform2":    # the uniform map is abs 2 (orig is not read by abs)
            np.testing.assert_array_equal(got, ctx.error_bound(np.zeros(diff.shape, np.uint8), diff.copy(), "abs", [2.0], SKIP))
        n = diff.size
        for off in (0, 1):        # device buffers: on the allocation's alignment, and one element off every wider one
            td = torch.zeros(n + 16, dtype=torch.int16, device="cuda")
            tm = torch.zeros(h * w + 16, dtype=torch.uint8, device="cuda")
            td[off: off + n] = torch.from_numpy(diff.reshape(-1)).cuda()
            tm[off: off + h * w] = torch.from_numpy(M.reshape(-1)).cuda()
            torch.cuda.synchronize()
            ctx.error_bound_map(td[off: off + n], tm[off: off + h * w], shape, SKIP)
            ctx.synchronize()     # (device outputs are stream-ordered, not complete on return)
            np.testing.assert_array_equal(td[off: off + n].cpu().numpy().reshape(diff.shape), want, err_msg="device, %s offset %d" % (name, off))
            assert not td[:off].any().item() and not td[off + n:].any().item()


# -------------------------------------------------------------------------------------------------- 2. the lattice seam
@pytest.mark.parametrize("h,w", SIZES)
def test_lattice_seam_is_the_numpy_statement(ctx, seam_want, h, w):
    import torch
    from tezip_amd import boundmap as bm
    shape = (8, h, w)
    for name in MAPS:
        diff, M, _ = seam_want(h, w, name)
        want = bm.quantise(diff, M, SKIP, "lattice")
        np.testing.assert_array_equal(ctx.lattice_bound_map(diff.copy(), M, shape, SKIP), want, err_msg=name)
        assert (want != diff).any() and (np.abs(want.astype(np.int64) - diff) <= M[None, :, :, None]).all()
        n = diff.size
        for off in (0, 1):
            td = torch.zeros(n + 16, dtype=torch.int16, device="cuda")
            tm = torch.zeros(h * w + 16, dtype=torch.uint8, device="cuda")
            td[off: off + n] = torch.from_numpy(diff.reshape(-1)).cuda()
            tm[off: off + h * w] = torch.from_numpy(M.reshape(-1)).cuda()
            torch.cuda.synchronize()
            ctx.lattice_bound_map(td[off: off + n], tm[off: off + h * w], shape, SKIP)
            ctx.synchronize()
            np.testing.assert_array_equal(td[off: off + n].cpu().numpy().reshape(diff.shape), want, err_msg="device, %s offset %d" % (name, off))
            assert not td[:off].any().item() and not td[off + n:].any().item()


# ------------------------------------------------------------------------------- 3. tz_encode against the unfused chain
def _gray(frames):
    return np.ascontiguousarray(np.repeat(frames[..., :1], 3, axis=-1))


JOBS = {"scene64": TF._scene64, "padded": TF._scene_padded}      # 64 x 80: the fused fronts apply; 61 x 90: padded, the unfused kernels
LAYOUTS = {"flat": (3, 0, 0), "channel": (3, 1, 0), "plane": (3, 0, 1), "gray": (1, 0, 0)}   # payload channels, delta stride, plane


def _set(ctx, channels, stride, plane):
    ctx.set_delta_plane(0)
    ctx.set_delta_stride(0)
    ctx.set_payload_channels(channels)
    ctx.set_delta_stride(stride)
    ctx.set_delta_plane(plane)


def _want_payload(sd, stack, channels, stride, plane, entropy):
    x = np.ascontiguousarray(stack[..., :1] if channels == 1 else stack)
    return sd.payload_from_delta(x, entropy, 3 if stride else 1, plane=bool(plane))


@pytest.mark.parametrize("quant", ["greedy", "lattice"])
@pytest.mark.parametrize("job", sorted(JOBS))
def test_encode_under_a_map_is_the_unfused_chain(ctx, job, quant):
    from tezip_amd import frametarget
    from tezip_amd import sdelta as sd
    colour = JOBS[job]()
    nt, h, w, _ = colour.shape
    shape = (nt, h, w)
    try:
        for frames, layouts in ((colour, ("flat", "channel", "plane")), (_gray(colour), ("gray",))):
            ctx.set_bound_map(None)
            ctx.set_quantiser("greedy")
            _set(ctx, 3, 0, 0)
            key = TT._rollout(ctx, frames, 0, 4)
            if frames is colour:
                TT._nontrivial(ctx, frames, key)
            skip = np.array(frametarget.fixed_frames(key, 0), np.uint8)
            lossless = ctx.encode_delta("abs", [0.0]).copy()
            ctx.set_quantiser(quant)
            abs2 = {}
            for lay in layouts:      # the uniform jobs, nothing set
                _set(ctx, *LAYOUTS[lay])
                abs2[lay] = [np.array(a, copy=True) for a in ctx.encode("abs", [2.0], True)[:2]]
                abs0 = [np.array(a, copy=True) for a in ctx.encode("abs", [0.0], True)[:2]]
                ctx.set_bound_map(np.full((h, w), 2, np.uint8))      # the uniform map is the abs k job, byte for byte
                got = ctx.encode("abs", [77.0], True)                # (b0 is not read)
                np.testing.assert_array_equal(got[0], abs2[lay][0], err_msg="uniform map, " + lay)
                np.testing.assert_array_equal(got[1], abs2[lay][1])
                ctx.set_bound_map(np.zeros((h, w), np.uint8))        # the zero map is the lossless job
                got = ctx.encode("abs", [77.0], True)
                np.testing.assert_array_equal(got[0], abs0[0], err_msg="zero map, " + lay)
                np.testing.assert_array_equal(got[1], abs0[1])
                ctx.set_bound_map(None)
            for name in ("roi", "random", "wide"):
                M = make_map(name, h, w)
                seam = ctx.lattice_bound_map if quant == "lattice" else ctx.error_bound_map
                stack = seam(lossless.copy(), M, shape, skip)
                assert (stack != lossless).any() and (np.abs(stack.astype(np.int64) - lossless) <= M[None, :, :, None]).all()
                ctx.set_bound_map(M)
                assert ctx.get_bound_map() == (h, w)
                _set(ctx, 3, 0, 0)
                np.testing.assert_array_equal(ctx.encode_delta("abs", [0.0]), stack, err_msg="tz_encode_delta, " + name)
                for lay in layouts:
                    channels, stride, plane = LAYOUTS[lay]
                    _set(ctx, channels, stride, plane)
                    for entropy in (True, False):
                        payload, table, _ = ctx.encode("abs", [0.0], entropy)
                        want_p, want_t = _want_payload(sd, stack, channels, stride, plane, entropy)
                        np.testing.assert_array_equal(np.asarray(payload).reshape(-1), want_p, err_msg="%s %s entropy %s" % (name, lay, entropy))
                        if entropy:
                            np.testing.assert_array_equal(table, want_t)
                        else:
                            assert table is None
                    if channels == 3:        # the delta tap is the same stack, and the payload beside it the same payload
                        p2, t2, tap = ctx.encode("abs", [0.0], True, want_delta=True)
                        np.testing.assert_array_equal(tap, stack)
                        np.testing.assert_array_equal(np.asarray(p2).reshape(-1), _want_payload(sd, stack, channels, stride, plane, True)[0])
                    if (nt * h * w * channels) % 8 == 0:    # --shuffle: the byte planes of the same payload
                        payload, table, _ = ctx.encode("abs", [0.0], True)
                        planes, _, _ = ctx.encode("abs", [0.0], True, shuffle=True)
                        np.testing.assert_array_equal(ctx.byte_unshuffle(np.asarray(planes).view(np.uint8).reshape(-1)).reshape(-1),
                                                      np.asarray(payload).reshape(-1))
                ctx.set_bound_map(None)
            if frames is colour and job == "scene64" and quant == "greedy":
                # the route: the direct-from-predictions front serves the map job where it serves the uniform one (no delta stack)
                _set(ctx, 3, 0, 0)
                launches = {}
                for which, m in (("abs", None), ("map", make_map("roi", h, w))):
                    ctx.set_bound_map(m)
                    ctx.prof_enable(True)
                    ctx.prof_reset()
                    ctx.encode("abs", [2.0], True)
                    launches[which] = {k: v[1] for k, v in ctx.prof_get().items()}
                    ctx.prof_enable(False)
                assert launches["map"]["delta"] == 0 == launches["abs"]["delta"], launches
    finally:
        ctx.prof_enable(False)
        ctx.set_bound_map(None)
        ctx.set_quantiser("greedy")
        _set(ctx, 3, 0, 0)


# -------------------------------------------------------------------------------------------------- 4. decode and check
@pytest.mark.parametrize("quant", ["greedy", "lattice"])
def test_decoded_frames_hold_the_map_and_the_check_kernel_counts(quant):
    import torch
    from tezip_amd import _lib
    from tezip_amd import boundmap as bm
    frames = TF._scene_padded()
    nt, h, w, _ = frames.shape
    cfg, wts = TT._model()
    enc, dec = _lib.Context(0), _lib.Context(0)
    try:
        for c in (enc, dec):
            c.load_model(cfg, wts)
            c.prepare(_lib.pad8(h), _lib.pad8(w), max_batch=4)
        key, _ = enc.rollout(frames, 0, 4)
        enc.set_quantiser(quant)
        keys = np.where(key[:, None, None, None], frames, 0).astype(np.uint8)
        dec.rollout_decode(keys, 0)
        bites = {}
        for name in ("roi", "random", "wide"):
            M = make_map(name, h, w)
            enc.set_bound_map(M)
            payload, table, _ = enc.encode("abs", [0.0], True)
            payload = np.array(payload, copy=True)
            out = np.asarray(dec.decode(payload, table))
            err = np.abs(out.astype(np.int64) - frames)
            assert (err <= M[None, :, :, None]).all() and err.max() > 0, name
            np.testing.assert_array_equal(out[:, M == 0], frames[:, M == 0])                     # M = 0: restored exactly
            rec = enc.encode_map_check(payload, table)
            assert not rec["violations"].any() and not rec["max_excess"].any()
            enc.encode("abs", [0.0], True, payload="resident")
            np.testing.assert_array_equal(enc.encode_map_check("resident", table), rec)
            # against the map tightened by 1 wherever it is positive the check must count, and count what numpy counts
            tight = (M - (M > 0)).astype(np.uint8)
            want = bm.check(frames, out, tight)
            bites[name] = (sum(r["violations"] for r in want), max(r["max_excess"] for r in want))
            got = enc.map_check(frames, out, tight, (nt, h, w))
            assert [int(v) for v in got["violations"]] == [r["violations"] for r in want]
            assert [int(v) for v in got["max_excess"]] == [r["max_excess"] for r in want]
            to, td, tm = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (frames, out, tight))   # device stacks
            torch.cuda.synchronize()
            np.testing.assert_array_equal(enc.map_check(to, td, tm, (nt, h, w)), got)
            print(quant, name, "worst error", int(err.max()), "violations against the tightened map:", [r["violations"] for r in want])
        # the check cannot pass vacuously: the tolerances of "roi" and "random" are used up somewhere (one of 255 never is)
        assert bites["roi"][0] > 0 and bites["roi"][1] == 1 and bites["random"][0] > 0 and bites["random"][1] == 1, bites
    finally:
        enc.close()
        dec.close()


# ---------------------------------------------------------------------------------------------------------- 5. probes
@pytest.mark.parametrize("quant", ["greedy", "lattice"])
def test_probes_under_a_map(ctx, quant):
    frames = TF._scene_padded()
    nt, h, w, _ = frames.shape
    try:
        TT._rollout(ctx, frames, 0, 4)
        ctx.set_quantiser(quant)
        ctx.set_bound_map(make_map("roi", h, w))
        payload, table, _ = ctx.encode("abs", [0.0], True)
        quality = TT._records(ctx.encode_quality(payload, table))
        np.testing.assert_array_equal(TT._records(ctx.bound_probe("abs", [0.0])), quality)
        assert quality[:, 0].sum() > 0 and quality[:, 1].max() <= 6
        recs = ctx.sdelta_probe("abs", [0.0], True, "huffd")
        for i, mode in enumerate(("flat", "channel", "plane")):
            SA._set_layout(ctx, mode)
            want = SA._real(ctx, "huffd", 0.0, True)
            assert (int(recs[i]["bytes"]), int(recs[i]["dist"]), int(recs[i]["table_len"])) == (want["bytes"], want["dist"], want["table_len"]), mode
    finally:
        SA._set_layout(ctx, "flat")
        ctx.set_bound_map(None)
        ctx.set_quantiser("greedy")


# -------------------------------------------------------------------------------------------------------- 6. refusals
def test_refusals_while_a_map_is_set():
    from tezip_amd import _lib
    c = _lib.Context(0)
    try:
        frames = TF._scene64()
        nt, h, w, _ = frames.shape
        TT._rollout(c, frames, 0, 4)
        before = [np.array(a, copy=True) for a in c.encode("abs", [2.0], True)[:2]]
        M = make_map("roi", h, w)
        stack = np.zeros(frames.shape, np.int16)
        out = np.zeros(nt, _lib.QUALITY_DTYPE)
        bounds = np.full(nt, 3.0)
        c.set_bound_map(M)
        want = c.encode_delta("abs", [0.0]).copy()
        # frame bounds while a map is set: refused, both settings as they were
        assert c.lib.tz_set_frame_bounds(c.h, bounds.ctypes.data, nt) == -1
        with pytest.raises(_lib.TezipError, match="bound map"):
            c.set_frame_bounds(bounds)
        assert c.get_frame_bounds() == 0 and c.get_bound_map() == (h, w)
        np.testing.assert_array_equal(c.encode_delta("abs", [0.0]), want)
        # and the other way round
        c.set_bound_map(None)
        assert c.get_bound_map() is None
        c.set_frame_bounds(bounds)
        by_frames = c.encode_delta("abs", [0.0]).copy()
        assert c.lib.tz_set_bound_map(c.h, M.ctypes.data, h, w) == -1
        with pytest.raises(_lib.TezipError, match="frame bounds"):
            c.set_bound_map(M)
        assert c.get_frame_bounds() == nt and c.get_bound_map() is None
        np.testing.assert_array_equal(c.encode_delta("abs", [0.0]), by_frames)
        c.set_frame_bounds(None)
        c.set_bound_map(M)
        # a mode other than abs
        for mode in (1, 2, 3):
            assert c.lib.tz_encode_delta(c.h, mode, 0.01, 0.01, stack.ctypes.data) == -1
            assert c.lib.tz_bound_probe(c.h, mode, 0.01, 0.01, out.ctypes.data) == -1
        with pytest.raises(_lib.TezipError, match="abs"):
            c.encode("pwrel", [0.01], True)
        # the sharded entry points and the size probe
        hist, edge = np.zeros(_lib.TZ_NBINS, np.uint64), np.zeros(2, np.int16)
        assert c.lib.tz_encode_begin(c.h, 0, 2.0, 0.0, 1, hist.ctypes.data, edge.ctypes.data) == -6       # TZ_ERR_UNSUPPORTED
        one = np.zeros(1, _lib.SIZE_DTYPE)
        assert c.lib.tz_size_probe(c.h, 0, 2.0, 0.0, 1, 2, one.ctypes.data) == -6
        with pytest.raises(_lib.TezipError, match="bound map"):
            c.size_probe("abs", [2.0], True, "huffd")
        # a map of another size
        c.set_bound_map(M[:, :-1])
        assert c.lib.tz_encode_delta(c.h, 0, 2.0, 0.0, stack.ctypes.data) == -1
        with pytest.raises(_lib.TezipError, match="own size"):
            c.encode("abs", [2.0], True)
        assert c.lib.tz_set_bound_map(c.h, M.ctypes.data, 0, w) == -1
        # a change of the map drops a resident payload
        c.set_bound_map(M)
        _, table, _ = c.encode("abs", [0.0], True, payload="resident")
        c.encode_quality("resident", table)
        c.set_bound_map(make_map("random", h, w))
        with pytest.raises(_lib.TezipError):
            c.encode_quality("resident", table)
        # cleared: an abs 2 job's payload is what it was before the map was set, and the sharded entry serves again
        c.set_bound_map(None)
        again = c.encode("abs", [2.0], True)
        np.testing.assert_array_equal(again[0], before[0])
        np.testing.assert_array_equal(again[1], before[1])
        assert c.lib.tz_encode_begin(c.h, 0, 2.0, 0.0, 1, hist.ctypes.data, edge.ctypes.data) == 0
        rec = np.zeros(nt, _lib.MAP_DTYPE)
        assert c.lib.tz_encode_map_check(c.h, None, 0, None, -1, 0, rec.ctypes.data) == -4               # no map: TZ_ERR_STATE
        assert c.lib.tz_set_bound_map(None, None, 0, 0) == -1 and c.lib.tz_get_bound_map(None, None, None) == -1
    finally:
        c.close()


# ------------------------------------------------------------------------------------------ 7. the command line end to end
def test_cli_roi_job_and_the_uniform_map(tmp_path, capsys):
    from PIL import Image
    from tezip_amd import _lib, weights
    from tezip_amd import boundmap as bm
    frames = TF._scene_padded()
    nt, h, w, _ = frames.shape
    cfg, wts = TT._model()
    mdir, ddir = str(tmp_path / "model"), tmp_path / "data"
    weights.save_model(mdir, cfg, wts, _lib.pad8(h), _lib.pad8(w))
    ddir.mkdir()
    names = ["f_%03d.png" % t for t in range(nt)]
    for t, n in enumerate(names):
        Image.fromarray(frames[t]).save(ddir / n)
    M = make_map("roi", h, w)
    Image.fromarray(M).save(tmp_path / "roi.png")
    job = ["-p", "0", "-w", "4"]
    comp, udir = str(tmp_path / "comp"), str(tmp_path / "dec")
    code, out = TR._main(["-c", mdir, str(ddir), comp] + job + ["-m", "abs", "--bound-map", str(tmp_path / "roi.png"), "--report", "--coder", "huffd"], capsys)
    assert code == 0, out
    lines = out.splitlines()
    assert "abs" in lines and bm.stdout_line(M) in lines and bm.HELD_LINE in lines, out
    assert bm.stdout_line(M) == "bound map: %dx%d, abs 0..6, %.1f %% of pixels exact" % (h, w, 100.0 * 260 / (h * w))
    quality = json.load(open(os.path.join(comp, "quality.json")))
    assert quality["bound_map"] == {"file": str(tmp_path / "roi.png"), "max": 6, "violations": 0, "max_excess": 0}
    assert [fr["violations"] for fr in quality["per_frame"]] == [0] * nt and quality["mode"] == "abs" and quality["bound"] == []
    assert json.load(open(os.path.join(comp, "tezip_amd.json")))["bound_map"] == {"max": 6, "exact_pixels": 260}
    code, out = TR._main(["-u", mdir, comp, udir], capsys)                                  # no flag for the new content
    assert code == 0, out
    dec = TR._images(udir, names).astype(np.int64)
    err = np.abs(dec - frames)
    assert (err <= M[None, :, :, None]).all() and 0 < err.max() <= 6
    np.testing.assert_array_equal(dec[:, 5:18, 3:23], frames[:, 5:18, 3:23])                # exact inside the zero rectangle
    assert bm.main([str(tmp_path / "roi.png"), str(ddir), udir]) == 0                       # and the CPU tool agrees
    capsys.readouterr()
    # a uniform .npy map writes the three reference files byte for byte as -m abs -b k does
    np.save(tmp_path / "k3.npy", np.full((h, w), 3, np.uint8))
    a, b = str(tmp_path / "comp_map"), str(tmp_path / "comp_abs")
    code, out = TR._main(["-c", mdir, str(ddir), a] + job + ["-m", "abs", "--bound-map", str(tmp_path / "k3.npy")], capsys)
    assert code == 0, out
    code, out = TR._main(["-c", mdir, str(ddir), b] + job + ["-m", "abs", "-b", "3"], capsys)
    assert code == 0, out
    for name in ("filename.txt", "key_frame.dat", "entropy.dat"):
        assert open(os.path.join(a, name), "rb").read() == open(os.path.join(b, name), "rb").read(), name
