"""TZ-CLM1, the closed loop under one abs bound per pixel (tezip_amd/closedmap.py), on the CPU: the slow statement against first
principles -- a brute-force loop per sample, the bound, exact pixels, uniform and zero maps against closedloop.encode and
predselect.encode, the open-loop formulas under the map, the unchanged decoders -- the kernels' division shortcut against integer
division at every pair it can meet, and every refusal of --loop-map before a GPU is touched.  tests/test_gpu_closedmap.py holds the
library to this statement."""
import numpy as np
import pytest

import closedloop_jobs as J
import closedmap_jobs as M

NET_TRIPLES = [(7, 0, 3), (8, 1, 3)]


def _q(d, e):
    """TZ-QL1 on one delta with the radius e, written out."""
    if e == 0:
        return d
    s = 2 * e + 1
    k = (abs(d) + e) // s * s
    return max(-255, min(255, k if d > 0 else -k))


def test_the_statement_against_a_loop_per_sample():
    from tezip_amd import closedloop
    nt, p, win = 7, 0, 3
    h, w = M.SIZES[0]
    frames, net, m = M.frames("translating", nt, h, w), J.predictor(h, w), M.the_map(h, w)
    want = M.statement("translating", nt, h, w, p, win)
    hp, wp = closedloop.pad8(h), closedloop.pad8(w)
    np.testing.assert_array_equal(want["key"], closedloop.key_mask(nt, p, win))
    for t in range(nt):
        if want["key"][t]:
            np.testing.assert_array_equal(want["dec"][t], frames[t])
            assert not want["q"][t].any()                        # (p = 0: every fixed frame is a group's first)
            continue
        pred = np.asarray(net.next(closedloop.u8_to_f32(want["dec"][t - 1], hp, wp)), np.float32)   # the feeding rule
        np.testing.assert_array_equal(pred.view(np.uint32), want["pred"][t].view(np.uint32))
        for y in range(h):
            for x in range(w):
                for c in range(3):
                    xv = int(np.float32(pred[y, x, c]) * np.float32(255.0))
                    q = _q(xv - int(frames[t, y, x, c]), int(m[y, x]))
                    assert want["q"][t, y, x, c] == q and want["dec"][t, y, x, c] == max(0, min(255, xv - q)), (t, y, x, c)


@pytest.mark.parametrize("select", [False, True])
@pytest.mark.parametrize("h,w", M.SIZES)
@pytest.mark.parametrize("nt,p,win", NET_TRIPLES)
def test_the_bound_holds_and_exact_pixels_are_exact(nt, p, win, h, w, select):
    scene = "flicker" if select else "translating"
    frames, m = M.frames(scene, nt, h, w), M.the_map(h, w)
    want = M.statement(scene, nt, h, w, p, win, "map", select)
    err = np.abs(want["dec"].astype(int) - frames.astype(int))
    assert (err <= m[None, :, :, None]).all()
    assert err.max() > 6                                          # (and the wide tolerances are used)
    assert (m == 0).sum() > 0 and not err[:, m == 0].any()
    np.testing.assert_array_equal(want["dec"][want["key"]], frames[want["key"]])


@pytest.mark.parametrize("h,w", M.SIZES)
@pytest.mark.parametrize("nt,p,win", NET_TRIPLES)
def test_the_map_matters_at_most_samples(nt, p, win, h, w):
    """A job that indexed the map wrongly would decode to other bytes: 83 % of the samples differ under the map rolled by a pixel,
    92-94 % of q differ from the uniform-255 job."""
    assert 0.80 < M.check_map_matters("translating", nt, h, w, p, win) < 0.86
    a, f = M.statement("translating", nt, h, w, p, win), M.statement("translating", nt, h, w, p, win, "full")
    nk = ~a["key"]
    assert 0.91 < float((a["q"][nk] != f["q"][nk]).mean()) < 0.95


@pytest.mark.parametrize("h,w", M.SIZES)
@pytest.mark.parametrize("nt,p,win", M.TRIPLES)
def test_selection_is_mixed_and_depends_on_the_map(nt, p, win, h, w):
    want = M.statement("flicker", nt, h, w, p, win, "map", True)
    assert M.check_mixed(want) == M.PREV_TILES[h, w][nt, p, win]
    full = M.statement("flicker", nt, h, w, p, win, "full", True)
    nk = ~want["key"]
    assert not full["modes"].any()                                # under 255 every one of those tiles chooses differently
    assert int((want["modes"][nk] != full["modes"][nk]).sum()) == M.PREV_TILES[h, w][nt, p, win][0]
    assert not want["modes"][want["key"]].any()


def test_selection_against_first_principles():
    """Per tile: the costs under the pixel's own E, a tie to the network, the chosen x, and pv in the patched stack."""
    from tezip_amd import closedloop, predselect
    nt, p, win = 7, 0, 3
    h, w = M.SIZES[0]
    frames, m = M.frames("flicker", nt, h, w), M.the_map(h, w)
    want = M.statement("flicker", nt, h, w, p, win, "map", True)
    quant = np.vectorize(_q)
    for t in np.nonzero(~want["key"])[0]:
        orig, prev = frames[t].astype(np.int64), want["dec"][t - 1].astype(np.int64)
        x_net = closedloop.x_hat(want["pred"][t], h, w)
        e = np.repeat(m[..., None].astype(np.int64), 3, axis=2)
        for ty in range((h + 15) // 16):
            for tx in range((w + 15) // 16):
                sl = (slice(16 * ty, 16 * ty + 16), slice(16 * tx, 16 * tx + 16))
                cn = int(np.abs(quant(x_net[sl] - orig[sl], e[sl])).sum())
                cp = int(np.abs(quant(prev[sl] - orig[sl], e[sl])).sum())
                assert want["modes"][t, ty, tx] == (1 if cp < cn else 0), (t, ty, tx)
                x = prev[sl] if cp < cn else x_net[sl]
                q = quant(x - orig[sl], e[sl])
                np.testing.assert_array_equal(want["q"][t][sl], q)
                np.testing.assert_array_equal(want["dec"][t][sl], np.clip(x - q, 0, 255))
                if cp < cn:
                    np.testing.assert_array_equal(want["patched"][t][sl], predselect.pv(prev[sl]))
                else:
                    np.testing.assert_array_equal(want["patched"][t][sl].view(np.uint32), want["pred"][t][sl].view(np.uint32))
        np.testing.assert_array_equal(want["patched"][t][h:].view(np.uint32), want["pred"][t][h:].view(np.uint32))


@pytest.mark.parametrize("select", [False, True])
@pytest.mark.parametrize("h,w", M.SIZES)
@pytest.mark.parametrize("nt,p,win", NET_TRIPLES)
def test_uniform_and_zero_maps_are_the_closed_job(nt, p, win, h, w, select):
    from tezip_amd import closedloop, predselect
    scene = "flicker" if select else "translating"
    frames = M.frames(scene, nt, h, w)
    for which, bound, quant in (("six", [6.0], "lattice"), ("zero", [0.0], "greedy")):
        got = M.statement(scene, nt, h, w, p, win, which, select)
        if select:
            want = predselect.encode(frames, p, win, "abs", bound, quant, J.predictor(h, w))
            names = ("key", "q", "dec", "modes")
            np.testing.assert_array_equal(got["patched"].view(np.uint32), want["patched"].view(np.uint32))
        else:
            want = closedloop.encode(frames, p, win, "abs", bound, quant, J.predictor(h, w))
            names = ("key", "q", "dec")
        for name in names:
            np.testing.assert_array_equal(got[name], want[name], err_msg=which + " " + name)
        np.testing.assert_array_equal(got["pred"].view(np.uint32), want["pred"].view(np.uint32))
        if which == "zero":
            np.testing.assert_array_equal(got["dec"], frames)


@pytest.mark.parametrize("select", [False, True])
@pytest.mark.parametrize("nt,p,win", NET_TRIPLES)
def test_the_open_loop_formulas_and_the_decoders(nt, p, win, select):
    from tezip_amd import boundmap, closedloop, closedmap, predselect
    h, w = M.SIZES[1]
    scene = "flicker" if select else "translating"
    frames, m = M.frames(scene, nt, h, w), M.the_map(h, w)
    want = M.statement(scene, nt, h, w, p, win, "map", select)
    final = want["patched"] if select else want["pred"]
    np.testing.assert_array_equal(closedmap.open_loop_q(final, frames, p, win, m), want["q"])
    # (the same through the open loop's own helper: zeroed group firsts, boundmap.quantise on what is not skipped)
    d = closedloop.open_loop_q(final, frames, p, win, "abs", [0.0], "greedy").astype(np.int64)
    skip = closedloop.group_first(nt, p, win)
    skip[:p] = True
    np.testing.assert_array_equal(boundmap.quantise(d, m, skip, "lattice"), want["q"])
    kf = np.zeros_like(frames)
    kf[want["key"]] = frames[want["key"]]
    for layout in J.LAYOUTS:
        payload, table = closedloop.payload_of(want["q"], layout)
        if select:
            got = predselect.decode(kf, p, payload, table, layout, want["modes"], J.predictor(h, w))
            np.testing.assert_array_equal(got["patched"].view(np.uint32), want["patched"].view(np.uint32))
        else:
            got = closedloop.decode(kf, p, payload, table, layout, J.predictor(h, w))
        np.testing.assert_array_equal(got["dec"], want["dec"])
        np.testing.assert_array_equal(got["key"], want["key"])


def test_the_division_shortcut_at_every_pair():
    """(|d| + E) div (2E + 1) by one float reciprocal: all 511 numerators |d| + E <= 510 x 256 radii, with the reciprocal correctly
    rounded and one ulp either way (the hardware's approximate reciprocal lies in between)."""
    from tezip_amd import closedmap
    n, e = np.meshgrid(np.arange(511), np.arange(256), indexing="ij")      # n: the numerator |d| + E itself
    want = n // (2 * e + 1)
    for ulp in (-1, 0, 1):
        np.testing.assert_array_equal(closedmap.div_shortcut(n - e, e, ulp), want, err_msg="ulp %d" % ulp)
    # and the quantiser built on it is TZ-QL1 at every (d, E) of the domain
    from tezip_amd import lattice
    d, e = np.meshgrid(np.arange(-255, 256), np.arange(256), indexing="ij")
    k = closedmap.div_shortcut(np.abs(d), e) * (2 * e + 1)
    q = np.where(e == 0, d, np.sign(d) * np.minimum(k, 255))
    np.testing.assert_array_equal(q, lattice.quantise_e(d, e.astype(np.float64)))


def test_the_statement_checks_its_map():
    from tezip_amd import closedmap
    nt, p, win = 7, 0, 3
    h, w = M.SIZES[0]
    frames = M.frames("translating", nt, h, w)
    for bad in (np.zeros((h, w + 1), np.uint8), np.zeros((h, w), np.int32), np.zeros((h, w, 3), np.uint8)):
        with pytest.raises(ValueError):
            closedmap.encode(frames, p, win, bad, J.predictor(h, w))
    assert closedmap.stdout_line(M.the_map(h, w)).startswith("loop map: 24x40, abs 0..255, ") and "(TZ-CLM1)" in closedmap.stdout_line(M.the_map(h, w))
    m = np.full((512, 512), 6, np.uint8)
    m[:256, :256] = 0
    assert closedmap.stdout_line(m) == "loop map: 512x512, abs 0..6, 25.0 % of pixels exact (TZ-CLM1)"


# ------------------------------------------------------------------------------------------------- the flag's refusals
def test_check_flags():
    from tezip_amd import closedmap
    cf = closedmap.check_flags
    ok = dict(loop_map="m.npy", loop="closed", quant="lattice", mode="abs", bound=[])
    assert cf(**ok) is None and cf(**dict(ok, pred="select")) is None and cf(**dict(ok, pred="net")) is None
    assert cf(None, "open", None, "rel", [0.1], gray=True, target_psnr=40.0, pred="motion") is None   # no flag: nothing to say
    assert cf(**dict(ok, compressing=False)).startswith("--loop-map is valid with -c")
    for loop in (None, "open"):
        assert "add --loop closed" in cf(**dict(ok, loop=loop))
    for quant in (None, "greedy"):
        assert "add --quant lattice" in cf(**dict(ok, quant=quant))
    assert "takes the place of -b" in cf(**dict(ok, bound=[2.0]))
    for mode in (None, "rel", "absrel", "pwrel"):
        assert "-m abs" in cf(**dict(ok, mode=mode))
    assert "--pred motion" in cf(**dict(ok, pred="motion"))
    for kw, other in ((dict(threshold=0.01), "-t"), (dict(sweep=True), "--sweep"), (dict(gray=True), "--gray"),
                      (dict(target_psnr=40.0), "--target-psnr"), (dict(target_ratio=4.0), "--target-ratio"),
                      (dict(per_frame=True), "--per-frame"), (dict(frame_bounds="f.json"), "--frame-bounds"),
                      (dict(bound_map="m.npy"), "--bound-map"), (dict(loop_psnr=36.0), "--loop-psnr"),
                      (dict(loop_bounds="b.json"), "--loop-bounds")):
        msg = cf(**dict(ok, **kw))
        assert msg and msg.startswith("--loop-map cannot be combined with %s " % other), (other, msg)
    assert "sharded" in cf(**dict(ok, sharded=True))


def _cli(argv):
    from tezip_amd import tezip
    return tezip.build_parser().parse_args(argv)


C = ["-c", "m", "d", "o", "-p", "0", "-w", "3"]
MAP = ["--loop", "closed", "--quant", "lattice", "-m", "abs", "--loop-map", "MAP"]


@pytest.mark.parametrize("argv,needle", [
    (["-u", "m", "d", "o", "--loop-map", "MAP"], "--loop-map is valid with -c"),
    (["-l", "m", "d", "--loop-map", "MAP"], "--loop-map is valid with -c"),
    (C + ["--quant", "lattice", "-m", "abs", "--loop-map", "MAP"], "add --loop closed"),
    (C + ["--loop", "open", "--quant", "lattice", "-m", "abs", "--loop-map", "MAP"], "add --loop closed"),
    (C + ["--loop", "closed", "-m", "abs", "--loop-map", "MAP"], "add --quant lattice"),
    (C + ["--loop", "closed", "--quant", "greedy", "-m", "abs", "--loop-map", "MAP"], "add --quant lattice"),
    (C + MAP + ["-b", "2"], "takes the place of -b"),
    (C + ["--loop", "closed", "--quant", "lattice", "-m", "rel", "--loop-map", "MAP"], "-m abs"),
    (C + ["--loop", "closed", "--quant", "lattice", "--loop-map", "MAP"], "-m abs"),
    (C + MAP + ["--pred", "motion"], "--pred motion"),
    (C + MAP + ["--bound-map", "MAP"], "--bound-map"),
    (C + ["--loop", "closed", "--quant", "lattice", "--loop-map", "MAP", "--loop-psnr", "36"], "--loop-psnr"),
    (C + MAP + ["--loop-bounds", "b.json"], "--loop-bounds"),
    (C + MAP + ["--target-psnr", "40"], "--target-psnr"),
    (C + MAP + ["--target-ratio", "4", "--coder", "huffd"], "--target-ratio"),
    (C + MAP + ["--target-psnr", "40", "--per-frame"], "--target-psnr"),
    (C + MAP + ["--frame-bounds", "f.json"], "--frame-bounds"),
    (C + MAP + ["--gray"], "--gray"),
    (["-c", "m", "d", "o", "-p", "0", "-t", "0.01"] + MAP, "-t"),
    (["-c", "m", "d", "o", "-p", "0", "--sweep"] + MAP, "--sweep"),
    (C + ["--loop", "closed", "--quant", "lattice", "-m", "abs", "--loop-map", "MISSING.npy"], "cannot be read"),
    (C + ["--loop", "closed", "--quant", "lattice", "-m", "abs", "--loop-map", "FLOAT.npy"], "2-D uint8 array"),
    (C + ["--loop", "closed", "--quant", "lattice", "-m", "abs", "--loop-map", "CUBE.npy"], "2-D uint8 array"),
    (C + ["--loop", "closed", "--quant", "lattice", "-m", "abs", "--loop-map", "COLOUR.png"], "has colour"),
    (C + ["--loop", "closed", "--quant", "lattice", "-m", "abs", "--loop-map", "GARBAGE.png"], "cannot be read"),
])
def test_cli_refuses_before_a_gpu_is_touched(argv, needle, capsys, tmp_path, monkeypatch):
    from PIL import Image
    from tezip_amd import tezip
    monkeypatch.setattr(tezip, "probe_gpu", lambda force: pytest.fail("a GPU was probed"))
    out = tmp_path / "o"
    np.save(tmp_path / "MAP", np.zeros((8, 8), np.uint8))
    np.save(tmp_path / "FLOAT.npy", np.zeros((8, 8), np.float32))
    np.save(tmp_path / "CUBE.npy", np.zeros((8, 8, 2), np.uint8))
    colour = np.zeros((8, 8, 3), np.uint8)
    colour[..., 1] = 9
    Image.fromarray(colour).save(tmp_path / "COLOUR.png")
    (tmp_path / "GARBAGE.png").write_bytes(b"not an image")
    files = {"MAP": "MAP.npy", "FLOAT.npy": "FLOAT.npy", "CUBE.npy": "CUBE.npy", "COLOUR.png": "COLOUR.png", "GARBAGE.png": "GARBAGE.png",
             "MISSING.npy": "MISSING.npy"}
    argv = [str(out) if a == "o" else str(tmp_path / files[a]) if a in files else a for a in argv]
    with pytest.raises(SystemExit) as e:
        tezip.main(_cli(argv))
    assert e.value.code == 2
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    assert len(lines) == 1 and lines[0].startswith("ERROR:") and needle in lines[0], lines
    assert not out.exists()


def test_cli_refuses_a_sharded_job(capsys, tmp_path, monkeypatch):
    from tezip_amd import tezip
    np.save(tmp_path / "MAP", np.zeros((8, 8), np.uint8))
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setattr(tezip, "probe_gpu", lambda force: pytest.fail("a GPU was probed"))
    with pytest.raises(SystemExit) as e:
        tezip.main(_cli(C + [str(tmp_path / "MAP.npy") if a == "MAP" else a for a in MAP]))
    assert e.value.code == 2
    out = capsys.readouterr().out
    assert out.startswith("ERROR: --loop-map") and "sharded" in out


def test_the_existing_refusal_keeps_its_words(capsys, monkeypatch):
    """--bound-map with --loop closed is refused as it was, in the words it used."""
    from tezip_amd import tezip
    monkeypatch.setattr(tezip, "probe_gpu", lambda force: pytest.fail("a GPU was probed"))
    with pytest.raises(SystemExit) as e:
        tezip.main(_cli(C + ["--loop", "closed", "--quant", "lattice", "-m", "abs", "--bound-map", "m.npy"]))
    assert e.value.code == 2
    assert capsys.readouterr().out.startswith("ERROR: --loop closed cannot be combined with --bound-map (the loop takes one bound)")


def test_cli_passes_the_flag_to_compress_run(tmp_path, monkeypatch, capsys):
    from tezip_amd import compress, tezip
    calls = []
    monkeypatch.setattr(tezip, "probe_gpu", lambda force: True)
    monkeypatch.setattr(compress, "run", lambda *a, **kw: calls.append((a, kw)))
    path = tmp_path / "m.npy"
    np.save(path, np.zeros((8, 8), np.uint8))
    flags = ["--loop", "closed", "--quant", "lattice", "-m", "abs", "--loop-map", str(path)]
    tezip.main(_cli(C + flags + ["--sdelta", "auto", "--coder", "huffd", "--key-coder", "huff", "--report", "--ssim", "--digests"]))
    a, kw = calls[0]
    assert a[:8] == ("m", "d", "o", 0, 3, None, "abs", [])
    assert kw == dict(SHUFFLE=False, REPORT=True, CODER="huffd", KEY_CODER="huff", DIGESTS=True, SDELTA="auto", SSIM=True, QUANT="lattice",
                      LOOP="closed", LOOP_MAP=str(path))
    assert capsys.readouterr().out.splitlines()[-1] == "abs"
    tezip.main(_cli(C + flags + ["--pred", "select", "--shuffle"]))
    a, kw = calls[1]
    assert kw["LOOP_MAP"] == str(path) and kw["PRED"] == "select" and kw["SHUFFLE"] is True
    # the jobs without the flag are called as they were
    tezip.main(_cli(C + ["-m", "abs", "-b", "2", "--loop", "closed", "--quant", "lattice"]))
    assert "LOOP_MAP" not in calls[2][1]


@pytest.mark.parametrize("kw,needle", [
    (dict(LOOP_MAP=np.zeros((8, 8), np.uint8), QUANT="lattice"), "add --loop closed"),
    (dict(LOOP_MAP=np.zeros((8, 8), np.uint8), LOOP="closed"), "add --quant lattice"),
    (dict(LOOP_MAP=np.zeros((8, 8), np.uint8), LOOP="closed", QUANT="lattice", PRED="motion"), "--pred motion"),
    (dict(LOOP_MAP=np.zeros((8, 8), np.uint8), LOOP="closed", QUANT="lattice", BOUND_MAP="m.npy"), "--bound-map"),
    (dict(LOOP_MAP=np.zeros((8, 8), np.uint8), LOOP="closed", QUANT="lattice", LOOP_PSNR=36.0), "--loop-psnr"),
    (dict(LOOP_MAP=np.zeros((8, 8), np.float32), LOOP="closed", QUANT="lattice"), "LOOP_MAP is a float32 array"),
    (dict(LOOP_MAP="nowhere.npy", LOOP="closed", QUANT="lattice"), "nowhere.npy cannot be read"),
])
def test_run_refuses_before_a_gpu_is_touched(kw, needle, capsys, tmp_path, monkeypatch):
    from tezip_amd import compress
    monkeypatch.setattr(compress, "make_context", lambda *a, **k: pytest.fail("a context was made"))
    with pytest.raises(SystemExit) as e:
        compress.run("m", "d", str(tmp_path / "o"), 0, 3, None, "abs", [], True, False, True, **kw)
    assert e.value.code == 2
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    assert len(lines) == 1 and lines[0].startswith("ERROR:") and needle in lines[0], lines


def test_run_refuses_a_map_of_the_wrong_size(capsys, tmp_path, monkeypatch):
    from PIL import Image
    from tezip_amd import compress
    monkeypatch.setattr(compress, "make_context", lambda *a, **k: pytest.fail("a context was made"))
    monkeypatch.setattr(compress, "open_model", lambda *a, **k: pytest.fail("the model was read"))
    d = tmp_path / "d"
    d.mkdir()
    for t in range(3):
        Image.fromarray(np.full((8, 8, 3), t, np.uint8)).save(d / ("f%d.png" % t))
    path = tmp_path / "m.npy"
    np.save(path, np.zeros((8, 9), np.uint8))
    for spec, name in ((str(path), str(path)), (np.zeros((9, 8), np.uint8), "LOOP_MAP")):
        with pytest.raises(SystemExit) as e:
            compress.run("m", str(d), str(tmp_path / "o"), 0, 3, None, "abs", [], True, False, True, LOOP="closed", QUANT="lattice", LOOP_MAP=spec)
        assert e.value.code == 2
        out = capsys.readouterr().out.strip()
        assert out.startswith("ERROR: bound map %s is " % name) and out.endswith("for images of 8 x 8: a map has the images' own size"), out
