"""TZ-CLF1, the closed loop under one abs bound per frame (tezip_amd/closedframes.py), on the CPU: the slow statement against first
principles -- the guarantee of every searched frame by brute force over all 511 candidates, the feeding rule, the open-loop
formulas under per-frame bounds, uniform bounds against closedloop.encode, zeros against the lossless job -- and every refusal of
--loop-psnr / --loop-bounds before a GPU is touched.  tests/test_gpu_closedframes.py holds the library to this statement."""
import json

import numpy as np
import pytest

import closedframes_jobs as F
import closedloop_jobs as J


def _sse_table(x, orig):
    """sse(k) for k = 0 .. 510, from the formulas of TZ-QL1 and the decoder's clamp written out here."""
    d = x - orig
    out = []
    for k in range(511):
        e = min(255, k // 2)
        s = 2 * e + 1
        q = d if e == 0 else np.clip(np.sign(d) * ((np.abs(d) + e) // s) * s, -255, 255)
        err = np.clip(x - q, 0, 255) - orig
        out.append(int((err * err).sum()))
    return out


@pytest.mark.parametrize("job", sorted(F.EXPECTED_K))
def test_the_search_against_brute_force(job):
    from tezip_amd import closedframes, closedloop
    nt, h, w, p, win, db = job
    want = F.searched(nt, h, w, p, win, db)
    assert F.check_spread(want) == F.EXPECTED_K[job]
    frames, net, limit = F.frames(nt, h, w), J.predictor(h, w), F.limit_of(db, h, w)
    hp, wp = closedloop.pad8(h), closedloop.pad8(w)
    np.testing.assert_array_equal(want["key"], closedloop.key_mask(nt, p, win))
    for t in range(nt):
        orig = frames[t].astype(np.int64)
        if want["key"][t]:
            np.testing.assert_array_equal(want["dec"][t], frames[t])
            assert want["k"][t] == 0 and want["bounds"][t] == 0 and want["sse"][t] == 0
            assert all(row[t] == closedframes.NOT_RUN for row in want["trace"])
            continue
        # the feeding rule: the prediction comes from the DECODED frame in front
        pred = np.asarray(net.next(closedloop.u8_to_f32(want["dec"][t - 1], hp, wp)), np.float32)
        np.testing.assert_array_equal(pred.view(np.uint32), want["pred"][t].view(np.uint32))
        x = (pred[:h, :w] * np.float32(255.0)).astype(np.int64)
        table = _sse_table(x, orig)
        k = want["k"][t]
        assert table[k] <= limit and (k == 510 or table[k + 1] > limit), (t, k)      # the guarantee
        assert want["sse"][t] == table[k] and want["bounds"][t] == k / 2.0
        lo, hi, r = 0, 511, 0                                                         # the bisection, replayed on the table
        while hi - lo > 1:
            mid = (lo + hi) // 2
            assert want["trace"][r][t] == table[mid], (t, r)
            lo, hi = (mid, hi) if table[mid] <= limit else (lo, mid)
            r += 1
        assert lo == k and r <= closedframes.ROUNDS
        assert all(want["trace"][i][t] == closedframes.NOT_RUN for i in range(r, closedframes.ROUNDS))
        # the frame is decoded under E = floor(k / 2)
        e = k // 2
        s = 2 * e + 1
        d = x - orig
        q = d if e == 0 else np.clip(np.sign(d) * ((np.abs(d) + e) // s) * s, -255, 255)
        np.testing.assert_array_equal(want["q"][t], q)
        np.testing.assert_array_equal(want["dec"][t], np.clip(x - q, 0, 255))
        assert int(((want["dec"][t].astype(np.int64) - orig) ** 2).sum()) == table[k]


def test_not_monotone_is_why_it_is_a_boundary():
    """The statement promises a boundary; say so with a table that has a passing candidate above a failing one, if this job has
    one, and in any case that the result is no larger than the largest passing candidate."""
    nt, h, w, p, win, db = 7, 61, 90, 0, 3, 36.0
    want = F.searched(nt, h, w, p, win, db)
    limit = F.limit_of(db, h, w)
    t = 1
    x = (want["pred"][t][:h, :w] * np.float32(255.0)).astype(np.int64)
    table = _sse_table(x, F.frames(nt, h, w)[t].astype(np.int64))
    assert want["k"][t] <= max(k for k in range(511) if table[k] <= limit)


@pytest.mark.parametrize("nt,p,win", F.TRIPLES)
def test_given_bounds_the_open_loop_formulas_and_the_decoder(nt, p, win):
    from tezip_amd import closedframes, closedloop
    h, w = F.SIZES[1]
    frames = F.frames(nt, h, w)
    want = F.with_bounds(nt, h, w, p, win, tuple(F.given(nt)))
    bounds = want["bounds"]
    assert [b for b, k in zip(bounds, want["key"]) if k] == [0.0] * int(want["key"].sum())
    assert [b for b, k in zip(bounds, want["key"]) if not k] == [b for b, k in zip(F.given(nt), want["key"]) if not k]
    assert want["sse"] == [0] * nt and want["k"] == [0] * nt
    for t in range(nt):                                   # every sample within its frame's radius, which 255 caps
        err = np.abs(want["dec"][t].astype(int) - frames[t].astype(int)).max()
        assert err <= min(255, int(bounds[t])), t
    # the back half's formulas on the final predictions give the loop's q again
    np.testing.assert_array_equal(closedframes.open_loop_q(want["pred"], frames, p, win, bounds), want["q"])
    kf = np.zeros_like(frames)
    kf[want["key"]] = frames[want["key"]]
    for layout in J.LAYOUTS:
        payload, table = closedloop.payload_of(want["q"], layout)
        got = closedloop.decode(kf, p, payload, table, layout, J.predictor(h, w))
        np.testing.assert_array_equal(got["dec"], want["dec"])
        np.testing.assert_array_equal(got["key"], want["key"])


def test_a_search_replays_as_given_bounds():
    from tezip_amd import closedframes
    nt, h, w, p, win, db = 7, 61, 90, 0, 3, 30.0
    a = F.searched(nt, h, w, p, win, db)
    b = F.with_bounds(nt, h, w, p, win, tuple(float(v) for v in a["bounds"]))
    for name in ("key", "q", "dec"):
        np.testing.assert_array_equal(a[name], b[name])
    np.testing.assert_array_equal(a["pred"].view(np.uint32), b["pred"].view(np.uint32))
    np.testing.assert_array_equal(closedframes.open_loop_q(a["pred"], F.frames(nt, h, w), p, win, a["bounds"]), a["q"])


@pytest.mark.parametrize("b,other", [(6.0, ((6.0,), "lattice")), (0.0, ((0.0,), "greedy")), (0.9, ((0.0,), "greedy"))])
def test_uniform_bounds_are_the_closed_job(b, other):
    """A uniform list is closedloop.encode's job; zeros (and every bound below 1) the lossless one."""
    from tezip_amd import closedframes, closedloop
    nt, p, win = 8, 1, 3
    h, w = F.SIZES[0]
    frames = F.frames(nt, h, w)
    got = closedframes.encode(frames, p, win, J.predictor(h, w), bounds=[b] * nt)
    want = closedloop.encode(frames, p, win, "abs", list(other[0]), other[1], J.predictor(h, w))
    for name in ("key", "q", "dec"):
        np.testing.assert_array_equal(got[name], want[name])
    np.testing.assert_array_equal(got["pred"].view(np.uint32), want["pred"].view(np.uint32))


def test_limit_zero_is_the_lossless_job_without_a_probe():
    from tezip_amd import closedframes
    nt, p, win = 7, 0, 3
    h, w = F.SIZES[0]
    frames = F.frames(nt, h, w)
    got = closedframes.encode(frames, p, win, J.predictor(h, w), limit=0)
    np.testing.assert_array_equal(got["dec"], frames)
    assert got["k"] == [0] * nt and all(v == closedframes.NOT_RUN for row in got["trace"] for v in row)
    with pytest.raises(ValueError):
        closedframes.encode(frames, p, win, J.predictor(h, w))
    with pytest.raises(ValueError):
        closedframes.encode(frames, p, win, J.predictor(h, w), bounds=[0.0] * nt, limit=5)
    for bad in ([-1.0] + [0.0] * (nt - 1), [float("nan")] * nt, [float("inf")] * nt, [1.0] * (nt - 1)):
        with pytest.raises(ValueError):
            closedframes.encode(frames, p, win, J.predictor(h, w), bounds=bad)


# ------------------------------------------------------------------------------------------------- bound_search.json
def test_bound_search_json_replays_through_loop_bounds(tmp_path):
    from tezip_amd import closedframes, frametarget
    nt, h, w, p, win, db = 7, 61, 90, 0, 3, 36.0
    want = F.searched(nt, h, w, p, win, db)
    limit = F.limit_of(db, h, w)
    doc = closedframes.make(db, h * w * 3, limit, [bool(k) for k in want["key"]], ["f%d.png" % t for t in range(nt)], want["bounds"],
                            want["sse"], want["trace"])
    assert doc["definition"] == "TZ-CLF1" and doc["sse_limit"] == limit and doc["frame_samples"] == h * w * 3
    assert doc["target_psnr_db"] == db and doc["probes"] == 9 and len(doc["trace"]) == 9
    assert [fr["k"] for fr in doc["frames"]] == want["k"] and [fr["sse"] for fr in doc["frames"]] == want["sse"]
    assert [fr["fixed"] for fr in doc["frames"]] == [bool(k) for k in want["key"]]
    assert set(doc["frames"][1]) == {"index", "name", "fixed", "k", "bound", "sse"}
    assert doc["trace"][0]["sse"][0] is None and doc["trace"][0]["sse"][1] == want["trace"][0][1]
    assert closedframes.stdout_line(doc) == ("loop target: PSNR >= 36 dB in every frame -> abs bounds 5.5..8.5 "
                                             "(TZ-CLF1, 4 of 7 frames searched)")
    path = closedframes.write(str(tmp_path), doc)
    assert path.endswith("bound_search.json")
    assert closedframes.load(path) == list(want["bounds"]) == json.load(open(path))["frame_bounds"]
    assert frametarget.load(path) == list(want["bounds"])                      # and through --frame-bounds, as before
    nothing = closedframes.make(db, h * w * 3, 0, [True] * nt, None, [0.0] * nt, [0] * nt, [])
    assert closedframes.stdout_line(nothing).endswith("-> nothing to search")
    assert closedframes.explicit_line([0.0, 7.0, 3.5]) == "loop bounds: 3 frames, abs 0..7"


def test_load_names_its_flag_and_frame_bounds_keeps_its_words(tmp_path):
    from tezip_amd import closedframes, frametarget
    missing = str(tmp_path / "none.json")
    with pytest.raises(ValueError, match=r"^--loop-bounds .*none\.json: cannot be read"):
        closedframes.load(missing)
    with pytest.raises(ValueError, match=r"^--frame-bounds .*none\.json: cannot be read"):
        frametarget.load(missing)
    bad = tmp_path / "bad.json"
    bad.write_text("{not json")
    with pytest.raises(ValueError, match=r"^--loop-bounds .*bad\.json: not JSON"):
        closedframes.load(str(bad))
    bad.write_text(json.dumps({"bounds": [1]}))
    with pytest.raises(ValueError, match="frame_bounds"):
        closedframes.load(str(bad))
    bad.write_text(json.dumps([1, -2]))
    with pytest.raises(ValueError, match="entry 1"):
        closedframes.load(str(bad))
    with pytest.raises(ValueError, match="^LOOP_BOUNDS: entry 0"):
        closedframes.load([float("nan")])
    with pytest.raises(ValueError, match="^FRAME_BOUNDS: entry 0"):
        frametarget.load([float("nan")])
    assert closedframes.load(np.array([1, 2.5])) == [1.0, 2.5]
    assert closedframes.check_length([1.0, 2.0], 2, "x.json") is None
    assert closedframes.check_length([1.0, 2.0], 3, "x.json") == "--loop-bounds x.json: 2 bounds for 3 images"
    assert closedframes.check_length([1.0], 3, [1.0]) == "LOOP_BOUNDS: 1 bounds for 3 images"
    assert frametarget.check_length([1.0], 3, "x.json") == "--frame-bounds x.json: 1 bounds for 3 images"


# ------------------------------------------------------------------------------------------------- the flags' refusals
def test_check_flags():
    from tezip_amd import closedframes
    cf = closedframes.check_flags
    psnr = dict(loop_psnr=36.0, loop_bounds=None, loop="closed", quant="lattice", mode=None, bound=[])
    given = dict(loop_psnr=None, loop_bounds="b.json", loop="closed", quant="lattice", mode="abs", bound=[])
    assert cf(**psnr) is None and cf(**given) is None
    assert cf(None, None, "open", None, "rel", [0.1], gray=True, target_psnr=40.0) is None   # neither flag: nothing to say
    for ok in (psnr, given):
        flag = "--loop-psnr" if ok is psnr else "--loop-bounds"
        assert cf(**dict(ok, compressing=False)).startswith(flag + " is valid with -c")
        for loop in (None, "open"):
            assert "add --loop closed" in cf(**dict(ok, loop=loop))
        for quant in (None, "greedy"):
            assert "add --quant lattice" in cf(**dict(ok, quant=quant))
        assert "-b" in cf(**dict(ok, bound=[2.0]))
        for pred in ("select", "motion"):
            assert "--pred " + pred in cf(**dict(ok, pred=pred))
        assert cf(**dict(ok, pred="net")) is None
        for kw, other in ((dict(threshold=0.01), "-t"), (dict(sweep=True), "--sweep"), (dict(gray=True), "--gray"),
                          (dict(target_psnr=40.0), "--target-psnr"), (dict(target_ratio=4.0), "--target-ratio"),
                          (dict(per_frame=True), "--per-frame"), (dict(frame_bounds="f.json"), "--frame-bounds"),
                          (dict(bound_map="m.npy"), "--bound-map")):
            msg = cf(**dict(ok, **kw))
            assert msg and msg.startswith("%s cannot be combined with %s " % (flag, other)), (flag, other, msg)
        assert "sharded" in cf(**dict(ok, sharded=True))
    assert "one of the two" in cf(**dict(psnr, loop_bounds="b.json"))
    assert "-m" in cf(**dict(psnr, mode="abs")) and "-m" in cf(**dict(psnr, mode="rel"))
    for mode in (None, "rel", "absrel", "pwrel"):
        assert "-m abs" in cf(**dict(given, mode=mode))
    for db in (0.0, -3.0, float("nan"), float("inf")):
        msg = cf(**dict(psnr, loop_psnr=db))
        assert msg and msg.startswith("--loop-psnr must be"), msg


def _cli(argv):
    from tezip_amd import tezip
    return tezip.build_parser().parse_args(argv)


C = ["-c", "m", "d", "o", "-p", "0", "-w", "3"]
PSNR = ["--loop", "closed", "--quant", "lattice", "--loop-psnr", "36"]
GIVEN = ["--loop", "closed", "--quant", "lattice", "-m", "abs", "--loop-bounds", "B"]


@pytest.mark.parametrize("argv,needle", [
    (["-u", "m", "d", "o", "--loop-psnr", "36"], "--loop-psnr is valid with -c"),
    (["-u", "m", "d", "o", "--loop-bounds", "B"], "--loop-bounds is valid with -c"),
    (["-l", "m", "d", "--loop-psnr", "36"], "--loop-psnr is valid with -c"),
    (["-l", "m", "d", "--loop-bounds", "B"], "--loop-bounds is valid with -c"),
    (C + ["--quant", "lattice", "--loop-psnr", "36"], "add --loop closed"),
    (C + ["--loop", "open", "--quant", "lattice", "--loop-psnr", "36"], "add --loop closed"),
    (C + ["--loop", "closed", "--loop-psnr", "36"], "add --quant lattice"),
    (C + ["--loop", "closed", "--quant", "greedy", "-m", "abs", "--loop-bounds", "B"], "add --quant lattice"),
    (C + ["--quant", "lattice", "-m", "abs", "--loop-bounds", "B"], "add --loop closed"),
    (C + PSNR + ["-m", "abs", "--loop-bounds", "B"], "one of the two"),
    (C + PSNR + ["-b", "2"], "-b"),
    (C + GIVEN + ["-b", "2"], "-b"),
    (C + PSNR + ["-m", "abs"], "takes the place of -m"),
    (C + ["--loop", "closed", "--quant", "lattice", "-m", "rel", "--loop-bounds", "B"], "-m abs"),
    (C + ["--loop", "closed", "--quant", "lattice", "--loop-bounds", "B"], "-m abs"),
    (C + PSNR + ["--pred", "select"], "--pred select"),
    (C + GIVEN + ["--pred", "motion"], "--pred motion"),
    (C + PSNR + ["--target-psnr", "40"], "--target-psnr"),
    (C + PSNR + ["--target-ratio", "4", "--coder", "huffd"], "--target-ratio"),
    (C + PSNR + ["--target-psnr", "40", "--per-frame"], "--target-psnr"),
    (C + GIVEN + ["--frame-bounds", "f.json"], "--frame-bounds"),
    (C + GIVEN + ["--bound-map", "m.npy"], "--bound-map"),
    (C + PSNR + ["--gray"], "--gray"),
    (["-c", "m", "d", "o", "-p", "0", "-t", "0.01"] + PSNR, "-t"),
    (["-c", "m", "d", "o", "-p", "0", "--sweep"] + PSNR, "--sweep"),
    (C + ["--loop", "closed", "--quant", "lattice", "--loop-psnr", "0"], "--loop-psnr must be"),
    (C + ["--loop", "closed", "--quant", "lattice", "--loop-psnr", "nan"], "--loop-psnr must be"),
    (C + ["--loop", "closed", "--quant", "lattice", "--loop-psnr", "-5"], "--loop-psnr must be"),
    (C + ["--loop", "closed", "--quant", "lattice", "-m", "abs", "--loop-bounds", "MISSING"], "cannot be read"),
    (C + ["--loop", "closed", "--quant", "lattice", "-m", "abs", "--loop-bounds", "MALFORMED"], "not JSON"),
    (C + ["--loop", "closed", "--quant", "lattice", "-m", "abs", "--loop-bounds", "NEGATIVE"], "entry 1"),
])
def test_cli_refuses_before_a_gpu_is_touched(argv, needle, capsys, tmp_path, monkeypatch):
    from tezip_amd import tezip
    monkeypatch.setattr(tezip, "probe_gpu", lambda force: pytest.fail("a GPU was probed"))
    out = tmp_path / "o"
    files = {"B": "[0, 1, 2, 3, 4, 5, 6]", "MALFORMED": "[1, 2", "NEGATIVE": "[1, -1]"}
    for name, text in files.items():
        (tmp_path / name).write_text(text)
    argv = [str(out) if a == "o" else str(tmp_path / a) if a in files or a == "MISSING" else a for a in argv]
    with pytest.raises(SystemExit) as e:
        tezip.main(_cli(argv))
    assert e.value.code == 2
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    assert len(lines) == 1 and lines[0].startswith("ERROR:") and needle in lines[0], lines
    assert not out.exists()


@pytest.mark.parametrize("flags", [PSNR, GIVEN])
def test_cli_refuses_a_sharded_job(flags, capsys, tmp_path, monkeypatch):
    from tezip_amd import tezip
    (tmp_path / "B").write_text("[0, 1, 2]")
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setattr(tezip, "probe_gpu", lambda force: pytest.fail("a GPU was probed"))
    with pytest.raises(SystemExit) as e:
        tezip.main(_cli(C + [str(tmp_path / "B") if a == "B" else a for a in flags]))
    assert e.value.code == 2
    out = capsys.readouterr().out
    assert out.startswith("ERROR:") and "sharded" in out


def test_the_existing_refusals_keep_their_words(capsys, monkeypatch):
    """With the new flags absent, the closed loop refuses what it refused, in the words it used."""
    from tezip_amd import closedloop, tezip
    monkeypatch.setattr(tezip, "probe_gpu", lambda force: pytest.fail("a GPU was probed"))
    for extra, flag in ((["--target-psnr", "40"], "--target-psnr"), (["--target-psnr", "40", "--per-frame"], "--target-psnr"),
                        (["-m", "abs", "--frame-bounds", "f.json"], "--frame-bounds"), (["-m", "abs", "--bound-map", "m.npy"], "--bound-map")):
        with pytest.raises(SystemExit) as e:
            tezip.main(_cli(C + ["--loop", "closed"] + extra))
        assert e.value.code == 2
        out = capsys.readouterr().out
        assert out.startswith("ERROR: --loop closed cannot be combined with %s " % flag), out
    assert closedloop.check_flags("closed", "abs", [0.0], None, target_psnr=40.0) == (
        "--loop closed cannot be combined with --target-psnr (a target's probes assume predictions that do not depend on the bound)")


def test_cli_passes_the_flags_to_compress_run(tmp_path, monkeypatch, capsys):
    from tezip_amd import compress, tezip
    calls = []
    monkeypatch.setattr(tezip, "probe_gpu", lambda force: True)
    monkeypatch.setattr(compress, "run", lambda *a, **kw: calls.append((a, kw)))
    path = tmp_path / "b.json"
    path.write_text("[0, 1, 2]")
    tezip.main(_cli(C + PSNR + ["--sdelta", "auto", "--coder", "huffd", "--key-coder", "huff", "--report", "--ssim", "--digests"]))
    a, kw = calls[0]
    assert a[:8] == ("m", "d", "o", 0, 3, None, "abs", [])
    assert kw == dict(SHUFFLE=False, REPORT=True, CODER="huffd", KEY_CODER="huff", DIGESTS=True, SDELTA="auto", SSIM=True, QUANT="lattice",
                      LOOP="closed", LOOP_PSNR=36.0)
    assert capsys.readouterr().out.splitlines()[-1] == "abs"
    tezip.main(_cli(C + ["--loop", "closed", "--quant", "lattice", "-m", "abs", "--loop-bounds", str(path), "--shuffle"]))
    a, kw = calls[1]
    assert a[:8] == ("m", "d", "o", 0, 3, None, "abs", [])
    assert kw["LOOP_BOUNDS"] == str(path) and "LOOP_PSNR" not in kw and kw["SHUFFLE"] is True and kw["LOOP"] == "closed"
    # the jobs without the flags are called as they were
    tezip.main(_cli(C + ["-m", "abs", "-b", "2", "--loop", "closed", "--quant", "lattice"]))
    assert "LOOP_PSNR" not in calls[2][1] and "LOOP_BOUNDS" not in calls[2][1]


@pytest.mark.parametrize("kw,needle", [
    (dict(LOOP_PSNR=36.0, QUANT="lattice"), "add --loop closed"),
    (dict(LOOP_PSNR=36.0, LOOP="closed"), "add --quant lattice"),
    (dict(LOOP_PSNR=36.0, LOOP="closed", QUANT="lattice", PRED="select"), "--pred select"),
    (dict(LOOP_PSNR=36.0, LOOP_BOUNDS=[1.0, 2.0], LOOP="closed", QUANT="lattice"), "one of the two"),
    (dict(LOOP_PSNR=0.0, LOOP="closed", QUANT="lattice"), "--loop-psnr must be"),
    (dict(LOOP_BOUNDS=[1.0, -2.0], LOOP="closed", QUANT="lattice"), "LOOP_BOUNDS: entry 1"),
    (dict(LOOP_BOUNDS=[1.0, 2.0], LOOP="closed", QUANT="lattice", BOUND_MAP="m.npy"), "--bound-map"),
])
def test_run_refuses_before_a_gpu_is_touched(kw, needle, capsys, tmp_path, monkeypatch):
    from tezip_amd import compress
    monkeypatch.setattr(compress, "make_context", lambda *a, **k: pytest.fail("a context was made"))
    with pytest.raises(SystemExit) as e:
        compress.run("m", "d", str(tmp_path / "o"), 0, 3, None, "abs", [], True, False, True, **kw)
    assert e.value.code == 2
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    assert len(lines) == 1 and lines[0].startswith("ERROR:") and needle in lines[0], lines


def test_run_refuses_a_list_of_the_wrong_length(capsys, tmp_path, monkeypatch):
    from PIL import Image
    from tezip_amd import compress
    monkeypatch.setattr(compress, "make_context", lambda *a, **k: pytest.fail("a context was made"))
    monkeypatch.setattr(compress, "open_model", lambda *a, **k: pytest.fail("the model was read"))
    d = tmp_path / "d"
    d.mkdir()
    for t in range(3):
        Image.fromarray(np.full((8, 8, 3), t, np.uint8)).save(d / ("f%d.png" % t))
    with pytest.raises(SystemExit) as e:
        compress.run("m", str(d), str(tmp_path / "o"), 0, 3, None, "abs", [], True, False, True, LOOP="closed", QUANT="lattice",
                     LOOP_BOUNDS=[1.0, 2.0])
    assert e.value.code == 2
    assert capsys.readouterr().out.strip() == "ERROR: LOOP_BOUNDS: 2 bounds for 3 images"
