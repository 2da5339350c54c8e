"""Per-frame abs bounds on the CPU (`-c --target-psnr DB --per-frame`, `-c -m abs --frame-bounds FILE`; definition TZ-TPSNR-F1,
tezip_amd/frametarget.py): the search against synthetic probes and against the C oracle's quantiser, bound_search.json, the
parser of --frame-bounds, every refusal of the command line and of compress.run, and the C ABI's declarations."""
import json
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ft():
    from tezip_amd import frametarget
    return frametarget


# ------------------------------------------------------------------------------------------------ 1. the search
def _tables(nt, seed):
    """per frame a deliberately NON-monotone sse(k), k = 0 .. 511: a rising trend with dips below earlier values"""
    rng = np.random.default_rng(seed)
    tabs = []
    for f in range(nt):
        trend = np.arange(512, dtype=np.int64) ** 2 * int(rng.integers(1, 9)) // (f + 1)
        wobble = rng.integers(-3000, 3001, 512)
        t = np.maximum(trend + wobble * (np.arange(512) > 3), 0)
        t[0] = 0
        tabs.append(t)
    return tabs


def _table_probe(tabs, fixed, calls):
    def probe(cand):
        calls.append(list(cand))
        assert all(c == 0 for c, fx in zip(cand, fixed) if fx), "a fixed frame rides along at 0"
        return [int(tabs[f][c]) for f, c in enumerate(cand)]
    return probe


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
@pytest.mark.parametrize("limit", [1, 777, 20000, 150000, 10 ** 9])
def test_search_holds_the_guarantee_per_frame(ft, seed, limit):
    from tezip_amd import target
    nt = 9
    fixed = [f in (0, 1, 5) for f in range(nt)]
    tabs = _tables(nt, seed)
    assert any((np.diff(t) < 0).any() for t in tabs)
    calls = []
    ks, sse, trace = ft.search(_table_probe(tabs, fixed, calls), limit, fixed)
    assert len(calls) == len(trace) <= 9
    for f in range(nt):
        if fixed[f]:
            assert ks[f] == 0 and sse[f] == 0 and all(t["k"][f] is None and t["sse"][f] is None and t["pass"][f] is None for t in trace)
            continue
        assert 0 <= ks[f] <= target.K_MAX
        assert tabs[f][ks[f]] <= limit and sse[f] == tabs[f][ks[f]]
        assert ks[f] == target.K_MAX or tabs[f][ks[f] + 1] > limit      # a boundary (not necessarily the largest passing k)
        assert all(t["pass"][f] == (t["sse"][f] <= limit) and t["sse"][f] == tabs[f][t["k"][f]] for t in trace)
        # the frame's own probes are target.search's on its own table: the frames are independent
        k1, tr1 = target.search(lambda k: int(tabs[f][k]), limit)
        assert k1 == ks[f] and [t["k"][f] for t in trace][:len(tr1)] == [t["k"] for t in tr1]
        assert all(t["k"][f] == ks[f] for t in trace[len(tr1):])          # finished: rides along at lo


def test_search_without_probes(ft):
    def never(cand):
        pytest.fail("no probe is wanted")
    assert ft.search(never, 0, [True, False, False]) == ([0, 0, 0], [0, 0, 0], [])
    assert ft.search(never, 5000, [True, True]) == ([0, 0], [0, 0], [])
    assert ft.search(never, 5000, []) == ([], [], [])
    with pytest.raises(ValueError):
        ft.search(lambda cand: [0], 10, [False, False])


def test_fixed_frames(ft):
    key = np.array([1, 0, 0, 0, 1, 0, 0, 0], np.uint8)
    assert ft.fixed_frames(key, 0) == [True, False, False, False, True, False, False, False]
    assert ft.fixed_frames(np.array([0, 0, 0, 1, 0], np.uint8), 2) == [True, True, False, True, False]
    assert ft.fixed_frames(np.array([0, 0], np.uint8), 0) == [True, False]


def test_document_round_trips_through_json(ft, tmp_path):
    from tezip_amd import target
    nt = 6
    fixed = [f in (0, 3) for f in range(nt)]
    tabs = _tables(nt, 7)
    limit = target.sse_limit(40, 64 * 80 * 3)
    ks, sse, trace = ft.search(_table_probe(tabs, fixed, []), limit, fixed)
    names = ["f_%d.png" % f for f in range(nt)]
    doc = ft.make(40, 64 * 80 * 3, limit, fixed, names, ks, sse, trace)
    path = ft.write(str(tmp_path), doc)
    assert os.path.basename(path) == "bound_search.json"
    back = json.load(open(path))
    assert back == doc and back == json.loads(json.dumps(doc))
    assert back["definition"] == "TZ-TPSNR-F1" and back["target_psnr_db"] == 40.0 and back["frame_samples"] == 64 * 80 * 3
    assert back["sse_limit"] == limit and back["probes"] == len(trace) == len(back["trace"])
    assert sorted(back["trace"][0]) == ["k", "pass", "sse"] and back["trace"][0]["k"][0] is None
    assert [fr["index"] for fr in back["frames"]] == list(range(nt)) and [fr["name"] for fr in back["frames"]] == names
    assert sorted(back["frames"][1]) == ["bound", "fixed", "index", "k", "name", "sse"]
    assert back["frame_bounds"] == [0.0 if fixed[f] else ks[f] / 2 for f in range(nt)]
    assert ft.load(path) == back["frame_bounds"]                       # the file replays as --frame-bounds
    line = ft.stdout_line(back)
    searched = [b for b, fx in zip(back["frame_bounds"], fixed) if not fx]
    assert line == "target: PSNR >= 40 dB in every frame -> abs bounds %g..%g (%d probes, 4 of 6 frames searched)" % (
        min(searched), max(searched), len(trace))
    none = ft.make(40, 10, 5, [True, True], None, [0, 0], [0, 0], [])
    assert ft.stdout_line(none) == "target: PSNR >= 40 dB in every frame -> nothing to search"


# ------------------------------------------------------------------- 2. end to end against the C oracle's quantiser
def test_search_over_the_oracles_quantiser_holds_every_frame_to_the_floor(ft):
    """8 x 64 x 80 translating_scene, -w 4, the window's key frame as the prediction of every frame of the window"""
    from oracle import coracle
    from tezip_amd import synth, target
    coracle.build()
    frames = synth.translating_scene(8, 64, 80)
    nt = len(frames)
    key = np.array([f % 4 == 0 for f in range(nt)])
    fixed = ft.fixed_frames(key, 0)
    delta = [(frames[f - f % 4].astype(np.int16) - frames[f].astype(np.int16)) for f in range(nt)]
    memo = {}

    def sse_of(f, k):
        if (f, k) not in memo:
            q = delta[f] if k == 0 else coracle.error_bound_frame(frames[f], delta[f], "abs", [k / 2])
            memo[f, k] = int(target.errors_of(frames[f][None], delta[f][None], q[None])[0, 0])
        return memo[f, k]

    limit = target.sse_limit(40, 64 * 80 * 3)
    ks, sse, trace = ft.search(lambda cand: [sse_of(f, k) for f, k in enumerate(cand)], limit, fixed)
    print("k", ks, "sse", sse, "limit", limit)
    assert len(trace) <= 9
    for f in range(nt):
        if fixed[f]:
            assert ks[f] == 0
            continue
        assert 1 <= ks[f] <= 509 and sse[f] == sse_of(f, ks[f]) <= limit
        assert sse_of(f, ks[f] + 1) > limit                               # one more oracle call per frame
        assert 10 * np.log10(64 * 80 * 3 * 65025.0 / sse[f]) >= 40.0
    # the uniform bound of the sequence target leaves frames under the floor: what the flag is for
    k_seq, _ = target.search(lambda k: sum(sse_of(f, k) for f in range(nt)), target.sse_limit(40, frames.size))
    assert any(sse_of(f, k_seq) > limit for f in range(nt) if not fixed[f])
    assert ks == [0, 8, 9, 9, 0, 8, 9, 9] and k_seq == 10                 # the figures of DESIGN.md section 9's table


# ------------------------------------------------------------------------------------------- 3. --frame-bounds FILE
def _file(tmp_path, text, name="b.json"):
    p = tmp_path / name
    p.write_text(text)
    return str(p)


def test_frame_bounds_file_forms(ft, tmp_path):
    assert ft.load(_file(tmp_path, "[0, 2.5, 7]")) == [0.0, 2.5, 7.0]
    assert ft.load(_file(tmp_path, '{"frame_bounds": [1, 0.0], "definition": "x"}')) == [1.0, 0.0]
    assert ft.load([0, 1.5, np.float64(3)]) == [0.0, 1.5, 3.0] and ft.load(np.array([2.0, 4.0])) == [2.0, 4.0]
    assert ft.check_length([1.0, 2.0], 2, "x.json") is None
    msg = ft.check_length([1.0, 2.0], 3, "x.json")
    assert "x.json" in msg and "2 bounds for 3 images" in msg
    assert ft.explicit_line([0.0, 3.5, 7.0]) == "frame bounds: 3 frames, abs 0..7"


@pytest.mark.parametrize("text,word", [
    ("[1, null, 2]", "entry 1"),
    ("[1, 2, NaN]", "entry 2"),
    ("[-0.5]", "entry 0"),
    ("[1, Infinity]", "entry 1"),
    ('[1, "2"]', "entry 1"),
    ("[true]", "entry 0"),
    ("[]", "no bounds"),
    ("[1, 2", "not JSON"),
    ("not json", "not JSON"),
    ('{"bounds": [1]}', "frame_bounds"),
    ('{"frame_bounds": 3}', "list"),
    ("3", "list"),
])
def test_frame_bounds_file_refusals_name_file_and_index(ft, tmp_path, text, word):
    path = _file(tmp_path, text)
    with pytest.raises(ValueError) as e:
        ft.load(path)
    assert path in str(e.value) and word in str(e.value)


def test_frame_bounds_unreadable_and_bad_sequences(ft, tmp_path):
    missing = str(tmp_path / "nothing.json")
    with pytest.raises(ValueError) as e:
        ft.load(missing)
    assert missing in str(e.value) and "cannot be read" in str(e.value)
    for seq, word in (([1.0, float("nan")], "entry 1"), ([-1], "entry 0"), ([None], "entry 0"), (5, "sequence")):
        with pytest.raises(ValueError) as e:
            ft.load(seq)
        assert "FRAME_BOUNDS" in str(e.value) and word in str(e.value)


# ------------------------------------------------------------------------------------------------- 4. the refusals
def _args(extra):
    from tezip_amd import tezip
    return tezip, tezip.build_parser().parse_args(extra)


JOB = ["-c", "m", "d", "o", "-p", "0", "-w", "4"]
GOOD = "@good@"   # replaced by a readable bounds file
BAD = "@bad@"     # replaced by a malformed one


@pytest.mark.parametrize("argv,env,word", [
    (JOB + ["--per-frame"], {}, "--target-psnr"),
    (JOB + ["-m", "abs", "-b", "2", "--per-frame"], {}, "--target-psnr"),
    (JOB + ["--per-frame", "--target-ratio", "4", "--coder", "huffd"], {}, "--target-ratio"),
    (JOB + ["--per-frame", "--target-psnr", "40", "--target-ratio", "4", "--coder", "huffd"], {}, "--target-ratio"),
    (JOB + ["-m", "abs", "-b", "2", "--frame-bounds", GOOD], {}, "-b"),
    (JOB + ["--frame-bounds", GOOD, "--target-psnr", "40"], {}, "--target-psnr"),
    (JOB + ["-m", "abs", "--frame-bounds", GOOD, "--target-psnr", "40", "--per-frame"], {}, "--target-psnr"),
    (JOB + ["-m", "abs", "--frame-bounds", GOOD, "--target-ratio", "4", "--coder", "huffd"], {}, "--target-ratio"),
    (JOB + ["-m", "rel", "--frame-bounds", GOOD], {}, "-m abs"),
    (JOB + ["-m", "pwrel", "--frame-bounds", GOOD], {}, "-m abs"),
    (JOB + ["--frame-bounds", GOOD], {}, "-m abs"),
    (["-u", "m", "c", "d", "--per-frame"], {}, "-c"),
    (["-u", "m", "c", "d", "--frame-bounds", GOOD], {}, "-c"),
    (["-l", "m", "d", "--per-frame"], {}, "-c"),
    (["-l", "m", "d", "--frame-bounds", GOOD], {}, "-c"),
    (["-c", "m", "d", "o", "-p", "0", "--sweep", "4", "8", "--target-psnr", "40", "--per-frame"], {}, "--sweep"),
    (["-c", "m", "d", "o", "-p", "0", "-m", "abs", "--sweep", "4", "8", "--frame-bounds", GOOD], {}, "--sweep"),
    (JOB + ["--target-psnr", "40", "--per-frame"], {"WORLD_SIZE": "2"}, "sharded"),
    (JOB + ["-m", "abs", "--frame-bounds", GOOD], {"WORLD_SIZE": "2"}, "sharded"),
    (JOB + ["-m", "abs", "--frame-bounds", BAD], {}, "entry 1"),
    (JOB + ["-m", "abs", "--frame-bounds", "@missing@"], {}, "cannot be read"),
])
def test_cli_refusals(monkeypatch, capsys, tmp_path, argv, env, word):
    good, bad = _file(tmp_path, "[0, 1, 2, 3]", "good.json"), _file(tmp_path, "[0, -1]", "bad.json")
    argv = [{GOOD: good, BAD: bad, "@missing@": str(tmp_path / "missing.json")}.get(a, a) for a in argv]
    tezip, arg = _args(argv)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setattr(tezip, "probe_gpu", lambda force: pytest.fail("refused before a GPU is touched"))
    with pytest.raises(SystemExit) as e:
        tezip.main(arg)
    out = capsys.readouterr().out
    assert e.value.code == 2 and out.startswith("ERROR:") and word in out and len(out.strip().splitlines()) == 1, out
    if BAD in argv or "@missing@" in argv:
        assert argv[-1] in out          # the message names the file


def test_flags_are_accepted_where_they_are_valid_and_reach_run(monkeypatch, capsys, tmp_path):
    from tezip_amd import compress
    good = _file(tmp_path, "[0, 1, 2, 3]", "good.json")
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    seen = {}
    monkeypatch.setattr(compress, "run", lambda *a, **kw: seen.update(kw, args=a))
    tezip, arg = _args(JOB + ["--target-psnr", "40", "--per-frame", "--coder", "huffd", "--key-coder", "huffg", "--gray", "--sdelta", "channel",
                              "--report", "--ssim", "--digests", "-n"])
    monkeypatch.setattr(tezip, "probe_gpu", lambda force: True)
    tezip.main(arg)
    assert seen["PER_FRAME"] is True and seen["FRAME_BOUNDS"] is None and seen["TARGET_PSNR"] == 40.0 and seen["CODER"] == "huffd"
    assert seen["args"][6:8] == ("abs", []) and seen["SDELTA"] == "channel" and seen["GRAY"] and seen["DIGESTS"] and seen["SSIM"]
    assert "abs" in capsys.readouterr().out.splitlines()          # printed where the reference prints the mode
    seen.clear()
    tezip.main(_args(JOB + ["-m", "abs", "--frame-bounds", good, "--shuffle", "-v"])[1])
    assert seen["PER_FRAME"] is False and seen["FRAME_BOUNDS"] == good and seen["TARGET_PSNR"] is None and seen["SHUFFLE"] is True
    assert seen["args"][6:8] == ("abs", []) and "abs" in capsys.readouterr().out.splitlines()
    for argv in (JOB + ["-m", "abs", "-b", "2"], JOB + ["--target-psnr", "40"]):      # the jobs without the flags are the calls they were
        seen.clear()
        tezip.main(_args(argv)[1])
        assert "PER_FRAME" not in seen and "FRAME_BOUNDS" not in seen


def test_a_direct_caller_of_run_is_refused(monkeypatch, capsys, tmp_path):
    from tezip_amd import compress
    monkeypatch.setattr(compress, "make_context", lambda *a, **k: pytest.fail("refused before a GPU is touched"))
    run = lambda mode, bound, **kw: compress.run("m", str(tmp_path), str(tmp_path / "o"), 0, 4, None, mode, bound, True, False, True, **kw)  # noqa: E731
    cases = [
        (("abs", []), dict(PER_FRAME=True), "--target-psnr"),
        (("abs", []), dict(PER_FRAME=True, TARGET_RATIO=4.0, CODER="huffd"), "--target-ratio"),
        (("abs", [2.0]), dict(FRAME_BOUNDS=[0, 1]), "-b"),
        (("rel", []), dict(FRAME_BOUNDS=[0, 1]), "-m abs"),
        (("abs", []), dict(FRAME_BOUNDS=[0, 1], TARGET_PSNR=40.0), "--target-psnr"),
        (("abs", []), dict(FRAME_BOUNDS=[0, float("nan")]), "entry 1"),
        (("abs", []), dict(FRAME_BOUNDS=[0, -2.0]), "entry 1"),
        (("abs", []), dict(FRAME_BOUNDS=str(tmp_path / "none.json")), "cannot be read"),
    ]
    for (mode, bound), kw, word in cases:
        with pytest.raises(SystemExit) as e:
            run(mode, bound, **kw)
        out = capsys.readouterr().out
        assert e.value.code == 2 and out.startswith("ERROR:") and word in out and len(out.strip().splitlines()) == 1, (kw, out)
    monkeypatch.setattr(compress.tzdist, "active", lambda: (0, 2))
    for kw in (dict(PER_FRAME=True, TARGET_PSNR=40.0), dict(FRAME_BOUNDS=[0, 1])):
        with pytest.raises(SystemExit) as e:
            run("abs", [], **kw)
        assert e.value.code == 2 and "sharded" in capsys.readouterr().out


def test_a_list_of_the_wrong_length_is_refused_once_the_directory_is_listed(monkeypatch, capsys, tmp_path):
    from PIL import Image
    from tezip_amd import compress
    ddir = tmp_path / "data"
    ddir.mkdir()
    for t in range(3):
        Image.fromarray(np.full((8, 8, 3), 40 * t, np.uint8)).save(ddir / ("f_%d.png" % t))
    monkeypatch.setattr(compress, "open_model", lambda d: pytest.fail("refused before the model is read"))
    monkeypatch.setattr(compress, "make_context", lambda *a, **k: pytest.fail("refused before a GPU is touched"))
    path = _file(tmp_path, "[0, 1, 2, 3]")
    for spec in (path, [0.0, 1.0]):
        with pytest.raises(SystemExit) as e:
            compress.run("m", str(ddir), str(tmp_path / "o"), 0, 4, None, "abs", [], True, False, True, FRAME_BOUNDS=spec)
        out = capsys.readouterr().out
        assert e.value.code == 2 and out.startswith("ERROR:") and "for 3 images" in out and len(out.strip().splitlines()) == 1
    assert path in out or "FRAME_BOUNDS" in out
    assert not os.path.exists(tmp_path / "o")


# ---------------------------------------------------------------------------------------------------- 5. the C ABI
def test_the_abi_declares_and_binds_the_three_names():
    from tezip_amd import _lib
    text = open(os.path.join(ROOT, "include", "tezip_hip.h")).read()
    for name in ("tz_set_frame_bounds", "tz_get_frame_bounds", "tz_error_bound_frames"):
        assert re.search(r"int\s+%s\s*\(" % name, text) and name in _lib.EXPORTS
    for name in ("set_frame_bounds", "get_frame_bounds", "error_bound_frames"):
        assert callable(getattr(_lib.Context, name))
