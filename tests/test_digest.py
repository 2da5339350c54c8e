"""CPU checks of the per-frame digests (`tezip.py -c --digests`, `-u --verify`): the numpy statement of TZD64 in
tezip_amd/digest.py against its known answers and its two guarantees (one changed sample, two exchanged samples),
frame_digests.json, the CLI refusals that must not touch a GPU, and `python -m tezip_amd.digest --check`."""
import copy
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

from tezip_amd import digest


def _rule(n):
    return ((7 * np.arange(n, dtype=np.int64)) % 251).astype(np.uint8)


# ------------------------------------------------------------------------------------------------------ the digest
@pytest.mark.parametrize("data,want", [
    (np.zeros(0, np.uint8), "0000000000000000"),
    (np.zeros(1, np.uint8), "e220a8397b1dcdaf"),
    (np.zeros(3, np.uint8), "42c0e022cd447754"),
    (np.arange(256, dtype=np.uint8), "4727d0502ccffeb0"),
    (_rule(61 * 90 * 3).reshape(61, 90, 3), "e5ec1ae43dfdc69b"),
    (_rule(8 * 700000 * 3).reshape(8, 700000, 3), "61f0594597e474b8"),   # i >= 2^24: 256 * i leaves 32 bits
], ids=["empty", "one_byte", "three_bytes", "all_bytes", "61x90", "8x700000"])
def test_known_answers(data, want):
    assert "%016x" % digest.frame_digest(data) == want


@pytest.mark.parametrize("shape", [(1, 1, 3), (8, 8, 3), (61, 90, 3)])
def test_stack_digests_are_the_frames_digests(shape):
    rng = np.random.default_rng(sum(shape))
    stack = rng.integers(0, 256, (5,) + shape, dtype=np.uint8)
    got = digest.stack_digests(stack)
    assert got.dtype == np.uint64 and got.shape == (5,)
    assert [int(d) for d in got] == [digest.frame_digest(f) for f in stack]
    assert len(set(int(d) for d in got)) == 5


def test_one_changed_sample_changes_the_digest():
    frame = np.random.default_rng(1).integers(0, 256, (61, 90, 3), dtype=np.uint8)
    clean = digest.frame_digest(frame)
    flat = frame.reshape(-1)
    for i in (0, flat.size // 2, flat.size - 1):
        for delta in (1, 255):
            bad = flat.copy()
            bad[i] = (int(bad[i]) + delta) & 0xFF
            assert digest.frame_digest(bad.reshape(frame.shape)) != clean, (i, delta)


def test_two_exchanged_samples_change_the_digest():
    frame = np.random.default_rng(2).integers(0, 256, (8, 8, 3), dtype=np.uint8)
    clean = digest.frame_digest(frame)
    flat = frame.reshape(-1)
    n = 0
    for i, j in ((0, 1), (5, 100), (flat.size - 2, flat.size - 1), (0, flat.size - 1)):
        if flat[i] == flat[j]:
            continue
        bad = flat.copy()
        bad[i], bad[j] = flat[j], flat[i]
        assert digest.frame_digest(bad) != clean, (i, j)
        n += 1
    assert n >= 3


# --------------------------------------------------------------------------------------------- frame_digests.json
def _doc(nt=4, shape=(8, 8, 3), seed=3):
    rng = np.random.default_rng(seed)
    dec = rng.integers(0, 256, (nt,) + shape, dtype=np.uint8)
    org = dec.copy()
    org[1, 0, 0, 0] ^= 1
    return digest.make(digest.stack_digests(dec), digest.stack_digests(org), shape), dec, org


def test_file_round_trip(tmp_path):
    doc, dec, org = _doc()
    assert digest.read(str(tmp_path)) is None and not digest.present(str(tmp_path))
    digest.write(str(tmp_path), doc)
    assert digest.present(str(tmp_path))
    back = digest.read(str(tmp_path), frames=4, shape=(8, 8, 3))
    assert back == doc
    assert sorted(back) == ["algorithm", "decoded", "format", "frames", "original", "shape"]
    assert back["format"] == 1 and back["algorithm"] == "TZD64-1" and back["frames"] == 4 and back["shape"] == [8, 8, 3]
    assert back["decoded"] == ["%016x" % digest.frame_digest(f) for f in dec]
    assert back["original"] == ["%016x" % digest.frame_digest(f) for f in org]
    assert back["decoded"][1] != back["original"][1] and back["decoded"][0] == back["original"][0]
    assert digest.mismatches(back, digest.stack_digests(dec)) == []
    assert digest.mismatches(back, digest.stack_digests(org)) == [1]
    assert digest.mismatches(back, digest.stack_digests(org[1:3]), first=1) == [1]
    assert digest.mismatches(back, digest.stack_digests(org[2:]), first=2) == []


def _edit(doc, **kw):
    d = copy.deepcopy(doc)
    d.update(kw)
    return d


def test_every_validation_error_names_its_field(tmp_path):
    doc, _, _ = _doc()
    good = doc["decoded"]
    cases = [
        (_edit(doc, format=2), {}, "format"),
        (_edit(doc, algorithm="TZD64-2"), {}, "algorithm"),
        (_edit(doc, decoded=good[:3]), {}, "decoded"),
        (_edit(doc, original=good + good[:1]), {}, "original"),
        (_edit(doc, decoded=good[:3] + [good[3].upper() if good[3] != good[3].upper() else "ABCDEF0123456789"]), {}, "decoded"),
        (_edit(doc, decoded=good[:3] + [good[3][:15]]), {}, "decoded"),
        (_edit(doc, original=good[:3] + [good[3][:15] + "g"]), {}, "original"),
        (_edit(doc, original=good[:3] + [int(good[3], 16)]), {}, "original"),
        (_edit(doc, frames=5), {}, "decoded"),                      # the lists no longer have `frames` entries
        (_edit(doc, frames=0), {}, "frames"),
        (_edit(doc, shape=[8, 8, 4]), {}, "shape"),
        (_edit(doc, shape=[8, 8]), {}, "shape"),
        (doc, {"frames": 5}, "frames"),                             # against the stream
        (doc, {"frames": 4, "shape": (8, 9, 3)}, "shape"),
        (doc, {"frames": 4, "shape": (4, 16, 3)}, "shape"),         # as many bytes per frame, another image
    ]
    for bad, against, field in cases:
        with pytest.raises(ValueError) as e:
            digest.validate(bad, **against)
        assert "field %r" % field in str(e.value), (field, str(e.value))
    assert digest.validate(doc, frames=4, shape=(8, 8, 3)) is doc
    with open(tmp_path / digest.NAME, "w") as f:
        f.write(json.dumps(doc)[:-20])
    with pytest.raises(ValueError) as e:
        digest.read(str(tmp_path))
    assert "damaged" in str(e.value)


def test_mismatch_lines_name_ten_frames_and_count_the_rest():
    names = ["f%02d.png" % i for i in range(30)]
    lines = digest.mismatch_lines([7], names)
    assert lines == ["ERROR: frame 7 (f07.png) does not match its recorded digest"]
    lines = digest.mismatch_lines(list(range(3, 28)), names)
    assert len(lines) == 11 and lines[9] == "ERROR: frame 12 (f12.png) does not match its recorded digest"
    assert "15 more" in lines[10]


# ------------------------------------------------------------------------------------------------------ CLI refusals
def _cli(args, env_extra=None):
    env = dict(os.environ)
    env.update(env_extra or {})
    return subprocess.run([sys.executable, "-m", "tezip_amd.tezip"] + args, cwd=ROOT, env=env, capture_output=True, text=True,
                          timeout=120)


_JOB = ["-p", "0", "-w", "5", "-m", "abs", "-b", "2"]


@pytest.mark.parametrize("args,env,flag", [
    (["-u", "M", "SRC", "{out}", "--digests"], {}, "--digests"),
    (["-l", "M", "SRC", "--digests"], {}, "--digests"),
    (["-c", "M", "SRC", "{out}", "-p", "0", "--sweep", "5", "10", "-m", "abs", "-b", "2", "--digests"], {}, "--digests"),
    (["-c", "M", "SRC", "{out}"] + _JOB + ["--digests"], {"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"}, "--digests"),
    (["-c", "M", "SRC", "{out}"] + _JOB + ["--verify", "auto"], {}, "--verify"),
    (["-l", "M", "SRC", "--verify", "off"], {}, "--verify"),
    (["-u", "M", "{empty}", "{out}", "--verify", "require"], {}, "--verify require"),
    (["-u", "M", "{recorded}", "{out}", "--verify", "require"], {"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"},
     "--verify require"),
])
def test_refusals_exit_2_before_a_device_is_opened(tmp_path, args, env, flag):
    out = tmp_path / "out"
    empty = tmp_path / "empty"
    empty.mkdir()
    recorded = tmp_path / "recorded"
    recorded.mkdir()
    digest.write(str(recorded), _doc()[0])
    sub = {"{out}": str(out), "{empty}": str(empty), "{recorded}": str(recorded)}
    r = _cli([sub.get(a, a) for a in args], env)
    assert r.returncode == 2, r.stdout + r.stderr
    assert r.stdout.startswith("ERROR:") and flag in r.stdout
    assert "GPU MODE" not in r.stdout and "CPU MODE" not in r.stdout      # refused before the device probe
    assert not out.exists()


def test_the_new_flags_are_not_in_the_refusals_of_other_jobs():
    from tezip_amd import tezip
    p = tezip.build_parser()
    plain_c = p.parse_args(["-c", "m", "d", "o"] + _JOB)
    plain_u = p.parse_args(["-u", "m", "d", "o"])
    assert plain_c.digests is False and plain_u.verify is None      # absent: the calls of today
    for arg in (plain_c, plain_u):
        assert tezip.check_digests_flag(arg) is None and tezip.check_verify_flag(arg) is None
    assert tezip.check_digests_flag(p.parse_args(["-c", "m", "d", "o"] + _JOB + ["--digests", "--report", "--shuffle"])) is None
    assert tezip.check_digests_flag(p.parse_args(["-c", "m", "d", "o"] + _JOB + ["--digests", "--coder", "huffr", "--key-coder",
                                                                                 "huff"])) is None
    for mode in ("auto", "off"):     # neither needs the file
        assert tezip.check_verify_flag(p.parse_args(["-u", "m", "d", "o", "--verify", mode, "--frames", "1:2"])) is None


# ----------------------------------------------------------------------------------------- python -m tezip_amd.digest
def _check(cdir, idir):
    return subprocess.run([sys.executable, "-m", "tezip_amd.digest", "--check", str(cdir), str(idir)], cwd=ROOT,
                          capture_output=True, text=True, timeout=120)


def test_check_tool_on_a_small_directory(tmp_path):
    from PIL import Image
    doc, dec, _ = _doc(nt=4, shape=(8, 8, 3), seed=5)
    cdir, idir = tmp_path / "comp", tmp_path / "images"
    cdir.mkdir()
    idir.mkdir()
    names = ["im_%d.png" % i for i in range(4)]
    with open(cdir / "filename.txt", "w", encoding="UTF-8") as f:
        f.write("1\n" + "".join(n + "\n" for n in names))
    digest.write(str(cdir), doc)
    for n, frame in zip(names, dec):
        Image.fromarray(frame).save(idir / n)
    r = _check(cdir, idir)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.splitlines() == ["verified: 4 frames"]
    bad = dec[2].copy()
    bad[3, 4, 1] ^= 0x10                       # one pixel of one image
    Image.fromarray(bad).save(idir / names[2])
    r = _check(cdir, idir)
    assert r.returncode == 3, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == 1 and "frame 2 (im_2.png)" in lines[0]
    os.remove(cdir / digest.NAME)              # no records: unusable, not "verified"
    assert _check(cdir, idir).returncode == 2
