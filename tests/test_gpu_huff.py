"""The opt-in Huffman coder on the GPU: k_huff_size / k_huff_scan / k_huff_enc write the numpy encoder's bytes, k_huff_dec
reads both back bit-exactly (tezip_amd/huff.py is the specification); `-c --coder huff` then `-u` writes what `-c` then
`-u` writes.  No test feeds the decoder a corrupted body: the header's validation is tested on the CPU
(tests/test_huff.py), the body clamps are in the kernel's text."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_huff import assert_fills_the_image, filling_payloads, golden_payloads, synthetic_payloads

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from tezip_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _inputs():
    """(name, payload, lengths): lengths None = the optimal code of the payload's own counts."""
    from tezip_amd import huff
    out = [(name, pay, None) for name, pay, _, _, _ in golden_payloads()] + [(name, pay, None) for name, pay in synthetic_payloads(huff)]
    rng = np.random.default_rng(11)
    out.append(("geometric_8M", np.minimum(rng.geometric(0.25, 8 << 20) - 1, 1020).astype(np.int16), None))
    return out + filling_payloads(huff)      # given codes: chunks that fill the LDS image, runs that end on words, an incomplete code


def _code(pay):
    from tezip_amd import huff
    base = int(pay.min())
    return huff.code_lengths(np.bincount(pay.astype(np.int64) - base)), base


def _check_pair(ctx, name, pay, ln=None):
    from tezip_amd import huff
    base = int(pay.min())
    if ln is None:
        ln, base = _code(pay)
    want = np.frombuffer(huff.pack_body(*huff.encode_body(pay, ln, base)), np.uint8)
    got = ctx.huff_encode_buf(pay, ln, base)
    assert got.size == want.size and (got == want).all(), "%s: the GPU stream differs from the numpy encoder's" % name
    assert (ctx.huff_decode_buf(got, pay.size, ln, base) == pay).all(), "%s: GPU decode of the GPU stream" % name
    assert (ctx.huff_decode_buf(np.array(want), pay.size, ln, base) == pay).all(), "%s: GPU decode of the numpy stream" % name
    nruns, nchunks = huff.geometry(pay.size)
    co, rb = got[: nchunks * 4].view("<u4"), got[nchunks * 4: nchunks * 4 + nruns * 2].view("<u2")
    words = got[huff.body_bytes(pay.size, 0):].view("<u4")
    assert (huff.decode_body(co, rb, words, pay.size, ln, base) == pay).all(), "%s: numpy decode of the GPU stream" % name
    return co, rb


def test_gpu_stream_is_the_numpy_stream(ctx):
    from tezip_amd import huff
    seen = set()
    for name, pay, ln in _inputs():
        co, rb = _check_pair(ctx, name, pay, ln)
        if name.startswith("all12"):                                    # or the test is not testing the bound
            assert_fills_the_image(huff, name, pay.size, co, rb)
            seen.add("all12")
        if name.startswith("all1_"):
            assert (rb[:-1] == 256).all() and rb[-1] == 1
            seen.add("all1")
    assert seen == {"all12", "all1"}


def test_device_buffers_two_bytes_off_alignment(ctx):
    import torch
    rng = np.random.default_rng(5)
    pay = np.minimum(rng.geometric(0.3, 3 * 16384 + 777) - 1, 500).astype(np.int16)
    ln, base = _code(pay)
    from tezip_amd import huff
    want = np.frombuffer(huff.pack_body(*huff.encode_body(pay, ln, base)), np.uint8)
    dev = torch.empty(pay.size + 9, dtype=torch.int16, device="cuda")
    assert dev.data_ptr() % 16 == 0
    off = dev[1: 1 + pay.size]                                          # 2 bytes off a 16-byte boundary
    off.copy_(torch.from_numpy(pay))
    torch.cuda.synchronize()
    got = ctx.huff_encode_buf(off, ln, base)
    assert got.size == want.size and (got == want).all()
    out = torch.zeros(pay.size + 9, dtype=torch.int16, device="cuda")
    ctx.huff_decode_buf(got, pay.size, ln, base, out=out[1: 1 + pay.size])
    torch.cuda.synchronize()
    res = out.cpu().numpy()
    assert (res[1: 1 + pay.size] == pay).all() and res[0] == 0 and (res[1 + pay.size:] == 0).all()
    host = np.zeros(pay.size + 8, np.int16)[1: 1 + pay.size]            # a host array off alignment is staged
    host[...] = pay
    assert (ctx.huff_encode_buf(np.ascontiguousarray(host), ln, base) == want).all()


def test_bad_arguments_are_refused_before_a_launch(ctx):
    from tezip_amd import _lib
    pay = np.arange(600, dtype=np.int16) % 7
    ln, base = _code(pay)
    for bad_ln in (np.array([1, 1, 1], np.uint8), np.array([13, 1], np.uint8), np.zeros(4, np.uint8), np.ones(2112, np.uint8)):
        with pytest.raises(_lib.TezipError) as e:                       # Kraft > 1, a length of 13, no symbol, A > TZ_NBINS
            ctx.huff_encode_buf(pay, bad_ln, 0)
        assert e.value.status == -1
    with pytest.raises(_lib.TezipError) as e:                           # a payload value without a code: found by the size pass
        ctx.huff_encode_buf(pay, np.array([1, 1], np.uint8), 0)
    assert e.value.status == -1
    good = ctx.huff_encode_buf(pay, ln, base)
    for kw in (dict(n=pay.size, run=128), dict(n=pay.size * 200), dict(n=0)):
        with pytest.raises(_lib.TezipError) as e:                       # another R; a stream too short for n's index; n = 0
            ctx.huff_decode_buf(good, kw["n"], ln, base, run=kw.get("run", 256))
        assert e.value.status == -1
    with pytest.raises(_lib.TezipError) as e:
        _lib.Context(0).huff_encode(ln, base)                           # no resident payload
    assert e.value.status == -4
    assert (ctx.huff_decode_buf(good, pay.size, ln, base) == pay).all()  # the context still works


_POISON_SCRIPT = r"""
import sys
import numpy as np
sys.path.insert(0, %r)
sys.path.insert(0, %r)
from tezip_amd import _lib, huff
from test_huff import synthetic_payloads
ctx = _lib.Context(0)
for name, pay in synthetic_payloads(huff):
    base = int(pay.min())
    ln = huff.code_lengths(np.bincount(pay.astype(np.int64) - base))
    want = np.frombuffer(huff.pack_body(*huff.encode_body(pay, ln, base)), np.uint8)
    for rep in range(2):      # (the second call reuses pool blocks the first one filled)
        got = ctx.huff_encode_buf(pay, ln, base)
        assert got.size == want.size and (got == want).all(), name
        assert (ctx.huff_decode_buf(got, pay.size, ln, base) == pay).all(), name
ctx.close()
print("poison ok")
"""


@pytest.mark.parametrize("poison", ["0xA5", "0x00", "165"])
def test_same_bytes_under_poison(poison, tmp_path):
    """TEZIP_POISON fills every device buffer handed out before its use (tests/test_gpu_poison.py): the coder's streams
    must not depend on what its buffers held.  (The variable is read with atoi: 165 is 0xA5.)"""
    script = tmp_path / "poison_job.py"
    script.write_text(_POISON_SCRIPT % (ROOT, os.path.join(ROOT, "tests")))
    env = dict(os.environ, TEZIP_POISON=poison)
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, str(script)], cwd=ROOT, capture_output=True, text=True, env=env,
                       timeout=330)
    assert r.returncode == 0 and "poison ok" in r.stdout, r.stdout + r.stderr


# ---------------------------------------------------------------------------------------------------------- CLI
def _cli(args, timeout=300, env=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run(["timeout", "-k", "10", str(timeout), sys.executable, "-m", "tezip_amd.tezip"] + args, cwd=ROOT,
                          capture_output=True, text=True, timeout=timeout + 30, env=e)


@pytest.fixture(scope="module")
def job_dirs(tmp_path_factory):
    from PIL import Image
    from tezip_amd import synth, weights
    from tezip_amd.prednet import PredNetConfig
    tmp = tmp_path_factory.mktemp("huffcli")
    nt, h, w = 16, 29, 43
    cfg = PredNetConfig(stack_sizes=(3, 16, 32))
    wts = cfg.init_weights(seed=4, bias_scale=0.2)
    frames = synth.translating_scene(nt, h, w, seed=5)
    mdir = str(tmp / "model")
    weights.save_model(mdir, cfg, wts, 32, 48)
    ddir = tmp / "data"
    ddir.mkdir()
    names = ["f_%03d.png" % t for t in range(nt)]
    for t in range(nt):
        Image.fromarray(frames[t]).save(ddir / names[t])
    return tmp, mdir, str(ddir), names, (nt, h, w)


def _read(d, n):
    return open(os.path.join(d, n), "rb").read()


@pytest.mark.parametrize("tag,job", [
    ("lossless", ["-p", "1", "-w", "4", "-m", "abs", "-b", "0"]),
    ("abs2", ["-p", "1", "-w", "4", "-m", "abs", "-b", "2"]),
    ("no_entropy", ["-p", "0", "-w", "5", "-m", "abs", "-b", "2", "-n"]),
])
def test_cli_huff_job_decodes_to_the_zstd_jobs_images(job_dirs, tag, job):
    from tezip_amd import huff
    tmp, mdir, ddir, names, (nt, h, w) = job_dirs
    cz, ch = str(tmp / ("cz_" + tag)), str(tmp / ("ch_" + tag))
    rz = _cli(["-c", mdir, ddir, cz] + job + ["--report"])
    assert rz.returncode == 0, rz.stdout + rz.stderr
    rh = _cli(["-c", mdir, ddir, ch] + job + ["--report", "--coder", "huff", "-v"])
    assert rh.returncode == 0, rh.stdout + rh.stderr
    assert any(ln.startswith("huffman_coding:") for ln in rh.stdout.splitlines())
    for n in ("filename.txt", "key_frame.dat", "tezip_amd.json"):
        assert _read(cz, n) == _read(ch, n), n
    assert _read(cz, "entropy.dat")[:4] == b"\x28\xb5\x2f\xfd"          # without the flag: the reference's zstd frame
    eh = _read(ch, "entropy.dat")
    assert eh[:4] == b"TZH1"
    parsed = huff.parse(eh, key_len=nt * h * w * 3)
    assert parsed.shape == (1, nt, h, w, 3) and (parsed.table is None) == ("-n" in job)

    def pick(out, key):
        return [ln for ln in out.splitlines() if ln.startswith(key)]

    for key in ("max_abs_err:", "PSNR:"):
        assert pick(rz.stdout, key) == pick(rh.stdout, key) and len(pick(rh.stdout, key)) == 1, key
    doc = json.load(open(os.path.join(ch, "quality.json")))
    stored = sum(os.path.getsize(os.path.join(ch, n)) for n in ("filename.txt", "key_frame.dat", "entropy.dat"))
    assert doc["ratio"] == nt * h * w * 3 / stored
    uz, uh, ur, un = (str(tmp / (k + tag)) for k in ("uz_", "uh_", "ur_", "un_"))
    assert _cli(["-u", mdir, cz, uz]).returncode == 0
    r = _cli(["-u", mdir, ch, uh])
    assert r.returncode == 0, r.stdout + r.stderr
    assert sorted(os.listdir(uh)) == names
    for n in names:
        assert _read(uz, n) == _read(uh, n), n
    r = _cli(["-u", mdir, ch, ur, "--frames", "3:9"])
    assert r.returncode == 0, r.stdout + r.stderr
    assert sorted(os.listdir(ur)) == names[3:9]
    for n in names[3:9]:
        assert _read(ur, n) == _read(uh, n), n
    r = _cli(["-u", mdir, ch, un], env={"TEZIP_NO_STREAMING": "1"})    # the whole-array path reads the same file
    assert r.returncode == 0, r.stdout + r.stderr
    for n in names:
        assert _read(un, n) == _read(uh, n), n


def test_resident_forms_match_the_buffer_forms(ctx):
    """tz_huff_counts / tz_huff_encode / tz_huff_get on the payload of an encode, tz_huff_begin / put / decode into the
    payload buffer: the same bytes as the stand-alone forms, and the staged payload decodes like a payload_put one."""
    from tezip_amd import huff, synth
    from tezip_amd.prednet import PredNetConfig
    cfg = PredNetConfig(stack_sizes=(3, 16, 32))
    wts = cfg.init_weights(seed=2, bias_scale=0.2)
    nt, h, w = 12, 40, 56
    frames = synth.translating_scene(nt, h, w, seed=3)
    ctx.load_model(cfg, wts)
    ctx.prepare(40, 56, 4)
    for entropy in (True, False):
        key, _ = ctx.rollout(frames, 1, 4)
        _, table, _ = ctx.encode("abs", [2.0], entropy, payload="resident")
        pay = ctx.payload_get(0, nt * h * w * 3)
        counts, base = ctx.huff_counts()
        assert base == int(pay.min()) and (counts == np.bincount(pay.astype(np.int64) - base)).all()
        ln = huff.code_lengths(counts)
        nbytes = ctx.huff_encode(ln, base)
        body = np.concatenate([ctx.huff_get(0, 1000), ctx.huff_get(1000, nbytes - 1000)])
        want = np.frombuffer(huff.pack_body(*huff.encode_body(pay, ln, base)), np.uint8)
        assert body.size == want.size and (body == want).all()
        assert (ctx.payload_get(0, pay.size) == pay).all()              # the payload is left as it was
        kf = np.zeros_like(frames)
        kf[key] = frames[key]
        ctx.rollout_decode(kf, 1)
        ref = ctx.decode(pay, table)
        ctx.huff_begin(body.size, pay.size, ln, base)
        ctx.huff_put(0, body[:4096])
        ctx.huff_put(4096, body[4096:])
        ctx.huff_decode()
        assert (ctx.payload_get(0, pay.size) == pay).all()
        assert (ctx.decode(None, table) == ref).all()
