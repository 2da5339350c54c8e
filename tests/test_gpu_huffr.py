"""The opt-in Huffman coder with repeat tokens on the GPU: k_huffr_count gives the numpy tokeniser's histogram, k_huffr_size /
k_huff_scan / k_huffr_enc write the numpy encoder's bytes, k_huffr_dec reads both back bit-exactly (tezip_amd/huffr.py is the
specification); `-c --coder huffr` then `-u` writes what `-c` then `-u` writes.  No test feeds the decoder a corrupted body:
the container's validation and the decoding rules for arbitrary bits are tested on the CPU (tests/test_huffr.py), the body
clamps are in the kernel's text."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from test_huff import assert_fills_the_image, golden_payloads, synthetic_payloads

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from tezip_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _inputs():
    """(name, payload, lengths): lengths None = the optimal code of the payload's own token counts."""
    from tezip_amd import huff
    out = [(name, pay, None) for name, pay, _, _, _ in golden_payloads()] + [(name, pay, None) for name, pay in synthetic_payloads(huff)]
    rng = np.random.default_rng(11)
    out.append(("all_equal", np.full(5 * 16384 + 300, -7, np.int16), None))
    out.append(("no_match", (np.arange(3 * 16384 + 1234) % 7).astype(np.int16), None))      # s[j] != s[j - 3] everywhere
    runs = np.repeat(rng.integers(0, 50, (40000, 3)), rng.geometric(0.05, 40000), 0).reshape(-1).astype(np.int16)    # pixels repeat
    out.append(("pixel_runs_n%d" % (runs.size - 5), runs[: runs.size - 5], None))           # long stretches, n % 8 != 0
    out.append(("geometric_8M", np.minimum(rng.geometric(0.25, 8 << 20) - 1, 1020).astype(np.int16), None))
    # a given code of 2111 + 8 lengths of 12: without a match every run is R * L bits and every chunk fills the LDS image
    all12 = np.full(2111 + 8, 12, np.uint8)
    out.append(("all12_no_match", (np.arange(2 * 16384 + 300) % 2111).astype(np.int16), all12))
    assert int(runs.min()) == 0
    out.append(("all12_pixel_runs", runs[: runs.size - 5], all12))
    return out


def _code(pay):
    from tezip_amd import huffr
    base = int(pay.min())
    return huffr.code_lengths(huffr.token_counts(pay, base, int(pay.max()) - base + 1)), base


def _check_pair(ctx, name, pay, ln=None):
    from tezip_amd import huffr
    base = int(pay.min())
    A = int(pay.max()) - base + 1
    want_counts = huffr.token_counts(pay, base, A)
    counts, gbase = ctx.huffr_counts(pay)
    assert gbase == base and counts.size == A + 8 and (counts == want_counts).all(), "%s: k_huffr_count against the numpy tokeniser" % name
    if ln is None:
        ln = huffr.code_lengths(counts)
    want = np.frombuffer(huffr.pack_body(*huffr.encode_body(pay, ln, base)), np.uint8)
    got = ctx.huffr_encode_buf(pay, ln, base)
    assert got.size == want.size and (got == want).all(), "%s: the GPU stream differs from the numpy encoder's" % name
    assert (ctx.huffr_decode_buf(got, pay.size, ln, base) == pay).all(), "%s: GPU decode of the GPU stream" % name
    assert (ctx.huffr_decode_buf(np.array(want), pay.size, ln, base) == pay).all(), "%s: GPU decode of the numpy stream" % name
    nruns, nchunks = huffr.geometry(pay.size)
    co, rb = got[: nchunks * 4].view("<u4"), got[nchunks * 4: nchunks * 4 + nruns * 2].view("<u2")
    words = got[huffr.body_bytes(pay.size, 0):].view("<u4")
    assert (huffr.decode_body(co, rb, words, pay.size, ln, base) == pay).all(), "%s: numpy decode of the GPU stream" % name
    return co, rb


def test_gpu_stream_is_the_numpy_stream(ctx):
    from tezip_amd import huffr
    filled = 0
    for name, pay, ln in _inputs():
        assert not name.endswith("no_match") or huffr_tokens(pay) == 0
        co, rb = _check_pair(ctx, name, pay, ln)
        if name == "all12_no_match":                                    # or the test is not testing the bound
            assert_fills_the_image(huffr, name, pay.size, co, rb)
            filled += 1
    assert filled == 1


def huffr_tokens(pay):
    from tezip_amd import huffr
    base = int(pay.min())
    A = int(pay.max()) - base + 1
    return int(huffr.token_counts(pay, base, A)[A:].sum())


def test_device_buffers_two_bytes_off_alignment(ctx):
    import torch
    from tezip_amd import huffr
    rng = np.random.default_rng(5)
    pay = np.repeat(np.minimum(rng.geometric(0.3, (9000, 3)) - 1, 500), rng.integers(1, 4, 9000), 0).reshape(-1)[: 3 * 16384 + 777].astype(np.int16)
    ln, base = _code(pay)
    want = np.frombuffer(huffr.pack_body(*huffr.encode_body(pay, ln, base)), np.uint8)
    dev = torch.empty(pay.size + 9, dtype=torch.int16, device="cuda")
    assert dev.data_ptr() % 16 == 0
    off = dev[1: 1 + pay.size]                                          # 2 bytes off a 16-byte boundary
    off.copy_(torch.from_numpy(pay))
    torch.cuda.synchronize()
    counts, gbase = ctx.huffr_counts(off)
    assert gbase == base and (counts == huffr.token_counts(pay, base, counts.size - 8)).all()
    got = ctx.huffr_encode_buf(off, ln, base)
    assert got.size == want.size and (got == want).all()
    out = torch.zeros(pay.size + 9, dtype=torch.int16, device="cuda")
    ctx.huffr_decode_buf(got, pay.size, ln, base, out=out[1: 1 + pay.size])
    torch.cuda.synchronize()
    res = out.cpu().numpy()
    assert (res[1: 1 + pay.size] == pay).all() and res[0] == 0 and (res[1 + pay.size:] == 0).all()
    host = np.zeros(pay.size + 8, np.int16)[1: 1 + pay.size]            # a host array off alignment is staged
    host[...] = pay
    assert (ctx.huffr_encode_buf(np.ascontiguousarray(host), ln, base) == want).all()


def test_bad_arguments_are_refused_before_a_launch(ctx):
    from tezip_amd import _lib
    pay = (np.arange(600, dtype=np.int16) // 5) % 7
    ln, base = _code(pay)
    tok = [0] * 8
    for bad_ln in (np.array([1, 1, 1] + tok, np.uint8), np.array([13, 1] + tok, np.uint8), np.zeros(4 + 8, np.uint8),
                   np.array([0, 0] + [3] * 8, np.uint8), np.ones(2112 + 8, np.uint8), np.ones(8, np.uint8)):
        with pytest.raises(_lib.TezipError) as e:     # Kraft > 1, a length of 13, no symbol, no literal, A > TZ_NBINS, A = 0
            ctx.huffr_encode_buf(pay, bad_ln, 0)
        assert e.value.status == -1
    with pytest.raises(_lib.TezipError) as e:                           # the payload needs tokens the code has none for
        ctx.huffr_encode_buf(pay, np.array([3] * 7 + [0] * 8, np.uint8), 0)
    assert e.value.status == -1
    good = ctx.huffr_encode_buf(pay, ln, base)
    for kw in (dict(n=pay.size, run=128), dict(n=pay.size * 200), dict(n=0)):
        with pytest.raises(_lib.TezipError) as e:                       # another R; a stream too short for n's index; n = 0
            ctx.huffr_decode_buf(good, kw["n"], ln, base, run=kw.get("run", 256))
        assert e.value.status == -1
    fresh = _lib.Context(0)
    for call in (lambda: fresh.huffr_encode(ln, base), fresh.huffr_counts, fresh.huffr_decode):
        with pytest.raises(_lib.TezipError) as e:                       # no resident payload / nothing staged
            call()
        assert e.value.status == -4
    fresh.close()
    assert (ctx.huffr_decode_buf(good, pay.size, ln, base) == pay).all()  # the context still works


_POISON_SCRIPT = r"""
import sys
import numpy as np
sys.path.insert(0, %r)
sys.path.insert(0, %r)
from tezip_amd import _lib, huff, huffr
from test_huff import synthetic_payloads
ctx = _lib.Context(0)
pays = synthetic_payloads(huff) + [("pixel_runs", np.repeat(np.arange(9000) %% 11, 3).repeat(2)[:50001].astype(np.int16))]
for name, pay in pays:
    base = int(pay.min())
    want_counts = huffr.token_counts(pay, base, int(pay.max()) - base + 1)
    ln = huffr.code_lengths(want_counts)
    want = np.frombuffer(huffr.pack_body(*huffr.encode_body(pay, ln, base)), np.uint8)
    for rep in range(2):      # (the second call reuses pool blocks the first one filled)
        counts, gbase = ctx.huffr_counts(pay)
        assert gbase == base and (counts == want_counts).all(), name
        got = ctx.huffr_encode_buf(pay, ln, base)
        assert got.size == want.size and (got == want).all(), name
        assert (ctx.huffr_decode_buf(got, pay.size, ln, base) == pay).all(), name
ctx.close()
print("poison ok")
"""


@pytest.mark.parametrize("poison", ["0xA5", "0x00"])
def test_same_bytes_under_poison(poison, tmp_path):
    """TEZIP_POISON fills every device buffer handed out before its use (tests/test_gpu_poison.py): the coder's streams
    must not depend on what its buffers held."""
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
    tmp = tmp_path_factory.mktemp("huffrcli")
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
def test_cli_huffr_job_decodes_to_the_zstd_jobs_images(job_dirs, tag, job):
    from tezip_amd import huff, huffr
    tmp, mdir, ddir, names, (nt, h, w) = job_dirs
    cz, ch, cr = str(tmp / ("cz_" + tag)), str(tmp / ("ch_" + tag)), str(tmp / ("cr_" + tag))
    rz = _cli(["-c", mdir, ddir, cz] + job + ["--report"])
    assert rz.returncode == 0, rz.stdout + rz.stderr
    assert _cli(["-c", mdir, ddir, ch] + job + ["--coder", "huff"]).returncode == 0
    rr = _cli(["-c", mdir, ddir, cr] + job + ["--report", "--coder", "huffr", "-v"])
    assert rr.returncode == 0, rr.stdout + rr.stderr
    assert any(ln.startswith("huffman_coding:") for ln in rr.stdout.splitlines())
    for n in ("filename.txt", "key_frame.dat", "tezip_amd.json"):
        assert _read(cz, n) == _read(cr, n), n
    er, eh = _read(cr, "entropy.dat"), _read(ch, "entropy.dat")
    assert er[:4] == b"TZR1" and eh[:4] == b"TZH1"
    parsed = huffr.parse(er, key_len=nt * h * w * 3)
    assert parsed.shape == (1, nt, h, w, 3) and (parsed.table is None) == ("-n" in job)
    pay = huff.decode_file(eh)[0]                                       # the same payload under both coders, and the file is
    assert (huffr.decode_file(er)[0] == pay).all()                      # the numpy encoder's, byte for byte
    assert er == huffr.encode_file(pay, parsed.table, parsed.shape, parsed.warm_up, base=parsed.base)
    print("%s: TZR1 %d bytes, TZH1 %d bytes, zstd-9 %d bytes" % (tag, len(er), len(eh), len(_read(cz, "entropy.dat"))))

    def pick(out, key):
        return [ln for ln in out.splitlines() if ln.startswith(key)]

    for key in ("max_abs_err:", "PSNR:"):
        assert pick(rz.stdout, key) == pick(rr.stdout, key) and len(pick(rr.stdout, key)) == 1, key
    doc = json.load(open(os.path.join(cr, "quality.json")))
    stored = sum(os.path.getsize(os.path.join(cr, n)) for n in ("filename.txt", "key_frame.dat", "entropy.dat"))
    assert doc["ratio"] == nt * h * w * 3 / stored
    assert len(pick(rr.stdout, "ratio:")) == 1 and float(pick(rr.stdout, "ratio:")[0].split(":")[1].split()[0]) == pytest.approx(doc["ratio"], rel=1e-3)
    uz, uh, ur, un = (str(tmp / (k + tag)) for k in ("uz_", "uh_", "ur_", "un_"))
    assert _cli(["-u", mdir, cz, uz]).returncode == 0
    r = _cli(["-u", mdir, cr, uh])
    assert r.returncode == 0, r.stdout + r.stderr
    assert sorted(os.listdir(uh)) == names
    for n in names:
        assert _read(uz, n) == _read(uh, n), n
    r = _cli(["-u", mdir, cr, ur, "--frames", "3:9"])
    assert r.returncode == 0, r.stdout + r.stderr
    assert sorted(os.listdir(ur)) == names[3:9]
    for n in names[3:9]:
        assert _read(ur, n) == _read(uh, n), n
    r = _cli(["-u", mdir, cr, un], env={"TEZIP_NO_STREAMING": "1"})    # the whole-array path reads the same file
    assert r.returncode == 0, r.stdout + r.stderr
    for n in names:
        assert _read(un, n) == _read(uh, n), n


def test_resident_forms_match_the_buffer_forms(ctx):
    """tz_huffr_counts / encode / get on the payload of an encode, tz_huffr_begin / put / decode into the payload buffer: the
    same bytes as the stand-alone forms, the staged payload decodes like a payload_put one, and neither decoder expands
    the stream staged for the other."""
    from tezip_amd import _lib, huff, huffr, synth
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
        counts, base = ctx.huffr_counts()
        assert base == int(pay.min()) and (counts == huffr.token_counts(pay, base, counts.size - 8)).all()
        assert (ctx.huffr_counts(pay)[0] == counts).all()
        ln = huffr.code_lengths(counts)
        nbytes = ctx.huffr_encode(ln, base)
        body = np.concatenate([ctx.huffr_get(0, 1000), ctx.huffr_get(1000, nbytes - 1000)])
        want = np.frombuffer(huffr.pack_body(*huffr.encode_body(pay, ln, base)), np.uint8)
        assert body.size == want.size and (body == want).all()
        assert (ctx.huffr_encode_buf(pay, ln, base) == want).all()
        assert (ctx.payload_get(0, pay.size) == pay).all()              # the payload is left as it was
        hcounts, hbase = ctx.huff_counts()                              # the Huffman coder beside it is what it was
        hl = huff.code_lengths(hcounts)
        hbytes = ctx.huff_encode(hl, hbase)
        assert (ctx.huff_get(0, hbytes) == np.frombuffer(huff.pack_body(*huff.encode_body(pay, hl, hbase)), np.uint8)).all()
        kf = np.zeros_like(frames)
        kf[key] = frames[key]
        ctx.rollout_decode(kf, 1)
        ref = ctx.decode(pay, table)
        ctx.huffr_begin(body.size, pay.size, ln, base)
        ctx.huffr_put(0, body[:4096])
        ctx.huffr_put(4096, body[4096:])
        with pytest.raises(_lib.TezipError) as e:
            ctx.huff_decode()                                           # a TZR1 stream is staged, not a TZH1 one
        assert e.value.status == -4
        ctx.huffr_decode()
        assert (ctx.payload_get(0, pay.size) == pay).all()
        assert (ctx.decode(None, table) == ref).all()


def test_tzh1_file_of_the_parent_commit_still_decodes(ctx):
    """tests/golden/huff_tzh1_parent.dat was written by `huff.encode_file` before this coder existed: TZH1 bytes are what they
    were, on the CPU and through k_huff_dec."""
    from tezip_amd import huff
    data = np.fromfile(os.path.join(GOLDEN, "huff_tzh1_parent.dat"), np.uint8)
    pay, p = huff.decode_file(data)
    assert bytes(data) == huff.encode_file(pay, p.table, p.shape, p.warm_up, base=p.base)
    assert (ctx.huff_decode_buf(np.ascontiguousarray(p.body), p.n, p.lengths, p.base) == pay).all()
    assert (ctx.huff_encode_buf(pay, p.lengths, p.base) == p.body).all()
