"""The opt-in Huffman coder that picks its match distance on the GPU: k_huffd_count gives the three histograms of the numpy
tokeniser from one read, the size / pack / expand kernels at every distance write and read the numpy encoder's bytes
(tezip_amd/huffd.py is the specification), the distance-3 stream is tz_huffr_*'s; `-c --coder huffd` writes huffd.encode_file's
file and `-u` restores what the other coders' jobs restore.  No test feeds the decoder a corrupted body: the container's
validation and the decoding rules for arbitrary bits are tested on the CPU (tests/test_huffd.py), the body clamps are the
ones k_huffr_dec has."""
import contextlib
import io
import json
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# around the match distances, a run's end (256) and a chunk's end (16384)
SIZES = (1, 2, 3, 4, 255, 256, 257, 16383, 16384, 16385, 3 * 16384 + 77)


@pytest.fixture(scope="module")
def ctx():
    from tezip_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def families(n):
    """name -> int16[n]"""
    rng = np.random.default_rng(n)
    out = {}
    out["constant"] = np.full(n, -7, np.int16)                       # every run: one literal, then T_7 with m = 255
    m = [v for k in range(8) for v in ((1 << k) - 1, 1 << k)]       # distance-1 stretches of 2^k - 1 and 2^k matches
    groups = np.repeat(np.arange(len(m)) % 5 + 3 * (np.arange(len(m)) % 2), np.array(m) + 1)
    out["stretches"] = np.tile(groups, n // groups.size + 1)[:n].astype(np.int16)
    out["triple"] = np.tile(np.array([5, -3, 17], np.int16), n // 3 + 1)[:n]
    iid = rng.integers(0, 2111, n)
    if n >= 2:
        iid[0], iid[-1] = 0, 2110                                    # A = 2111 at every size but 1
    out["iid_2111"] = iid.astype(np.int16)
    out["two_symbols"] = rng.integers(0, 2, n).astype(np.int16)
    return out


def _device(pay, offset):
    """The payload in a device buffer that starts `offset` elements behind a 16-byte boundary."""
    import torch
    dev = torch.empty(pay.size + 16, dtype=torch.int16, device="cuda")
    assert dev.data_ptr() % 16 == 0
    view = dev[offset: offset + pay.size]
    view.copy_(torch.from_numpy(pay))
    torch.cuda.synchronize()
    return view


@pytest.mark.parametrize("n", SIZES)
def test_kernels_against_numpy(ctx, n):
    import torch
    from tezip_amd import huffd, huffr
    for name, pay in families(n).items():
        base = int(pay.min())
        A = int(pay.max()) - base + 1
        want3 = huffd.token_counts(pay, base, A)
        if name == "constant":                                       # a literal per run, and T_7 from 128 matches on
            assert want3[1][:A].sum() == (n + 255) // 256 and want3[1][A + 7] == n // 256 + (n % 256 >= 129)
        bodies = {}
        for offset in (0, 1):                                        # 16-byte aligned, and the element-wise path
            dev = _device(pay, offset)
            counts3, gbase = ctx.huffd_counts(dev)
            assert gbase == base and counts3.shape == (3, A + 8), (name, offset)
            assert (counts3 == want3).all(), "%s offset %d: k_huffd_count against the numpy tokeniser" % (name, offset)
            for i, dist in enumerate(huffd.DISTS):
                ln = huffd.lengths_of(counts3[i], dist)
                if (dist, "want") not in bodies:
                    bodies[dist, "want"] = np.frombuffer(huffd.pack_body(*huffd.encode_body(pay, ln, base, dist)), np.uint8)
                want = bodies[dist, "want"]
                got = ctx.huffd_encode_buf(dev, ln, base, dist)
                assert got.size == want.size and (got == want).all(), "%s offset %d D = %d: GPU stream against numpy's" % (name, offset, dist)
                out = torch.zeros(pay.size + 16, dtype=torch.int16, device="cuda")
                ctx.huffd_decode_buf(got, pay.size, ln, base, dist, out=out[offset: offset + pay.size])
                torch.cuda.synchronize()
                res = out.cpu().numpy()
                assert (res[offset: offset + pay.size] == pay).all(), "%s offset %d D = %d: GPU decode" % (name, offset, dist)
                assert not res[:offset].any() and not res[offset + pay.size:].any(), (name, offset, dist)
                if dist == 3:
                    assert (ctx.huffr_encode_buf(dev, ln, base) == got).all(), "%s offset %d: D = 3 is TZR1's stream" % (name, offset)
                    assert (ln == huffr.code_lengths(counts3[2])).all()
                if dist == 0:
                    assert (ctx.huff_encode_buf(pay, ln[:A], base) == got).all(), "%s offset %d: D = 0 is TZH1's stream" % (name, offset)


def test_refusals_and_staged_streams(ctx):
    from tezip_amd import _lib, huffd
    pay = families(3 * 16384 + 77)["stretches"]
    base = int(pay.min())
    counts3, _ = ctx.huffd_counts(pay)
    ln1 = huffd.lengths_of(counts3[1], 1)
    body = ctx.huffd_encode_buf(pay, ln1, base, 1).copy()
    for call in (lambda: ctx.huffd_begin(body.size, pay.size, ln1, base, 2),
                 lambda: ctx.huffd_encode_buf(pay, ln1, base, 2),
                 lambda: ctx.huffd_decode_buf(body, pay.size, ln1, base, -1),
                 lambda: ctx.huffd_decode_buf(body, pay.size, ln1, base, 0),      # token lengths under D = 0
                 lambda: ctx.huffd_begin(body.size, pay.size, ln1, base, 0)):
        with pytest.raises(_lib.TezipError) as e:
            call()
        assert e.value.status == -1                                              # TZ_ERR_INVALID
    ctx.huffd_begin(body.size, pay.size, ln1, base, 1)
    half = body.size // 2
    assert half > 0
    ctx.huffd_put(0, body[:half])
    ctx.huffd_put(half, body[half:])
    for other in (ctx.huffr_decode, ctx.huff_decode):
        with pytest.raises(_lib.TezipError) as e:
            other()                                                              # a TZR2 stream is staged
        assert e.value.status == -4                                              # TZ_ERR_STATE
    ctx.huffd_decode()
    assert (ctx.payload_get(0, pay.size) == pay).all()
    ln3 = huffd.lengths_of(counts3[2], 3)
    body3 = ctx.huffr_encode_buf(pay, ln3, base).copy()
    ctx.huffr_begin(body3.size, pay.size, ln3, base)
    ctx.huffr_put(0, body3)
    with pytest.raises(_lib.TezipError) as e:
        ctx.huffd_decode()                                                       # ... and the other way round
    assert e.value.status == -4
    ctx.huffr_decode()
    assert (ctx.payload_get(0, pay.size) == pay).all()
    fresh = _lib.Context(0)
    for call in (lambda: fresh.huffd_encode(ln1, base, 1), fresh.huffd_counts, fresh.huffd_decode):
        with pytest.raises(_lib.TezipError) as e:                                # no resident payload / nothing staged
            call()
        assert e.value.status == -4
    fresh.close()


# ------------------------------------------------------------------------------------------------------------ the CLI
NT = 10
LINE = re.compile(r"^coder: huffd, match distance (\d) \(bits: none (\d+), 1: (\d+), 3: (\d+)\)$", re.M)


def _read(d, n):
    with open(os.path.join(d, n), "rb") as f:
        return f.read()


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


@pytest.fixture(scope="module")
def jobs(tmp_path_factory):
    from PIL import Image
    from tezip_amd import _lib, synth, weights
    from tezip_amd.prednet import PredNetConfig
    tmp = tmp_path_factory.mktemp("huffd")
    cfg = PredNetConfig(stack_sizes=(3, 16, 32))
    wts = cfg.init_weights(seed=4, bias_scale=0.2)
    out = {}
    for name, frames in (("gray", synth.moving_blobs(NT, 64, 64)), ("colour", synth.translating_scene(NT, 61, 90))):
        mdir, ddir = str(tmp / (name + "_model")), tmp / (name + "_data")
        weights.save_model(mdir, cfg, wts, _lib.pad8(frames.shape[1]), _lib.pad8(frames.shape[2]))
        ddir.mkdir()
        names = ["f_%03d.png" % t for t in range(NT)]
        for t, f in enumerate(frames):
            Image.fromarray(f).save(ddir / names[t])
        out[name] = (mdir, str(ddir), names, frames)
    os.environ.pop("WORLD_SIZE", None)
    return tmp, out


def _check_file(text, huffd_dir, huff_dir):
    """entropy.dat of the huffd job is huffd.encode_file of the payload the huff job of the same flags stored, and the printed
    line is what huffd.choose gives from that payload's counts.  -> the parsed file."""
    from tezip_amd import huff, huffd
    eh, ed = _read(huff_dir, "entropy.dat"), _read(huffd_dir, "entropy.dat")
    assert eh[:4] == b"TZH1" and ed[:4] == b"TZR2"
    pay, ph = huff.decode_file(eh)
    p = huffd.parse(ed)
    assert p.shape == ph.shape and p.warm_up == ph.warm_up and p.base == ph.base
    assert ed == huffd.encode_file(pay, p.table, p.shape, p.warm_up, base=p.base)
    dist, _, costs = huffd.choose(huffd.token_counts(pay, p.base, p.A))
    found = LINE.findall(text)
    assert len(found) == 1 and tuple(int(v) for v in found[0]) == (dist,) + tuple(costs), text
    assert p.dist == dist
    assert (huffd.decode_file(ed)[0] == pay).all()
    return p


def test_cli_lossless_gray_job(jobs, monkeypatch):
    tmp, sets = jobs
    mdir, ddir, names, frames = sets["gray"]
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("TEZIP_NO_STREAMING", raising=False)
    base = ["-p", "0", "-w", "4", "-m", "abs", "-b", "0", "--gray"]
    cd, ch, ud = (str(tmp / k) for k in ("g0_cd", "g0_ch", "g0_ud"))
    code, text = _tezip(["-c", mdir, ddir, cd] + base + ["--coder", "huffd"])
    assert code == 0 and "gray: yes" in text, text
    code, t2 = _tezip(["-c", mdir, ddir, ch] + base + ["--coder", "huff"])
    assert code == 0 and "coder: huffd" not in t2, t2
    p = _check_file(text, cd, ch)
    assert p.shape == (1, NT, 64, 64, 1)
    for n in ("filename.txt", "key_frame.dat"):
        assert _read(cd, n) == _read(ch, n), n
    code, text = _tezip(["-u", mdir, cd, ud])
    assert code == 0, text
    assert sorted(os.listdir(ud)) == names
    from PIL import Image
    for t, nm in enumerate(names):
        assert (np.asarray(Image.open(os.path.join(ud, nm))) == frames[t]).all(), nm   # lossless: the images byte for byte


def test_cli_lossy_gray_job_with_the_other_flags(jobs, monkeypatch):
    from PIL import Image
    tmp, sets = jobs
    mdir, ddir, names, frames = sets["gray"]
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("TEZIP_NO_STREAMING", raising=False)
    base = ["-p", "0", "-w", "4", "-m", "abs", "-b", "2", "--gray"]
    cd, ch, ud, ur = (str(tmp / k) for k in ("g2_cd", "g2_ch", "g2_ud", "g2_ur"))
    code, text = _tezip(["-c", mdir, ddir, cd] + base + ["--coder", "huffd", "--report", "--ssim", "--digests"])
    assert code == 0 and "gray: yes" in text, text
    assert json.loads(_read(cd, "quality.json"))["max_abs_err"] <= 2
    code, _ = _tezip(["-c", mdir, ddir, ch] + base + ["--coder", "huff"])
    assert code == 0
    _check_file(text, cd, ch)
    code, text = _tezip(["-u", mdir, cd, ud, "--verify", "require"])
    assert code == 0 and "verified: %d frames" % NT in text, text
    for t, nm in enumerate(names):
        got = np.asarray(Image.open(os.path.join(ud, nm)))
        assert int(np.abs(got.astype(int) - frames[t].astype(int)).max()) <= 2, nm
    code, text = _tezip(["-u", mdir, cd, ur, "--frames", "3:6", "--verify", "require"])
    assert code == 0, text
    assert sorted(os.listdir(ur)) == names[3:6]
    for nm in names[3:6]:
        assert _read(ur, nm) == _read(ud, nm), nm


def test_cli_colour_job_and_the_whole_array_path(jobs, monkeypatch):
    tmp, sets = jobs
    mdir, ddir, names, frames = sets["colour"]
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("TEZIP_NO_STREAMING", raising=False)
    base = ["-p", "1", "-w", "4", "-m", "abs", "-b", "2", "--key-coder", "huff"]
    cd, ch, ud, uh, us = (str(tmp / k) for k in ("c2_cd", "c2_ch", "c2_ud", "c2_uh", "c2_us"))
    code, text = _tezip(["-c", mdir, ddir, cd] + base + ["--coder", "huffd"])
    assert code == 0, text
    code, _ = _tezip(["-c", mdir, ddir, ch] + base + ["--coder", "huff"])
    assert code == 0
    p = _check_file(text, cd, ch)
    assert p.shape == (1, NT, 61, 90, 3)
    for src, dst in ((cd, ud), (ch, uh)):
        code, text = _tezip(["-u", mdir, src, dst])
        assert code == 0, text
    monkeypatch.setenv("TEZIP_NO_STREAMING", "1")                      # the whole-array path of -u reads the same file
    code, text = _tezip(["-u", mdir, cd, us])
    assert code == 0, text
    for nm in names:
        assert _read(ud, nm) == _read(uh, nm) == _read(us, nm), nm
