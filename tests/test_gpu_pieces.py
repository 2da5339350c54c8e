"""Every `-c` and `-u` moves its data between host and HBM in pieces through small rings of reused host buffers; at the sizes
of the other tests each of those loops runs once.  Here the piece sizes (module constants of tezip_amd/compress.py and
tezip_amd/decompress.py, read when a run starts) are shrunk until every loop iterates, returns to a used ring slot, cuts the
trailer of entropy.dat and ends on a short last piece.  Each such run is held to three references, none of them the code
under test: the ONE-PIECE run of the same job (the constants untouched), the source images, and for the coded files the numpy
decoders of tezip_amd/huff.py, huffr.py and keycoder.py.  The expected number of pieces stands in a comment and is asserted
on the context's calls, so a constant that is no longer read is noticed.

The job is the one of tests/test_gpu_huff.py: 16 frames of synth.translating_scene at 29 x 43 under a (3, 16, 32) model padded
to 32 x 48, `-p 1 -w 4`, lossless (abs 0) and abs 2.  n = 16 * 29 * 43 * 3 = 59 856 payload elements; a frame is fb = 3 741
bytes, a multiple of neither 2 nor 16."""
import collections
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

NT, H, W = 16, 29, 43
FB = H * W * 3                   # 3 741
N = NT * FB                      # 59 856
BOUNDS = [0.0, 2.0]
# the values the piece sizes have when nobody touches them: a one-piece run is a run under these
UNTOUCHED = {("compress", "PAYLOAD_CHUNK"): 8 << 20, ("compress", "KEY_PREFETCH_BYTES"): 256 << 20, ("compress", "HUFF_PIECE"): 16 << 20,
             ("decompress", "PUT_PIECE"): 16 << 20, ("decompress", "FETCH_WINDOW_BYTES"): 16 << 20,
             ("decompress", "PREFETCH_PIECE_BYTES"): 16 << 20, ("decompress", "PREFETCH_DEPTH"): 8}


def _pieces(total, piece):
    return (total + piece - 1) // piece


def _read(d, n):
    with open(os.path.join(d, n), "rb") as f:
        return f.read()


def _mods():
    from tezip_amd import compress, decompress
    return {"compress": compress, "decompress": decompress}


def _same(a, b, what, piece=None):
    """Two byte strings are equal; if not: the first differing byte, and the piece it lies in."""
    if a == b:
        return
    x, y = np.frombuffer(a, np.uint8), np.frombuffer(b, np.uint8)
    m = min(x.size, y.size)
    d = np.nonzero(x[:m] != y[:m])[0]
    at = int(d[0]) if d.size else m
    where = "" if not piece else " (piece %d of %d-byte pieces)" % (at // piece, piece)
    pytest.fail("%s: %d against %d bytes, first difference at byte %d%s, %d bytes differ" % (what, x.size, y.size, at, where, d.size))


class Job:
    def __init__(self, tmp):
        from PIL import Image
        from tezip_amd import synth, weights
        from tezip_amd.prednet import PredNetConfig
        self.tmp = tmp
        cfg = PredNetConfig(stack_sizes=(3, 16, 32))
        wts = cfg.init_weights(seed=4, bias_scale=0.2)
        self.frames = synth.translating_scene(NT, H, W, seed=5)
        self.mdir = str(tmp / "model")
        weights.save_model(self.mdir, cfg, wts, 32, 48)
        ddir = tmp / "data"
        ddir.mkdir()
        self.ddir = str(ddir)
        self.names = ["f_%03d.png" % t for t in range(NT)]
        for t in range(NT):
            Image.fromarray(self.frames[t]).save(ddir / self.names[t])
        self.refs = {}
        self.seq = 0

    def path(self, tag):
        self.seq += 1
        return str(self.tmp / ("%s_%03d" % (tag, self.seq)))

    def c(self, bound, coder="zstd", key_coder="zstd", entropy=True, window=4, tag="c"):
        from tezip_amd import compress
        out = self.path(tag)
        compress.run(self.mdir, self.ddir, out, 1, window, None, "abs", [bound], True, False, entropy, CODER=coder, KEY_CODER=key_coder)
        return out

    def u(self, cdir, frames=None, tag="u"):
        from tezip_amd import decompress
        out = self.path(tag)
        decompress.run(self.mdir, cdir, out, True, False, frames=frames)
        return out

    def _untouched(self, fn):
        """fn() with every piece size at its untouched value and the early rollout on, whatever the calling test has set."""
        mods = _mods()
        saved = {k: getattr(mods[k[0]], k[1]) for k in UNTOUCHED}
        env = os.environ.pop("TEZIP_NO_EARLY_ROLLOUT", None)
        try:
            for k, v in UNTOUCHED.items():
                setattr(mods[k[0]], k[1], v)
            return fn()
        finally:
            for k, v in saved.items():
                setattr(mods[k[0]], k[1], v)
            if env is not None:
                os.environ["TEZIP_NO_EARLY_ROLLOUT"] = env

    def ref_c(self, bound, coder="zstd", key_coder="zstd", entropy=True, window=4):
        """The one-piece `-c` of a job (made once, never changed)."""
        key = ("c", bound, coder, key_coder, entropy, window)
        if key not in self.refs:
            self.refs[key] = self._untouched(lambda: self.c(bound, coder, key_coder, entropy, window, tag="ref_c"))
        return self.refs[key]

    def ref_u(self, bound, coder="zstd", key_coder="zstd", entropy=True, window=4):
        """The one-piece `-u` of the one-piece `-c`, itself checked against the source images."""
        key = ("u", bound, coder, key_coder, entropy, window)
        if key not in self.refs:
            cdir = self.ref_c(bound, coder, key_coder, entropy, window)
            self.refs[key] = self._untouched(lambda: self.u(cdir, tag="ref_u"))
            self.against_source(self.refs[key], bound)
        return self.refs[key]

    def against_source(self, udir, bound, lo=0, hi=NT):
        """Reference 2: lossless restores the source exactly, abs 2 within 2 at every sample."""
        from PIL import Image
        assert sorted(os.listdir(udir)) == self.names[lo:hi]
        for t in range(lo, hi):
            img = np.array(Image.open(os.path.join(udir, self.names[t])))
            assert img.shape == (H, W, 3) and img.dtype == np.uint8
            err = int(np.abs(img.astype(np.int64) - self.frames[t].astype(np.int64)).max())
            assert err <= int(bound), "frame %d of %s: worst sample error %d, bound %g" % (t, udir, err, bound)

    def payload(self, bound, entropy=True):
        """(payload, table | None) of the one-piece zstd run."""
        from tezip_amd import decompress, zstd
        pay, tab, shape, p = decompress.parse_stream(zstd.decompress(_read(self.ref_c(bound, entropy=entropy), "entropy.dat")))
        assert shape == (1, NT, H, W, 3) and p == 1 and pay.size == N
        return pay, tab

    def key_stack(self, bound, window=4):
        """The zero-except-keys stack, built from the SOURCE frames at the key indices of the one-piece zstd run."""
        from tezip_amd import zstd
        got = np.frombuffer(zstd.decompress(_read(self.ref_c(bound, window=window), "key_frame.dat")), np.uint8).reshape(NT, H, W, 3)
        idx = np.nonzero(got.reshape(NT, -1).any(axis=1))[0]
        want = np.zeros_like(self.frames)
        want[idx] = self.frames[idx]
        assert (got == want).all() and idx.size >= (NT if window == 1 else 4)
        return want, idx

    def same_compressed(self, cdir, ref, piece=None):
        """Reference 1 for a `-c`: coded files, filename.txt and tezip_amd.json byte for byte, zstd files by content."""
        from tezip_amd import zstd
        assert sorted(os.listdir(cdir)) == sorted(os.listdir(ref))
        for n in ("filename.txt", "tezip_amd.json"):
            _same(_read(cdir, n), _read(ref, n), n)
        for n in ("entropy.dat", "key_frame.dat"):
            a, b = _read(cdir, n), _read(ref, n)
            assert a[:4] == b[:4], n
            if a[:4] in (b"TZH1", b"TZR1", b"TZK1"):
                _same(a, b, n, piece)
            else:
                _same(zstd.decompress(a), zstd.decompress(b), n + " (decompressed)", piece)

    def coded_against_numpy(self, cdir, bound, window=4):
        """Reference 3: the numpy decoders of the coded files against the zstd run's payload and the key stack."""
        from tezip_amd import huff, huffr, keycoder
        e, k = _read(cdir, "entropy.dat"), _read(cdir, "key_frame.dat")
        fmt = {b"TZH1": huff, b"TZR1": huffr}.get(e[:4])
        if fmt is not None:
            pay, tab = self.payload(bound)
            dec, parsed = fmt.decode_file(e, key_len=N)
            assert (dec == pay).all() and (parsed.table == tab).all() and parsed.warm_up == 1
        if k[:4] == b"TZK1":
            want, idx = self.key_stack(bound, window)
            assert keycoder.parse(k).idx.tolist() == idx.tolist() and (keycoder.decode_file(k) == want).all()
        return fmt is not None or k[:4] == b"TZK1"

    def same_images(self, udir, ref, bound, lo=0, hi=NT):
        """References 1 and 2 for a `-u`."""
        assert sorted(os.listdir(udir)) == self.names[lo:hi]
        for n in self.names[lo:hi]:
            _same(_read(udir, n), _read(ref, n), n)
        self.against_source(udir, bound, lo, hi)


@pytest.fixture(scope="module")
def job(tmp_path_factory):
    mods = _mods()
    for (m, name), v in UNTOUCHED.items():
        assert getattr(mods[m], name) == v, "%s.%s" % (m, name)
    return Job(tmp_path_factory.mktemp("pieces"))


@pytest.fixture(autouse=True)
def _plain_env(monkeypatch):
    for v in ("WORLD_SIZE", "TEZIP_NO_STREAMING", "TEZIP_NO_EARLY_ROLLOUT", "TEZIP_TIMING"):
        monkeypatch.delenv(v, raising=False)


@pytest.fixture
def calls(monkeypatch):
    """Counts the context's piece calls, so that the piece counts in the comments below are asserted and not only claimed."""
    from tezip_amd import _lib
    counter = collections.Counter()
    for name in ("payload_get", "payload_put", "huff_get", "huff_put", "huffr_put", "keys_get", "keys_put", "frames_get", "frames_put",
                 "decoded_get"):
        def wrap(self, *a, _orig=getattr(_lib.Context, name), _name=name, **k):
            counter[_name] += 1
            return _orig(self, *a, **k)
        monkeypatch.setattr(_lib.Context, name, wrap)
    return counter


# --------------------------------------------------------------------------------------------------------------- -c
@pytest.mark.parametrize("bound", BOUNDS)
def test_c_zstd_payload_in_pieces(job, monkeypatch, calls, bound):
    """compress._stream_outputs, payload_get pieces of PAYLOAD_CHUNK elements into bufs[k % 2].  n = 59 856:
    chunk n -> 1 piece; n - 1 -> 2, the last of one element; 8 190 -> 8 pieces at offsets 12 bytes off a 16-byte boundary
    (7 * 8 190 + 2 526), each buffer used four times; 20 000 -> 3 (2 * 20 000 + 19 856)."""
    from tezip_amd import compress
    ref = job.ref_c(bound)
    last = None
    for chunk, want in ((N, 1), (N - 1, 2), (8190, 8), (20000, 3)):
        monkeypatch.setattr(compress, "PAYLOAD_CHUNK", chunk)
        calls.clear()
        last = job.c(bound)
        assert calls["payload_get"] == want == _pieces(N, chunk)
        job.same_compressed(last, ref, piece=2 * chunk)
    monkeypatch.setattr(compress, "PAYLOAD_CHUNK", UNTOUCHED["compress", "PAYLOAD_CHUNK"])
    job.same_images(job.u(last), job.ref_u(bound), bound)


@pytest.mark.parametrize("bound", BOUNDS)
@pytest.mark.parametrize("which", ["huff", "huffr", "key"])
def test_c_coded_stream_in_pieces(job, monkeypatch, calls, bound, which):
    """compress._huff_entropy_file (--coder huff / huffr) and _huff_key_file (--key-coder huff), huff_get / keys_get pieces of
    HUFF_PIECE bytes into bufs[k % 2].  With S the coded stream's bytes in the one-piece file (tens of KB): 1 000 ->
    ceil(S / 1000) pieces, 4 097 -> ceil(S / 4097), every one but the first at an odd offset, S - 1 -> 2, the last of one byte."""
    from tezip_amd import compress, huff, huffr, keycoder
    coder, key_coder = (which, "zstd") if which != "key" else ("zstd", "huff")
    ref = job.ref_c(bound, coder, key_coder)
    if which == "key":
        S, get = keycoder.parse(_read(ref, "key_frame.dat")).body.size, "keys_get"
    else:
        S, get = {"huff": huff, "huffr": huffr}[which].parse(_read(ref, "entropy.dat")).body.size, "huff_get"
    assert S > 2 * 4097                                                  # at least three pieces of 4 097, nine of 1 000
    assert job.coded_against_numpy(ref, bound)
    last = None
    for piece in (1000, 4097, S - 1):
        monkeypatch.setattr(compress, "HUFF_PIECE", piece)
        calls.clear()
        last = job.c(bound, coder, key_coder)
        assert calls[get] == _pieces(S, piece) >= 2 and calls["huff_get"] + calls["keys_get"] == calls[get]
        job.same_compressed(last, ref, piece)
        assert job.coded_against_numpy(last, bound)
    monkeypatch.setattr(compress, "HUFF_PIECE", UNTOUCHED["compress", "HUFF_PIECE"])
    job.same_images(job.u(last), job.ref_u(bound, coder, key_coder), bound)


@pytest.mark.parametrize("bound", BOUNDS)
def test_c_key_frames_one_by_one(job, monkeypatch, calls, bound):
    """compress._stream_outputs, third branch: with KEY_PREFETCH_BYTES = 0 every key frame is fetched when the compressor
    reaches it (frames_get once per key frame: 16 with -w 1, where every frame is one), and key_frame.dat holds what the
    prefetch branch's holds."""
    from tezip_amd import compress, zstd
    for window in (4, 1):
        ref = job.ref_c(bound, window=window)
        want, idx = job.key_stack(bound, window)
        assert window != 1 or idx.size == NT
        monkeypatch.setattr(compress, "KEY_PREFETCH_BYTES", 0)
        calls.clear()
        got = job.c(bound, window=window)
        assert calls["frames_get"] == idx.size
        monkeypatch.setattr(compress, "KEY_PREFETCH_BYTES", UNTOUCHED["compress", "KEY_PREFETCH_BYTES"])
        job.same_compressed(got, ref, FB)
        _same(zstd.decompress(_read(got, "key_frame.dat")), want.tobytes(), "key_frame.dat against the source frames", FB)
        job.same_images(job.u(got), job.ref_u(bound, window=window), bound)


# --------------------------------------------------------------------------------------------------------------- -u
def _cuts(ent, T):
    """_Prefetch piece bytes that cut the trailer of a stream of `ent` bytes with a table of T values (T = -1: none)."""
    cuts = [ent - 2,                         # 2 pieces, the last one element: warm_up alone
            ent - 8]                         # 2 pieces, cut inside the seven values T | shape | warm_up
    if T >= 0:
        cuts += [ent - 2 * (7 + T // 2),     # 2 pieces, cut inside the table
                 ent - 2 * (7 + T)]          # 2 pieces, cut exactly between payload and table
    return cuts


@pytest.mark.parametrize("bound", BOUNDS)
@pytest.mark.parametrize("early", [True, False])
def test_u_zstd_trailer_cut_by_a_piece(job, monkeypatch, calls, bound, early):
    """decompress._run_streaming: _Prefetch's ring (depth + 2 buffers) into payload_put at running offsets, the trailer
    rebuilt from the last TAIL_ELEMS = 2 119 values of consecutive pieces.  ent = 2 * (n + T + 7) bytes; four piece sizes that
    make 2 pieces and cut the trailer at its four seams (_cuts), then 2 048 bytes with depth 1: ceil(ent / 2048) >= 59
    pieces of 1 024 values -- the tail is assembled from three of them, the ring of 3 buffers is reused about 20 times.
    With the sidecar's early rollout, and without it (the trailer then decides everything)."""
    from tezip_amd import decompress
    cdir, ref = job.ref_c(bound), job.ref_u(bound)
    pay, tab = job.payload(bound)
    ent, T = 2 * (N + len(tab) + 7), len(tab)
    assert T >= 2 and decompress.TAIL_ELEMS == 2119
    if not early:
        monkeypatch.setenv("TEZIP_NO_EARLY_ROLLOUT", "1")
    for piece, depth in [(p, None) for p in _cuts(ent, T)] + [(2048, 1)]:
        monkeypatch.setattr(decompress, "PREFETCH_PIECE_BYTES", piece)
        if depth is not None:
            monkeypatch.setattr(decompress, "PREFETCH_DEPTH", depth)
        calls.clear()
        got = job.u(cdir)
        assert calls["payload_put"] == _pieces(ent, piece) == (2 if depth is None else calls["payload_put"])
        assert depth is None or calls["payload_put"] >= 59
        job.same_images(got, ref, bound)


@pytest.mark.parametrize("bound", BOUNDS)
def test_u_zstd_trailer_without_a_table_cut_by_a_piece(job, monkeypatch, calls, bound):
    """The `-n` job: no table, the trailer is -1 | shape | warm_up, ent = 2 * (n + 7); cut in front of warm_up and inside
    the seven values, with and without the early rollout: 2 pieces each."""
    from tezip_amd import decompress
    cdir, ref = job.ref_c(bound, entropy=False), job.ref_u(bound, entropy=False)
    pay, tab = job.payload(bound, entropy=False)
    assert tab is None
    ent = 2 * (N + 7)
    for early in (True, False):
        if not early:
            monkeypatch.setenv("TEZIP_NO_EARLY_ROLLOUT", "1")
        for piece in _cuts(ent, -1):
            monkeypatch.setattr(decompress, "PREFETCH_PIECE_BYTES", piece)
            calls.clear()
            got = job.u(cdir)
            assert calls["payload_put"] == 2
            job.same_images(got, ref, bound)


@pytest.mark.parametrize("bound", BOUNDS)
def test_u_fetch_windows_wrap_the_ring(job, monkeypatch, calls, bound):
    """decompress._run_streaming: per = FETCH_WINDOW_BYTES // fb frames per window -- key_frame.dat is staged by frames_put in
    pieces of `per` frames, the decoded frames come back by decoded_get into a ring of 3 whose slots the PNG encoders still
    hold.  fb, 2 fb, 5 fb, 5 fb + 1 -> per = 1, 2, 5, 5 -> 16, 8, 4, 4 windows (the ring wraps; with per = 5 the last window
    is one frame).  frames = (3, 9) starts and ends inside windows: per = 4 -> [3, 7) [7, 9), per = 5 -> [3, 8) [8, 9)."""
    from tezip_amd import decompress
    cdir, ref = job.ref_c(bound), job.ref_u(bound)
    for window, want in ((FB, 16), (2 * FB, 8), (5 * FB, 4), (5 * FB + 1, 4)):
        monkeypatch.setattr(decompress, "FETCH_WINDOW_BYTES", window)
        calls.clear()
        got = job.u(cdir)
        assert calls["decoded_get"] == want == _pieces(NT, window // FB) and calls["frames_put"] == want
        job.same_images(got, ref, bound)
    for per in (4, 5):
        monkeypatch.setattr(decompress, "FETCH_WINDOW_BYTES", per * FB)
        calls.clear()
        got = job.u(cdir, frames=(3, 9))
        assert calls["decoded_get"] == 2 and calls["frames_put"] == _pieces(NT, per)
        job.same_images(got, ref, bound, 3, 9)


@pytest.mark.parametrize("bound", BOUNDS)
@pytest.mark.parametrize("coder", ["huff", "huffr"])
def test_u_coded_bodies_in_pieces(job, monkeypatch, calls, bound, coder):
    """decompress._run_streaming and stage_coded_keys: huff_put / huffr_put / keys_put of the coded bodies in pieces of
    PUT_PIECE bytes.  Bodies of S (entropy.dat) and K (key_frame.dat) bytes: 1 000 -> ceil(S / 1000) and ceil(K / 1000)
    pieces, 4 097 -> ceil(S / 4097) and ceil(K / 4097), every later offset odd."""
    from tezip_amd import decompress, huff, huffr, keycoder
    fmt, put = {"huff": (huff, "huff_put"), "huffr": (huffr, "huffr_put")}[coder]
    for key_coder in ("zstd", "huff"):
        cdir, ref = job.ref_c(bound, coder, key_coder), job.ref_u(bound, coder, key_coder)
        assert job.coded_against_numpy(cdir, bound)
        S = fmt.parse(_read(cdir, "entropy.dat")).body.size
        K = keycoder.parse(_read(cdir, "key_frame.dat")).body.size if key_coder == "huff" else 0
        for piece in (1000, 4097):
            monkeypatch.setattr(decompress, "PUT_PIECE", piece)
            calls.clear()
            got = job.u(cdir)
            assert calls[put] == _pieces(S, piece) >= 2 and calls["keys_put"] == _pieces(K, piece) and (K == 0 or calls["keys_put"] >= 2)
            job.same_images(got, ref, bound)
        monkeypatch.setattr(decompress, "PUT_PIECE", UNTOUCHED["decompress", "PUT_PIECE"])


# ------------------------------------------------------------------------------------------- everything small, poisoned
SMALL = [("compress", "PAYLOAD_CHUNK", 8190), ("compress", "KEY_PREFETCH_BYTES", 0), ("compress", "HUFF_PIECE", 1000),
         ("decompress", "PUT_PIECE", 1000), ("decompress", "FETCH_WINDOW_BYTES", 2 * FB), ("decompress", "PREFETCH_PIECE_BYTES", 2048),
         ("decompress", "PREFETCH_DEPTH", 1)]

_POISON_SCRIPT = r"""
import json
import sys
sys.path.insert(0, %r)
from tezip_amd import compress, decompress
plan = json.load(open(sys.argv[1]))
mods = {"compress": compress, "decompress": decompress}
for m, name, value in plan["set"]:
    assert hasattr(mods[m], name), name
    setattr(mods[m], name, value)
for j in plan["jobs"]:
    compress.run(plan["model"], plan["data"], j["c"], 1, 4, None, "abs", [j["bound"]], True, False, True, CODER=plan["coder"],
                 KEY_CODER=plan["key_coder"])
    decompress.run(plan["model"], j["c"], j["u"], True, False)
print("pieces ok")
"""


@pytest.mark.parametrize("coder", ["zstd", "huff", "huffr"])
def test_all_pieces_small_under_poison(job, tmp_path, coder):
    """`-c` then `-u` with every piece size small at once (SMALL: 8 payload_get pieces, key frames one by one, coded streams
    and bodies in 1 000-byte pieces, 59 or more _Prefetch pieces through a ring of 3, 8 fetch windows) in a fresh process
    under TEZIP_POISON=0xA5, which fills every device buffer handed out before its use: stale bytes in a reused buffer or a
    skipped piece cannot give the one-piece run's files.  The Huffman coders run with --key-coder huff."""
    key_coder = "zstd" if coder == "zstd" else "huff"
    plan = dict(model=job.mdir, data=job.ddir, coder=coder, key_coder=key_coder, set=SMALL,
                jobs=[dict(bound=b, c=job.path("poison_c"), u=job.path("poison_u")) for b in BOUNDS])
    (tmp_path / "plan.json").write_text(json.dumps(plan))
    script = tmp_path / "pieces_job.py"
    script.write_text(_POISON_SCRIPT % ROOT)
    env = dict(os.environ, TEZIP_POISON="0xA5")
    for v in ("WORLD_SIZE", "TEZIP_NO_STREAMING", "TEZIP_NO_EARLY_ROLLOUT"):
        env.pop(v, None)
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, str(script), str(tmp_path / "plan.json")], cwd=ROOT,
                       capture_output=True, text=True, env=env, timeout=330)
    assert r.returncode == 0 and "pieces ok" in r.stdout, r.stdout + r.stderr
    for j in plan["jobs"]:
        job.same_compressed(j["c"], job.ref_c(j["bound"], coder, key_coder), 1000)
        job.coded_against_numpy(j["c"], j["bound"])
        job.same_images(j["u"], job.ref_u(j["bound"], coder, key_coder), j["bound"])
