"""Uniform per-model constants (-m gpu): G0_l, C0_l and Ahat0_l come from the t = 0 pass over an all-zero input.
tz_model_prepare MEASURES where they are one value per column (k_uniform_ring: every pixel against the centre pixel, bit for
bit -> a ring width per array and level) and where they repeat tile by tile (every pixel against the reference tile), and
k_wino takes that one row, or the reference tile, instead of the tile's own per-pixel loads of G0_l and C0_l inside the
ring (tz_prednet.hip measure_uniform, ConvArgs::init_u / aux_u / init_tring / aux_tring).  On such a tile the substitute IS
the array's value, so nothing may change: every case runs a few predictor steps under TZ-PA2 through the C ABI and compares
predictions and per-level taps BIT FOR BIT with (a) the C oracle and (b) the same job in a child process with
TEZIP_UNIFORM=0 (the per-pixel loads everywhere).  Cases that look at the measured rings run the job in a fresh child with
TEZIP_UNIFORM_LOG=1 and parse its stderr."""
import functools
import json
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import pytest  # noqa: E402

from tezip_amd.prednet import PredNetConfig  # noqa: E402

pytestmark = pytest.mark.gpu

DEFAULT = ((3, 48, 96, 192), None)
OTHER = ((3, 32, 64), (3, 48, 32))      # R_stack_sizes != stack_sizes: 48-column A blocks (NT = 3), as tests/test_gpu_wino.py
SATURATED_SIZE = 256                    # the smallest size of this file: its log reports uniform tiles for S4 and S16 there
LOG_LINE = re.compile(r"uniform constants, level (\d+) (G0|C0|Ahat0) \((\d+)x(\d+)\): w (-?\d+), 16x16 tiles (\d+) uniform (\d+) non-uniform")


def _spec(hp, wp, batch, bias, shape=DEFAULT, gain=1.0, seed=123):
    """A job: `batch` windows, so many frames that the last call is a batch of one (whose taps the library holds).  `gain`
    multiplies every weight array (tests/regimes.py: the saturated models)."""
    return (shape, float(bias), hp, wp, batch, 3 if batch == 1 else batch + 1, float(gain), int(seed))


def regime_spec(regime):
    """A saturated model of tests/regimes.py at SATURATED_SIZE."""
    import regimes
    bias, gain = regimes.REGIMES[regime]
    return _spec(SATURATED_SIZE, SATURATED_SIZE, 1, bias, gain=gain, seed=regimes.SEED)


def _model(spec):
    (stack, rstack), bias, hp, wp, _, n, gain, seed = spec
    cfg = PredNetConfig(stack_sizes=stack, R_stack_sizes=rstack)
    w = cfg.init_weights(seed=seed, bias_scale=bias)
    if gain != 1.0:
        from regimes import scaled
        w = scaled(w, gain)
    frames = np.random.default_rng(hp * 31 + wp).integers(0, 256, (n, hp, wp, 3)).astype(np.float32) / np.float32(255)
    return cfg, w, frames


def _names(cfg):
    return ["pred"] + ["e%d" % l for l in range(cfg.nb_layers)] + ["r%d" % l for l in range(cfg.nb_layers)]


def run_job(spec):
    """The job on the GPU, in this process: predictions of all frames, the taps of the last one, k_wino launches."""
    from tezip_amd import _lib
    cfg, w, frames = _model(spec)
    c = _lib.Context(0)
    try:
        c.set_contract(2)
        c.load_model(cfg, w)
        c.prepare(spec[2], spec[3], max_batch=spec[4])
        c.prof_enable(True)
        c.prof_reset()
        out = {"pred": c.predict_next(frames)}
        out["n_wino"] = np.array(c.prof_get()["wino_pa2"][1])
        c.prof_enable(False)
        for l in range(cfg.nb_layers):
            out["e%d" % l] = c.predict_tap(0, l)
            out["r%d" % l] = c.predict_tap(1, l)
    finally:
        c.close()
    return out


def _child(spec, tmp_path, tag, **env):
    """The same job in a fresh process with `env` set: (results, stderr)."""
    out = str(tmp_path / (tag + ".npz"))
    e = dict(os.environ)
    for k in ("TEZIP_UNIFORM", "TEZIP_UNIFORM_LOG", "TEZIP_EPART"):
        e.pop(k, None)
    e.update({k: str(v) for k, v in env.items()})
    r = subprocess.run([sys.executable, os.path.abspath(__file__), json.dumps(spec), out], env=e, cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    with np.load(out) as z:
        return {k: z[k] for k in z.files}, r.stderr


@functools.lru_cache(maxsize=None)
def _oracle(spec):
    """Computed once per (model, size, frames); shared by the cases over the same job and never written to."""
    from oracle import coracle
    cfg, w, frames = _model(spec)
    net = coracle.CPredNet(w, cfg.stack_sizes, cfg.R_stack_sizes, spec[2], spec[3]).set_contract(2)
    pred = np.empty_like(frames)
    for i in range(len(frames) - 1):
        pred[i] = net.next(frames[i])
    pred[-1], dbg = net.next(frames[-1], debug=True)
    ref = {"pred": pred}
    for l in range(cfg.nb_layers):
        ref["e%d" % l], ref["r%d" % l], ref["c%d" % l] = dbg["e"][l], dbg["r"][l], dbg["c"][l]
    for v in ref.values():
        v.setflags(write=False)
    return ref


def _same(got, want, what, cfg):
    for k in _names(cfg):
        np.testing.assert_array_equal(got[k], want[k], err_msg="%s: %s" % (what, k))


def _check(spec, got, tmp_path, **env):
    """(a) against the C oracle, (b) against a child process that never takes the shortcut."""
    cfg = _model(spec)[0]
    oracle_spec = spec[:4] + (1,) + spec[5:]          # (the oracle has no batches)
    _same(got, _oracle(oracle_spec), "against the C oracle", cfg)
    off, _ = _child(spec, tmp_path, "off", TEZIP_UNIFORM=0, **env)
    _same(got, off, "against TEZIP_UNIFORM=0", cfg)
    return off


def _log(stderr):
    rows = {(int(m[1]), m[2]): dict(H=int(m[3]), W=int(m[4]), w=int(m[5]), uniform=int(m[6]), other=int(m[7]))
            for m in (LOG_LINE.search(ln) for ln in stderr.splitlines()) if m}
    assert rows, stderr[-1500:]
    return rows


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ("TEZIP_UNIFORM", "TEZIP_UNIFORM_LOG", "TEZIP_EPART"):
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("batch", [1, 3])
def test_biased_model_256(batch, tmp_path):
    """Levels 1 and 2 have 8 x 8 and 4 x 4 tiles, level 3 (2 x 2 tiles) has border tiles only.  B = 3: the items of a batch
    share the constants."""
    spec = _spec(256, 256, batch, 0.1)
    _check(spec, run_job(spec), tmp_path)


def test_biased_model_384_has_both_kinds_of_tiles_at_every_level(tmp_path):
    """The smallest square at which level 3 (48 x 48) has an interior tile: every k_wino launch mixes both kinds of tiles.
    The log assertions are the issue's: a shortcut tile and a per-pixel tile for G0 at EVERY level, 0 < w <= 16 for G0 and
    Ahat0.  With biases only level 3 is ONE value away from the border (w 1; C0: 0); at levels 2, 1, 0 the collapsed taps of
    the upsampled source make the interior repeat with period 2, 4, 8, and the tiles there qualify because they equal the
    reference tile (`repeating tiles: w` of the log line; expected 2, 4, 8 for G0 and Ahat0)."""
    spec = _spec(384, 384, 1, 0.1)
    got, err = _child(spec, tmp_path, "on", TEZIP_UNIFORM_LOG=1)
    _check(spec, got, tmp_path)
    rows = _log(err)
    for key in sorted(rows):
        print("level %d %s: %r" % (key + (rows[key],)))
    for l in reversed(range(4)):
        g0 = rows[(l, "G0")]
        assert g0["uniform"] >= 1 and g0["other"] >= 1, (l, g0)
        for k in ("G0", "Ahat0"):
            assert 0 < rows[(l, k)]["w"] <= 16, (l, k, rows[(l, k)])
        assert -1 <= rows[(l, "C0")]["w"] <= 16, (l, rows[(l, "C0")])


def test_ragged_biased_model_264x280(tmp_path):
    """Levels 132 x 140, 66 x 70, 33 x 35: cut tiles at the right and bottom edges and an odd top level.  A tile that touches
    an edge of the plane never qualifies, a cut one least of all."""
    spec = _spec(264, 280, 1, 0.1)
    got, err = _child(spec, tmp_path, "on", TEZIP_UNIFORM_LOG=1)
    _check(spec, got, tmp_path)
    for (l, k), row in _log(err).items():
        ty, tx = (row["H"] + 15) // 16, (row["W"] + 15) // 16
        print("level %d %s: %r" % (l, k, row))
        assert row["uniform"] + row["other"] == ty * tx
        if k != "C0":                                           # (C0 of the top level is the biases alone: w = 0)
            assert row["w"] != 0, (l, k, row)                   # zero padding reaches G0 and Ahat0 of every level
        if row["w"] > 0:
            assert row["uniform"] <= max(ty - 2, 0) * max(tx - 2, 0), (l, k, row)
        if row["w"] < 0:
            assert row["uniform"] == 0, (l, k, row)


def test_zero_bias_model_is_uniform_everywhere(tmp_path):
    """The bench's model: every constant is 0 over the whole plane -- w = 0, border tiles take the shortcut as well."""
    spec = _spec(256, 256, 1, 0.0)
    got, err = _child(spec, tmp_path, "on", TEZIP_UNIFORM_LOG=1)
    _check(spec, got, tmp_path)
    rows = _log(err)
    assert len(rows) == 12
    for key, row in rows.items():
        assert row["w"] == 0 and row["other"] == 0 and row["uniform"] == (row["H"] // 16) * (row["W"] // 16), (key, row)


@pytest.mark.parametrize("epart", [1, 0])
def test_split_gate_launches(epart, tmp_path, monkeypatch):
    """'E-part ahead' forced on (levels 1 and 2, whose constants repeat tile by tile): the side launch <4, EPI_RAW, false>
    starts from G0's reference tile, the launch on the critical path from P_l (per item: never a shortcut) and still takes
    the cell state from the reference tile.  Forced off: the fused launch."""
    monkeypatch.setenv("TEZIP_EPART", str(epart))
    spec = _spec(256, 256, 1, 0.1)
    got = run_job(spec)
    assert got["n_wino"] == (7 if epart else 5) * 3, got["n_wino"]
    off = _check(spec, got, tmp_path, TEZIP_EPART=epart)
    assert off["n_wino"] == got["n_wino"]


def test_model_with_other_r_stack_sizes(tmp_path):
    spec = _spec(256, 256, 1, 0.1, OTHER)
    _check(spec, run_job(spec), tmp_path)


@pytest.mark.parametrize("regime", ["S4", "S16"])
def test_saturated_model_keeps_its_uniform_tiles(regime, tmp_path):
    """The models of tests/regimes.py (every weight array times 4 / 16): G0 and C0 hold clipped gates and cell states past
    tanh's polynomial branch, the per-frame values the clamp of Ahat_0.  k_uniform_ring compares bits, so it must measure
    such constants as well as any: the default run, the run with per-pixel loads everywhere and the C oracle agree in every
    BIT (a zero of the other sign would be a difference), and the log still reports shortcut tiles -- the substitute path
    is what ran."""
    from regimes import assert_same_bits
    spec = regime_spec(regime)
    cfg = _model(spec)[0]
    got, err = _child(spec, tmp_path, "on", TEZIP_UNIFORM_LOG=1)
    off = _check(spec, got, tmp_path)
    want = _oracle(spec[:4] + (1,) + spec[5:])
    for k in _names(cfg):
        assert_same_bits(got[k], want[k], "%s against the C oracle: %s" % (regime, k))
        assert_same_bits(got[k], off[k], "%s against TEZIP_UNIFORM=0: %s" % (regime, k))
    assert (want["pred"] == 1.0).any() and (want["pred"] == 0.0).any()
    rows = _log(err)
    for key in sorted(rows):
        print("level %d %s: %r" % (key + (rows[key],)))
    assert sum(row["uniform"] for row in rows.values()) >= 1, rows
    assert any(rows[(l, "G0")]["uniform"] >= 1 for l in range(cfg.nb_layers)), rows


if __name__ == "__main__":   # the child process of _child: the job named on the command line, results into an .npz
    spec_ = json.loads(sys.argv[1])
    spec_ = (tuple(tuple(s) if s is not None else None for s in spec_[0]),) + tuple(spec_[1:])
    np.savez(sys.argv[2], **run_job(spec_))
