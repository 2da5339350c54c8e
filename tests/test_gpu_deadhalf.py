"""Dead halves of the error maps (-m gpu).  Where the per-model constant Ahat0_l is +-0 over the whole plane (measured at
every prepare), E_l = [relu(Ahat0 - a) | relu(a - Ahat0)] over a >= +0 is [+0 | a] bit for bit, and the LDS-DMA writers of
E_l -- the POOL_ERR epilogues of k_conv16b (A_0) and k_wino (A_1, A_2), the e0_out epilogue of k_conv_small -- load no Ahat0,
subtract nothing and store the live half alone; the dead half keeps the +0 tz_model_prepare filled it with (DESIGN.md
section 5).  TEZIP_DEADHALF=0: both halves computed and stored, as before.

Every case runs tests/deadhalf_jobs.py's job under TZ-PA2 and compares predictions, rollout and the E / R taps of every level
after one step, after three steps and behind a rollout of windows of three, as bit patterns."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (ROOT, os.path.join(ROOT, "tests")):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

import pytest  # noqa: E402

import dead0_models as D  # noqa: E402
import deadhalf_jobs as J  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = [(hp, wp, b) for hp, wp in J.SIZES for b in (1, 3)]


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in J.ENV:
        monkeypatch.delenv(k, raising=False)


def _dead_halves_are_plus_zero(out, cfg):
    for pre in ("", "a", "q"):
        for l in range(cfg.nb_layers):
            e = out[pre + "e%d" % l]
            c = e.shape[-1] // 2
            assert (D.bits(e[..., :c]) == 0).all(), (pre, l)
            assert np.abs(e[..., c:]).max() > 0, (pre, l)          # (the live half is not a plane of zeros)


def _check(spec, dead=True):
    cfg = D.model(spec)[0]
    # the job with the skip on, then the unskipped kernels in the SAME context: they read zeros where nothing was stored
    on, gen = J.run_job(spec, impls=(1, 0))
    off, = J.run_job(spec, TEZIP_DEADHALF=0)
    J.same_bits(on, off, "against TEZIP_DEADHALF=0", cfg)
    J.same_bits(on, gen, "tz_set_conv_impl(0) behind steps taken with the skip on", cfg)
    J.same_bits(on, J.oracle(spec), "against the C oracle", cfg, rollout_taps=False)
    if dead:
        _dead_halves_are_plus_zero(on, cfg)
        _dead_halves_are_plus_zero(off, cfg)
    return on


@pytest.mark.parametrize("hp,wp,batch", CASES)
def test_zero_bias_model_of_the_bench_shape(hp, wp, batch):
    _check(D.spec("zero", hp, wp, batch))


@pytest.mark.parametrize("hp,wp,batch", CASES)
def test_small_model(hp, wp, batch):
    """(3, 16, 32): A_0 at one column tile of k_conv16b."""
    _check(D.spec("zero", hp, wp, batch, shape=D.SMALL, seed=13))


def test_the_log_names_the_levels(capfd):
    spec = D.spec("zero", 64, 64, 1)
    capfd.readouterr()
    J.run_job(spec, TEZIP_DEADHALF_LOG=1)
    err = capfd.readouterr().err
    for l in range(4):
        assert "[tezip] dead half, level %d: Ahat0 +-0 over the whole plane: yes" % l in err, err[-1500:]
    J.run_job(spec)
    assert "dead half" not in capfd.readouterr().err               # nothing is printed unless asked


@pytest.mark.parametrize("hp,wp,batch", [(64, 64, 3), (48, 80, 1)])
def test_biased_model_has_no_dead_half(hp, wp, batch, capfd):
    spec = D.spec("bias", hp, wp, batch, seed=31)
    capfd.readouterr()
    J.run_job(spec, TEZIP_DEADHALF_LOG=1)
    err = capfd.readouterr().err
    assert "dead half, level 0" in err and "plane: yes" not in err, err[-1500:]
    on = _check(spec, dead=False)
    assert all(np.abs(on["e%d" % l][..., : on["e%d" % l].shape[-1] // 2]).max() > 0 for l in range(4))


def test_the_zero_fill_belongs_to_prepare():
    """One context prepared at 64 x 64, run, then prepared at 48 x 80: the second size's maps are new allocations, and their
    dead halves must read +0 just the same."""
    spec = D.spec("zero", 64, 64, 3)
    spec2 = D.spec("zero", 48, 80, 3)
    cfg = D.model(spec)[0]
    _, second = J.run_job(spec, then=(48, 80))
    off, = J.run_job(spec2, TEZIP_DEADHALF=0)
    J.same_bits(second, off, "re-prepared at 48 x 80 against a fresh context with TEZIP_DEADHALF=0", cfg)
    _dead_halves_are_plus_zero(second, cfg)


def test_cli_round_trip_64(tmp_path, monkeypatch):
    """-c then -u of a 64 x 64 job with the zero-bias model: every file of the compressed directory and every decoded frame
    is the same with the skip on and off."""
    from PIL import Image
    from tezip_amd import compress, decompress, synth, weights
    from tezip_amd.prednet import PredNetConfig
    cfg = PredNetConfig()
    mdir = str(tmp_path / "model")
    weights.save_model(mdir, cfg, cfg.init_weights(seed=123), 64, 64)
    frames = synth.translating_scene(7, 64, 64, seed=31)
    ddir = tmp_path / "data"
    ddir.mkdir()
    for t in range(frames.shape[0]):
        Image.fromarray(frames[t], mode="RGB").save(ddir / ("frame_%03d.png" % t))
    got = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("TEZIP_DEADHALF", mode)
        cdir, udir = str(tmp_path / ("comp" + mode)), str(tmp_path / ("out" + mode))
        compress.run(mdir, str(ddir), cdir, 0, 3, None, "abs", [0.0], True, False, True)
        decompress.run(mdir, cdir, udir, True, False)
        got[mode] = ({f: open(os.path.join(cdir, f), "rb").read() for f in sorted(os.listdir(cdir))},
                     np.stack([np.array(Image.open(os.path.join(udir, "frame_%03d.png" % t))) for t in range(7)]))
    assert sorted(got["1"][0]) == sorted(got["0"][0]) and got["1"][0], sorted(got["1"][0])
    for f in got["1"][0]:
        assert got["1"][0][f] == got["0"][0][f], f
    np.testing.assert_array_equal(got["1"][1], got["0"][1])
    np.testing.assert_array_equal(got["1"][1], frames)               # (lossless: the output is the input)
