"""Dead forget gates (-m gpu): the LSTM update of a gate convolution is c = f * c_prev + i * g, and c_prev is the per-model
constant C0_l.  Where every word of C0_l is +0, f * c_prev is +0 for every f that is not NaN and c = (+0) + i * g: the
k_wino gate launches of the level, fused or split, take a stage image packed WITHOUT the forget-gate columns -- three column
tiles instead of four, EPI_LSTM3 / EPI_RAW3 (tz_prednet.hip measure_deadf / launch_wino; tests/test_deadf_oracle.py states the lemma on the C oracle).
tz_model_prepare MEASURES the property; nothing is assumed.

Every case runs a few predictor steps under TZ-PA2 (set_contract(2)) through the C ABI and compares predictions and every
level's E / R taps as BIT PATTERNS with (a) the same job in a fresh child with TEZIP_DEADF=0, (b) tz_set_conv_impl(0) (k_wino_ref,
which keeps four gates) and (c) the C oracle under contract 2.  What was measured is read from the TEZIP_DEADF_LOG=1 lines of a
fresh child and compared with the rule restated on the numpy oracle's C0_l (tests/deadf_models.py)."""
import functools
import json
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (ROOT, os.path.join(ROOT, "tests")):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

import pytest  # noqa: E402

import deadf_models as D  # noqa: E402

pytestmark = pytest.mark.gpu

ENV = ("TEZIP_DEADF", "TEZIP_DEADF_LOG", "TEZIP_DEADSRC", "TEZIP_DEADSRC_LOG", "TEZIP_UNIFORM", "TEZIP_UNIFORM_LOG", "TEZIP_EPART",
       "TEZIP_WINO_IPW")
LOG_LINE = re.compile(r"\[tezip\] dead forget gate, level (\d+): C0 \+0 everywhere: (yes|no), forget-gate columns left out: (yes|no)(?: \((.*)\))?$")


def _names(cfg):
    return ["pred"] + ["e%d" % l for l in range(cfg.nb_layers)] + ["r%d" % l for l in range(cfg.nb_layers)]


def run_job(spec, impl=1):
    """The job on the GPU, in this process: predictions of all frames, the taps of the last one, k_wino launches."""
    from tezip_amd import _lib
    cfg, w, frames = D.model(spec)
    c = _lib.Context(0)
    try:
        c.set_contract(2)
        c.set_conv_impl(impl)
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
    for k in ENV:
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
    cfg, w, frames = D.model(spec)
    net = coracle.CPredNet(w, cfg.stack_sizes, cfg.R_stack_sizes, spec[2], spec[3]).set_contract(2)
    pred = np.empty_like(frames)
    for i in range(len(frames) - 1):
        pred[i] = net.next(frames[i])
    pred[-1], dbg = net.next(frames[-1], debug=True)
    ref = {"pred": pred}
    for l in range(cfg.nb_layers):
        ref["e%d" % l], ref["r%d" % l] = dbg["e"][l], dbg["r"][l]
    for v in ref.values():
        v.setflags(write=False)
    return ref


def _same_bits(got, want, what, cfg):
    for k in _names(cfg):
        np.testing.assert_array_equal(D.bits(got[k]), D.bits(want[k]), err_msg="%s: %s" % (what, k))


def _log(stderr):
    rows = {int(m[1]): dict(zero=m[2] == "yes", out=m[3] == "yes", why=m[4] or "")
            for m in (LOG_LINE.search(ln) for ln in stderr.splitlines()) if m}
    assert rows, stderr[-1500:]
    return rows


def _check_log(spec, rows, rule_spec=None, kept=None):
    """Every level >= 1 has its line; `C0 +0 everywhere` == the rule on the numpy oracle's C0_l; the columns are left out exactly
    there, except at the levels `kept` names ({level: part of the reason the line must give})."""
    cfg = D.model(spec)[0]
    exp = D.c0_is_plus_zero(rule_spec or spec)
    assert set(rows) == set(range(1, cfg.nb_layers)), rows
    for l, row in sorted(rows.items()):
        print("level %d: %r" % (l, row))
        assert row["zero"] == exp[l], (l, row, exp)
        if kept and l in kept:
            assert not row["out"] and kept[l] in row["why"], (l, row)
        else:
            assert row["out"] == row["zero"], (l, row)
            assert ("3 of 4 column tiles" in row["why"]) == row["out"], (l, row)
    return exp


def _check(spec, tmp_path, ref_impl=True, oracle=True, rule_spec=None, kept=None, **env):
    """(The children run the fused step, TEZIP_EPART=0: whether a batch size splits is otherwise MEASURED per prepared model,
    and the launch counts below would compare two measurements.  The split form: test_forced_split_on_the_zero_bias_model.)"""
    cfg = D.model(spec)[0]
    env.setdefault("TEZIP_EPART", 0)
    on, err = _child(spec, tmp_path, "on", TEZIP_DEADF_LOG=1, **env)
    rows = _log(err)
    assert "dead source" not in err
    off, err_off = _child(spec, tmp_path, "off", TEZIP_DEADF=0, **env)
    assert "dead forget gate" not in err_off and "dead source" not in err_off   # nothing is printed unless asked
    _same_bits(on, off, "against TEZIP_DEADF=0", cfg)
    assert on["n_wino"] == off["n_wino"]                             # no launch added or removed
    if ref_impl:
        _same_bits(on, run_job(spec, impl=0), "against tz_set_conv_impl(0)", cfg)
    if oracle:
        _same_bits(on, _oracle(spec[:4] + (1,) + spec[5:]), "against the C oracle", cfg)   # (the oracle has no batches)
    exp = _check_log(spec, rows, rule_spec, kept)
    return on, rows, exp


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("hp,wp,batch", [(64, 64, 1), (64, 64, 3), (72, 88, 1), (72, 88, 3)])
def test_zero_bias_model_leaves_the_forget_gate_out_at_every_level(hp, wp, batch, tmp_path):
    """Keras' default initialisation (the bench's model): C0_l = +0 at every level.  72 x 88: cut tiles at levels 2 and 3."""
    on, rows, exp = _check(D.spec("zero", hp, wp, batch), tmp_path)
    assert exp == {1: True, 2: True, 3: True} and all(r["out"] for r in rows.values()), rows
    assert all(np.abs(on["r%d" % l]).max() > 0 for l in range(4))
    if batch == 1:   # ... and with the split decided by measurement, whichever way it falls
        _same_bits(run_job(D.spec("zero", hp, wp, batch)), on, "E-part ahead by measurement", D.model(D.spec("zero", hp, wp, batch))[0])


@pytest.mark.parametrize("ipw", [1, 2, 4, 5])
def test_five_and_eight_column_blocks_at_every_ipw(ipw, tmp_path):
    """(3, 80, 128) at 72 x 88, zero biases: five column blocks at level 1, eight at level 2; TEZIP_WINO_IPW = every proper
    divisor of either (1; 1, 2, 4) and 5 (a level-1 workgroup then walks all of its tile's blocks).  A value that does not
    divide a launch's block count leaves that launch its own choice."""
    _, rows, exp = _check(D.spec("zero", 72, 88, 1, shape=D.M9, seed=13), tmp_path, ref_impl=ipw == 1, TEZIP_WINO_IPW=ipw)
    assert exp == {1: True, 2: True} and all(r["out"] for r in rows.values()), rows


def test_two_models_that_differ_in_the_forget_gate_only_give_the_same_bits():
    """The lemma on the device: every forget-gate kernel and bias overwritten, the skip on."""
    a, b = D.spec("zero", 72, 88, 1), D.spec("zero_f", 72, 88, 1)
    cfg = D.model(a)[0]
    assert D.c0_is_plus_zero(b) == {1: True, 2: True, 3: True}
    got = run_job(b)
    _same_bits(got, run_job(a), "forget gate overwritten", cfg)
    _same_bits(got, _oracle(b), "against the C oracle of the overwritten model", cfg)


@pytest.mark.parametrize("hp,wp,batch,seed", [(64, 64, 3, 123), (72, 88, 1, 31)])
def test_biased_models_leave_nothing_out(hp, wp, batch, seed, tmp_path):
    _, rows, exp = _check(D.spec("bias", hp, wp, batch, seed=seed), tmp_path)
    assert not any(exp.values()) and not any(r["out"] for r in rows.values()), rows


def test_mixed_model_leaves_it_out_where_c0_is_zero_only(tmp_path):
    """Zero biases except the c-gate bias of level 1: C0_3 = C0_2 = +0, C0_1 is not."""
    spec = D.spec("mixed", 72, 88, 3)
    assert D.c0_is_plus_zero(spec) == {1: False, 2: True, 3: True}
    _, rows, _ = _check(spec, tmp_path)
    assert [rows[l]["out"] for l in (1, 2, 3)] == [False, True, True], rows


def test_a_plane_that_is_zero_in_the_interior_but_not_on_the_border(tmp_path):
    """C0_2 is exactly +0 everywhere but on its left and right border columns, where the zero padding takes one of the two
    taps away -- a measurement that looked at the interior, or at one pixel, would call the level dead.  Asserted on the numpy
    arrays, interior and border both; the log must say that nothing is left out there."""
    spec = D.spec("border", 64, 64, 1)
    c2 = D.c0_numpy(spec)[2]
    assert (D.bits(c2[:, 1:-1]) == 0).all()
    assert np.abs(c2[:, 0]).min() > 1e-3 and np.abs(c2[:, -1]).min() > 1e-3
    _, rows, _ = _check(spec, tmp_path)
    assert rows[2] == dict(zero=False, out=False, why=""), rows
    assert not any(r["out"] for r in rows.values()), rows


def test_a_non_finite_forget_gate_weight_keeps_four_gates(tmp_path):
    """One +inf in the forget gate of level 2, on a channel of E_2 (the t = 0 pass reads no error map, so C0_2 is still +0):
    that level keeps four gates -- its forget gate may be NaN --, the others do not.  Compared with TEZIP_DEADF=0 only (what the
    hardware makes of a NaN is its business).  The rule is restated on the model without the weight: numpy's t = 0 pass does
    multiply the zero error map by it."""
    spec = D.spec("inf_f", 64, 64, 1)
    _, rows, _ = _check(spec, tmp_path, ref_impl=False, oracle=False, rule_spec=D.spec("zero", 64, 64, 1), kept={2: "not finite"})
    assert [(rows[l]["zero"], rows[l]["out"]) for l in (1, 2, 3)] == [(True, True), (True, False), (True, True)], rows


def test_the_sign_of_zero(tmp_path):
    """tests/regimes.py D19 (zero biases: the skip is active) at 24 x 40 with the gain lowered to 10^-21.5, where g of level 1 is
    the smallest negative subnormal in hundreds of elements and i * g = 0.5 g rounds to -0.  c = (+0) + (-0) is +0 and r = o *
    tanh(c) is +0; a `+ 0.0f` folded away would leave c = -0 and r = -0.  r must match the oracle in every bit."""
    spec = D.spec("D19", 24, 40, 1, seed=215)
    counts = D.negative_zero_products(spec)
    print("products i * g that are -0, per level:", counts)
    assert counts[1] >= 300, counts
    on, rows, exp = _check(spec, tmp_path)
    assert exp == {1: True, 2: True, 3: True} and all(r["out"] for r in rows.values()), rows
    assert int((D.bits(on["r1"]) == 0).sum()) >= counts[1] // 2      # (the oracle's sums are not numpy's to the last bit)


def test_forced_split_on_the_zero_bias_model(monkeypatch):
    """'E-part ahead' forced (TEZIP_EPART=1): the side launches <3, EPI_RAW3, false> of levels 1 and 2 leave rows of 3 R columns
    in P_l, the <3, EPI_LSTM3, true, NOSAME> launches start from them.  Bit-identical to the fused three-gate step and to the
    oracle; 5 k_wino launches per predictor call fused, 7 split, two calls."""
    spec = D.spec("zero", 72, 88, 3)
    cfg = D.model(spec)[0]
    got = {}
    for mode in (0, 1):
        monkeypatch.setenv("TEZIP_EPART", str(mode))
        got[mode] = run_job(spec)
        assert got[mode]["n_wino"] == (14 if mode else 10), (mode, got[mode]["n_wino"])
    _same_bits(got[1], got[0], "split against fused", cfg)
    _same_bits(got[1], _oracle(spec[:4] + (1,) + spec[5:]), "split against the C oracle", cfg)


def test_cli_round_trip_256(tmp_path):
    """-c then -u of a 256 x 256 job with the zero-bias model, contract by default (TZ-PA2 at this size: every fused gate launch of
    encoder and decoder runs three gates), lossless: the output is the input."""
    from PIL import Image
    from tezip_amd import compress, decompress, synth, weights
    from tezip_amd.prednet import PredNetConfig
    cfg = PredNetConfig()
    mdir = str(tmp_path / "model")
    weights.save_model(mdir, cfg, cfg.init_weights(seed=123), 256, 256)
    frames = synth.translating_scene(5, 256, 256, seed=31)
    ddir = tmp_path / "data"
    ddir.mkdir()
    for t in range(frames.shape[0]):
        Image.fromarray(frames[t], mode="RGB").save(ddir / ("frame_%03d.png" % t))
    cdir, udir = str(tmp_path / "comp"), str(tmp_path / "out")
    compress.run(mdir, str(ddir), cdir, 0, 3, None, "abs", [0.0], True, False, True)
    decompress.run(mdir, cdir, udir, True, False)
    got = np.stack([np.array(Image.open(os.path.join(udir, "frame_%03d.png" % t))) for t in range(5)])
    np.testing.assert_array_equal(got, frames)


if __name__ == "__main__":   # the child process of _child: the job named on the command line, results into an .npz
    spec_ = json.loads(sys.argv[1])
    spec_ = (spec_[0], tuple(tuple(s) if s is not None else None for s in spec_[1])) + tuple(spec_[2:])
    np.savez(sys.argv[2], **run_job(spec_))
