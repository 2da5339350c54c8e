"""The two-quad stage of the three-tile k_wino launches (-m gpu): k_wino2 (tezip_amd/csrc/tz_wino_kernels.hip.h) walks two channel
quads per stage over a dense stage image, in a ring of three double slots.  It is taken where a three-tile convolution's executed
stages are a multiple of 6 per source (tz_prednet.hip choose_wino_forms / launch_wino); every chain is the same fmaf chain over the
channels in ascending order, so every bit is k_wino's.

Every case runs, under TZ-PA2 (set_contract(2)) through the C ABI: predict_next on a few frames (one step each), predict_next on
those predictions and once more on the result (three chained calls), and a rollout of windows of three frames (the cell state and
the error maps carried from step to step).  Predictions and every level's E / R taps are compared as BIT PATTERNS between
(a) the new form on, (b) TEZIP_WINO2Q=0 in the same process, (c) tz_set_conv_impl(0) (k_wino_ref) and (d) the C oracle under
contract 2.  Which form every k_wino convolution takes is read from the TEZIP_WINO2Q_LOG=1 lines.  The GPU side of a case runs in
one child process under a time limit."""
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

ENV = ("TEZIP_WINO2Q", "TEZIP_WINO2Q_LOG", "TEZIP_DEADF", "TEZIP_DEADSRC", "TEZIP_DEADHALF", "TEZIP_UNIFORM", "TEZIP_EPART", "TEZIP_WINO_IPW")
LOG_LINE = re.compile(r"\[tezip\] k_wino stage, level (\d+) (gates|A): (\d+) \+ (\d+) stages, (three|four) column tiles: (two-quad|one-quad)(?: \((.*)\))?$")
WIN = 3
M6 = ((3, 32, 64, 128), None)   # zero biases: the live blocks of E_l give 8, 16 and 32 stages, the upsampled sources 16 and 32
SIZES = [(32, 32), (48, 80), (64, 64)]   # one tile at level 1 and ragged top levels; ragged tiles both ways; whole tiles


def _frames(spec):
    """(float frames of the predict_next calls -- the last call is a batch of one, whose taps the library holds --, uint8 frames of the rollout)"""
    hp, wp, batch = spec[2], spec[3], spec[4]
    rng = np.random.default_rng(977 * hp + wp)
    x = rng.integers(0, 256, (batch + 1 if batch > 1 else 2, hp, wp, 3)).astype(np.float32) / np.float32(255)
    if spec[0] == "D19":   # (the construction of the sign-of-zero case counts its -0 products on its own last frame)
        x = D.model(spec)[2]
    return x,rng.integers(0, 256, (batch * WIN, hp, wp, 3)).astype(np.uint8)


def _names(cfg):
    taps = ["e%d" % l for l in range(cfg.nb_layers)] + ["r%d" % l for l in range(cfg.nb_layers)]
    return ["p1", "p2", "p3", "roll"] + taps + ["a" + t for t in taps]


def run_job(spec, impl=1, **env):
    """The job on the GPU with `env` set while the context is made and the model prepared (the switches are read there)."""
    from tezip_amd import _lib
    cfg, w, _ = D.model(spec)
    hp, wp, batch = spec[2], spec[3], spec[4]
    x, u8 = _frames(spec)
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    c = None
    try:
        c = _lib.Context(0)
        c.set_contract(2)
        c.set_conv_impl(impl)
        c.load_model(cfg, w)
        c.prepare(hp, wp, max_batch=batch)
        c.prof_enable(True)
        c.prof_reset()
        out = {"p1": c.predict_next(x)}
        for l in range(cfg.nb_layers):
            out["e%d" % l], out["r%d" % l] = c.predict_tap(0, l), c.predict_tap(1, l)
        out["p2"] = c.predict_next(out["p1"])
        out["p3"] = c.predict_next(out["p2"])
        for l in range(cfg.nb_layers):
            out["ae%d" % l], out["ar%d" % l] = c.predict_tap(0, l), c.predict_tap(1, l)
        key, _ = c.rollout(u8, 0, WIN)
        roll = c.get_predictions()
        roll[key] = 0                                            # (slots of key frames hold no prediction)
        out["roll"], out["key"] = roll, key
        out["n_wino"] = np.array(c.prof_get()["wino_pa2"][1])
        c.prof_enable(False)
    finally:
        if c is not None:
            c.close()
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return out


def _child(spec, tmp_path, variants, **env):
    """The variants {name: (impl, env)} of the job one after the other in ONE fresh process under a time limit, `env` set for all of
    them: {name: results}, {name: that variant's part of stderr}."""
    out = str(tmp_path / "job.npz")
    e = dict(os.environ)
    for k in ENV:
        e.pop(k, None)
    e.update({k: str(v) for k, v in env.items()})
    r = subprocess.run([sys.executable, os.path.abspath(__file__), json.dumps(spec), out, json.dumps(variants)], env=e, cwd=ROOT,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    res = {name: {} for name in variants}
    with np.load(out) as z:
        for k in z.files:
            name, what = k.split("/", 1)
            res[name][what] = z[k]
    logs, cur = {name: [] for name in variants}, None
    for ln in r.stderr.splitlines():
        if ln.startswith("## variant "):
            cur = ln[len("## variant "):]
        elif cur is not None:
            logs[cur].append(ln)
    return res, {k: "\n".join(v) for k, v in logs.items()}


@functools.lru_cache(maxsize=None)
def _oracle(spec):
    """The C oracle under contract 2, computed once per job; shared by the cases over it and never written to."""
    from oracle import coracle
    from oracle import oracle as O
    cfg, w, _ = D.model(spec)
    hp, wp = spec[2], spec[3]
    net = coracle.CPredNet(w, cfg.stack_sizes, cfg.R_stack_sizes, hp, wp).set_contract(2)
    x, u8 = _frames(spec)
    ref = {k: np.empty_like(x) for k in ("p1", "p2", "p3")}
    for i in range(len(x)):
        ref["p1"][i], d1 = net.next(x[i], debug=True)
        ref["p2"][i] = net.next(ref["p1"][i])
        ref["p3"][i], d3 = net.next(ref["p2"][i], debug=True)
    for l in range(cfg.nb_layers):
        ref["e%d" % l], ref["r%d" % l], ref["ae%d" % l], ref["ar%d" % l] = d1["e"][l], d1["r"][l], d3["e"][l], d3["r"][l]

    class P:
        def c0(self, a, b):
            return net.c0()

        def next(self, f):
            return net.next(np.asarray(f, np.float32))

    ro = O.rollout(u8, 0, WIN, None, P())
    roll = np.zeros((len(u8), hp, wp, 3), np.float32)
    for start, preds in ro["groups"]:
        for i, p in enumerate(preds):
            roll[start + i] = p
    roll[ro["key"]] = 0
    ref["roll"], ref["key"] = roll, ro["key"]
    for v in ref.values():
        v.setflags(write=False)
    return ref


def _same_bits(got, want, what, cfg):
    np.testing.assert_array_equal(got["key"], want["key"], err_msg=what + ": key frames")
    for k in _names(cfg):
        np.testing.assert_array_equal(D.bits(got[k]), D.bits(want[k]), err_msg="%s: %s" % (what, k))


def _log(stderr):
    """{(level, 'gates' | 'A'): dict(same, up, tiles, form, why)} of one prepare."""
    rows = {(int(m[1]), m[2]): dict(same=int(m[3]), up=int(m[4]), tiles=m[5], form=m[6], why=m[7] or "")
            for m in (LOG_LINE.search(ln) for ln in stderr.splitlines()) if m}
    assert rows, stderr[-1500:]
    return rows


def _check(spec, tmp_path, ref_impl=True, **env):
    """The four references of a job agree in every bit; -> (results of the new form, its log rows).  (The step is the fused one
    unless a case says otherwise: whether a batch size splits is otherwise MEASURED per prepared model.)"""
    cfg = D.model(spec)[0]
    env.setdefault("TEZIP_EPART", 0)
    variants = {"on": (1, {"TEZIP_WINO2Q_LOG": 1}), "off": (1, {"TEZIP_WINO2Q": 0})}
    if ref_impl:
        variants["ref"] = (0, {})
    res, logs = _child(spec, tmp_path, variants, **env)
    rows = _log(logs["on"])
    for row in sorted(rows.items()):
        print(row)
    assert "k_wino stage" not in logs["off"]                        # nothing is printed unless asked
    _same_bits(res["on"], res["off"], "against TEZIP_WINO2Q=0", cfg)
    assert res["on"]["n_wino"] == res["off"]["n_wino"] > 0          # no launch added or removed
    if ref_impl:
        _same_bits(res["on"], res["ref"], "against tz_set_conv_impl(0)", cfg)
    _same_bits(res["on"], _oracle(spec), "against the C oracle", cfg)
    # the rule, restated on what the line itself says
    for key, row in rows.items():
        fits = row["tiles"] == "three" and row["same"] % 6 == 0 and row["up"] % 6 == 0
        assert (row["form"] == "two-quad") == fits, (key, row)
    return res["on"], rows


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("hp,wp", SIZES)
def test_zero_bias_model_takes_the_two_quad_stage_at_every_three_tile_convolution(hp, wp, batch, tmp_path):
    """The bench's model: 12 + 24, 24 + 48 and 48 stages of gates, 12 of A_1; A_2 has four column tiles and stays."""
    on, rows = _check(D.spec("zero", hp, wp, batch), tmp_path)
    assert {k: (r["same"], r["up"], r["tiles"], r["form"]) for k, r in rows.items()} == {
        (1, "gates"): (12, 24, "three", "two-quad"), (1, "A"): (12, 0, "three", "two-quad"), (2, "gates"): (24, 48, "three", "two-quad"),
        (2, "A"): (24, 0, "four", "one-quad"), (3, "gates"): (48, 0, "three", "two-quad")}, rows
    assert all(np.abs(on["r%d" % l]).max() > 0 for l in range(4))


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("hp,wp", SIZES)
def test_stage_counts_that_do_not_divide_by_six_fall_back(hp, wp, batch, tmp_path):
    """(3, 32, 64, 128), zero biases: three-tile gate launches of 8 + 16, 16 + 32 and 32 stages -- none fits the ring."""
    _, rows = _check(D.spec("zero", hp, wp, batch, shape=M6), tmp_path)
    gates = {k[0]: (r["same"], r["up"], r["tiles"], r["form"], r["why"]) for k, r in rows.items() if k[1] == "gates"}
    why = "stages not a multiple of 6"
    assert gates == {1: (8, 16, "three", "one-quad", why), 2: (16, 32, "three", "one-quad", why), 3: (32, 0, "three", "one-quad", why)}, rows
    assert all(r["form"] == "one-quad" for r in rows.values()), rows


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("hp,wp", SIZES)
def test_biased_model_has_one_three_tile_convolution(hp, wp, batch, tmp_path):
    """bias_scale 0.1: every gate convolution keeps four gates; A_1 (96 columns = two blocks of three tiles) walks all 24 stages of
    E_1 and takes the two-quad stage."""
    _, rows = _check(D.spec("bias", hp, wp, batch), tmp_path)
    assert [k for k, r in rows.items() if r["tiles"] == "three"] == [(1, "A")], rows
    assert (rows[(1, "A")]["same"], rows[(1, "A")]["form"]) == (24, "two-quad"), rows
    assert all(r["form"] == "one-quad" for k, r in rows.items() if k != (1, "A")), rows


@pytest.mark.parametrize("hp,wp,batch", [(48, 80, 3), (64, 64, 1)])
def test_forced_split(hp, wp, batch, tmp_path):
    """'E-part ahead' forced (TEZIP_EPART=1): the side launches <EPI_RAW3> walk the live stages of E_l from an even first stage,
    the <EPI_LSTM3, true, NOSAME> launches start at stage 24 / 48 of the block; both in the two-quad form.  The same bits as the
    fused step."""
    spec = D.spec("zero", hp, wp, batch)
    split, rows = _check(spec, tmp_path, TEZIP_EPART=1)
    assert all(r["form"] == "two-quad" for r in rows.values() if r["tiles"] == "three"), rows
    res, _ = _child(spec, tmp_path, {"fused": (1, {})}, TEZIP_EPART=0)
    assert split["n_wino"] > res["fused"]["n_wino"]
    _same_bits(split, res["fused"], "split against fused", D.model(spec)[0])


@pytest.mark.parametrize("ipw", [1, 2, 3, 4, 6, 12])
def test_every_legal_ipw(ipw, tmp_path):
    """3, 6 and 12 column blocks of gates, 2 of A_1: TEZIP_WINO_IPW = every divisor of one of them.  An item must start in ring slot
    0 whatever came before it; a value that does not divide a launch's block count leaves that launch its own choice."""
    _, rows = _check(D.spec("zero", 48, 80, 1), tmp_path, ref_impl=ipw == 1, TEZIP_WINO_IPW=ipw)
    assert sum(r["form"] == "two-quad" for r in rows.values()) == 4, rows


def test_split_decided_by_measurement(tmp_path):
    """Batch 1 with the split measured per prepared model, whichever way it falls: the same bits as the fused step."""
    spec = D.spec("zero", 64, 64, 1)
    res, _ = _child(spec, tmp_path, {"measured": (1, {})})
    _same_bits(res["measured"], _oracle(spec), "E-part ahead by measurement", D.model(spec)[0])


def test_the_sign_of_zero(tmp_path):
    """The construction of tests/test_gpu_deadf.py::test_the_sign_of_zero: g of level 1 is the smallest negative subnormal in
    hundreds of elements, sums go subnormal and products round to -0.  The start of a chain is the literal +0 on the FIRST quad of
    an item only: a second quad that started from +0 again, or a first one that did not, shows in the sign and the low bits."""
    spec = D.spec("D19", 24, 40, 1, seed=215)
    counts = D.negative_zero_products(spec)
    print("products i * g that are -0, per level:", counts)
    assert counts[1] >= 300, counts
    on, rows = _check(spec, tmp_path)
    assert sum(r["form"] == "two-quad" for r in rows.values()) == 4, rows
    assert int((D.bits(on["r1"]) == 0).sum()) >= counts[1] // 2      # (the oracle's sums are not numpy's to the last bit)


if __name__ == "__main__":   # the child process of _child: the variants of the job named on the command line, results into an .npz
    spec_ = json.loads(sys.argv[1])
    spec_ = (spec_[0], tuple(tuple(s) if s is not None else None for s in spec_[1])) + tuple(spec_[2:])
    got = {}
    for name_, (impl_, env_) in json.loads(sys.argv[3]).items():
        sys.stderr.write("## variant %s\n" % name_)
        sys.stderr.flush()
        for k_, v_ in run_job(spec_, impl=impl_, **env_).items():
            got["%s/%s" % (name_, k_)] = v_
    np.savez(sys.argv[2], **got)
