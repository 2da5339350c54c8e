"""The job, its C-oracle reference and the comparison of tests/test_gpu_deadhalf.py.

One job = a context under TZ-PA2 (set_contract(2): k_wino runs at every frame size), three predictor steps from `batch`
frames (tz_predict_next: k_err0 forms E_0), the taps of every level after the first and after the third step, then a rollout
of windows of three frames (from its second step on a window takes E_0 from the k_conv_small epilogue of the step before) and
the taps behind it.  The switches are read per prepare (or per context), so a job sets them around its own context."""
import functools
import os

import numpy as np

import dead0_models as D

WIN = 3
SIZES = [(32, 32), (48, 80), (64, 64)]   # level 1 exactly one 16 x 16 tile; ragged tiles whose halo leaves the image; 4 x 4 tiles
ENV = ("TEZIP_DEADHALF", "TEZIP_DEADHALF_LOG", "TEZIP_DEAD0", "TEZIP_DEAD0_LOG", "TEZIP_DEADSRC", "TEZIP_DEADSRC_LOG",
       "TEZIP_DEADF", "TEZIP_DEADF_LOG", "TEZIP_EPART", "TEZIP_WINO_IPW", "TEZIP_UNIFORM")


def tap_names(cfg, pre=""):
    return [pre + "e%d" % l for l in range(cfg.nb_layers)] + [pre + "r%d" % l for l in range(cfg.nb_layers)]


def names(cfg, rollout_taps=True):
    return ["p1", "p2", "p3", "roll"] + tap_names(cfg) + tap_names(cfg, "a") + (tap_names(cfg, "q") if rollout_taps else [])


def _frames(spec):
    return D.as_float(D.frames_u8(spec[4], spec[2], spec[3]))


def _steps(c, cfg, spec):
    hp, wp, batch = spec[2], spec[3], spec[4]
    out = {"p1": c.predict_next(_frames(spec))}
    for l in range(cfg.nb_layers):
        out["e%d" % l], out["r%d" % l] = c.predict_tap(0, l), c.predict_tap(1, l)
    out["p2"] = c.predict_next(out["p1"])
    out["p3"] = c.predict_next(out["p2"])
    for l in range(cfg.nb_layers):
        out["ae%d" % l], out["ar%d" % l] = c.predict_tap(0, l), c.predict_tap(1, l)
    u8 = D.frames_u8(batch * WIN, hp, wp, seed=7)
    key, _ = c.rollout(u8, 0, WIN)
    roll = c.get_predictions()
    roll[key] = 0                                            # (slots of key frames hold no prediction)
    out["roll"], out["key"] = roll, key
    for l in range(cfg.nb_layers):
        out["qe%d" % l], out["qr%d" % l] = c.predict_tap(0, l), c.predict_tap(1, l)
    return out


def run_job(spec, impls=(1,), then=None, **env):
    """The job once per entry of `impls` (tz_set_conv_impl), all in ONE context prepared with `env` set; `then`: a second
    (hp, wp) the same context is prepared at afterwards, the job run there once more.  Returns a list of results."""
    from tezip_amd import _lib
    cfg, w = D.model(spec)
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    c = None
    try:
        c = _lib.Context(0)
        c.set_contract(2)
        c.load_model(cfg, w)
        c.prepare(spec[2], spec[3], max_batch=spec[4])
        outs = []
        for impl in impls:
            c.set_conv_impl(impl)
            outs.append(_steps(c, cfg, spec))
        if then:
            spec2 = spec[:2] + tuple(then) + spec[4:]
            c.set_conv_impl(1)
            c.prepare(spec2[2], spec2[3], max_batch=spec2[4])
            outs.append(_steps(c, cfg, spec2))
    finally:
        if c is not None:
            c.close()
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return outs


@functools.lru_cache(maxsize=None)
def oracle(spec):
    """The C oracle under contract 2, computed once per job, shared and never written to.  (It has no batches, and no taps
    behind a rollout.)"""
    from oracle import coracle
    from oracle import oracle as O
    cfg, w = D.model(spec)
    hp, wp, batch = spec[2], spec[3], spec[4]
    net = coracle.CPredNet(w, cfg.stack_sizes, cfg.R_stack_sizes, hp, wp).set_contract(2)
    x = _frames(spec)
    ref = {k: np.empty_like(x) for k in ("p1", "p2", "p3")}
    d1 = d3 = None
    for i in range(len(x)):
        ref["p1"][i], da = net.next(x[i], debug=True)
        ref["p2"][i] = net.next(ref["p1"][i])
        ref["p3"][i], db = net.next(ref["p2"][i], debug=True)
        if i == 0:                                               # (tz_predict_tap reads batch slot 0)
            d1, d3 = da, db
    for l in range(cfg.nb_layers):
        ref["e%d" % l], ref["r%d" % l], ref["ae%d" % l], ref["ar%d" % l] = d1["e"][l], d1["r"][l], d3["e"][l], d3["r"][l]

    class P:
        def c0(self, a, b):
            return net.c0()

        def next(self, f):
            return net.next(np.asarray(f, np.float32))

    u8 = D.frames_u8(batch * WIN, hp, wp, seed=7)
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


def same_bits(got, want, what, cfg, rollout_taps=True):
    np.testing.assert_array_equal(got["key"], want["key"], err_msg=what + ": key frames")
    for k in names(cfg, rollout_taps):
        np.testing.assert_array_equal(D.bits(got[k]), D.bits(want[k]), err_msg="%s: %s" % (what, k))
