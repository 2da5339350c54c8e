"""Jobs of the rollout-scheduler tests (tests/test_gpu_slotcap.py, tests/test_gpu_two_groups.py, tests/test_gpu_caller_stream.py):
how a predictor step is LAUNCHED -- which levels run their gate convolution as two launches for a batch (tz_prednet.hip
epart_levels, Pcap[l]), the rollout as two groups of windows on two streams (tz_api.hip run_schedule, TEZIP_SPLIT=1), a context
on a caller's stream (tz_ctx_create) -- never changes a bit of what it computes.

A job is a dict that travels to a child process as JSON: a model of tests/deadf_models.py, a frame size, the slots prepared,
windows of three uint8 frames behind `warm_up` frames, and what to do with them.  The switches are read when the context is made
and at prepare, so every variant sets its own while it does both.  Run as a script, this file is that child: the variants named
in a JSON file one after the other in ONE fresh process (the parent's time limit is the job's), results into an .npz."""
import functools
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (ROOT, os.path.join(ROOT, "tests")):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

import deadf_models as D  # noqa: E402

WIN = 3
ENV = ("TEZIP_EPART", "TEZIP_EPART_LOG", "TEZIP_EPART_LEVELS", "TEZIP_SPLIT", "TEZIP_SPLIT_LOG", "TEZIP_WINO2Q", "TEZIP_WINO2Q_LOG",
       "TEZIP_DEADF", "TEZIP_DEADSRC", "TEZIP_DEADHALF", "TEZIP_UNIFORM", "TEZIP_WINO_IPW", "TEZIP_LAT_SPLIT", "TEZIP_PA")
PROF = ("wino_pa2", "convlat_small_grid", "conv16_lds_dma", "conv16b_level0", "conv_small_valu", "conv3x3_general", "conv3x3_mfma", "err0")


def job(kind, hp, wp, max_batch, nwin, warm_up=0, contract=2, **more):
    """kind: 'zero' | 'bias' (tests/deadf_models.py, the default model shape).  more: impl (tz_set_conv_impl's 0 / 1), lat (None |
    'never' | 'always'), env {name: value}, prof (count launches: tz_prof_enable), again (a second rollout), next (tz_predict_next on
    three frames between the two), encode [mode, bound] (and decode what it gave on the same context), stream (None | 'default' |
    'high': a torch stream of that priority as the context's)."""
    return dict(kind=kind, hp=hp, wp=wp, max_batch=max_batch, nwin=nwin, warm_up=warm_up, contract=contract, **more)


def model(kind):
    cfg, w, _ = D.model(D.spec(kind, 8, 8, 1))
    return cfg, w


def _block(hp, wp, tag, n, pattern=0):
    return np.random.default_rng([hp, wp, tag, pattern]).integers(0, 256, (n, hp, wp, 3)).astype(np.uint8)


def frames(hp, wp, nwin, warm_up=0, pattern=0):
    """`warm_up` frames, then `nwin` windows of three.  A window's frames depend on the frame size and the window's number alone, so
    that jobs of different lengths share their oracle steps."""
    return np.concatenate([_block(hp, wp, 10 ** 6, warm_up, pattern)] + [_block(hp, wp, w, WIN, pattern) for w in range(nwin)])


def floats(hp, wp):
    """The three frames of a job's tz_predict_next call."""
    return np.random.default_rng([hp, wp, 2 * 10 ** 6]).integers(0, 256, (3, hp, wp, 3)).astype(np.float32) / np.float32(255)


def run_job(j):
    """The job on the GPU: {name: array}."""
    from tezip_amd import _lib
    cfg, w = model(j["kind"])
    hp, wp, p = j["hp"], j["wp"], j["warm_up"]
    u8 = frames(hp, wp, j["nwin"], p)
    env = {k: str(v) for k, v in j.get("env", {}).items()}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    out, c, s = {}, None, None
    try:
        if j.get("stream"):
            import torch
            s = torch.cuda.Stream(priority=-1 if j["stream"] == "high" else 0)
            c = _lib.Context(0, stream=s.cuda_stream)
            out["stream_is_the_callers"] = np.array(c.stream_ptr() == s.cuda_stream)
        else:
            c = _lib.Context(0)
        c.set_contract(j["contract"])
        c.set_conv_impl(j.get("impl", 1), j.get("lat"))
        c.load_model(cfg, w)
        c.prepare(hp, wp, max_batch=j["max_batch"])
        out["contract"] = np.array(c.get_contract())
        if j.get("prof"):
            c.prof_enable(True)
            c.prof_reset()
        key, _ = c.rollout(u8, p, WIN)
        if j.get("prof"):
            got = c.prof_get()
            for k in PROF:
                if k in got:
                    out["n_" + k] = np.array(got[k][1])
            c.prof_enable(False)
        roll = c.get_predictions()
        roll[key] = 0                                            # (slots of key frames hold no prediction)
        out["roll"], out["key"] = roll, key
        for l in range(cfg.nb_layers):                           # slot 0 of the last predictor call
            out["e%d" % l], out["r%d" % l] = c.predict_tap(0, l), c.predict_tap(1, l)
        if j.get("encode"):
            mode, bound = j["encode"]
            payload, table, _ = c.encode(mode, [bound], True)
            out["payload"], out["table"] = np.array(payload), table
        if j.get("next"):
            out["next"] = c.predict_next(floats(hp, wp))
        if j.get("again"):
            key2, _ = c.rollout(u8, p, WIN)
            roll2 = c.get_predictions()
            roll2[key2] = 0
            out["roll2"], out["key2"] = roll2, key2
        if j.get("encode"):                                      # the decoder's rollout, under the same switches
            c.rollout_decode(np.where(key[:, None, None, None], u8, 0).astype(np.uint8), p)
            out["decoded"] = np.array(c.decode(out["payload"], out["table"]))
    finally:
        if c is not None:
            c.close()
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    if s is not None:                                            # the stream was never the context's to destroy
        import torch
        with torch.cuda.stream(s):
            t = torch.full((1 << 16,), 3, dtype=torch.int32, device="cuda") * 5
        s.synchronize()
        out["stream_alive"] = np.array(int(t.sum().item()) == 15 << 16)
    return out


def run_ordering(j):
    """A context on a torch stream, with torch as the producer and the consumer of its device buffers and no synchronisation
    between them: see tests/test_gpu_caller_stream.py."""
    import torch
    from tezip_amd import _lib
    cfg, w = model(j["kind"])
    hp, wp = j["hp"], j["wp"]
    x, y = frames(hp, wp, j["nwin"]), frames(hp, wp, j["nwin"], pattern=1)          # patterns X and Y
    mode, bound = j["encode"]
    out = {}
    s = torch.cuda.Stream()
    c = _lib.Context(0, stream=s.cuda_stream)
    try:
        c.set_contract(j["contract"])
        c.load_model(cfg, w)
        c.prepare(hp, wp, max_batch=j["max_batch"])
        for name, f in (("x", x), ("y", y)):                     # what a synchronised run gives for either pattern
            c.rollout(f, 0, WIN)
            payload, table, _ = c.encode(mode, [bound], True)
            c.synchronize()
            out["payload_" + name], out["table_" + name] = np.array(payload), table
        with torch.cuda.stream(s):
            held = torch.from_numpy(x).cuda()
            new = torch.from_numpy(y).cuda()
            a = torch.randn(4096, 4096, device="cuda")
            b = torch.randn(4096, 4096, device="cuda") / 64
            payload = torch.empty(x.size, dtype=torch.int16, device="cuda")
            torch.cuda.synchronize()
            for _ in range(48):                                  # a producer that is long for the GPU ...
                a = a @ b
            held.copy_(new)                                      # ... and whose last operation puts Y where X was
            c.rollout(held, 0, WIN)
            _, table, _ = c.encode(mode, [bound], True, payload=payload)
            held.zero_()                                         # the consumer's side: torch takes the frames back at once
            out["payload_got"] = payload.cpu().numpy()           # torch reads the payload on s
            out["table_got"] = table
            _, table2, _ = c.encode(mode, [bound], True, payload=payload)   # the context's own copy of the frames is whole
            out["payload_again"], out["table_again"] = payload.cpu().numpy(), table2
            out["producer_finite"] = np.array(bool(torch.isfinite(a).all().item()))
    finally:
        c.close()
    return out


def child(tmp_path, variants, timeout=240, **env):
    """The variants {name: job} one after the other in ONE fresh process under a time limit, `env` set for all of them:
    {name: results}, {name: that variant's part of stderr}."""
    spec, out = str(tmp_path / "variants.json"), str(tmp_path / "job.npz")
    with open(spec, "w") as f:
        json.dump(variants, f)
    e = dict(os.environ)
    for k in ENV:
        e.pop(k, None)
    e.update({k: str(v) for k, v in env.items()})
    r = subprocess.run([sys.executable, os.path.abspath(__file__), spec, out], env=e, cwd=ROOT, capture_output=True, text=True,
                       timeout=timeout)
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
def oracle_window(kind, hp, wp, contract, w):
    """The C oracle's two predictions of window `w`, computed once; shared and never written to."""
    from oracle import coracle
    net = _net(kind, hp, wp, contract)
    p1 = net.next(coracle.u8_to_f32_frame(_block(hp, wp, w, WIN)[0], hp, wp))
    p2 = net.next(p1)
    for a in (p1, p2):
        a.setflags(write=False)
    return p1, p2


@functools.lru_cache(maxsize=None)
def _net(kind, hp, wp, contract):
    from oracle import coracle
    cfg, wts = model(kind)
    return coracle.CPredNet(wts, cfg.stack_sizes, cfg.R_stack_sizes, hp, wp).set_contract(contract)


def same_bits(got, want, what, names=("roll", "e0", "e1", "e2", "e3", "r0", "r1", "r2", "r3")):
    np.testing.assert_array_equal(got["key"], want["key"], err_msg=what + ": key frames")
    for k in names:
        np.testing.assert_array_equal(D.bits(got[k]), D.bits(want[k]), err_msg="%s: %s" % (what, k))


def oracle_bits(got, j, windows, what):
    """predictions[warm_up + 3 w + d] of the job's result are the oracle's under j's contract, for the windows named and both depths."""
    for w in windows:
        ref = oracle_window(j["kind"], j["hp"], j["wp"], j["contract"], w)
        for d in (1, 2):
            f = j["warm_up"] + WIN * w + d
            assert not got["key"][f]
            np.testing.assert_array_equal(D.bits(got["roll"][f]), D.bits(ref[d - 1]), err_msg="%s: window %d depth %d" % (what, w, d))


if __name__ == "__main__":
    with open(sys.argv[1]) as f_:
        variants_ = json.load(f_)
    if any(j_.get("stream") or j_.get("ordering") for j_ in variants_.values()):
        import torch  # noqa: F401  (ahead of the library, as in a program that hands it torch streams: both then share ONE HIP runtime)
    got_ = {}
    for name_, j_ in variants_.items():
        sys.stderr.write("## variant %s\n" % name_)
        sys.stderr.flush()
        for k_, v_ in (run_ordering(j_) if j_.get("ordering") else run_job(j_)).items():
            got_["%s/%s" % (name_, k_)] = v_
    np.savez(sys.argv[2], **got_)
