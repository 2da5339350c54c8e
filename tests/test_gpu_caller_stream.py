"""A context on a caller's stream (-m gpu): Context(dev, stream=s.cuda_stream) with a torch stream, the way tezip_amd/_lib.py
documents to run next to torch without explicit synchronisation.  tz_ctx_create has logic of its own for it: the stream is not
the context's to destroy, and one that is not at the device's greatest priority turns 'E-part ahead' off unless TEZIP_EPART says
otherwise.  Every comparison is of bit patterns; the GPU side of a case runs in one child process under a time limit
(tests/sched_jobs.py)."""
import numpy as np
import pytest

import sched_jobs as S

pytestmark = pytest.mark.gpu


def test_same_bits_and_the_stream_handed_back(tmp_path):
    """C.1: rollout, encode and decode of a small lossy job on a torch stream of default and of high priority equal those of a
    context with its own stream; tz_ctx_stream returns the caller's handle; after tz_ctx_destroy the torch stream still runs a
    kernel and synchronises."""
    j = S.job("zero", 64, 64, 3, 4, contract=2, encode=["abs", 2.0])
    res, _ = S.child(tmp_path, {"own": j, "default": dict(j, stream="default"), "high": dict(j, stream="high")})
    for name in ("default", "high"):
        S.same_bits(res[name], res["own"], name + " against the context's own stream")
        for k in ("payload", "table", "decoded"):
            np.testing.assert_array_equal(res[name][k], res["own"][k], err_msg="%s: %s" % (name, k))
        assert res[name]["stream_is_the_callers"] and res[name]["stream_alive"]
    assert np.abs(res["own"]["decoded"].astype(int) - S.frames(64, 64, 4).astype(int)).max() <= 3
    S.oracle_bits(res["default"], j, (0, 3), "default priority")


def test_the_priority_rule(tmp_path):
    """C.2: 256x256, one window in flight.  On a stream of default priority the split is off by rule, not by measurement: 5 k_wino
    launches per step; TEZIP_EPART=1 still forces it: 7, the same bits.  On a stream of the greatest priority the measurement
    decides: 5 or 7."""
    j = S.job("zero", 256, 256, 1, 1, contract=2, prof=True)
    res, logs = S.child(tmp_path, {"own": dict(j, env={"TEZIP_EPART": 0}), "default": dict(j, stream="default", env={"TEZIP_EPART_LOG": 1}),
                                   "forced": dict(j, stream="default", env={"TEZIP_EPART": 1}),
                                   "high": dict(j, stream="high", env={"TEZIP_EPART_LOG": 1})})
    counts = {k: int(r["n_wino_pa2"]) for k, r in res.items()}
    print(counts)
    print(logs["high"])
    for name in ("default", "forced", "high"):
        S.same_bits(res[name], res["own"], name + " against the context's own stream")
    steps = 2
    assert counts["own"] == 5 * steps
    assert counts["default"] == 5 * steps
    assert "E-part ahead" not in logs["default"]            # nothing was measured
    assert counts["forced"] == 7 * steps
    assert counts["high"] in (5 * steps, 7 * steps)
    S.oracle_bits(res["default"], j, (0,), "default priority")


def test_ordering_without_host_synchronisation(tmp_path):
    """C.3: under torch.cuda.stream(s) a device tensor holds frames X; a producer that is long for the GPU (48 matrix products of
    4096x4096) is queued whose last operation overwrites them with Y; rollout and encode(payload=<device tensor>) are issued at
    once, torch zeroes the frame tensor right behind them and reads the payload on s.  A library that queued any of this off the
    caller's stream without an event would give the payload of X, of zeros or garbage; a correct one can never fail this, however
    the timing falls."""
    j = S.job("zero", 64, 64, 3, 3, contract=2, encode=["abs", 2.0], ordering=True)
    res, _ = S.child(tmp_path, {"run": j})
    r = res["run"]
    assert r["producer_finite"]
    assert not np.array_equal(r["payload_x"], r["payload_y"])                   # (the two patterns can be told apart)
    np.testing.assert_array_equal(r["payload_got"], r["payload_y"])
    np.testing.assert_array_equal(r["table_got"], r["table_y"])
    np.testing.assert_array_equal(r["payload_again"], r["payload_y"])
    np.testing.assert_array_equal(r["table_again"], r["table_y"])
