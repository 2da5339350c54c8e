"""The forms of the encoder against each other on a MI355X: tz_encode is the one-shard case of tz_encode_begin /
tz_encode_finish (payload and table byte for byte, into every kind of output), tz_encode_delta is the delta stack that
tz_encode taps, and the encoder's resident data is dropped by every call that ends it."""
import numpy as np
import pytest

from tezip_amd import _lib, synth
from tezip_amd.prednet import PredNetConfig

pytestmark = pytest.mark.gpu
CFG = PredNetConfig(stack_sizes=(3, 16, 32))
NT, H, W = 12, 24, 40
N = NT * H * W * 3
TZ_ERR_STATE = -4
# abs 0 (lossless), abs 0.4 (an identity tolerance: the fused lossless pass), abs 2 (lossy), and the other three modes
MODES = [("abs", [0.0]), ("abs", [0.4]), ("abs", [2.0]), ("rel", [0.01]), ("pwrel", [0.05]), ("absrel", [2.0, 0.01])]
OUTS = ["pageable", "pinned", "pinned_deferred", "device", "resident"]


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    c.load_model(CFG, CFG.init_weights(seed=3, bias_scale=0.2))
    c.prepare(H, W, max_batch=4)
    yield c
    c.close()


@pytest.fixture(scope="module")
def frames():
    return synth.turbulence(NT, H, W, seed=11)


def _rollout(ctx, frames, kind):
    if kind == "swp":
        return ctx.rollout(frames, 1, 4)[0]
    _, mse = ctx.rollout(frames, 1, None, 1e9, want_mse=True)
    return ctx.rollout(frames, 1, None, float(np.median(mse[2:])))[0]


def _out(kind):
    if kind == "pageable":
        return np.full(N, -7, np.int16)
    if kind in ("pinned", "pinned_deferred"):
        buf = _lib.pinned_empty(N, np.int16)
        buf[...] = -7
        return buf
    if kind == "device":
        import torch
        buf = torch.full((N,), -7, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()                      # (the context writes it on a stream of its own)
        return buf
    return "resident"


def _host(ctx, out):
    if isinstance(out, str):
        return ctx.payload_get(0, N)
    if isinstance(out, np.ndarray):
        return np.array(out)
    ctx.synchronize()
    return out.cpu().numpy()


def _encode(ctx, mode, bound, entropy, kind, shuffle=False):
    out = _out(kind)
    ctx.set_payload_deferred(kind == "pinned_deferred")
    try:
        _, table, _ = ctx.encode(mode, bound, entropy, payload=out, shuffle=shuffle)
        ctx.payload_wait()
    finally:
        ctx.set_payload_deferred(False)
    return _host(ctx, out), table


def _one_shard(ctx, mode, bound, entropy, kind):
    hist, first, last = ctx.encode_begin(mode, bound, entropy)
    table = ctx.build_table(hist) if entropy else None
    out = _out("pinned" if kind == "pinned_deferred" else kind)
    ret = ctx.encode_finish(None, table, out=out)
    if not isinstance(out, str):
        assert ret is out
    return _host(ctx, out), table, first, last


@pytest.mark.parametrize("kind", OUTS)
@pytest.mark.parametrize("entropy", [True, False])
@pytest.mark.parametrize("mode,bound", MODES)
@pytest.mark.parametrize("rollout", ["swp", "dwp"])
def test_whole_encode_is_the_one_shard_begin_finish(ctx, frames, rollout, mode, bound, entropy, kind):
    _rollout(ctx, frames, rollout)
    payload, table = _encode(ctx, mode, bound, entropy, kind)
    assert not (payload == -7).all()
    got, got_table, first, last = _one_shard(ctx, mode, bound, entropy, kind)
    np.testing.assert_array_equal(got, payload)
    if entropy:
        assert got_table.dtype == table.dtype and got_table.tobytes() == table.tobytes()
    else:
        assert table is None and got_table is None
    # the edges begin reports are those of the quantised delta stack the encode taps
    _, _, delta = ctx.encode(mode, bound, entropy, want_delta=True)
    assert (first, last) == (int(delta.reshape(-1)[0]), int(delta.reshape(-1)[-1]))


@pytest.mark.parametrize("entropy", [True, False])
@pytest.mark.parametrize("mode,bound", [MODES[0], MODES[2], MODES[5]])
@pytest.mark.parametrize("rollout", ["swp", "dwp"])
def test_shuffled_encode_is_the_shuffled_one_shard_payload(ctx, frames, rollout, mode, bound, entropy):
    _rollout(ctx, frames, rollout)
    for kind in ("pageable", "device", "resident"):
        planes, table = _encode(ctx, mode, bound, entropy, kind, shuffle=True)
        plain, got_table, _, _ = _one_shard(ctx, mode, bound, entropy, "pageable")
        np.testing.assert_array_equal(planes.view(np.uint8), ctx.byte_shuffle(plain), err_msg=kind)
        assert (table is None) == (got_table is None)
        if entropy:
            np.testing.assert_array_equal(got_table, table)


@pytest.mark.parametrize("mode,bound", MODES)
@pytest.mark.parametrize("rollout", ["swp", "dwp"])
def test_encode_delta_is_the_delta_encode_taps(ctx, frames, rollout, mode, bound):
    _rollout(ctx, frames, rollout)
    _, _, tapped = ctx.encode(mode, bound, True, want_delta=True)
    np.testing.assert_array_equal(ctx.encode_delta(mode, bound), tapped)
    import torch
    dev = torch.empty((NT, H, W, 3), dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    ctx.encode_delta(mode, bound, out=dev)
    ctx.synchronize()
    np.testing.assert_array_equal(dev.cpu().numpy(), tapped)


def _refused(call, message):
    with pytest.raises(_lib.TezipError) as e:
        call()
    assert e.value.status == TZ_ERR_STATE
    assert message in str(e.value)


def test_encoder_state_edges(ctx, frames):
    finish = "tz_encode_finish needs a tz_encode_begin first"
    resident = "no resident payload of a tz_encode on this rollout"
    # a fresh context: no begin
    fresh = _lib.Context(0)
    try:
        fresh.load_model(CFG, CFG.init_weights(seed=3, bias_scale=0.2))
        fresh.prepare(H, W, max_batch=4)
        fresh.rollout(frames, 1, 4)
        _refused(lambda: fresh.encode_finish(None, None), finish)
    finally:
        fresh.close()
    # a begin belongs to its rollout: another rollout, a decoder rollout or a staged payload ends it
    for end in (lambda: ctx.rollout(frames, 1, 4), lambda: ctx.rollout_decode(frames, 1), lambda: ctx.payload_begin(N)):
        ctx.rollout(frames, 1, 4)
        hist, _, _ = ctx.encode_begin("abs", [2.0], True)
        table = ctx.build_table(hist)
        end()
        _refused(lambda: ctx.encode_finish(None, table), finish)
    # a finish consumes its begin
    ctx.rollout(frames, 1, 4)
    hist, _, _ = ctx.encode_begin("abs", [2.0], True)
    table = ctx.build_table(hist)
    ctx.encode_finish(None, table)
    _refused(lambda: ctx.encode_finish(None, table), finish)
    # the resident payload of a tz_encode is gone once a begin or a staged payload overwrites it
    for over in (lambda: ctx.encode_begin("abs", [2.0], True), lambda: ctx.payload_begin(N)):
        ctx.rollout(frames, 1, 4)
        _, table, _ = ctx.encode("abs", [2.0], True, payload="resident")
        ctx.encode_quality("resident", table)          # (accepted before)
        over()
        _refused(lambda: ctx.encode_quality("resident", table), resident)
