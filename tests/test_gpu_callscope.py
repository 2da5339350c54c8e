"""Every entry point hands its pool blocks back on every path it leaves by: tz_pool_held is 0 after refusals that come
after a hand-out, and after every call of one complete job; the same job run again on the same context leaves the pool with
the blocks it had, so the pool recycles and does not grow.

The entry points open one call scope (tz_call, csrc/tz_internal.h) whose destructor is the only release.  The library
before the scope passes these tests too on every path a test can reach: its one leak (tz_act_probe) sat behind a HIP call
that does not fail in practice.  The tests are here so that a later entry point written without a scope fails them."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NT, H, W, WINDOW = 12, 64, 64, 4


def _model():
    from tezip_amd.prednet import PredNetConfig
    cfg = PredNetConfig(stack_sizes=(3, 16, 32))
    return cfg, cfg.init_weights(seed=4, bias_scale=0.2)


@pytest.fixture(scope="module")
def frames():
    from tezip_amd import synth
    return synth.moving_blobs(NT, H, W)                                  # gray: the three channels are equal


@pytest.fixture()
def ctx():
    from tezip_amd import _lib
    cfg, wts = _model()
    c = _lib.Context(0)
    c.load_model(cfg, wts)
    c.prepare(H, W, WINDOW)
    yield c
    c.close()


def _refused(ctx, call, status, text):
    from tezip_amd import _lib
    with pytest.raises(_lib.TezipError) as e:
        call()
    assert e.value.status == status and text in str(e.value), str(e.value)
    assert ctx.pool_held()[0] == 0, "a refused call kept pool blocks: %s" % text


def test_fresh_context_holds_nothing():
    from tezip_amd import _lib
    c = _lib.Context(0)
    try:
        assert c.pool_held() == (0, 0)
    finally:
        c.close()


def test_refusals_behind_a_hand_out_release_the_pool(ctx, frames):
    from tezip_amd import huff
    pay = (np.arange(600, dtype=np.int16) % 7).astype(np.int16)          # a host array: staged in a pool block
    ln = huff.code_lengths(np.bincount(pay))
    good = ctx.huff_encode_buf(pay, ln, 0)
    assert ctx.pool_held()[0] == 0
    # one byte short of the stream: behind tz_dev_in and the hand-outs of huff_encode_dev
    _refused(ctx, lambda: ctx.huff_encode_buf(pay, ln, 0, out=np.empty(good.size - 1, np.uint8)), -1, "the buffer holds %d" % (good.size - 1))
    # a value present in the input has length 0: the size pass finds it, three hand-outs in
    hole = ln.copy()
    hole[3] = 0
    _refused(ctx, lambda: ctx.huff_encode_buf(pay, hole, 0), -1, "give no code")
    # a span of 3001 values, more than TZ_NBINS: found behind the hand-outs of the count
    wide = np.array([-1500, 1500] * 300, np.int16)
    _refused(ctx, lambda: ctx.huffr_counts(wide), -1, "span more than 2111 symbols")
    assert (ctx.huff_encode_buf(pay, ln, 0) == good).all()              # the context still works
    # a one-channel payload of a stack with one coloured pixel: behind the hand-outs of the gray check
    coloured = frames.copy()
    coloured[NT - 1, H - 1, W - 1, 2] ^= 1
    ctx.rollout(coloured, 0, WINDOW)
    assert ctx.pool_held()[0] == 0
    ctx.set_payload_channels(1)
    _refused(ctx, lambda: ctx.encode("abs", [2.0], True), -1, "frame %d has colour" % (NT - 1))
    _refused(ctx, lambda: ctx.bound_probe("abs", [2.0]), -1, "frame %d has colour" % (NT - 1))
    ctx.set_payload_channels(3)
    assert ctx.encode("abs", [2.0], True)[0].size == frames.size and ctx.pool_held()[0] == 0


def _job(ctx, frames):
    """One complete job; pool_held()[0] == 0 after every call.  Returns the pool's block count at the end."""
    from tezip_amd import huff, keycoder

    def step(value=None):
        held = ctx.pool_held()[0]
        assert held == 0, "call %d of the job left %d pool blocks handed out" % (step.n, held)
        step.n += 1
        return value

    step.n = 0
    ctx.frames_begin(NT, H, W)
    ctx.frames_put(0, frames)
    key = step(ctx.rollout(None, 0, WINDOW))[0]
    payload, table, _ = step(ctx.encode("abs", [2.0], True))            # a host payload with a table
    assert table is not None and payload.size == frames.size
    step(ctx.encode_quality(payload, table))
    step(ctx.encode_digests(payload, table))
    step(ctx.encode_ssim(payload, table))
    step(ctx.bound_probe("abs", [2.0]))
    step(ctx.encode("abs", [2.0], True, payload="resident"))
    counts, base = step(ctx.huff_counts())
    nbytes = step(ctx.huff_encode(huff.code_lengths(counts), base))
    step(ctx.huff_get(0, nbytes))
    keys = np.flatnonzero(key)
    kc = step(ctx.keys_counts(keys))
    assert step(ctx.keys_gray(keys)).all()
    pred = keycoder.choose_predictors(kc)
    step(ctx.keys_encode(keys, pred, huff.code_lengths(keycoder.chosen_counts(kc, pred))))
    key_stack = np.where(key[:, None, None, None], frames, 0).astype(np.uint8)
    step(ctx.rollout_decode(key_stack, 0))
    step(ctx.decode(payload, table, out="resident"))
    step(ctx.decode_range(payload, table, NT - 2, 2, out="resident"))
    digests = step(ctx.decoded_digests(NT - 2, 2))
    assert digests.size == 2
    return ctx.pool_held()[1]


def test_a_job_releases_after_every_call_and_the_pool_does_not_grow(ctx, frames):
    blocks = _job(ctx, frames)
    assert blocks > 0
    assert _job(ctx, frames) == blocks, "the same job again made the pool grow"
