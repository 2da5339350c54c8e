"""The rollout as two groups of windows on two streams (-m gpu): TEZIP_SPLIT=1, read when the context is made (tz_api.hip
run_schedule).  The windows are dealt alternately to group A (activation slots 0 .. capA - 1, the context's stream) and group B
(slots capA .. max_batch - 1, a second stream); it is the only way slot0 > 0 reaches tz_model_predict_batch_dev -- every
`+ slot0 * stride` of the gate and A convolutions' arguments, the P[l] offsets, the level-0 error maps k_conv_small leaves for the
next step of its group, and `slot0 + n <= Pcap[l]`.

Every case is compared bit for bit with the same job without the switch, and with the C oracle at the first and the last window of
either group.  That the two groups ran is read from the TEZIP_SPLIT_LOG=1 line (the switch is off while launches are counted:
profiling keeps one stream).  The GPU side of a case runs in one child process under a time limit (tests/sched_jobs.py)."""
import re

import numpy as np
import pytest

import sched_jobs as S

pytestmark = pytest.mark.gpu

LOG_LINE = re.compile(r"\[tezip\] two-group rollout: caps (\d+) \+ (\d+), batches (\d+) \+ (\d+)$")
ON = {"TEZIP_SPLIT": 1, "TEZIP_SPLIT_LOG": 1}


def _lines(stderr):
    return [tuple(int(v) for v in m.groups()) for m in (LOG_LINE.search(ln) for ln in stderr.splitlines()) if m]


def _expect(max_batch, nwin):
    """run_schedule restated: even windows to group A, odd ones to B; per depth ceil(windows / cap) batches, two depths."""
    cap_a, cap_b = (max_batch + 1) // 2, max_batch // 2
    n_a, n_b = (nwin + 1) // 2, nwin // 2
    return cap_a, cap_b, 2 * -(-n_a // cap_a), 2 * -(-n_b // cap_b)


def _ends(nwin):
    """The first and the last window of either group."""
    last_a = nwin - 1 if (nwin - 1) % 2 == 0 else nwin - 2
    return sorted({0, last_a, 1, nwin - 1 if last_a != nwin - 1 else nwin - 2})


@pytest.mark.parametrize("max_batch", [2, 3, 5])
@pytest.mark.parametrize("hp,wp", [(64, 64), (48, 80)])
@pytest.mark.parametrize("kind", ["zero", "bias"])
@pytest.mark.parametrize("contract", [2, 1])
def test_two_groups_give_the_bits_of_one(contract, kind, hp, wp, max_batch, tmp_path):
    """B.1, B.2: 2 max_batch + 1 windows, so that the groups differ in slots (capA != capB for odd max_batch) and in batches;
    warm-up 0 and 1."""
    nwin = 2 * max_batch + 1
    variants = {}
    for p in (0, 1):
        variants["one%d" % p] = S.job(kind, hp, wp, max_batch, nwin, p, contract)
        variants["two%d" % p] = S.job(kind, hp, wp, max_batch, nwin, p, contract, env=ON)
    res, logs = S.child(tmp_path, variants)
    for p in (0, 1):
        one, two = res["one%d" % p], res["two%d" % p]
        lines = _lines(logs["two%d" % p])
        print("warm-up %d:" % p, lines)
        assert lines == [_expect(max_batch, nwin)], logs["two%d" % p][-1500:]
        assert not _lines(logs["one%d" % p])
        assert one["contract"] == two["contract"] == contract
        S.same_bits(two, one, "two groups against one, warm-up %d" % p, names=("roll",))
        for r in (one, two):
            S.oracle_bits(r, variants["one%d" % p], _ends(nwin), "warm-up %d" % p)


@pytest.mark.parametrize("kind", ["zero", "bias"])
def test_group_b_past_the_buffer_of_level_1(kind, tmp_path):
    """B.3: 128x128, 56 slots, 56 windows, contract by size (TZ-PA1): group B sits at slot 28, so slot0 + n = 56 > Pcap[1] = 53
    while group A fits."""
    j = S.job(kind, 128, 128, 56, 56, contract=0)
    res, logs = S.child(tmp_path, {"one": j, "two": dict(j, env=ON)})
    lines = _lines(logs["two"])
    print(lines)
    assert lines == [(28, 28, 2, 2)], logs["two"][-1500:]
    assert res["one"]["contract"] == res["two"]["contract"] == 1
    S.same_bits(res["two"], res["one"], "two groups against one", names=("roll",))
    S.oracle_bits(res["two"], dict(j, contract=1), _ends(56), "two groups")


@pytest.mark.parametrize("contract", [2, 1])
def test_a_predict_next_between_two_rollouts(contract, tmp_path):
    """B.4: the level-0 error maps a rollout left at slot0 > 0, and the per-group bookkeeping of which step may skip k_err0, must
    not leak into what follows: tz_predict_next on three frames, then the rollout again."""
    j = S.job("zero", 64, 64, 3, 7, contract=contract, next=True, again=True)
    res, logs = S.child(tmp_path, {"one": j, "two": dict(j, env=ON)})
    assert _lines(logs["two"]) == [_expect(3, 7)] * 2, logs["two"][-1500:]
    one, two = res["one"], res["two"]
    S.same_bits(two, one, "two groups against one", names=("roll", "next"))
    np.testing.assert_array_equal(two["key2"], two["key"])
    np.testing.assert_array_equal(S.D.bits(two["roll2"]), S.D.bits(two["roll"]))
    np.testing.assert_array_equal(S.D.bits(one["roll2"]), S.D.bits(one["roll"]))
    S.oracle_bits(dict(two, roll=two["roll2"]), j, _ends(7), "second rollout")


@pytest.mark.parametrize("max_batch", [2, 3, 5])
@pytest.mark.parametrize("kind", ["zero", "bias"])
def test_the_decoder_in_two_groups_restores_a_lossless_job(kind, max_batch, tmp_path):
    """B.5: encoder and decoder rollout both under the switch; the payload is the one-group encoder's."""
    nwin = 2 * max_batch + 1
    j = S.job(kind, 48, 80, max_batch, nwin, 1, 2, encode=["abs", 0.0])
    res, logs = S.child(tmp_path, {"one": j, "two": dict(j, env=ON)})
    assert _lines(logs["two"]) == [_expect(max_batch, nwin)] * 2, logs["two"][-1500:]      # the encoder's rollout and the decoder's
    u8 = S.frames(48, 80, nwin, 1)
    for name in ("one", "two"):
        np.testing.assert_array_equal(res[name]["decoded"], u8, err_msg=name)
    np.testing.assert_array_equal(res["two"]["payload"], res["one"]["payload"])
    np.testing.assert_array_equal(res["two"]["table"], res["one"]["table"])
