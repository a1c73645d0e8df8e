"""qfec_build_acks on the GPU, whole buffers bit for bit against the rule of
tests/ack_rule.py: the ack's scalars, both CSR tables, their tails and the
state untouched (ack_device.py)."""
import numpy as np
import pytest

import ack_cases as K
import ack_device as D
import ack_rule as A

gpu = pytest.mark.gpu
U64 = np.uint64


def state_with(window, received, revived=(), least=0, n_conns=2, conn=0):
    """a state in which connection `conn` received exactly `received`, built
    through the rule"""
    state = A.new_state(n_conns, window)
    pns = np.array(sorted(received), U64)
    turn = dict(packet_number=pns, pkt_conn=np.full(len(pns), conn, np.uint32),
                entropy=((pns * U64(7) >> U64(1)) & U64(1)).astype(np.uint8))
    if len(revived):
        turn.update(status=np.ones(len(revived), np.uint8),
                    revived_idx=np.zeros(len(revived), np.uint8),
                    slot_key=np.array([conn << K.KEY_SHIFT | pn for pn in revived], U64),
                    key_shift=K.KEY_SHIFT)
    if least:
        turn.update(raise_conn=np.array([conn], np.uint32), raise_least=np.array([least], U64),
                    raise_hash=np.array([0x3c], np.uint8))
    return A.record_received(state, **turn)["state"]


def run(ctx, state, ack_conn, max_ranges, max_revived, **how):
    want = A.build_acks(state, ack_conn, max_ranges, max_revived)
    D.build(ctx, D.DevState(state), np.asarray(ack_conn, np.uint32), max_ranges, max_revived,
            want, **how)
    return want


@gpu
@pytest.mark.parametrize("gaps", [0, 1, 4, 5])
def test_interval_counts(ctx, gaps):
    """0, 1, max_ranges and max_ranges + 1 intervals at max_ranges = 4"""
    missing = {3 + 4 * i for i in range(gaps)}
    state = state_with(64, set(range(1, 30)) - missing)
    want = run(ctx, state, [0], 4, 0)
    assert want["range_ptr"].tolist() == [0, min(gaps, 4)]
    assert want["truncated"].tolist() == [int(gaps > 4)]
    assert want["largest"].tolist() == [18 if gaps > 4 else 29]


@gpu
def test_interval_at_the_least(ctx):
    """an interval that touches lo, on a new connection and behind a raise"""
    want = run(ctx, state_with(64, {3, 4, 9}), [0], 8, 0)
    assert want["range_lo"].tolist() == [1, 5] and want["range_hi"].tolist() == [3, 9]
    want = run(ctx, state_with(64, {1, 2, 3, 9, 12}, least=5), [0], 8, 0)
    assert want["range_lo"].tolist() == [5, 10] and want["range_hi"].tolist() == [9, 12]
    assert want["hash"][0] == 0x3c ^ (9 * 7 >> 1 & 1) << 1 ^ (12 * 7 >> 1 & 1) << 4


@gpu
@pytest.mark.parametrize("max_revived", [0, 1, 2, 255])
def test_revived_lists(ctx, max_revived):
    """more revived than max_revived: the highest are listed, ascending; a
    truncated ack lists only those at or below its largest"""
    state = state_with(64, {1, 2, 5, 8, 11, 14, 20}, revived=[3, 6, 9, 13])
    want = run(ctx, state, [0], 255, max_revived)
    assert want["rev_pn"].tolist() == [3, 6, 9, 13][4 - min(4, max_revived):]
    want = run(ctx, state, [0], 2, max_revived, rev_pn=max_revived != 0)
    assert want["largest"][0] == 8 and want["truncated"][0] == 1
    assert want["rev_pn"].tolist() == [3, 6][2 - min(2, max_revived):]


@gpu
def test_nothing_live_repeats_and_range(ctx):
    """G < lo (a new connection, and one behind a jump), ack_conn repeated and
    out of range"""
    state = state_with(64, {1, 2, 4}, least=9, n_conns=3, conn=1)
    assert state["largest"][1] == 4 and state["least"][1] == 9
    want = run(ctx, state, [1, 0, 1, 3, 2, 1, 7], 3, 2)
    assert want["latched"] and want["largest"].tolist() == [4, 0, 4, 0, 0, 4, 0]
    assert want["hash"].tolist() == [0x3c, 0, 0x3c, 0, 0, 0x3c, 0]
    assert want["range_ptr"].tolist() == [0] * 8
    state = state_with(64, {1, 2, 4, 7}, revived=[3], n_conns=3, conn=1)
    want = run(ctx, state, [1, 1, 0, 1], 1, 1)
    assert want["range_ptr"].tolist() == [0, 1, 2, 2, 3] and want["truncated"].tolist() == [1, 1, 0, 1]


@gpu
@pytest.mark.parametrize("window,n_conns,max_ranges,max_revived", [
    (64, 1, 255, 255), (64, 3, 1, 0), (256, 3, 2, 1), (256, 257, 7, 3), (1024, 5, 40, 5)])
def test_random_states(ctx, window, n_conns, max_ranges, max_revived):
    """states grown by random turns (live ranges of several 64-cell trips at
    the larger windows), every connection and some twice, in a random order"""
    rng = np.random.default_rng(window + n_conns)
    state = A.new_state(n_conns, window)
    for call in range(5):
        turn = K.random_turn(rng, state, 30 * n_conns + 40, n_groups=12 * n_conns,
                             n_raise=n_conns // 3)
        state = A.record_received(state, **turn)["state"]
        conns = rng.permutation(np.r_[np.arange(n_conns), rng.integers(0, n_conns, 3)])
        want = run(ctx, state, conns, max_ranges, max_revived)
    assert want["range_ptr"][-1] > 0
    if max_revived and n_conns > 1:
        assert want["rev_ptr"][-1] > 0
    if max_ranges < 10:
        assert want["truncated"].any()
    if window > 64:  # a walk of more than one trip
        assert int((state["largest"] - np.maximum(state["least"], U64(1))).max()) > 64


@gpu
def test_empty_call(ctx):
    """n_acks == 0: the two pointers' first entries, nothing else"""
    run(ctx, state_with(64, {1, 2, 4}), [], 4, 4)
