"""qfec_build_acks on the GPU, whole buffers bit for bit against the rule of
tests/ack_rule.py: the ack's scalars, both CSR tables, their tails and the
state untouched (ack_device.py).  Beyond one trip of the scan over the acks
and beyond one full grid of waves the expectation is the whole-array rule, tied
to the sequential one on a sample of the same acks."""
import numpy as np
import pytest

import ack_cases as K
import ack_device as D
import ack_rule as A
from test_ack_rule import both_build
from turn_sizes import GRID_PER_CU, SCAN_BLOCK, TILE, ncu, wave_wrap

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


_big = {}


def big_state():
    """more connections than acks_walk_kernel's grid has waves, at window 64"""
    if not _big:
        n_conns = wave_wrap() + 40
        _big["state"] = K.grown_state(np.random.default_rng(6100), n_conns)
    return _big["state"]


def rows_of(ptr, table, acks):
    """the rows of a CSR table that belong to `acks`, in their order"""
    _, at, _ = A._ranges(ptr[:-1][acks], np.diff(ptr.astype(np.int64))[acks])
    return table[at.astype(np.int64)]


def run_big(ctx, ack_conn, max_ranges, max_revived):
    """the whole-array rule as the expectation, tied to the sequential one on
    300 of the same acks (the last among them)"""
    state = big_state()
    want = A.build_acks_np(state, ack_conn, max_ranges, max_revived)
    acks = np.unique(np.r_[np.random.default_rng(len(ack_conn)).integers(0, len(ack_conn), 299),
                           len(ack_conn) - 1])
    some = both_build(state, ack_conn[acks], max_ranges, max_revived)
    for k in ("largest", "hash", "truncated"):
        assert np.array_equal(some[k], want[k][acks]), k
    for ptr, tables in (("range_ptr", ("range_lo", "range_hi")), ("rev_ptr", ("rev_pn",))):
        assert np.array_equal(np.diff(some[ptr]), np.diff(want[ptr])[acks]), ptr
        for t in tables:
            assert np.array_equal(some[t], rows_of(want[ptr], want[t], acks)), t
    D.build(ctx, D.DevState(state), ack_conn, max_ranges, max_revived, want)
    return want


@gpu
@pytest.mark.parametrize("max_ranges,max_revived", [(3, 2), (255, 0), (1, 255)])
@pytest.mark.parametrize("n_acks", [SCAN_BLOCK, SCAN_BLOCK + 1, 2 * SCAN_BLOCK + 1])
def test_acks_beyond_one_scan_trip(ctx, n_acks, max_ranges, max_revived):
    """acks_scan_kernel scans range_ptr and rev_ptr, an ack a lane: from 1,025
    acks on both take a second trip with the first one's sum as its base (1,024
    acks fill one trip exactly: nothing lies behind entry 1,024 there)"""
    rng = np.random.default_rng(n_acks + max_ranges)
    state = big_state()
    conn = K.acks_ending_full(rng, state, n_acks, max_ranges, max_revived)
    conn[n_acks // 2:-1:3] = conn[:(n_acks - 1 - n_acks // 2 + 2) // 3]  # connections repeat
    assert np.unique(conn).size < n_acks - 100
    want = run_big(ctx, conn, max_ranges, max_revived)
    for ptr in ["range_ptr"] + (["rev_ptr"] if max_revived else []):
        assert want[ptr][SCAN_BLOCK] > 0, ptr
        if n_acks > SCAN_BLOCK:
            assert want[ptr][-1] - want[ptr][SCAN_BLOCK] > 0, \
                ptr + ": the acks no longer make the scan take a second trip"
    assert max_revived or want["rev_ptr"][-1] == 0


@gpu
def test_acks_beyond_one_grid(ctx):
    """one ack more than acks_walk_kernel's grid has waves: the first wave's
    second trip walks the last ack, a truncated one with revived packets"""
    n_acks = wave_wrap()
    assert n_acks > ncu() * GRID_PER_CU * TILE // 64, "the acks no longer make the grid loop"
    conn = K.acks_ending_full(np.random.default_rng(6200), big_state(), n_acks, 3, 2,
                              truncated=True)
    want = run_big(ctx, conn, 3, 2)
    assert want["truncated"][-1] == 1 and want["rev_ptr"][-1] > want["rev_ptr"][-2]
    assert want["range_ptr"][-1] - want["range_ptr"][-2] == 3


@gpu
def test_empty_call(ctx):
    """n_acks == 0: the two pointers' first entries, nothing else"""
    run(ctx, state_with(64, {1, 2, 4}), [], 4, 4)
