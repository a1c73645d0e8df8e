"""qfec_record_received on the GPU, whole buffers bit for bit against the rule
of tests/ack_rule.py (pinned by test_ack_rule.py): rcv_out, counts, the state
through live_cells, the inputs unchanged, nothing written behind an array's end
(ack_device.py).  The device runs on from its own state call after call, the
rule from the rule's: the cells outside the live range differ between the two
and must never matter.  On every round of tests/golden/ack_ref.npz the acks
built from the device's state are the reference's own."""
import numpy as np
import pytest

import ack_cases as K
import ack_device as D
import ack_rule as A
from turn_sizes import GRID_PER_CU, TILE, grid_wrap, ncu, wave_wrap

gpu = pytest.mark.gpu
U64 = np.uint64


def run_turns(ctx, state, turns, form=A.record_received, **how):
    dev = D.DevState(state)
    for turn in turns:
        want = form(state, **turn)
        D.record(ctx, dev, turn, want, **how)
        state = want["state"]
    return dev, state


def arrivals(pns, conn=0, flags=None, **more):
    pns = np.asarray(pns, U64)
    t = dict(packet_number=pns, pkt_conn=np.full(len(pns), conn, np.uint32), **more)
    if flags is not None:
        t["entropy"] = np.asarray(flags, np.uint8)
    return t


def raises(conn, least, hsh):
    return dict(raise_conn=np.asarray(conn, np.uint32), raise_least=np.asarray(least, U64),
                raise_hash=np.asarray(hsh, np.uint8))


@gpu
@pytest.mark.parametrize("window,n_conns,n_packets,calls", [
    (64, 1, 1, 6), (64, 1, 63, 6), (64, 3, 64, 6), (64, 3, 65, 40), (256, 3, 257, 8),
    (256, 257, 257, 6), (64, 257, 20011, 4), (256, 257, 20011, 3)])
def test_random_turns(ctx, window, n_conns, n_packets, calls):
    rng = np.random.default_rng(window + n_conns + n_packets)
    state = A.new_state(n_conns, window)
    dev = D.DevState(state)
    total = np.zeros(12, U64)
    for call in range(calls):
        turn = K.random_turn(rng, state, n_packets, n_groups=min(n_packets, 300),
                             n_raise=int(rng.integers(0, n_conns + 1)), bad_conn=call == 1)
        want = A.record_received(state, **turn)
        D.record(ctx, dev, turn, want)
        state, total = want["state"], total + want["counts"]
    if n_conns > 1 and n_packets * calls > 2000:  # every class and every count occurred
        assert (total > 0).all(), total
    if calls == 40:  # the ring went round several times
        assert int(state["largest"].min()) > 3 * window


def last_of_each_recorded(state, turn):
    """`turn` with its last packet, its last group and its last raise made ones
    that change the state: the packet RECORDED, the group's revived packet a
    missing one, the raise applied.  Each is asserted from the whole-array
    rule; returns the rule's result over the turn."""
    turn = {k: v.copy() if isinstance(v, np.ndarray) else v for k, v in turn.items()}
    w, nc = state["window"], len(state["least"])
    raised = np.zeros(nc + 1, bool)
    raised[np.minimum(turn["raise_conn"], nc)] = True
    # the packet: a number above the largest that no other packet of the turn
    # brings, of a connection nobody raises
    for c in np.flatnonzero(~raised[:nc]).tolist():
        others = set(turn["packet_number"][:-1][turn["pkt_conn"][:-1] == c].tolist())
        lo = max(int(state["least"][c]), 1)
        ahead = set(range(max(int(state["largest"][c]) + 1, lo), lo + w)) - others
        if ahead:  # (none where the window is full)
            break
    pn = min(ahead)
    turn["pkt_conn"][-1], turn["packet_number"][-1], turn["hdr"][-1] = c, pn, 0
    turn["entropy"][-1] = 1 << pn % 8
    # the raise: one above the least of its connection (in range: not the first of the table)
    r = int(turn["raise_conn"][-1])
    assert r < nc
    turn["raise_least"][-1] = int(state["least"][r]) + 1
    # the group: without it first, to find a packet that stays missing and unrevived
    turn["status"][-1] = 0
    before = A.record_received_np(state, **turn)
    st = before["state"]
    live = A.live_cells(st)
    lo = np.maximum(st["least"], U64(1))
    gaps = []
    for c2 in np.flatnonzero(~raised[:nc] & (st["largest"] > lo + U64(2))):
        gaps = [q for q in range(int(lo[c2]), int(st["largest"][c2])) if live[c2, q % w] == 0]
        if gaps:
            break
    free = np.setdiff1d(np.arange(len(turn["slot_key"])), turn["slot"])[0]
    turn["status"][-1], turn["revived_idx"][-1], turn["slot"][-1] = A.GROUP_REVIVED, 0, free
    turn["slot_key"][free] = c2 << K.KEY_SHIFT | gaps[0]
    want = A.record_received_np(state, **turn)
    assert want["rcv_out"][-1] == A.RECORDED
    assert want["state"]["cells"][c, pn % w] == A.RECEIVED | A.ENTROPY
    assert want["counts"][A.N_REVIVED] == before["counts"][A.N_REVIVED] + 1
    assert want["state"]["cells"][c2, gaps[0] % w] == A.REVIVED
    assert want["state"]["least"][r] == state["least"][r] + U64(1)
    return turn, want


@gpu
def test_a_turn_beyond_one_grid(ctx):
    """Two calls on one device state, each of one packet and one group more
    than a full grid of lanes and one raise more than a full grid of waves: the
    last packet, group and raise come in the first workgroup's second trip,
    each changes the state, and the twelve tallies hold both trips' counts."""
    n, n_raise = grid_wrap(), wave_wrap()
    grid = ncu() * GRID_PER_CU * TILE
    assert n - 1 >= grid and n_raise - 1 >= grid // 64, "the turn no longer makes the grids loop"
    rng = np.random.default_rng(6400)
    state = A.new_state(n_raise + 40, 64)
    dev = D.DevState(state)
    total = np.zeros(12, U64)
    for call in range(2):
        turn = K.random_turn(rng, state, n, n_groups=n, n_raise=n_raise, bad_conn=call == 1)
        turn, want = last_of_each_recorded(state, turn)
        assert want["latched"] == (call == 1)
        D.record(ctx, dev, turn, want)
        state, total = want["state"], total + want["counts"]
    assert (total > 0).all(), total


@gpu
@pytest.mark.parametrize("window", [64, 256])
def test_window_edge(ctx, window):
    """a largest that advances by window - 1 in one call, and a packet one
    beyond the window"""
    state = A.new_state(2, window)
    first = dict(packet_number=np.array([1, 1], U64), pkt_conn=np.array([0, 1], np.uint32))
    edge = dict(packet_number=np.array([window, window + 1], U64),
                pkt_conn=np.array([0, 1], np.uint32))
    want = A.record_received(A.record_received(state, **first)["state"], **edge)
    assert want["rcv_out"].tolist() == [A.RECORDED, A.OVERFLOW]
    assert want["state"]["largest"].tolist() == [window, 1]
    run_turns(ctx, state, [first, edge])


@gpu
def test_one_word_copies_and_duplicates(ctx):
    """four neighbouring numbers in one call (one word, four ORs), same-call
    copies with equal and with disagreeing flags, a copy of a packet of an
    earlier call, number 0"""
    state = A.new_state(2, 64)
    one = arrivals([8, 9, 10, 11, 13, 13, 14, 14, 0], conn=1, flags=[1, 0, 2, 0, 4, 4, 0, 8, 1])
    two = arrivals([9, 13, 14, 12], conn=1, flags=[2, 0, 0, 1])
    w1 = A.record_received(state, **one)
    assert w1["rcv_out"].tolist() == [A.RECORDED] * 8 + [A.STALE] and w1["counts"][A.N_NEW] == 6
    assert w1["state"]["cells"][1, 8:15].tolist() == [3, 1, 3, 1, 0, 3, 3]
    w2 = A.record_received(w1["state"], **two)
    assert w2["rcv_out"].tolist() == [A.DUPLICATE] * 3 + [A.RECORDED]
    run_turns(ctx, state, [one, two])


@gpu
def test_revived(ctx):
    """a revived packet that later arrives itself; revived at and above the
    largest, already received, slot out of range, no key: ignored"""
    state = A.new_state(2, 64)
    key = np.array([1 << K.KEY_SHIFT | 3, A.NO_KEY, 1 << K.KEY_SHIFT | 3], U64)
    one = arrivals([1, 2, 3, 5, 6], conn=1, flags=[1] * 5, status=np.array([1, 1, 1, 1, 1, 0, 1], np.uint8),
                   revived_idx=np.array([1, 3, 4, 0, 1, 1, 1], np.uint8),
                   slot=np.array([0, 0, 2, 2, 9, 0, 1], np.uint32), slot_key=key,
                   key_shift=K.KEY_SHIFT)
    w1 = A.record_received(state, **one)
    assert w1["counts"][A.N_REVIVED] == 1 and w1["counts"][A.N_NOT_MISSING] == 4
    assert w1["state"]["cells"][1, 4] == A.REVIVED
    two = arrivals([4], conn=1, flags=[0])
    assert A.record_received(w1["state"], **two)["state"]["cells"][1, 4] == A.REVIVED | A.RECEIVED
    run_turns(ctx, state, [one, two])
    # slot == NULL: group g has slot g
    three = dict(status=np.array([1, 2, 1], np.uint8), revived_idx=np.array([1, 1, 1], np.uint8),
                 slot_key=key, key_shift=K.KEY_SHIFT)
    run_turns(ctx, state, [arrivals([1, 2, 3, 5, 6, 7], conn=1), three])


@gpu
def test_raises(ctx):
    """a raise that drops a missing packet, one that drops none, one at G + 1,
    a jump, one at or below the least, one out of range"""
    state = A.new_state(6, 64)
    pns = [1, 2, 4, 5, 6]
    one = dict(packet_number=np.tile(np.array(pns, U64), 5),
               pkt_conn=np.repeat(np.arange(5, dtype=np.uint32), 5),
               entropy=np.tile(np.array([1, 1, 0, 1, 1], np.uint8), 5))
    one.update(raises([0, 1, 2, 3], [5, 3, 7, 9], [0x11, 0x22, 0x33, 0x44]))
    w1 = A.record_received(state, **one)
    assert w1["counts"][A.N_RAISED] == 4 and w1["counts"][A.N_DROPPED] == 2
    assert w1["counts"][A.N_JUMPS] == 1
    assert w1["state"]["hash"].tolist()[:5] == [0x11, 0x06, 0x33, 0x44, 0]
    two = raises([0, 1, 4, 6], [5, 2, 3, 4], [0x55, 0x66, 0x77, 0x88])
    w2 = A.record_received(w1["state"], **two)
    assert w2["latched"] and w2["counts"][A.N_RAISED] == 1
    # a packet between the largest and the least, after the jump: stale
    three = arrivals([8, 9, 10], conn=3)
    assert A.record_received(w2["state"], **three)["rcv_out"].tolist() == [A.STALE, A.RECORDED,
                                                                          A.RECORDED]
    run_turns(ctx, state, [one, two, three])


@gpu
@pytest.mark.parametrize("hdr,entropy,counts", [(False, True, True), (True, False, True),
                                                (True, True, False), (False, False, False)])
def test_null_arguments(ctx, hdr, entropy, counts):
    rng = np.random.default_rng(7)
    state = A.new_state(5, 64)
    turns = []
    for _ in range(3):
        turns.append(K.random_turn(rng, state, 300, n_groups=20, n_raise=2, hdr=hdr, entropy=entropy))
        state = A.record_received(state, **turns[-1])["state"]
    run_turns(ctx, A.new_state(5, 64), turns, counts=counts)


@gpu
def test_empty_call_and_flags(ctx):
    """nothing to do: counts zeroed, nothing else; QFEC_CACHED and
    QFEC_SMALL_GROUPS change nothing"""
    from libquic_amd import qfec
    state = A.new_state(3, 64)
    run_turns(ctx, state, [dict()])
    turn = K.random_turn(np.random.default_rng(3), state, 100, n_groups=10, n_raise=1)
    run_turns(ctx, state, [turn], flags=qfec.QFEC_CACHED | qfec.QFEC_SMALL_GROUPS)


@gpu
@pytest.mark.parametrize("window", [64, 256])
def test_reference_fixture(ctx, window):
    """tests/golden/ack_ref.npz, one call per round: after every round the acks
    built on the device are the reference manager's on every row"""
    f = K.fixture()
    nc = int(f["n_conns"])
    everyone = np.arange(nc, dtype=np.uint32)
    state = A.new_state(nc, window)
    dev = D.DevState(state)
    rows = 0
    for r in range(int(f["n_rounds"])):
        turn, ref, _ = K.fixture_round(f, r)
        want = A.record_received_np(state, **turn)
        D.record(ctx, dev, turn, want)
        state = want["state"]
        acks = A.build_acks_np(state, everyone, 255, 0)
        for k in ("largest", "hash", "range_ptr", "range_lo", "range_hi"):
            assert np.array_equal(acks[k], ref[k]), (r, k)
        D.build(ctx, dev, everyone, 255, 0, acks)
        rows += nc
    assert rows == 3840
