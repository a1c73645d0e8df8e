"""tests/ack_rule.py pinned: its sequential and its NumPy form against each
other over random multi-turn traces, and both against the reference
QuicReceivedPacketManager's recorded acks (tests/golden/ack_ref.npz, every
row), plus the statements of integration/libquic_fec.patch about a revived
packet.  CPU only."""
import numpy as np
import pytest

import ack_cases as K
import ack_rule as A

ACK_KEYS = ("largest", "hash", "truncated", "range_ptr", "range_lo", "range_hi", "rev_ptr",
            "rev_pn")


def both_record(state, turn):
    a, b = A.record_received(state, **turn), A.record_received_np(state, **turn)
    assert np.array_equal(a["rcv_out"], b["rcv_out"])
    assert np.array_equal(a["counts"], b["counts"]), (a["counts"], b["counts"])
    assert a["latched"] == b["latched"]
    assert A.same_state(a["state"], b["state"])
    assert a["counts"][:6].sum() == len(turn.get("packet_number", ()))
    return a


def both_build(state, ack_conn, max_ranges, max_revived):
    a = A.build_acks(state, ack_conn, max_ranges, max_revived)
    b = A.build_acks_np(state, ack_conn, max_ranges, max_revived)
    for k in ACK_KEYS:
        assert np.array_equal(a[k], b[k]), k
    assert a["latched"] == b["latched"]
    return a


@pytest.mark.parametrize("window,n_conns,seed", [(64, 1, 1), (64, 3, 2), (256, 17, 3), (64, 40, 4)])
def test_forms_agree_on_random_turns(window, n_conns, seed):
    rng = np.random.default_rng(seed)
    state = A.new_state(n_conns, window)
    seen = np.zeros(12, np.uint64)
    for turn_no in range(30):
        turn = K.random_turn(rng, state, int(rng.integers(0, 40 * n_conns + 2)),
                             n_groups=int(rng.integers(0, 4 * n_conns + 1)),
                             n_raise=int(rng.integers(0, n_conns + 1)), hdr=turn_no % 3 != 0,
                             entropy=turn_no % 4 != 0, bad_conn=turn_no % 5 == 4)
        r = both_record(state, turn)
        seen += r["counts"]
        state = r["state"]
        conns = np.r_[rng.integers(0, n_conns, n_conns + 2), n_conns].astype(np.uint32)
        for mr, mv in ((1, 0), (2, 1), (255, 255)):
            both_build(state, conns, mr, mv)
    assert (seen > 0).all(), seen  # every class and every count occurred
    # the ring went round several times
    assert int(state["largest"].max()) > 3 * window


def test_reference_fixture():
    f = K.fixture()
    nc, span = int(f["n_conns"]), int(f["span"])
    everyone = np.arange(nc, dtype=np.uint32)
    for window in (64, 256):
        assert span <= window
        state, rows = A.new_state(nc, window), 0
        for r in range(int(f["n_rounds"])):
            turn, want, taken = K.fixture_round(f, r)
            rec = both_record(state, turn)
            state = rec["state"]
            assert rec["counts"][A.OVERFLOW] == 0 and rec["counts"][A.N_JUMPS] == 0
            # what the reference took is what set a new cell; it took nothing else
            assert rec["counts"][A.N_NEW] == taken.sum()
            assert (rec["rcv_out"][taken != 0] == A.RECORDED).all()
            got = both_build(state, everyone, 255, 0)
            assert not got["truncated"].any()
            for k in ("largest", "hash", "range_ptr", "range_lo", "range_hi"):
                assert np.array_equal(got[k], want[k]), (window, r, k)
            rows += nc
        assert rows == 3840


def test_revived_packet():
    """integration/libquic_fec.patch: a revived packet stays missing, is not in
    the hash, and is erased when it arrives itself or falls below the least."""
    state = A.new_state(1, 64)
    key = np.array([0 << K.KEY_SHIFT | 3], np.uint64)  # the group of packets 3..
    first = dict(packet_number=np.array([1, 2, 3, 5, 6], np.uint64), pkt_conn=np.zeros(5, np.uint32),
                 entropy=np.ones(5, np.uint8), status=np.array([1], np.uint8),
                 revived_idx=np.array([1], np.uint8), slot_key=key, key_shift=K.KEY_SHIFT)
    r = both_record(state, first)
    assert r["counts"][A.N_REVIVED] == 1 and r["state"]["cells"][0, 4] == A.REVIVED
    ack = both_build(r["state"], [0], 255, 255)
    assert ack["range_lo"].tolist() == [4] and ack["range_hi"].tolist() == [5]
    assert ack["rev_pn"].tolist() == [4]
    want_hash = 0
    for pn in (1, 2, 3, 5, 6):
        want_hash ^= 1 << (pn % 8)
    assert ack["hash"][0] == want_hash
    # revived at or above the largest, and one already received: ignored
    for idx in (3, 4, 0):
        again = both_record(r["state"], dict(status=np.array([1], np.uint8),
                                             revived_idx=np.array([idx], np.uint8), slot_key=key,
                                             key_shift=K.KEY_SHIFT))
        assert again["counts"][A.N_NOT_MISSING] == 1 and A.same_state(again["state"], r["state"])
    # it arrives itself
    late = both_record(r["state"], dict(packet_number=np.array([4], np.uint64),
                                        pkt_conn=np.zeros(1, np.uint32)))
    ack = both_build(late["state"], [0], 255, 255)
    assert len(ack["rev_pn"]) == 0 and len(ack["range_lo"]) == 0
    # or falls below the least
    gone = both_record(r["state"], dict(raise_conn=np.array([0], np.uint32),
                                        raise_least=np.array([5], np.uint64),
                                        raise_hash=np.array([0x5a], np.uint8)))
    assert gone["counts"][A.N_DROPPED] == 1 and gone["state"]["hash"][0] == 0x5a
    ack = both_build(gone["state"], [0], 255, 255)
    assert len(ack["rev_pn"]) == 0 and len(ack["range_lo"]) == 0


def test_live_cells_masks_the_rest():
    state = A.new_state(2, 64)
    state["cells"][:] = 0xFF
    state["least"][:] = (70, 0)
    state["largest"][:] = (72, 0)
    live = A.live_cells(state)
    assert live[0].nonzero()[0].tolist() == [6, 7, 8] and not live[1].any()
