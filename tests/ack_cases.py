"""Inputs for the ack-state tests: random turns around a state (arrivals that
are new, late, copies, stale, number 0 and beyond the window; revived groups
with their slot table; raises of every kind), and the reference fixture
tests/golden/ack_ref.npz cut into its rounds."""
import os

import numpy as np

import ack_rule as A

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ack_ref.npz")
KEY_SHIFT = 40


def random_turn(rng, state, n_packets, n_groups=0, n_raise=0, hdr=True, entropy=True,
                bad_conn=False):
    """kwargs of ack_rule.record_received for one turn against `state`"""
    w, nc = state["window"], len(state["least"])
    conn = rng.integers(0, nc, n_packets)
    least, big = state["least"][conn].astype(np.int64), state["largest"][conn].astype(np.int64)
    lo = np.maximum(least, 1)
    kind = rng.random(n_packets)
    ahead = big + 1 + rng.integers(0, max(2, w // 4), n_packets)          # new, mostly in reach
    inside = lo + rng.integers(0, 1 << 30, n_packets) % np.maximum(big - lo + 1, 1)
    old = rng.integers(0, 1 << 30, n_packets) % lo                         # stale, 0 included
    far = lo + w + rng.integers(0, 3, n_packets) - 1                        # at the window's edge
    pn = np.where(kind < 0.6, ahead, np.where(kind < 0.85, inside, np.where(kind < 0.95, old, far)))
    t = dict(packet_number=pn.astype(np.uint64), pkt_conn=conn.astype(np.uint32), key_shift=KEY_SHIFT)
    if bad_conn and n_packets:
        t["pkt_conn"][rng.integers(0, n_packets, max(1, n_packets // 50))] = nc + 3
    if hdr:
        h = rng.integers(0, 8, n_packets).astype(np.uint8)
        h[rng.random(n_packets) < 0.05] = 0x80 + rng.integers(0, 7)
        t["hdr"] = h
    if entropy:  # the parse's entropy_out: flag << (pn % 8)
        t["entropy"] = (rng.integers(0, 2, n_packets) << (pn % 8)).astype(np.uint8)
    if n_groups:
        n_slots = n_groups + 5
        c = rng.integers(0, nc, n_slots)
        first = np.maximum(state["largest"][c].astype(np.int64) - rng.integers(0, w // 2, n_slots), 1)
        key = (c.astype(np.uint64) << np.uint64(KEY_SHIFT)) | first.astype(np.uint64)
        key[rng.random(n_slots) < 0.05] = A.NO_KEY
        key[rng.random(n_slots) < 0.03] = np.uint64((nc + 1) << KEY_SHIFT | 5)  # connection out of range
        slot = rng.permutation(n_slots)[:n_groups].astype(np.uint32)
        slot[rng.random(n_groups) < 0.03] = n_slots + 1
        t.update(status=rng.choice([0, 1, 1, 2], n_groups).astype(np.uint8),
                 revived_idx=rng.integers(0, 12, n_groups).astype(np.uint8), slot=slot,
                 slot_key=key)
    if n_raise:
        rc = rng.permutation(nc)[:n_raise]
        least, big = state["least"][rc].astype(np.int64), state["largest"][rc].astype(np.int64)
        kind = rng.random(len(rc))
        up = np.where(kind < 0.15, rng.integers(0, 1 << 30, len(rc)) % (least + 1),  # <= least
                      np.where(kind < 0.7, least + 1 + rng.integers(0, 1 << 30, len(rc)) %
                               np.maximum(big + w // 8 - least, 1),
                               np.where(kind < 0.85, big + 1, big + 2 + rng.integers(0, w, len(rc)))))
        t.update(raise_conn=rc.astype(np.uint32), raise_least=up.astype(np.uint64),
                 raise_hash=rng.integers(0, 256, len(rc)).astype(np.uint8))
        if bad_conn:
            t["raise_conn"][0] = nc
    return t


def grown_state(rng, n_conns, window=64, calls=2, per_conn=20):
    """a state of many connections grown by `calls` random turns through the
    whole-array rule: missing, revived and raised packets on every side"""
    state = A.new_state(n_conns, window)
    for _ in range(calls):
        turn = random_turn(rng, state, per_conn * n_conns, n_groups=6 * n_conns,
                           n_raise=n_conns // 3)
        state = A.record_received_np(state, **turn)["state"]
    return state


def acks_ending_full(rng, state, n_acks, max_ranges, max_revived, truncated=False):
    """ack_conn of n_acks random connections (repeats included); the last one's
    ack has intervals and (where any may be listed) revived packets, and is
    truncated at max_ranges if asked"""
    n_conns = len(state["least"])
    every = A.build_acks_np(state, np.arange(n_conns), max_ranges, max_revived)
    such = np.diff(every["range_ptr"]) > 0
    if max_revived:
        such &= np.diff(every["rev_ptr"]) > 0
    if truncated:
        such &= every["truncated"] != 0
    such = np.flatnonzero(such)
    assert such.size, "no connection has such an ack"
    conn = rng.integers(0, n_conns, n_acks).astype(np.uint32)
    conn[-1] = such[rng.integers(0, such.size)]
    return conn


def fixture():
    return np.load(GOLDEN)


def fixture_round(f, r):
    """round r of the fixture: (kwargs of record_received, the reference's acks
    of every connection after it: largest, hash, range_ptr, range_lo, range_hi)"""
    p0, p1 = int(f["pkt_ptr"][r]), int(f["pkt_ptr"][r + 1])
    r0, r1 = int(f["raise_ptr"][r]), int(f["raise_ptr"][r + 1])
    nc = int(f["n_conns"])
    turn = dict(packet_number=f["pkt_pn"][p0:p1], pkt_conn=f["pkt_conn"][p0:p1],
                entropy=f["pkt_flag"][p0:p1], raise_conn=f["raise_conn"][r0:r1],
                raise_least=f["raise_least"][r0:r1], raise_hash=f["raise_hash"][r0:r1])
    ptr = f["range_ptr"][r * nc:(r + 1) * nc + 1]
    acks = dict(largest=f["ack_largest"][r], hash=f["ack_hash"][r],
                range_ptr=(ptr - ptr[0]).astype(np.uint32),
                range_lo=f["range_lo"][ptr[0]:ptr[-1]], range_hi=f["range_hi"][ptr[0]:ptr[-1]])
    return turn, acks, f["pkt_taken"][p0:p1]
