"""The receiver's whole turn on one stream, ending in the acks:
qfec_write_private_headers -> seal -> (loss, reordering, a duplicate, a
corrupted tag) -> open -> qfec_parse_opened -> qfec_retire_groups ->
qfec_assign_slots -> qfec_bin_arrivals -> qfec_admit_ragged ->
qfec_accumulate_ragged -> qfec_revive_tracked -> qfec_record_received ->
qfec_build_acks, with ONE qfec_sync at the end.  The sender and the network
are test_hip_parse_turn's (about 40 groups on 6 connections, a packet of every
group lost).

Checked: every built ack, the truncated ones included, validates against the
sender's own entropy bookkeeping (qfec_entropy_cumulative_batch over what it
sent, qfec_entropy_validate_batch); the revived lists are the revive's own
revived_list mapped to packet numbers; and the acks equal those of the same
turn with the tables built by the host through tests/ack_rule.py."""
import numpy as np
import pytest

import ack_device as D
import ack_rule as A
import assign_turns as T
from libquic_amd import qfec
from test_hip_accumulate_ragged import dview
from test_hip_parse_turn import N_SLOTS, Turn, device_turn
from test_hip_retire_turn import N_CONNS, P64, SHIFT, Device

gpu = pytest.mark.gpu
U64 = np.uint64
WINDOW, ACK_CONNS = 256, 8  # (connections 6 and 7 never hear anything)


class Unsynced:
    """the context with the turn's sync put off: record and build are queued
    behind the revive before anything is waited for"""

    def __init__(self, ctx):
        self._ctx = ctx

    def __getattr__(self, name):
        return getattr(self._ctx, name)

    def sync(self):
        return qfec.QFEC_OK


@pytest.fixture(scope="module")
def turn():
    return Turn(9300)


def sender_entropy(t):
    """the sender's bookkeeping: per connection the hashes of its packet
    numbers from the first on (a number it never used: sent, lost, flag 0)"""
    pn, conn, hdr = np.array(t.s["pn"]), np.array(t.s["conn"]), np.array(t.s["hdr"])
    first = np.array([pn[conn == c].min() if (conn == c).any() else 1 for c in range(ACK_CONNS)])
    last = np.array([pn[conn == c].max() if (conn == c).any() else 0 for c in range(ACK_CONNS)])
    ptr = np.r_[0, np.cumsum(last - first + 1)]
    ent = np.zeros(ptr[-1], np.uint8)
    ent[ptr[conn] + pn - first[conn]] = (hdr & 1) << (pn % 8)
    return first.astype(U64), ptr.astype(U64), ent


@gpu
@pytest.mark.parametrize("cipher,max_ranges,max_revived", [("chacha20poly1305", 255, 255),
                                                           ("aes128gcm", 2, 1)])
def test_turn_to_acks(ctx, turn, cipher, max_ranges, max_revived):
    t, m = turn, turn.m
    first, ptr, ent = sender_entropy(t)
    # the ack state: every connection awaits its sender's first packet
    state = A.new_state(ACK_CONNS, WINDOW)
    state["least"][:] = first
    ack = D.DevState(state)
    everyone = np.arange(ACK_CONNS, dtype=np.uint32)
    conn = dview(everyone)
    marks = np.append(np.zeros(N_CONNS, U64), P64)
    dev = Device(ctx, T.KeyState(9301, N_SLOTS), marks)
    d = device_turn(Unsynced(ctx), cipher, t, dev)
    rcv_out, r_cnt = dview(np.full(m, 0xA5, np.uint8)), dview(np.zeros(12, U64))
    ctx.record_received(*ack.args(), packet_number=d["a_pn"], pkt_conn=d["a_conn"], n_packets=m,
                        rcv_out=rcv_out, hdr=d["hdr"], entropy=d["entropy"], status=d["st"],
                        revived_idx=d["ridx"], slot_key=dev.key, n_groups=N_SLOTS, n_slots=N_SLOTS,
                        key_shift=SHIFT, counts=r_cnt)
    o = dict(largest=dview(np.zeros(ACK_CONNS, U64)), hash=dview(np.zeros(ACK_CONNS, np.uint8)),
             truncated=dview(np.zeros(ACK_CONNS, np.uint8)),
             range_ptr=dview(np.zeros(ACK_CONNS + 1, np.uint32)),
             range_lo=dview(np.zeros(ACK_CONNS * max_ranges, U64)),
             range_hi=dview(np.zeros(ACK_CONNS * max_ranges, U64)),
             rev_ptr=dview(np.zeros(ACK_CONNS + 1, np.uint32)),
             rev_pn=dview(np.zeros(ACK_CONNS * max_revived, U64)))
    ctx.build_acks(conn, ACK_CONNS, *ack.args(), max_ranges, max_revived, o["largest"], o["hash"],
                   o["truncated"], o["range_ptr"], o["range_lo"], o["range_hi"], o["rev_ptr"],
                   o["rev_pn"])
    # the sender validates them (device tables throughout)
    cum, ok = dview(np.zeros(ent.size, np.uint8)), dview(np.full(ACK_CONNS, 0xA5, np.uint8))
    d_ptr, d_first = dview(ptr), dview(first)
    ctx.entropy_cumulative(dview(ent), d_ptr, None, ACK_CONNS, cum, n_packets=ent.size)
    ctx.entropy_validate(cum, d_ptr, d_first, None, ACK_CONNS, conn, o["largest"], o["hash"],
                         o["range_ptr"], o["range_lo"], o["range_hi"], ACK_CONNS, ok)
    assert ctx.sync() == qfec.QFEC_OK  # the turn's only one
    got = {k: D.host(v, v_dtype) for (k, v), v_dtype in zip(o.items(), (
        U64, np.uint8, np.uint8, np.uint32, U64, U64, np.uint32, U64))}
    # connections 0..5 heard something; every one of their acks validates
    assert D.host(ok, np.uint8)[:6].tolist() == [1] * 6
    if max_ranges == 2:
        assert got["truncated"][:6].all()
    else:
        assert not got["truncated"].any()
    # the same turn with the tables built by the host through the rule
    hdr, entropy = D.host(d["hdr"], np.uint8)[:m], D.host(d["entropy"], np.uint8)[:m]
    assert np.array_equal(hdr, t.parsed["hdr"]) and np.array_equal(entropy, t.parsed["entropy"])
    st, ridx = D.host(d["st"], np.uint8), D.host(d["ridx"], np.uint8)
    slot_key = D.host(dev.key, U64)[:N_SLOTS]
    want = A.record_received(state, packet_number=t.a_pn, pkt_conn=t.a_conn, hdr=hdr,
                             entropy=entropy, status=st, revived_idx=ridx, slot_key=slot_key,
                             key_shift=SHIFT)
    assert np.array_equal(D.host(rcv_out, np.uint8), want["rcv_out"])
    assert np.array_equal(D.host(r_cnt, U64), want["counts"])
    cnt = want["counts"]
    assert cnt[A.NOT_ACCEPTED] == 1 and cnt[A.RECORDED] == m - 1 and cnt[A.N_NEW] == m - 2
    assert A.same_state(ack.state(), want["state"])
    acks = A.build_acks(want["state"], everyone, max_ranges, max_revived)
    for k in ("largest", "hash", "truncated", "range_ptr", "rev_ptr"):
        assert np.array_equal(got[k], acks[k]), k
    for k, p in (("range_lo", "range_ptr"), ("range_hi", "range_ptr"), ("rev_pn", "rev_ptr")):
        assert np.array_equal(got[k][:acks[p][-1]], acks[k]), k
    # the revived lists are the revive's own list, as packet numbers
    n_rev = int((st == qfec.GROUP_REVIVED).sum())
    rlist = D.host(d["rlist"], U64)[:n_rev].astype(np.int64)
    assert rlist.tolist() == np.flatnonzero(st == qfec.GROUP_REVIVED).tolist()
    assert cnt[A.N_REVIVED] == n_rev and cnt[A.N_NOT_MISSING] == 0
    for c in range(ACK_CONNS):
        mine = sorted((int(k) & ((1 << SHIFT) - 1)) + int(ridx[s])
                      for s, k in zip(rlist, slot_key[rlist]) if int(k) >> SHIFT == c)
        mine = [pn for pn in mine if pn <= int(got["largest"][c])]
        listed = got["rev_pn"][got["rev_ptr"][c]:got["rev_ptr"][c + 1]].tolist()
        assert listed == mine[len(mine) - min(len(mine), max_revived):], c
    assert got["rev_ptr"][-1] > 0
