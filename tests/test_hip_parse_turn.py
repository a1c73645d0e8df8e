"""One turn end to end with real packet protection, every step on the device:
qfec_write_private_headers -> seal -> open -> qfec_parse_opened ->
qfec_retire_groups -> qfec_assign_slots -> qfec_bin_arrivals ->
qfec_admit_ragged -> qfec_accumulate_ragged -> qfec_revive_tracked, queued on
one stream with ONE qfec_sync at the end.

About 40 groups on 6 connections (K = 3 + connection, the negotiated size),
bodies of 1..200 bytes.  Between seal and open one packet of every group is
dropped (a data packet, in every fifth group the FEC packet), the arrival
order is shuffled, one arrival's tag is corrupted and one arrives twice.  The
private headers exist in cleartext nowhere on the receiver's side: what the
turn knows of groups and positions it has from the opened bytes.

Checked: the revived bodies are the dropped packets' bodies; and every table,
status and list equals the same turn fed HOST-built pkt_key, pkt_idx and body
tables -- on the device (test_hip_retire_turn.Device) and by the rules chained
(test_hip_retire_turn.rule_turn over tests/assign_turns.py).
"""
import types

import numpy as np
import pytest
import torch

import admit_rule as R
import assign_rule as AS
import assign_turns as T
import parse_rule as PR
from libquic_amd import qfec
from test_hip_accumulate_ragged import dview
from test_hip_retire_turn import N_CONNS, P32, P64, SHIFT, Device, check_turn, rule_turn
from test_hip_tracked_turn import MS, PAD, POISON, STRIDE, host

gpu = pytest.mark.gpu
DEV = "cuda:0"
AD, TAG, VERSION, N_SLOTS = 8, 12, 31, 64
KLEN = {"chacha20poly1305": 32, "aes128gcm": 16}


def tail(a, dtype):
    return np.append(np.asarray(a, dtype), np.zeros(1, dtype))


class Turn:
    """The sender's packets, what of them arrives and in which order, and what
    the receiver must make of it."""

    def __init__(self, seed, n_groups=40):
        rng = np.random.default_rng(seed)
        # ---- the sender: group g on connection g % 6, K = 3 + connection
        next_pn = [100 + 1000 * c for c in range(6)]
        s = dict(conn=[], pn=[], hdr=[], fo=[], body=[], group=[])
        self.dropped, self.parity_len = [], []
        for g in range(n_groups):
            c = g % 6
            k = 3 + c
            next_pn[c] += int(rng.integers(0, 3))  # packets outside any group in between
            first = next_pn[c]
            bodies = [rng.integers(0, 256, int(rng.integers(1, 201)), dtype=np.uint8)
                      for _ in range(k)]
            parity = np.zeros(max(b.size for b in bodies), np.uint8)
            for b in bodies:
                parity[:b.size] ^= b
            for i, b in enumerate(bodies + [parity]):
                s["conn"].append(c)
                s["pn"].append(first + i)
                s["hdr"].append((0x06 if i == k else 0x02) | int(rng.integers(0, 2)))
                s["fo"].append(i)
                s["body"].append(b)
                s["group"].append(g)
            next_pn[c] = first + k + 1
            self.dropped.append(k if g % 5 == 4 else int(rng.integers(0, k)))
            self.parity_len.append(parity.size)
        for c in range(6):  # and a packet in no group on every connection
            s["conn"].append(c)
            s["pn"].append(next_pn[c] + 5)
            s["hdr"].append(int(rng.integers(0, 2)))
            s["fo"].append(0)
            s["body"].append(rng.integers(0, 256, 40, dtype=np.uint8))
            s["group"].append(-1)
        self.n = n = len(s["pn"])
        self.s = s
        pt_len = np.array([b.size for b in s["body"]]) + np.where(np.array(s["group"]) >= 0, 2, 1)
        # the sender's arena: [associated data][private header, body], byte-packed
        self.ad_off = np.cumsum(AD + pt_len + 1) - (AD + pt_len + 1)
        self.pt_off, self.pt_len = self.ad_off + AD, pt_len
        self.arena = np.full(int(self.ad_off[-1] + AD + pt_len[-1]) + 8, 0xEE, np.uint8)
        self.ads = rng.integers(0, 256, (n, AD), dtype=np.uint8)
        for p in range(n):
            self.arena[self.ad_off[p]:self.ad_off[p] + AD] = self.ads[p]
            end = self.pt_off[p] + pt_len[p]
            self.arena[end - s["body"][p].size:end] = s["body"][p]
        # the wire: [associated data][ciphertext and tag]
        self.w_ad = np.cumsum(AD + pt_len + TAG + 3) - (AD + pt_len + TAG + 3)
        self.w_ct = self.w_ad + AD
        self.wire = np.full(int(self.w_ct[-1] + pt_len[-1] + TAG) + 8, POISON, np.uint8)
        for p in range(n):
            self.wire[self.w_ad[p]:self.w_ad[p] + AD] = self.ads[p]
        self.table = rng.integers(0, 256, (6, 36), dtype=np.uint8)  # a key and a prefix per connection
        # ---- the network: a drop per group, a duplicate, a shuffle, a corrupted tag
        group = np.array(s["group"])
        gone = {int(np.flatnonzero(group == g)[self.dropped[g]]) for g in range(n_groups)}
        arrive = [p for p in range(n) if p not in gone]
        self.dup = next(p for p in arrive if group[p] == 7 and s["fo"][p] < 3 + 7 % 6)
        arrive = np.array(arrive + [self.dup])[rng.permutation(len(arrive) + 1)]
        self.bad = int(next(p for p in arrive if group[p] == 11))
        self.arrive, self.m = arrive, len(arrive)
        # ---- the receiver's tables, in arrival order: all from the public header
        self.a_pn = np.array(s["pn"], np.uint64)[arrive]
        self.a_conn = np.array(s["conn"], np.uint32)[arrive]
        self.a_k = (3 + self.a_conn).astype(np.uint8)
        self.a_len = pt_len[arrive].astype(np.uint16)
        self.a_off = (np.cumsum(self.a_len.astype(np.int64) + 3) - self.a_len - 3 + 5).astype(np.uint64)
        self.a_ok = (arrive != self.bad).astype(np.uint8)
        # what the open leaves: the plaintexts of the arrivals that verify
        self.plain = np.full(int(self.a_off[-1]) + int(self.a_len[-1]) + 32, PAD, np.uint8)
        for a, p in enumerate(arrive):
            if p != self.bad:
                b = s["body"][p]
                head = [s["hdr"][p], s["fo"][p]] if group[p] >= 0 else [s["hdr"][p]]
                o = int(self.a_off[a])
                self.plain[o:o + len(head)] = head
                self.plain[o + len(head):o + len(head) + b.size] = b
        # the tables a host would build had it read those plaintexts back
        self.parsed = PR.parse_opened(self.plain, self.a_off, self.a_len, self.a_pn, self.a_conn,
                                      self.a_ok, VERSION, SHIFT)
        w = self.parsed
        self.h = dict(m=self.m, w=types.SimpleNamespace(plain=self.plain),
                      a_key=tail(w["key"], np.uint64), a_k=tail(self.a_k, np.uint8),
                      a_pt_off=tail(w["body_off"], np.uint64), a_ln=tail(w["body_len"], np.uint16),
                      a_idx=tail(w["idx"], np.uint8), a_good=tail(self.a_ok, np.uint8))


@pytest.fixture(scope="module")
def turn():
    return Turn(9300)


def device_turn(ctx, cipher, t, dev):
    """the whole turn queued from the sender's arena to the revive; one sync"""
    n, m, s, n_slots = t.n, t.m, t.s, N_SLOTS
    keys = dview(np.ascontiguousarray(t.table[:, :KLEN[cipher]]).ravel())
    prefixes = dview(np.ascontiguousarray(t.table[:, 32:]).ravel())
    seal, open_ = getattr(ctx, cipher + "_seal"), getattr(ctx, cipher + "_open")
    arrive = t.arrive
    d = dict(arena=dview(t.arena), wire=dview(t.wire), s_off=dview(t.pt_off.astype(np.uint64)),
             s_hdr=dview(np.array(s["hdr"], np.uint8)), s_fo=dview(np.array(s["fo"], np.uint8)),
             s_body=dview(np.full(n, P64)), s_cnt=dview(np.full(2, P64)),
             opened=torch.full((t.plain.size,), PAD, dtype=torch.uint8, device=DEV),
             ok=dview(np.full(m + 1, POISON, np.uint8)),
             a_off=dview(tail(t.a_off, np.uint64)), a_len=dview(tail(t.a_len, np.uint16)),
             a_pn=dview(tail(t.a_pn, np.uint64)), a_conn=dview(tail(t.a_conn, np.uint32)),
             k=dview(tail(t.a_k, np.uint8)),
             key=dview(np.full(m + 1, P64)), idx=dview(np.full(m + 1, POISON, np.uint8)),
             body_off=dview(np.full(m + 1, P64)), body_len=dview(np.full(m + 1, 0xA5A5, np.uint16)),
             hdr=dview(np.full(m + 1, POISON, np.uint8)),
             entropy=dview(np.full(m + 1, POISON, np.uint8)), p_cnt=dview(np.full(6, P64)),
             key_out=dview(np.full(m + 1, P64, np.uint64)),
             closed=dview(np.full(n_slots + 1, P32, np.uint32)), r_cnt=dview(np.zeros(5, np.uint64)),
             a_slot=dview(np.full(m + 1, POISON, np.uint32)), a_cnt=dview(np.zeros(5, np.uint64)),
             t_ptr=dview(np.full(n_slots + 1, POISON, np.uint32)),
             t_off=dview(np.full(m + 1, POISON, np.uint64)),
             t_ln=dview(np.full(m + 1, POISON, np.uint16)),
             t_idx=dview(np.full(m + 1, POISON, np.uint8)),
             t_ok=dview(np.full(m + 1, POISON, np.uint8)),
             t_src=dview(np.full(m + 1, POISON, np.uint32)), b_cnt=dview(np.zeros(3, np.uint64)),
             o_ptr=dview(np.full(n_slots + 1, POISON, np.uint32)),
             o_off=dview(np.zeros(m + 1, np.uint64)), o_ln=dview(np.zeros(m + 1, np.uint16)),
             v=dview(np.full(m + 1, POISON, np.uint8)), cnt=dview(np.zeros(4, np.uint64)),
             out=torch.full((n_slots * STRIDE + 32,), PAD, dtype=torch.uint8, device=DEV),
             olen=dview(np.zeros(n_slots, np.uint16)), st=dview(np.zeros(n_slots, np.uint8)),
             ridx=dview(np.zeros(n_slots, np.uint8)), rlist=dview(np.full(n_slots, P64, np.uint64)),
             counts=dview(np.zeros(3, np.uint64)),
             len_retired=torch.empty(n_slots + 1, dtype=torch.int16, device=DEV),
             slot_key=torch.empty(n_slots + 1, dtype=torch.int64, device=DEV),
             slot_k=torch.empty(n_slots + 1, dtype=torch.uint8, device=DEV))
    # ---- the sender
    ctx.write_private_headers(d["arena"], d["s_off"], d["s_hdr"], d["s_fo"], n, VERSION,
                              body_off_out=d["s_body"], counts=d["s_cnt"])
    pn, conn = np.array(s["pn"], np.uint64), np.array(s["conn"], np.uint32)
    path = np.zeros(n, np.uint8)
    ad_len = np.full(n, AD, np.uint16)
    seal(keys, prefixes, dview(conn), dview(pn), dview(path), d["arena"],
         dview(t.ad_off.astype(np.uint64)), dview(ad_len), d["s_off"],
         dview(t.pt_len.astype(np.uint16)), n, d["wire"], dview(t.w_ct.astype(np.uint64)))
    # ---- the network: the last byte of one tag (a device op on the same stream)
    at = int(t.w_ct[t.bad] + t.pt_len[t.bad] + TAG - 1)
    d["wire"][at:at + 1].bitwise_xor_(0x10)
    # ---- the receiver
    open_(keys, prefixes, dview(conn[arrive]), d["a_pn"], dview(path[arrive]), d["wire"],
          dview(t.w_ad[arrive].astype(np.uint64)), dview(ad_len[arrive]),
          dview(t.w_ct[arrive].astype(np.uint64)), dview((t.pt_len[arrive] + TAG).astype(np.uint16)),
          m, d["opened"], d["a_off"], d["ok"])
    ctx.parse_opened(d["opened"], d["a_off"], d["a_len"], d["a_pn"], d["a_conn"], m, VERSION, SHIFT,
                     d["key"], d["idx"], d["body_off"], d["body_len"], d["hdr"], pkt_ok=d["ok"],
                     entropy_out=d["entropy"], counts=d["p_cnt"])
    ctx.retire_groups(d["key"], m, dev.key, dev.len, n_slots, dev.marks, N_CONNS, SHIFT, 0,
                      d["key_out"], closed_list=d["closed"], counts=d["r_cnt"])
    d["len_retired"].copy_(dev.len)
    ctx.assign_slots(d["key_out"], d["k"], m, dev.key, dev.k, dev.len, n_slots, d["a_slot"],
                     counts=d["a_cnt"])
    d["slot_key"].copy_(dev.key)
    d["slot_k"].copy_(dev.k)
    ctx.bin_arrivals(d["a_slot"], d["body_off"], d["body_len"], d["idx"], d["ok"], m, n_slots,
                     d["t_ptr"], d["t_off"], d["t_ln"], d["t_idx"], pkt_ok_out=d["t_ok"],
                     src_out=d["t_src"], counts=d["b_cnt"])
    ctx.admit_ragged(d["t_off"], d["t_ln"], d["t_idx"], d["t_ok"], d["t_ptr"], n_slots, dev.k,
                     dev.maps, MS, dev.len, STRIDE, d["o_ptr"], d["o_off"], d["o_ln"], d["v"],
                     slot=None, n_slots=n_slots, counts=d["cnt"])
    ctx.accumulate_ragged(d["opened"], d["o_off"], d["o_ln"], d["o_ptr"], n_slots, dev.acc, STRIDE,
                          dev.len, slot=None, n_slots=n_slots)
    ctx.revive_tracked(dev.acc, STRIDE, dev.len, dev.maps, MS, dev.k, n_slots, d["out"],
                       dev.out_off, d["olen"], status=d["st"], slot=None, n_slots=n_slots,
                       revived_idx=d["ridx"], revived_list=d["rlist"], counts=d["counts"],
                       release_mask=T.MASK)
    assert ctx.sync() == qfec.QFEC_OK  # the turn's only one
    return d


@gpu
@pytest.mark.parametrize("cipher", ["chacha20poly1305", "aes128gcm"])
def test_turn_from_sealed_packets(ctx, turn, cipher):
    t = turn
    m, n_groups = t.m, len(t.dropped)
    marks = np.append(np.zeros(N_CONNS, np.uint64), P64)
    # the turn by the rules, from the host-built tables
    state = T.KeyState(9301, N_SLOTS)
    r = rule_turn(state, t.h, marks, [], 0, True)
    # ... on the device from the host-built tables
    host_dev = Device(ctx, T.KeyState(9301, N_SLOTS), marks)
    check_turn("host tables", host_dev.turn(t.h, [], 0, True), r, True, state, host_dev, marks)
    # ... and from the sealed packets alone
    dev = Device(ctx, T.KeyState(9301, N_SLOTS), marks)
    d = device_turn(ctx, cipher, t, dev)
    # the sender's headers went where the bodies were waiting
    assert host(d["s_cnt"], np.uint64).tolist() == [t.n, 0]
    grouped = np.array(t.s["group"]) >= 0
    assert np.array_equal(host(d["s_body"], np.uint64),
                          (t.pt_off + np.where(grouped, 2, 1)).astype(np.uint64))
    # the open's verdicts, and the parse against the rule
    assert np.array_equal(host(d["ok"], np.uint8), np.append(t.a_ok, POISON))
    for name, key, dtype in (("key", "key", np.uint64), ("idx", "idx", np.uint8),
                             ("body_off", "body_off", np.uint64), ("body_len", "body_len", np.uint16),
                             ("hdr", "hdr", np.uint8), ("entropy", "entropy", np.uint8)):
        assert np.array_equal(host(d[key], dtype)[:m], t.parsed[name]), name
    assert host(d["p_cnt"], np.uint64).tolist() == t.parsed["counts"].tolist()
    cnt = t.parsed["counts"]
    assert cnt[PR.N_FAILED] == 1 and cnt[PR.N_NONE] == 6 and cnt[PR.N_REJECTED] == 0
    assert cnt[PR.N_DATA] + cnt[PR.N_FEC] == m - 7 and cnt[PR.N_FEC] == n_groups - n_groups // 5 - \
        (t.s["fo"][t.bad] == 3 + t.s["conn"][t.bad])
    # every table of the turn equals the turn from host-built tables
    check_turn(cipher, d, r, True, state, dev, marks)
    # and the revived bodies are the dropped packets' bodies
    group = np.array(t.s["group"])
    revived = 0
    for g in range(n_groups):
        a = next(a for a, p in enumerate(t.arrive) if group[p] == g and p != t.bad)
        slot = int(r["a_slot"][a])
        assert slot != AS.NO_SLOT and r["slot_key"][slot] == ((g % 6) << SHIFT | t.s["pn"][t.arrive[a]]
                                                              - t.s["fo"][t.arrive[a]])
        k = 3 + g % 6
        if g == group[t.bad]:
            assert r["st"][slot] == R.UNREVIVABLE
        elif t.dropped[g] == k:
            assert r["st"][slot] == R.COMPLETE
        else:
            lost = t.s["body"][int(np.flatnonzero(group == g)[t.dropped[g]])]
            assert r["st"][slot] == R.REVIVED and r["ridx"][slot] == t.dropped[g]
            assert r["olen"][slot] == t.parity_len[g]
            row = host(d["out"], np.uint8)[slot * STRIDE:slot * STRIDE + t.parity_len[g]]
            assert np.array_equal(row[:lost.size], lost) and not row[lost.size:].any()
            revived += 1
    assert revived == n_groups - n_groups // 5 - 1 == int(r["counts"][R.REVIVED])
    # (the packet that arrived twice: folded once)
    src = r["t_src"][:m].tolist()
    assert sorted(int(r["v"][src.index(a)]) for a, p in enumerate(t.arrive) if p == t.dup) == \
        [R.ADMITTED, R.DUPLICATE]
