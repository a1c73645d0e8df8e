"""The receiver's turn with no raise from the host: test_hip_ack_wire_turn's turn
(sealed packets -> open -> qfec_parse_opened -> ... -> qfec_record_received ->
qfec_build_acks) with the peer's packets made of frames, some of them
STOP_WAITING, and qfec_scan_frames queued behind the parse.  The retire and the
record take the scan's dense state (raise_conn = sw_conn, raise_mark =
raise_least = sw_least, raise_hash = sw_hash, n_raise = their n_conns) where it
lies on the device; ONE qfec_sync at the end.

Checked: the frame table is the rule's over the opened bytes; and everything the
thresholds touch -- the packets the retire refuses, the closed slots, conn_mark,
every table of the turn, the ring and the built acks -- equals the same turn fed
the compact raises a host parsed out of the plaintexts (on the device, and by
the rules chained through tests/ack_rule.py)."""
import numpy as np
import pytest

import ack_device as D
import ack_rule as A
import assign_turns as T
import frames_cases as K
import frames_rule as FR
from libquic_amd import qfec
from test_hip_accumulate_ragged import dview
from test_hip_ack_turn import ACK_CONNS, WINDOW, Unsynced, sender_entropy
from test_hip_parse_turn import N_SLOTS, VERSION, Turn, device_turn
from test_hip_retire_turn import N_CONNS, P64, SHIFT, Device, check_turn, rule_turn

gpu = pytest.mark.gpu
U64 = np.uint64
MAX_FRAMES, FRM_CAP = 8, 1024


class FrameTurn(Turn):
    """Turn with every data packet's body made of frames (a group's FEC packet
    is their XOR, as before): a STOP_WAITING in some, a stream frame to the
    packet's end, pings where there is no room."""

    def __init__(self, seed):
        super().__init__(seed)
        rng = np.random.default_rng(seed + 1)
        s, group = self.s, np.array(self.s["group"])
        for p in range(self.n):
            if s["hdr"][p] & 4:
                continue
            size, pn = s["body"][p].size, s["pn"][p]
            body = b""
            if size >= 10 and rng.integers(0, 3) == 0:
                # (a threshold behind the connection's first two or three groups)
                least = min(pn, 100 + 1000 * s["conn"][p] + int(rng.integers(10, 20)))
                body = K.stop_waiting(pn, 6, least, int(rng.integers(0, 256)))
            rest = size - len(body)
            body += K.PING if rest == 1 else K.stream(p % 251 + 1, 0, rng.bytes(rest - 2),
                                                      length=False, id_len=1, off_len=0)
            s["body"][p] = np.frombuffer(body, np.uint8)
            assert len(body) == size
        for g in range(len(self.dropped)):  # the redundancy of the new bodies
            members = np.flatnonzero(group == g)
            parity = np.zeros(self.parity_len[g], np.uint8)
            for p in members[:-1]:
                parity[:s["body"][p].size] ^= s["body"][p]
            s["body"][members[-1]] = parity
        for p in range(self.n):  # the sender's arena and the receiver's plaintexts again
            end = self.pt_off[p] + self.pt_len[p]
            self.arena[end - s["body"][p].size:end] = s["body"][p]
        for a, p in enumerate(self.arrive):
            if p != self.bad:
                end = int(self.a_off[a]) + int(self.a_len[a])
                self.plain[end - s["body"][p].size:end] = s["body"][p]


@pytest.fixture(scope="module")
def turn():
    return FrameTurn(9300)


class Raising(Unsynced):
    """the turn's context with the retire's raises put in: the scan's dense
    state, queued behind the parse, or the lists a host built"""

    def __init__(self, ctx, m, raises=None):
        super().__init__(ctx)
        self.raises = raises
        if raises is None:
            self.sw = dict(seen=dview(np.zeros(N_CONNS + 1, U64)), least=dview(np.zeros(N_CONNS + 1, U64)),
                           hash=dview(np.zeros(N_CONNS + 1, np.uint8)),
                           conn=dview(np.full(N_CONNS + 1, 0xA5A5A5A5, np.uint32)))
            self.frm = {name: dview(np.full(FRM_CAP, 0xA5, np.uint8).repeat(np.dtype(dt).itemsize)
                                    .view(dt)) for name, dt in FR.COLUMNS}
            self.status = dview(np.full(m + 1, 0xA5, np.uint8))
            self.ptr = dview(np.full(m + 2, 0xA5A5A5A5, np.uint32))
            self.pn_len = dview(np.full(m + 1, 6, np.uint8))
            self.counts = dview(np.full(FR.N_COUNTS, P64))
        else:
            self.rc = dview(np.array([c for c, _, _ in raises] + [0], np.uint32))
            self.rm = dview(np.array([x for _, x, _ in raises] + [0], U64))
            self.rh = dview(np.array([h for _, _, h in raises] + [0], np.uint8))

    def parse_opened(self, data, pkt_off, pkt_len, packet_number, pkt_conn, n_packets, *args, **kw):
        self.parsed = dict(data=data, pn=packet_number, conn=pkt_conn, m=n_packets,
                           body_off=args[4], body_len=args[5], hdr=args[6])
        return self._ctx.parse_opened(data, pkt_off, pkt_len, packet_number, pkt_conn, n_packets,
                                      *args, **kw)

    def retire_groups(self, *args, **kw):
        if self.raises is None:
            p, f = self.parsed, self.frm
            self._ctx.scan_frames(p["data"], p["body_off"], p["body_len"], p["pn"], p["conn"],
                                  self.pn_len, p["m"], VERSION, MAX_FRAMES, self.status, self.ptr,
                                  self.sw["seen"], self.sw["least"], self.sw["hash"], self.sw["conn"],
                                  N_CONNS, hdr=p["hdr"], frm_pkt=f["pkt"], frm_type=f["type"],
                                  frm_flags=f["flags"], frm_off=f["off"], frm_len=f["len"],
                                  frm_id=f["id"], frm_val=f["val"], frm_code=f["code"],
                                  frm_cap=FRM_CAP, counts=self.counts)
            kw.update(raise_conn=self.sw["conn"], raise_mark=self.sw["least"], n_raise=N_CONNS)
        else:
            kw.update(raise_conn=self.rc, raise_mark=self.rm, n_raise=len(self.raises))
        return self._ctx.retire_groups(*args, **kw)

    def record_raises(self):
        if self.raises is None:  # the record's connections are the first ACK_CONNS
            return dict(raise_conn=self.sw["conn"], raise_least=self.sw["least"],
                        raise_hash=self.sw["hash"], n_raise=ACK_CONNS)
        return dict(raise_conn=self.rc, raise_least=self.rm, raise_hash=self.rh,
                    n_raise=len(self.raises))


def whole_turn(ctx, cipher, t, first, raises):
    """the turn to the built acks, one sync: (the wrapper, the device state,
    device_turn's tables, the ring, the acks)"""
    state = A.new_state(ACK_CONNS, WINDOW)
    state["least"][:] = first
    ack = D.DevState(state)
    dev = Device(ctx, T.KeyState(9301, N_SLOTS), np.append(np.zeros(N_CONNS, U64), P64))
    w = Raising(ctx, t.m, raises)
    d = device_turn(w, cipher, t, dev)
    ctx.record_received(*ack.args(), packet_number=d["a_pn"], pkt_conn=d["a_conn"], n_packets=t.m,
                        rcv_out=dview(np.zeros(t.m, np.uint8)), hdr=d["hdr"], entropy=d["entropy"],
                        status=d["st"], revived_idx=d["ridx"], slot_key=dev.key, n_groups=N_SLOTS,
                        n_slots=N_SLOTS, key_shift=SHIFT, **w.record_raises())
    n = ACK_CONNS
    o = dict(largest=dview(np.zeros(n, U64)), hash=dview(np.zeros(n, np.uint8)),
             truncated=dview(np.zeros(n, np.uint8)), range_ptr=dview(np.zeros(n + 1, np.uint32)),
             range_lo=dview(np.zeros(n * 255, U64)), range_hi=dview(np.zeros(n * 255, U64)),
             rev_ptr=dview(np.zeros(n + 1, np.uint32)), rev_pn=dview(np.zeros(n * 255, U64)))
    ctx.build_acks(dview(np.arange(n, dtype=np.uint32)), n, *ack.args(), 255, 255, o["largest"],
                   o["hash"], o["truncated"], o["range_ptr"], o["range_lo"], o["range_hi"],
                   o["rev_ptr"], o["rev_pn"])
    assert ctx.sync() == qfec.QFEC_OK  # the turn's only one
    acks = {k: D.host(v, dt) for (k, v), dt in zip(o.items(), (
        U64, np.uint8, np.uint8, np.uint32, U64, U64, np.uint32, U64))}
    return w, dev, d, ack.state(), acks, state


@gpu
@pytest.mark.parametrize("cipher", ["chacha20poly1305", "aes128gcm"])
def test_turn_without_host_raises(ctx, turn, cipher):
    t, m = turn, turn.m
    first, _, _ = sender_entropy(t)
    p = t.parsed
    pn_len = np.full(m, 6, np.uint8)
    # what a host would have had to do: read the plaintexts back and walk them
    want = FR.scan_arrays(t.plain, p["body_off"], p["body_len"], t.a_pn, t.a_conn, pn_len,
                          p["hdr"], VERSION, MAX_FRAMES, FRM_CAP, FR.new_state(N_CONNS), N_CONNS)
    raises = [(c, int(want["least"][c]), int(want["hash"][c]))
              for c in np.flatnonzero(want["seen"])]
    assert len(raises) == 6 and want["counts"][7] > 20 and not want["latched"]

    w, dev, d, ring, acks, state = whole_turn(ctx, cipher, t, first, None)
    # the scan, against the rule over the opened bytes
    assert np.array_equal(D.host(w.status, np.uint8)[:m], want["status"])
    assert np.array_equal(D.host(w.ptr, np.uint32)[:m + 1], want["ptr"])
    total = int(want["ptr"][-1])
    for name, dt in FR.COLUMNS:
        got = D.host(w.frm[name], dt)
        assert np.array_equal(got[:total], want["table"][name]), name
        assert (got[total:].view(np.uint8) == 0xA5).all(), name
    for k, dt in (("seen", U64), ("least", U64), ("hash", np.uint8), ("conn", np.uint32)):
        assert np.array_equal(D.host(w.sw[k], dt)[:N_CONNS], want[k]), k
    assert np.array_equal(D.host(w.counts, U64), want["counts"])
    # the turn by the rules, from the host-parsed raises
    marks = np.append(np.zeros(N_CONNS, U64), P64)
    rules = T.KeyState(9301, N_SLOTS)
    r = rule_turn(rules, t.h, marks, [(c, x) for c, x, _ in raises], 0, True)
    check_turn(cipher, d, r, True, rules, dev, marks)
    refused = (r["key_out"][:m] != t.h["a_key"][:m]).sum()
    assert refused > 10 and marks[:6].all()  # the thresholds bit: packets of groups below them
    hdr, entropy = D.host(d["hdr"], np.uint8)[:m], D.host(d["entropy"], np.uint8)[:m]
    rec = A.record_received(state, packet_number=t.a_pn, pkt_conn=t.a_conn, hdr=hdr,
                            entropy=entropy, status=D.host(d["st"], np.uint8),
                            revived_idx=D.host(d["ridx"], np.uint8),
                            slot_key=D.host(dev.key, U64)[:N_SLOTS], key_shift=SHIFT,
                            raise_conn=np.array([c for c, _, _ in raises], np.uint32),
                            raise_least=np.array([x for _, x, _ in raises], U64),
                            raise_hash=np.array([h for _, _, h in raises], np.uint8))
    assert A.same_state(ring, rec["state"])
    assert (rec["state"]["least"][:6] > first[:6]).all()  # every ring moved
    built = A.build_acks(rec["state"], np.arange(ACK_CONNS, dtype=np.uint32), 255, 255)
    for k in ("largest", "hash", "truncated", "range_ptr", "rev_ptr"):
        assert np.array_equal(acks[k], built[k]), k
    for k, ptr in (("range_lo", "range_ptr"), ("range_hi", "range_ptr"), ("rev_pn", "rev_ptr")):
        assert np.array_equal(acks[k][:built[ptr][-1]], built[k]), k

    # ... and the same turn on the device fed those raises from the host
    w2, dev2, d2, ring2, acks2, _ = whole_turn(ctx, cipher, t, first, raises)
    for key in ("key_out", "closed", "a_slot", "st", "ridx", "olen", "out", "r_cnt"):
        assert np.array_equal(d[key].cpu().numpy(), d2[key].cpu().numpy()), key
    assert np.array_equal(D.host(dev.marks, U64), D.host(dev2.marks, U64))
    assert np.array_equal(D.host(dev.len, np.uint16), D.host(dev2.len, np.uint16))
    assert A.same_state(ring, ring2)
    for k in acks:
        assert np.array_equal(acks[k], acks2[k]), k
