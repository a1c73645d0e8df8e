"""qfec_record_received and qfec_build_acks run on the device and compared, whole
buffers bit for bit, with tests/ack_rule.py.  The discipline of
test_hip_parse_opened.py: every array carries one trailing entry nobody owns
(POISON where the call could write; the ring a whole trailing word), the inputs
are compared unchanged, and the state is compared through ack_rule.live_cells,
the cells outside the live range being unspecified."""
import numpy as np
import pytest

import ack_rule as A
from libquic_amd import qfec
from test_hip_accumulate_ragged import dview

POISON8 = np.uint8(0xA5)
POISON32 = np.uint32(0xA5A5A5A5)
POISON64 = np.uint64(0xA5A5A5A5A5A5A5A5)
INPUTS = [("packet_number", np.uint64, POISON64), ("pkt_conn", np.uint32, POISON32),
          ("hdr", np.uint8, POISON8), ("entropy", np.uint8, POISON8), ("status", np.uint8, POISON8),
          ("revived_idx", np.uint8, POISON8), ("slot", np.uint32, POISON32),
          ("slot_key", np.uint64, POISON64), ("raise_conn", np.uint32, POISON32),
          ("raise_least", np.uint64, POISON64), ("raise_hash", np.uint8, POISON8)]


def host(t, dtype):
    return t.cpu().numpy().view(dtype)


def same(name, got, want):
    assert got.shape == want.shape, f"{name}: {got.shape} want {want.shape}"
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{name}: {bad.size} differ, first at {bad[0]}: {got[bad[0]]} " \
                          f"want {want[bad[0]]}"


def tail(a, dtype, poison, extra=1):
    return np.append(np.asarray(a, dtype), np.full(extra, poison, dtype))


def sync(ctx, latches):
    """-QUIC_INVALID_FEC_DATA once where something was out of range, then nothing"""
    if latches:
        with pytest.raises(qfec.InvalidFecData):
            ctx.sync()
    assert ctx.sync() == qfec.QFEC_OK


class DevState:
    """An ack state in device memory, each array with its trailing entry."""

    def __init__(self, state):
        self.window, self.n_conns = state["window"], len(state["least"])
        self.cells = dview(tail(state["cells"].reshape(-1), np.uint8, POISON8, 4))
        self.least = dview(tail(state["least"], np.uint64, POISON64))
        self.largest = dview(tail(state["largest"], np.uint64, POISON64))
        self.hash = dview(tail(state["hash"], np.uint8, POISON8))

    def args(self):
        return self.cells, self.least, self.largest, self.hash, self.n_conns, self.window

    def raw(self):
        return [host(self.cells, np.uint8).copy(), host(self.least, np.uint64).copy(),
                host(self.largest, np.uint64).copy(), host(self.hash, np.uint8).copy()]

    def state(self):
        """the state read back; nothing behind its ends was written"""
        cells, least, largest, hsh = self.raw()
        assert (cells[-4:] == POISON8).all() and least[-1] == POISON64
        assert largest[-1] == POISON64 and hsh[-1] == POISON8
        return dict(cells=cells[:-4].reshape(self.n_conns, self.window), least=least[:-1],
                    largest=largest[:-1], hash=hsh[:-1], window=self.window)


def record(ctx, dev, turn, want, counts=True, flags=0):
    """One qfec_record_received of `turn` (kwargs of ack_rule.record_received)
    on dev, compared with `want`, the rule's result over the state before."""
    turn = dict(turn)
    shift = turn.pop("key_shift", 40)
    n = len(turn.get("packet_number", ()))
    ng, nr = len(turn.get("status", ())), len(turn.get("raise_conn", ()))
    d, h = {}, {}
    for name, dtype, poison in INPUTS:
        if turn.get(name) is not None:
            h[name] = tail(turn[name], dtype, poison)
            d[name] = dview(h[name])
    out, cnt = dview(np.full(n + 1, POISON8)), dview(np.full(13, POISON64))
    ctx.record_received(*dev.args(), packet_number=d.get("packet_number"),
                        pkt_conn=d.get("pkt_conn"), n_packets=n, rcv_out=out, hdr=d.get("hdr"),
                        entropy=d.get("entropy"), status=d.get("status"),
                        revived_idx=d.get("revived_idx"), slot=d.get("slot"),
                        slot_key=d.get("slot_key"), n_groups=ng,
                        n_slots=len(turn.get("slot_key", ())), key_shift=shift,
                        raise_conn=d.get("raise_conn"), raise_least=d.get("raise_least"),
                        raise_hash=d.get("raise_hash"), n_raise=nr,
                        counts=cnt if counts else None, flags=flags)
    sync(ctx, want["latched"])
    same("rcv_out", host(out, np.uint8), tail(want["rcv_out"], np.uint8, POISON8))
    same("counts", host(cnt, np.uint64),
         tail(want["counts"], np.uint64, POISON64) if counts else np.full(13, POISON64))
    for name in d:
        same(name, host(d[name], h[name].dtype), h[name])
    got = dev.state()
    for k in ("least", "largest", "hash"):
        same(k, got[k], want["state"][k])
    same("live cells", A.live_cells(got).reshape(-1), A.live_cells(want["state"]).reshape(-1))


ACK_OUT = [("largest", np.uint64, POISON64), ("hash", np.uint8, POISON8),
           ("truncated", np.uint8, POISON8)]


def build(ctx, dev, ack_conn, max_ranges, max_revived, want, rev_pn=True, flags=0):
    """One qfec_build_acks compared with `want` (ack_rule.build_acks); the tables
    behind their used part, and the state, are as they were."""
    na = len(ack_conn)
    conn_h = tail(ack_conn, np.uint32, POISON32)
    conn = dview(conn_h)
    before = dev.raw()
    o = {name: dview(np.full(na + 1, poison, dtype)) for name, dtype, poison in ACK_OUT}
    rptr, vptr = dview(np.full(na + 2, POISON32)), dview(np.full(na + 2, POISON32))
    rlo = dview(np.full(na * max_ranges + 1, POISON64))
    rhi = dview(np.full(na * max_ranges + 1, POISON64))
    vpn = dview(np.full(na * max_revived + 1, POISON64))
    ctx.build_acks(conn, na, *dev.args(), max_ranges, max_revived, o["largest"], o["hash"],
                   o["truncated"], rptr, rlo, rhi, vptr, vpn if rev_pn else None, flags=flags)
    sync(ctx, want["latched"])
    for name, dtype, poison in ACK_OUT:
        same(name, host(o[name], dtype), tail(want[name], dtype, poison))
    same("range_ptr", host(rptr, np.uint32), tail(want["range_ptr"], np.uint32, POISON32))
    same("rev_ptr", host(vptr, np.uint32), tail(want["rev_ptr"], np.uint32, POISON32))
    for name, t, cap in (("range_lo", rlo, na * max_ranges), ("range_hi", rhi, na * max_ranges),
                         ("rev_pn", vpn, na * max_revived)):
        w = want[name]
        same(name, host(t, np.uint64), tail(w, np.uint64, POISON64, cap + 1 - len(w)))
    same("ack_conn", host(conn, np.uint32), conn_h)
    for name, a, b in zip(("cells", "least", "largest", "hash"), before, dev.raw()):
        same(name, b, a)
    return o, rptr, rlo, rhi, vptr, vpn
