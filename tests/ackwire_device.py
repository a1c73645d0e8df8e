"""qfec_write_ack_frames run on the device and compared, whole buffers byte for
byte, with tests/ackwire_rule.py.  The discipline of ack_device.py: every array
carries one trailing entry nobody owns, the output buffer is POISON all over
(so the guard bytes around every frame's slot are part of the comparison), and
the inputs, the ring included, are compared unchanged."""
import numpy as np

import ackwire_rule as R
from ack_device import POISON8, POISON32, POISON64, host, same, sync, tail
from test_hip_accumulate_ragged import dview

POISON16 = np.uint16(0xA5A5)
TABLES = [("ack_conn", np.uint32, POISON32), ("largest", np.uint64, POISON64),
          ("hash", np.uint8, POISON8), ("truncated", np.uint8, POISON8),
          ("range_ptr", np.uint32, POISON32), ("range_lo", np.uint64, POISON64),
          ("range_hi", np.uint64, POISON64), ("rev_ptr", np.uint32, POISON32),
          ("rev_pn", np.uint64, POISON64)]
OUTPUTS = [("out_len", np.uint16, POISON16), ("wire_largest", np.uint64, POISON64),
           ("wire_hash", np.uint8, POISON8), ("status", np.uint8, POISON8)]


def write(ctx, batch, cells, window, out_off, out_cap, out_bytes, prefix_len=0, counts=True,
          rev_pn=True, want=None):
    """One qfec_write_ack_frames over `batch` (ackwire_rule's dict) compared with
    the rule; returns the rule's result.  cells: uint8[n_conns, window]."""
    n, n_conns = len(batch["ack_conn"]), cells.shape[0]
    if want is None:
        want = R.write_ack_frames(batch, cells, window, np.full(out_bytes, POISON8), out_off,
                                  out_cap, prefix_len)
    h = {name: tail(batch[name], dtype, poison) for name, dtype, poison in TABLES}
    h["delay"] = None if batch.get("delay") is None else tail(batch["delay"], np.uint64, POISON64)
    h["out_off"] = tail(out_off, np.uint64, POISON64)
    h["out_cap"] = tail(out_cap, np.uint16, POISON16)
    h["cells"] = tail(cells.reshape(-1), np.uint8, POISON8, 4)
    d = {k: None if v is None else dview(v) for k, v in h.items()}
    o = {name: dview(np.full(n + 1, poison, dtype)) for name, dtype, poison in OUTPUTS}
    out, cnt = dview(np.full(out_bytes, POISON8)), dview(np.full(5, POISON64))
    ctx.write_ack_frames(d["ack_conn"], n, d["largest"], d["hash"], d["truncated"], d["range_ptr"],
                         d["range_lo"], d["range_hi"], d["rev_ptr"], d["rev_pn"] if rev_pn else None,
                         d["cells"], n_conns, window, out, d["out_off"], d["out_cap"], o["out_len"],
                         o["wire_largest"], o["wire_hash"], o["status"], ack_delay_us=d["delay"],
                         prefix_len=prefix_len, counts=cnt if counts else None)
    sync(ctx, want["latched"])
    same("out", host(out, np.uint8), want["out"])
    for name, dtype, poison in OUTPUTS:
        same(name, host(o[name], dtype), tail(want[name], dtype, poison))
    same("counts", host(cnt, np.uint64),
         tail(want["counts"], np.uint64, POISON64) if counts else np.full(5, POISON64))
    for k, v in h.items():
        if v is not None:
            same(k, host(d[k], v.dtype), v)
    return want


def slots(cap, slot=None, lead=5):
    """a slot per ack with guard bytes in front and behind: (out_off, bytes)"""
    slot = slot or int(max(int(np.max(cap, initial=0)), 1)) + 11
    off = np.arange(len(cap), dtype=np.uint64) * np.uint64(slot) + np.uint64(lead)
    return off, len(cap) * slot + lead + 16
