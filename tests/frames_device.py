"""qfec_scan_frames run on the device and compared, whole buffers bit for bit,
with tests/frames_rule.py (scan_arrays).  The discipline of ack_device.py: every
array carries one trailing entry nobody owns (POISON where the call could
write), the table is POISON all over, so that the entries at and beyond what
was listed, frm_cap included, are part of the comparison, and the inputs -- the
packets' bytes with the guard bytes around every body -- are compared unchanged."""
import numpy as np

import frames_rule as R
from ack_device import POISON8, POISON32, POISON64, host, same, sync, tail
from test_hip_accumulate_ragged import dview

POISON16 = np.uint16(0xA5A5)
POISON = {np.uint8: POISON8, np.uint16: POISON16, np.uint32: POISON32, np.uint64: POISON64}
INPUTS = [("body_off", np.uint64), ("body_len", np.uint16), ("pn", np.uint64),
          ("conn", np.uint32), ("pn_len", np.uint8), ("hdr", np.uint8)]
STATE = [("seen", np.uint64), ("least", np.uint64), ("hash", np.uint8)]


def scan(ctx, data, body_off, body_len, pn, conn, pn_len, hdr, version, max_frames, frm_cap,
         state, n_conns, counts=True, tables=True):
    """One qfec_scan_frames compared with the rule; returns the rule's result.
    tables=False passes NULL table pointers (frm_cap must be 0)."""
    n = len(body_off)
    want = R.scan_arrays(data, body_off, body_len, pn, conn, pn_len, hdr, version, max_frames,
                         frm_cap, state, n_conns)
    given = dict(body_off=body_off, body_len=body_len, pn=pn, conn=conn, pn_len=pn_len, hdr=hdr)
    h = {k: None if given[k] is None else tail(given[k], dt, POISON[dt]) for k, dt in INPUTS}
    h["data"] = np.asarray(data, np.uint8)
    d = {k: None if v is None else dview(v) for k, v in h.items()}
    st = {k: dview(tail(state[k], dt, POISON[dt])) for k, dt in STATE}
    sw_conn = dview(np.full(n_conns + 1, POISON32))
    status, ptr = dview(np.full(n + 1, POISON8)), dview(np.full(n + 2, POISON32))
    cols = {name: dview(np.full(frm_cap + 1, POISON[dt], dt)) for name, dt in R.COLUMNS}
    cnt = dview(np.full(R.N_COUNTS + 1, POISON64))
    t = cols if tables else {name: None for name in cols}
    ctx.scan_frames(d["data"], d["body_off"], d["body_len"], d["pn"], d["conn"], d["pn_len"], n,
                    version, max_frames, status, ptr, st["seen"], st["least"], st["hash"], sw_conn,
                    n_conns, hdr=d["hdr"], frm_pkt=t["pkt"], frm_type=t["type"],
                    frm_flags=t["flags"], frm_off=t["off"], frm_len=t["len"], frm_id=t["id"],
                    frm_val=t["val"], frm_code=t["code"], frm_cap=frm_cap,
                    counts=cnt if counts else None)
    sync(ctx, want["latched"])
    same("frm_status", host(status, np.uint8), tail(want["status"], np.uint8, POISON8))
    same("frm_ptr", host(ptr, np.uint32), tail(want["ptr"], np.uint32, POISON32))
    for name, dt in R.COLUMNS:
        w = want["table"][name]
        same("frm_" + name, host(cols[name], dt), tail(w, dt, POISON[dt], frm_cap + 1 - len(w)))
    for k, dt in STATE:
        same("sw_" + k, host(st[k], dt), tail(want[k], dt, POISON[dt]))
    # (an empty call succeeds before the buffers are looked at: sw_conn stays as it was)
    same("sw_conn", host(sw_conn, np.uint32),
         tail(want["conn"], np.uint32, POISON32) if n else np.full(n_conns + 1, POISON32))
    same("counts", host(cnt, np.uint64),
         tail(want["counts"], np.uint64, POISON64) if counts else np.full(R.N_COUNTS + 1, POISON64))
    for k, v in h.items():
        if v is not None:
            same(k, host(d[k], v.dtype), v)
    return want
