"""The host refusals of qfec_scan_frames, each alone and in the order
include/qfec.h gives them (with every later fault present as well, the earlier
one answers): QFEC_ERR_INTERNAL, its message, nothing launched and no buffer
written."""
import numpy as np
import pytest
import torch

from libquic_amd import qfec
from test_hip_accumulate_ragged import dview

gpu = pytest.mark.gpu
POISON = 0xA5
NP, NC, CAP = 6, 3, 10
SCAN = ["bytes", "body_off", "body_len", "packet_number", "pkt_conn", "pkt_pn_len", "hdr",
        "n_packets", "quic_version", "max_frames", "frm_status", "frm_ptr", "frm_pkt", "frm_type",
        "frm_flags", "frm_off", "frm_len", "frm_id", "frm_val", "frm_code", "frm_cap", "sw_seen",
        "sw_least", "sw_hash", "sw_conn", "n_conns", "counts", "flags"]
SCALARS = dict(n_packets=NP, quic_version=31, max_frames=8, frm_cap=CAP, n_conns=NC, flags=0)
OPTIONAL = ("hdr", "counts")
TABLES = ("frm_pkt", "frm_type", "frm_flags", "frm_off", "frm_len", "frm_id", "frm_val", "frm_code")
STATE = ("sw_seen", "sw_least", "sw_hash", "sw_conn")


def buffers():
    sizes = dict(bytes=64, body_off=8 * NP, body_len=2 * NP, packet_number=8 * NP, pkt_conn=4 * NP,
                 pkt_pn_len=NP, hdr=NP, frm_status=NP, frm_ptr=4 * (NP + 1), frm_pkt=4 * CAP,
                 frm_type=CAP, frm_flags=CAP, frm_off=8 * CAP, frm_len=2 * CAP, frm_id=4 * CAP,
                 frm_val=8 * CAP, frm_code=4 * CAP, sw_seen=8 * NC, sw_least=8 * NC, sw_hash=NC,
                 sw_conn=4 * NC, counts=8 * 13)
    return {k: dview(np.full(n, POISON, np.uint8)) for k, n in sizes.items()}


FLAGS = [dict(flags=f) for f in (qfec.QFEC_PTR_HOST, qfec.QFEC_PTR_MAPPED, qfec.QFEC_ASYNC)]
# (faults, a fragment of the message), in the order of the checks
LADDER = [(FLAGS[0], "device pointers only"), (dict(frm_status=None), "null buffer"),
          (dict(quic_version=34), "quic_version 34 outside [1, 33]"),
          (dict(max_frames=256), "max_frames 256 outside [1, 255]"),
          (dict(n_packets=1 << 32), "2^32 or more")]
ALONE = [(f, "device pointers only") for f in FLAGS[1:]] + [
    (dict([(k, None)]), "null buffer") for k in SCAN if k not in SCALARS and k not in OPTIONAL] + [
    (dict(quic_version=0), "quic_version 0"), (dict(max_frames=0), "max_frames 0"),
    (dict(n_conns=1 << 32), "2^32 or more"), (dict(frm_cap=1 << 32), "2^32 or more"),
    (dict(n_packets=1 << 29, max_frames=8), "2^32 or more")]


@gpu
def test_scan_frames_refusals(ctx):
    bufs = buffers()
    before = {k: t.cpu() for k, t in bufs.items()}
    good = dict(bufs, **SCALARS)

    def call(**kw):
        a = dict(good, **kw)
        rc = ctx.lib.qfec_scan_frames(ctx.ctx, *[qfec._ptr(a[x]) for x in SCAN])
        return rc, ctx.lib.qfec_last_error(ctx.ctx).decode()

    def untouched(but=()):
        assert ctx.sync() == qfec.QFEC_OK
        for k, t in bufs.items():
            assert k in but or torch.equal(t.cpu(), before[k]), k

    def refused(faults, fragment):
        rc, msg = call(**faults)
        assert rc == qfec.QFEC_ERR_INTERNAL and fragment in msg, (faults, rc, msg)
        untouched()

    for i, (_, fragment) in enumerate(LADDER):
        faults = {}
        for kw, _ in reversed(LADDER[i:]):
            faults.update(kw)
        refused(faults, fragment)
    for faults, fragment in ALONE:
        refused(faults, fragment)
    # nothing to do: decided before the buffers are looked at; counts zeroed, an empty table
    empty = {k: None for k in SCAN if k not in SCALARS and k not in ("counts", "frm_ptr")}
    rc, msg = call(n_packets=0, quic_version=99, max_frames=0, **empty)
    assert rc == qfec.QFEC_OK, msg
    untouched(but=("counts", "frm_ptr"))
    assert not bufs["counts"].cpu().numpy().any()
    ptr = bufs["frm_ptr"].cpu().numpy()
    assert not ptr[:4].any() and (ptr[4:] == POISON).all()
    rc, msg = call(n_packets=0, counts=None, frm_ptr=None, **empty)
    assert rc == qfec.QFEC_OK, msg
    # the tables with frm_cap == 0 and the state of no connection may be NULL: every
    # packet is then out of range, which is latched
    nulls = {k: None for k in TABLES + STATE}
    rc, msg = call(frm_cap=0, n_conns=0, hdr=None, counts=None, **nulls)
    assert rc == qfec.QFEC_OK, msg
    with pytest.raises(qfec.InvalidFecData):
        ctx.sync()
    # (pkt_pn_len is POISON, which is no length: that comes first)
    assert (bufs["frm_status"].cpu().numpy() == qfec.QFEC_FRM_PN_LEN).all()
    assert not bufs["frm_ptr"].cpu().numpy().any()
    untouched(but=("frm_status", "frm_ptr", "counts"))  # (counts: zeroed by the empty call above)
