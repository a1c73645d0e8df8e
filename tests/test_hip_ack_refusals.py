"""The host refusals of qfec_record_received and qfec_build_acks, each alone
and in the order include/qfec.h gives them (with every later fault present as
well, the earlier one answers): QFEC_ERR_INTERNAL, its message, nothing
launched and no buffer written."""
import numpy as np
import pytest
import torch

from libquic_amd import qfec
from test_hip_accumulate_ragged import dview

gpu = pytest.mark.gpu
POISON = 0xA5
N, NG, NS, NR, NC, NA, WINDOW = 9, 4, 6, 2, 3, 5, 64
RECORD = ["packet_number", "pkt_conn", "hdr", "entropy", "n_packets", "status", "revived_idx",
          "slot", "slot_key", "n_groups", "n_slots", "key_shift", "raise_conn", "raise_least",
          "raise_hash", "n_raise", "rcv_cells", "rcv_least", "rcv_largest", "rcv_hash", "n_conns",
          "window", "rcv_out", "counts", "flags"]
BUILD = ["ack_conn", "n_acks", "rcv_cells", "rcv_least", "rcv_largest", "rcv_hash", "n_conns",
         "window", "max_ranges", "max_revived", "largest_observed", "entropy_hash", "truncated",
         "range_ptr", "range_lo", "range_hi", "rev_ptr", "rev_pn", "flags"]
SCALARS = dict(n_packets=N, n_groups=NG, n_slots=NS, key_shift=40, n_raise=NR, n_conns=NC,
               window=WINDOW, flags=0, n_acks=NA, max_ranges=4, max_revived=2)


def buffers():
    sizes = dict(packet_number=8 * N, pkt_conn=4 * N, hdr=N, entropy=N, status=NG, revived_idx=NG,
                 slot=4 * NG, slot_key=8 * NS, raise_conn=4 * NR, raise_least=8 * NR, raise_hash=NR,
                 rcv_cells=NC * WINDOW, rcv_least=8 * NC, rcv_largest=8 * NC, rcv_hash=NC,
                 rcv_out=N, counts=8 * 12, ack_conn=4 * NA, largest_observed=8 * NA,
                 entropy_hash=NA, truncated=NA, range_ptr=4 * (NA + 1), range_lo=8 * NA * 4,
                 range_hi=8 * NA * 4, rev_ptr=4 * (NA + 1), rev_pn=8 * NA * 2)
    return {k: dview(np.full(n, POISON, np.uint8)) for k, n in sizes.items()}


FLAGS = [dict(flags=f) for f in (qfec.QFEC_PTR_HOST, qfec.QFEC_PTR_MAPPED, qfec.QFEC_ASYNC)]
# (faults, a fragment of the message), in the order of the checks
RECORD_LADDER = [(FLAGS[0], "device pointers only"), (dict(rcv_out=None), "null buffer"),
                 (dict(key_shift=64), "key_shift 64 outside [1, 63]"),
                 (dict(window=96), "window 96 is not a power of two"),
                 (dict(n_packets=1 << 32), "2^32 or more"),
                 (dict(slot=None, n_slots=NG - 1), "fewer slots than groups")]
RECORD_ALONE = [(f, "device pointers only") for f in FLAGS[1:]] + [
    (dict([(k, None)]), "null buffer") for k in RECORD
    if k not in SCALARS and k not in ("hdr", "entropy", "slot", "counts")] + [
    (dict(key_shift=0), "key_shift 0 outside"), (dict(window=32), "window 32"),
    (dict(window=1 << 17), "window 131072"), (dict(window=0), "window 0"),
    (dict(rcv_cells="odd"), "not 4-byte aligned"), (dict(n_groups=1 << 32), "2^32 or more"),
    (dict(n_slots=1 << 32), "2^32 or more"), (dict(n_raise=1 << 32), "2^32 or more"),
    (dict(n_conns=1 << 32), "2^32 or more")]
BUILD_LADDER = [(FLAGS[0], "device pointers only"), (dict(range_ptr=None), "null buffer"),
                (dict(max_ranges=0), "max_ranges 0 outside [1, 255]"),
                (dict(window=100), "window 100 is not a power of two"),
                (dict(n_acks=1 << 32), "2^32 or more")]
BUILD_ALONE = [(f, "device pointers only") for f in FLAGS[1:]] + [
    (dict([(k, None)]), "null buffer") for k in BUILD if k not in SCALARS] + [
    (dict(max_ranges=256), "max_ranges 256"), (dict(max_revived=256), "max_revived 256"),
    (dict(window=32), "window 32"), (dict(rcv_cells="odd"), "not 4-byte aligned"),
    (dict(n_conns=1 << 32), "2^32 or more"), (dict(n_acks=1 << 30), "2^32 or more")]  # (times max_ranges = 4)


def check(ctx, name, names, ladder, alone):
    bufs = buffers()
    before = {k: t.cpu() for k, t in bufs.items()}
    good = dict(bufs, **SCALARS)

    def call(**kw):
        a = dict(good, **kw)
        if isinstance(a["rcv_cells"], str):  # one byte into the ring
            a["rcv_cells"] = bufs["rcv_cells"][1:]
        rc = getattr(ctx.lib, name)(ctx.ctx, *[qfec._ptr(a[x]) for x in names])
        return rc, ctx.lib.qfec_last_error(ctx.ctx).decode()

    def refused(faults, fragment):
        rc, msg = call(**faults)
        assert rc == qfec.QFEC_ERR_INTERNAL and fragment in msg, (faults, rc, msg)
        assert ctx.sync() == qfec.QFEC_OK
        for k, t in bufs.items():
            assert torch.equal(t.cpu(), before[k]), (faults, k)

    for i, (_, fragment) in enumerate(ladder):
        faults = {}
        for kw, _ in reversed(ladder[i:]):
            faults.update(kw)
        refused(faults, fragment)
    for faults, fragment in alone:
        refused(faults, fragment)
    return call, bufs, before


@gpu
def test_record_refusals(ctx):
    call, bufs, before = check(ctx, "qfec_record_received", RECORD, RECORD_LADDER, RECORD_ALONE)
    # nothing to do: decided before the buffers are looked at; counts zeroed
    empty = {k: None for k in RECORD if k not in SCALARS and k != "counts"}
    rc, msg = call(n_packets=0, n_groups=0, n_raise=0, window=0, **empty)
    assert rc == qfec.QFEC_OK, msg
    assert ctx.sync() == qfec.QFEC_OK
    assert not bufs["counts"].cpu().numpy().any()
    for k, t in bufs.items():
        assert k == "counts" or torch.equal(t.cpu(), before[k]), k
    # the tables of a count that is 0 may be NULL; key_shift is then not looked at
    # (hdr is all 0xA5: every packet NOT_ACCEPTED, the state is not touched)
    rc, msg = call(n_groups=0, status=None, revived_idx=None, slot=None, slot_key=None,
                   key_shift=0, n_slots=0, n_raise=0, raise_conn=None, raise_least=None,
                   raise_hash=None, entropy=None)
    assert rc == qfec.QFEC_OK, msg
    assert ctx.sync() == qfec.QFEC_OK
    assert not bufs["rcv_out"].cpu().numpy().any()
    assert bufs["counts"].cpu().numpy().view(np.uint64).tolist() == [N] + [0] * 11
    for k in ("rcv_cells", "rcv_least", "rcv_largest", "rcv_hash"):
        assert torch.equal(bufs[k].cpu(), before[k]), k


@gpu
def test_build_refusals(ctx):
    call, bufs, before = check(ctx, "qfec_build_acks", BUILD, BUILD_LADDER, BUILD_ALONE)
    rc, msg = call(max_revived=0, rev_pn=None, n_acks=0)
    assert rc == qfec.QFEC_OK, msg
    assert ctx.sync() == qfec.QFEC_OK
    for k, t in bufs.items():
        got = t.cpu().numpy()
        if k in ("range_ptr", "rev_ptr"):
            assert not got[:4].any() and (got[4:] == POISON).all()
        else:
            assert torch.equal(t.cpu(), before[k]), k
