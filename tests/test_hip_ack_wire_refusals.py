"""The host refusals of qfec_write_ack_frames, each alone and in the order
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
NA, NC, WINDOW = 5, 3, 64
WRITE = ["ack_conn", "n_acks", "largest_observed", "entropy_hash", "truncated", "range_ptr",
         "range_lo", "range_hi", "rev_ptr", "rev_pn", "ack_delay_us", "rcv_cells", "n_conns",
         "window", "out", "out_off", "out_cap", "prefix_len", "out_len", "wire_largest", "wire_hash",
         "ack_status", "counts", "flags"]
SCALARS = dict(n_acks=NA, n_conns=NC, window=WINDOW, prefix_len=2, flags=0)
OPTIONAL = ("rev_pn", "ack_delay_us", "counts")


def buffers():
    sizes = dict(ack_conn=4 * NA, largest_observed=8 * NA, entropy_hash=NA, truncated=NA,
                 range_ptr=4 * (NA + 1), range_lo=8 * NA * 4, range_hi=8 * NA * 4,
                 rev_ptr=4 * (NA + 1), rev_pn=8 * NA * 2, ack_delay_us=8 * NA,
                 rcv_cells=NC * WINDOW, out=NA * 64, out_off=8 * NA, out_cap=2 * NA, out_len=2 * NA,
                 wire_largest=8 * NA, wire_hash=NA, ack_status=NA, counts=8 * 4)
    return {k: dview(np.full(n, POISON, np.uint8)) for k, n in sizes.items()}


FLAGS = [dict(flags=f) for f in (qfec.QFEC_PTR_HOST, qfec.QFEC_PTR_MAPPED, qfec.QFEC_ASYNC)]
# (faults, a fragment of the message), in the order of the checks
LADDER = [(FLAGS[0], "device pointers only"), (dict(out_len=None), "null buffer"),
          (dict(window=96), "window 96 is not a power of two"),
          (dict(n_acks=1 << 32), "2^32 or more"), (dict(prefix_len=65), "prefix_len 65 above 64")]
ALONE = [(f, "device pointers only") for f in FLAGS[1:]] + [
    (dict([(k, None)]), "null buffer") for k in WRITE if k not in SCALARS and k not in OPTIONAL] + [
    (dict(window=32), "window 32"), (dict(window=1 << 17), "window 131072"),
    (dict(window=0), "window 0"), (dict(rcv_cells="odd"), "not 4-byte aligned"),
    (dict(n_conns=1 << 32), "2^32 or more"), (dict(prefix_len=1 << 31), "above 64")]


@gpu
def test_write_ack_frames_refusals(ctx):
    bufs = buffers()
    before = {k: t.cpu() for k, t in bufs.items()}
    good = dict(bufs, **SCALARS)

    def call(**kw):
        a = dict(good, **kw)
        if isinstance(a["rcv_cells"], str):  # one byte into the ring
            a["rcv_cells"] = bufs["rcv_cells"][1:]
        rc = ctx.lib.qfec_write_ack_frames(ctx.ctx, *[qfec._ptr(a[x]) for x in WRITE])
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
    # nothing to do: decided before the buffers are looked at; counts zeroed
    empty = {k: None for k in WRITE if k not in SCALARS and k != "counts"}
    rc, msg = call(n_acks=0, window=0, prefix_len=99, **empty)
    assert rc == qfec.QFEC_OK, msg
    untouched(but=("counts",))
    assert not bufs["counts"].cpu().numpy().any()
    # the ring of no connection may be NULL: every ack is then out of range
    rc, msg = call(n_conns=0, rcv_cells=None, rev_pn=None, ack_delay_us=None, counts=None)
    assert rc == qfec.QFEC_OK, msg
    with pytest.raises(qfec.InvalidFecData):
        ctx.sync()
    assert not bufs["out_len"].cpu().numpy().any()
    assert (bufs["ack_status"].cpu().numpy() == qfec.QFEC_ACKW_RANGE).all()
    untouched(but=("counts", "out_len", "ack_status", "wire_largest", "wire_hash"))
