"""The order of the host checks of qfec_assign_slots: the ladder of
test_hip_bin_refusals.py for this one call.

The call starts with every host fault it knows at once and must name the first
of its order, then, that one mended, the next: the injected launch failure, bad
pointer flags, a null required buffer, 2^32 packets, 2^32 slots.  Then
n_packets == 0, which succeeds with null buffers and 2^32 slots still in place:
it is decided before them, and zeroes exactly five words of counts.  After
every refused call every buffer is as it was.  Last, n_slots == 0 with packets
present: an ordinary call that turns every keyed packet away.

Should a check go missing and the call launch: every pkt_key is QFEC_NO_KEY
and every slot is open (nothing is opened), and every buffer is sized for 9
packets and 12 slots.
"""
import numpy as np
import pytest
import torch

from libquic_amd import qfec
from test_hip_accumulate_ragged import dview

gpu = pytest.mark.gpu
DEV = "cuda:0"
POISON = 0xA5
POISON64 = 0xA5A5A5A5A5A5A5A5
N, N_SLOTS = 9, 12
BAD_FLAGS = qfec.QFEC_PTR_HOST | qfec.QFEC_PTR_MAPPED | qfec.QFEC_ASYNC
NAMES = ["key", "k", "n", "slot_key", "slot_k", "acc_len", "n_slots", "out", "counts", "flags"]
LADDER = [(dict(inject=True), -1, ["launch failure injected", "assign slots"]),
          (dict(flags=BAD_FLAGS), -1, ["device pointers only", "QFEC_ASYNC"]),
          (dict(slot_k=None), -1, ["null buffer"]),
          (dict(n=1 << 32), -1, ["2^32"]),
          (dict(n_slots=1 << 32), -1, ["2^32"])]


def poison(n):
    return torch.full((n,), POISON, dtype=torch.uint8, device=DEV)


def buffers():
    """Inputs a kernel would read: no packet has a key, every slot is open.
    Everything the call may write: POISON."""
    return dict(key=dview(np.full(N, qfec.QFEC_NO_KEY, np.uint64)), k=dview(np.ones(N, np.uint8)),
                acc_len=dview(np.full(N_SLOTS, 5, np.uint16)), slot_key=poison(N_SLOTS * 8),
                slot_k=poison(N_SLOTS), out=poison(N * 4), counts=poison(7 * 8))


@gpu
def test_refusal_order(ctx):
    bufs = buffers()
    before = {key: t.cpu() for key, t in bufs.items()}
    good = dict(bufs, n=N, n_slots=N_SLOTS, flags=0)

    def call(**kw):
        a = dict(good, **kw)
        inject = a.pop("inject", False)
        if inject:
            assert ctx.lib.qfec_debug_fail_launches(ctx.ctx, 1) == 0
        try:
            rc = ctx.lib.qfec_assign_slots(ctx.ctx, *[qfec._ptr(a[x]) for x in NAMES])
        finally:
            if inject:
                assert ctx.lib.qfec_debug_fail_launches(ctx.ctx, 0) == 0
        return rc, ctx.lib.qfec_last_error(ctx.ctx).decode()

    def untouched(but=()):
        assert ctx.sync() == qfec.QFEC_OK
        for key, t in bufs.items():
            assert key in but or torch.equal(t.cpu(), before[key]), key

    for i, (_, code, fragments) in enumerate(LADDER):
        faults = {}
        for kw, _, _ in reversed(LADDER[i:]):
            faults.update(kw)
        rc, msg = call(**faults)
        assert rc == code, (i, rc, msg)
        for fragment in fragments:
            assert fragment in msg, (i, msg)
        untouched()
    # each required buffer on its own; counts may be NULL
    for key in ("key", "k", "slot_key", "slot_k", "acc_len", "out"):
        rc, msg = call(**{key: None})
        assert rc == -1 and "null buffer" in msg, (key, rc, msg)
        untouched()
    # packets and slots that fit 32 bits each but not the call's table together
    rc, msg = call(n=(1 << 30) + 1, n_slots=N_SLOTS)
    assert rc == -1 and "2^30" in msg, (rc, msg)
    untouched()
    # n_packets == 0: decided before the buffers and the index range are looked at
    empty = {key: None for key in bufs if key != "counts"}
    empty.update(n=0, n_slots=1 << 32)
    rc, msg = call(counts=None, **empty)
    assert rc == qfec.QFEC_OK, msg
    untouched()
    rc, msg = call(**empty)
    assert rc == qfec.QFEC_OK, msg
    untouched(but=("counts",))
    words = bufs["counts"].cpu().numpy().view(np.uint64).tolist()
    assert words == [0, 0, 0, 0, 0, POISON64, POISON64]


@gpu
def test_no_slots_is_an_ordinary_call(ctx):
    """n_slots == 0 with packets present: nothing refused, the kernels run,
    every keyed packet is turned away and the per-slot buffers stay as they
    were"""
    key = np.array([3, qfec.QFEC_NO_KEY, 3, 0, 9, qfec.QFEC_NO_KEY, 1 << 63], np.uint64)
    n = key.size
    bufs = buffers()
    d_key, d_k = dview(key), dview(np.arange(n, dtype=np.uint8))
    out = dview(np.full(n + 1, 0xA5A5A5A5, np.uint32))
    ctx.assign_slots(d_key, d_k, n, bufs["slot_key"], bufs["slot_k"], bufs["acc_len"], 0, out,
                     counts=bufs["counts"])
    assert ctx.sync() == qfec.QFEC_OK
    assert out.cpu().numpy().view(np.uint32).tolist() == [qfec.QFEC_NO_SLOT] * n + [0xA5A5A5A5]
    words = bufs["counts"].cpu().numpy().view(np.uint64).tolist()
    assert words == [0, 0, 2, 0, 5, POISON64, POISON64]
    assert torch.equal(bufs["slot_key"].cpu(), poison(N_SLOTS * 8).cpu())
    assert torch.equal(bufs["slot_k"].cpu(), poison(N_SLOTS).cpu())
