"""The order of the host checks of qfec_bin_arrivals: the ladder of
test_hip_queued_refusals.py for this one call.

The call starts with every host fault it knows at once and must name the first
of its order, then, that one mended, the next: the injected launch failure, bad
pointer flags, a null required buffer, pkt_ok without pkt_ok_out, 2^32 packets,
2^32 slots.  Then n_slots == 0, which succeeds with the remaining faults (null
buffers, pkt_ok without pkt_ok_out, 2^32 packets) still in place: it is decided
before them, and zeroes exactly three words of counts.  After every refused
call every buffer is as it was.

No kernel runs but that memset.  Should a check go missing and the call launch:
every pkt_slot is QFEC_NO_SLOT (nothing is binned), and every buffer is sized
for 9 packets and 12 slots.
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
NAMES = ["slot", "off", "ln", "idx", "ok", "n", "n_slots", "ptr_out", "off_out", "ln_out",
         "idx_out", "ok_out", "src_out", "counts", "flags"]
LADDER = [(dict(inject=True), -1, ["launch failure injected", "bin arrivals"]),
          (dict(flags=BAD_FLAGS), -1, ["device pointers only", "QFEC_ASYNC"]),
          (dict(idx_out=None), -1, ["null buffer"]),
          (dict(ok_out=None), -1, ["pkt_ok given without pkt_ok_out"]),
          (dict(n=1 << 32), -1, ["2^32"]),
          (dict(n_slots=1 << 32), -1, ["2^32"])]


def poison(n):
    return torch.full((n,), POISON, dtype=torch.uint8, device=DEV)


def buffers():
    """Inputs a kernel would read: no packet has a slot.  Everything the call
    may write: POISON."""
    return dict(slot=dview(np.full(N, qfec.QFEC_NO_SLOT, np.uint32)),
                off=dview(np.zeros(N, np.uint64)), ln=dview(np.zeros(N, np.uint16)),
                idx=dview(np.zeros(N, np.uint8)), ok=dview(np.zeros(N, np.uint8)),
                ptr_out=poison((N_SLOTS + 1) * 4), off_out=poison(N * 8), ln_out=poison(N * 2),
                idx_out=poison(N), ok_out=poison(N), src_out=poison(N * 4), counts=poison(5 * 8))


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
            rc = ctx.lib.qfec_bin_arrivals(ctx.ctx, *[qfec._ptr(a[x]) for x in NAMES])
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
    # each required buffer on its own; the optional ones may be NULL together
    for key in ("slot", "off", "ln", "idx", "ptr_out", "off_out", "ln_out", "idx_out"):
        rc, msg = call(**{key: None})
        assert rc == -1 and "null buffer" in msg, (key, rc, msg)
        untouched()
    # n_slots == 0: decided before the buffers and the index range are looked at
    empty = {key: None for key in bufs if key not in ("counts", "ok")}
    empty.update(n=1 << 32, n_slots=0)
    rc, msg = call(counts=None, **empty)
    assert rc == qfec.QFEC_OK, msg
    untouched()
    rc, msg = call(**empty)
    assert rc == qfec.QFEC_OK, msg
    untouched(but=("counts",))
    words = bufs["counts"].cpu().numpy().view(np.uint64).tolist()
    assert words == [0, 0, 0, POISON64, POISON64]
