"""The order of the host checks of the seven queued, device-pointer-only calls
(qfec_revive_batch_strided, qfec_revive_ragged, qfec_accumulate_ragged,
qfec_emit_accumulated, qfec_revive_accumulated, qfec_admit_ragged,
qfec_revive_tracked).

The per-call test_host_refusals inject one fault at a time; here a call starts
with every host fault it knows at once and must name the first of its order,
then, that one mended, the next, down to the empty batch, which succeeds with
the remaining faults (null buffers, 2^32 slots) still in place: it is decided
before them.  After every refused call every buffer is as it was; counts is
zeroed by the empty batch alone, and only its 3 (admit: 4) words.

No kernel runs but that memset.  Should a check go missing and a call launch:
the tables a kernel reads are zeros (empty groups, which it refuses), and
every buffer is sized for 9 groups and 12 slots.
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
N, N_SLOTS, STRIDE, K, L = 9, 12, 1536, 10, 1350
BAD_FLAGS = qfec.QFEC_PTR_HOST | qfec.QFEC_PTR_MAPPED | qfec.QFEC_ASYNC

# (the arguments that carry the fault, the code, fragments of the message), in
# the call's order; a later entry's arguments yield to an earlier one's
INJECT = (dict(inject=True), -1, ["launch failure injected"])
ACC_STRIDE = (dict(stride=0), -5, ["accumulator stride 0"])
MAP_STRIDE = (dict(ms=0), -5, ["receive map stride 0"])
FLAGS = (dict(flags=BAD_FLAGS), -1, ["device pointers only", "QFEC_ASYNC"])
MASK = (dict(mask=8), -1, ["release_mask"])
GROUPS_2_32 = (dict(n=1 << 32), -1, ["2^32"])
FEWER_SLOTS = (dict(slot=None, n_slots=N - 1), -1, ["fewer slots than groups"])


def null(name):
    return ({name: None}, -1, ["null buffer"])


def zeros(n, dtype):
    return dview(np.zeros(n, dtype))


def poison(n):
    return torch.full((n,), POISON, dtype=torch.uint8, device=DEV)


def buffers():
    """Inputs a kernel would read: zeros.  Everything a call may write: POISON."""
    return dict(
        # fixed-shape rows and the ragged arena, parities, receive maps
        rows=poison(N * K * STRIDE), bytes=zeros(N * K * STRIDE, np.uint8),
        par=zeros(N * STRIDE, np.uint8), maps=zeros(N_SLOTS * 2, np.uint8),
        off=zeros(N * K, np.uint64), ln=zeros(N * K, np.uint16), ptr=zeros(N + 1, np.uint32),
        poff=zeros(N, np.uint64), plen=zeros(N, np.uint16),
        idx_in=zeros(N * K, np.uint8), ok=zeros(N * K, np.uint8),
        # running rows
        acc=poison(N_SLOTS * STRIDE), acc_len=poison(N_SLOTS * 2), acc_map=poison(N_SLOTS * 2),
        slot=dview(np.arange(N, dtype=np.uint32)), gk=zeros(N_SLOTS, np.uint8),
        # outputs
        out=poison(N * STRIDE), ooff=dview(np.arange(N, dtype=np.uint64) * np.uint64(STRIDE)),
        out_len=poison(N * 2), status=poison(N), idx=poison(N), lst=poison(N * 8),
        ptr_out=poison((N + 1) * 4), off_out=poison(N * K * 8), ln_out=poison(N * K * 2),
        verdict=poison(N * K), counts=poison(5 * 8))


SCALARS = dict(n=N, n_slots=N_SLOTS, stride=STRIDE, ms=2, k=K, L=L, rs=STRIDE, gs=K * STRIDE,
               ps=STRIDE, os=STRIDE, release=1, mask=7, flags=0)

# name: (the C-ABI's argument order, the ladder, words of counts the empty batch zeroes)
CALLS = {
    # the two older revive calls do not know the injected launch failure: it
    # is set with their first fault and changes nothing
    "qfec_revive_batch_strided": (
        ["rows", "par", "maps", "k", "L", "rs", "gs", "ps", "ms", "n", "out", "os", "status",
         "idx", "lst", "counts", "flags"],
        [(dict(inject=True, k=0), -5, ["FEC group size"]),
         (dict(ms=1), -5, ["receive map stride"]), FLAGS, null("status"),
         (dict(n=1 << 56), -1, ["2^56"])], 3),
    "qfec_revive_ragged": (
        ["bytes", "off", "ln", "ptr", "n", "par", "poff", "plen", "maps", "ms", "out", "ooff",
         "status", "idx", "lst", "counts", "flags"],
        [(dict(inject=True, ms=0), -5, ["receive map stride 0"]), FLAGS, null("status"),
         GROUPS_2_32], 3),
    "qfec_accumulate_ragged": (
        ["bytes", "off", "ln", "ptr", "n", "acc", "stride", "acc_len", "slot", "n_slots", "flags"],
        [INJECT, ACC_STRIDE, FLAGS, null("acc_len"), GROUPS_2_32, FEWER_SLOTS], 0),
    "qfec_emit_accumulated": (
        ["acc", "stride", "acc_len", "slot", "n_slots", "n", "out", "ooff", "out_len", "release",
         "flags"],
        [INJECT, ACC_STRIDE, FLAGS, null("out_len"), GROUPS_2_32, FEWER_SLOTS], 0),
    "qfec_revive_accumulated": (
        ["acc", "stride", "acc_len", "slot", "n_slots", "gk", "maps", "ms", "n", "out", "ooff",
         "out_len", "status", "idx", "lst", "counts", "mask", "flags"],
        [INJECT, ACC_STRIDE, MAP_STRIDE, FLAGS, MASK, null("status"), GROUPS_2_32, FEWER_SLOTS],
        3),
    "qfec_admit_ragged": (
        ["off", "ln", "idx_in", "ok", "ptr", "n", "slot", "n_slots", "gk", "acc_map", "ms",
         "acc_len", "stride", "ptr_out", "off_out", "ln_out", "verdict", "counts", "flags"],
        [INJECT, ACC_STRIDE, MAP_STRIDE, FLAGS, null("verdict"), GROUPS_2_32, FEWER_SLOTS], 4),
    "qfec_revive_tracked": (
        ["acc", "stride", "acc_len", "acc_map", "ms", "gk", "slot", "n_slots", "n", "out", "ooff",
         "out_len", "status", "idx", "lst", "counts", "mask", "flags"],
        [INJECT, ACC_STRIDE, MAP_STRIDE, FLAGS, MASK, null("status"), GROUPS_2_32, FEWER_SLOTS],
        3),
}


@gpu
@pytest.mark.parametrize("name", list(CALLS))
def test_refusal_order(ctx, name):
    names, ladder, count_words = CALLS[name]
    bufs = buffers()
    before = {key: t.cpu() for key, t in bufs.items()}
    good = dict(bufs, **SCALARS)

    def call(**kw):
        a = dict(good, **kw)
        inject = a.pop("inject", False)
        if inject:
            assert ctx.lib.qfec_debug_fail_launches(ctx.ctx, 1) == 0
        try:
            rc = getattr(ctx.lib, name)(ctx.ctx, *[qfec._ptr(a[x]) for x in names])
        finally:
            if inject:
                assert ctx.lib.qfec_debug_fail_launches(ctx.ctx, 0) == 0
        return rc, ctx.lib.qfec_last_error(ctx.ctx).decode()

    def untouched(but=()):
        assert ctx.sync() == qfec.QFEC_OK
        for key, t in bufs.items():
            assert key in but or torch.equal(t.cpu(), before[key]), key

    for i, (_, code, fragments) in enumerate(ladder):
        faults = {}
        for kw, _, _ in reversed(ladder[i:]):
            faults.update(kw)
        rc, msg = call(**faults)
        assert rc == code, (i, rc, msg)
        for fragment in fragments:
            assert fragment in msg, (i, msg)
        untouched()
    # the empty batch: decided before the buffers and the index range are looked at
    empty = {key: None for key in bufs if key in names and key != "counts"}
    empty.update(n=0)
    if "n_slots" in names:
        empty.update(n_slots=1 << 32)
    if count_words:
        rc, msg = call(counts=None, **empty)
        assert rc == qfec.QFEC_OK, msg
        untouched()
    rc, msg = call(**empty)
    assert rc == qfec.QFEC_OK, msg
    untouched(but=("counts",))
    words = bufs["counts"].cpu().numpy().view(np.uint64).tolist()
    assert words == [0] * count_words + [POISON64] * (5 - count_words)
