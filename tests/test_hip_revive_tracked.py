"""qfec_revive_tracked on the GPU: the receiver's close with K and the map read
by slot.  Two yardsticks, whole buffers each: the rule of tests/admit_rule.py
(pinned by test_admit_rule.py), and qfec_revive_accumulated itself, called on
the same device with group_k[g] = slot_k[slot[g]], the by-slot maps gathered
by group (zeroed where the slot is fresh) and a copy of acc_len.

Discipline as in test_hip_close_accumulated.py: every offset in range; slots no
group names hold a POISON row, length, K and map; a fresh slot's map is stale
(all ones or random); out is PAD-filled; revived_list is POISON past the count.
"""
import numpy as np
import pytest
import torch

import admit_rule as R
from libquic_amd import qfec
from test_hip_accumulate_ragged import dview
from test_hip_close_accumulated import (MSG as CLOSE_MSG, PAD, POISON, POISON16, POISON64, Rows,
                                        classify_one_byte, host, make_maps, place, same)
from turn_sizes import SCAN_BLOCK, SCAN_WRAP, TILE
import close_rule as CR

gpu = pytest.mark.gpu
DEV = "cuda:0"
KSET = [1, 7, 8, 15, 16, 31, 32, 63, 64, 254, 255]
MSG = {R.E_INDEX: CLOSE_MSG[CR.ERR_SLOT], R.E_GROUP: CLOSE_MSG[CR.ERR_GROUP],
       R.E_ROWLEN: CLOSE_MSG[CR.ERR_ROWLEN]}


def by_slot(rng, n_slots, slot, ks, gmaps, fresh=()):
    """slot_k and the maps as the admit keeps them: per slot, POISON where no
    group names it; the groups in `fresh` keep a stale map (all ones or the
    group's own) -- their rows must have length 0."""
    n = len(ks)
    named = np.arange(n) if slot is None else slot
    slot_k = np.full(n_slots, POISON, np.uint8)
    maps = np.full((n_slots + 1, gmaps.shape[1]), POISON, np.uint8)
    for g in range(n):
        s = int(named[g])
        if s < n_slots:
            slot_k[s], maps[s] = ks[g], gmaps[g]
            if g in fresh and rng.integers(0, 2):
                maps[s] = 0xFF
    return slot_k, maps


def outputs(n, size):
    return dict(out=torch.full((size,), PAD, dtype=torch.uint8, device=DEV),
                olen=dview(np.full(n, POISON16, np.uint16)),
                st=dview(np.full(n, POISON, np.uint8)), idx=dview(np.full(n, POISON, np.uint8)),
                rlist=dview(np.full(n, POISON64, np.uint64)),
                cnt=dview(np.full(3, POISON64, np.uint64)))


def run_tracked(ctx, rows, slot_k, maps, n, out_off, out_size, slot=None, mask=0, no_out=False,
                optional=True, sync=True):
    """One tracked revive against the rule and against qfec_revive_accumulated
    on the gathered inputs.  Returns the rule's latched bits per group."""
    n_slots, ms = rows.n_slots, maps.shape[1]
    want_out = np.full(out_size, PAD, np.uint8)
    want_olen = np.full(n, POISON16, np.uint16)
    want_st, want_idx = np.full(n, POISON, np.uint8), np.full(n, POISON, np.uint8)
    want_len = rows.acc_len.copy()
    errs, rlist, counts = R.revive_tracked(rows.acc, rows.stride, want_len, maps[:n_slots], slot_k,
                                           n, None if no_out else want_out, out_off, want_olen,
                                           want_st, want_idx, slot, mask)
    want_list = np.full(n, POISON64, np.uint64)
    want_list[:rlist.size] = rlist
    gk, gm = R.gather(maps[:n_slots], slot_k, rows.acc_len, n, slot)
    d_off = dview(out_off)
    d_slot = None if slot is None else dview(np.asarray(slot, np.uint32))
    d_k, d_maps, d_gk, d_gm = dview(slot_k), dview(maps), dview(gk), dview(gm)
    d_len2 = rows.d_len.clone()
    a, b = outputs(n, out_size), outputs(n, out_size)
    opt = lambda o: dict(revived_idx=o["idx"], revived_list=o["rlist"],  # noqa: E731
                         counts=o["cnt"]) if optional else {}
    ctx.revive_tracked(rows.d_acc, rows.stride, rows.d_len, d_maps, ms, d_k, n,
                       None if no_out else a["out"], None if no_out else d_off, a["olen"],
                       status=a["st"], slot=d_slot, n_slots=n_slots, release_mask=mask, **opt(a))
    ctx.revive_accumulated(rows.d_acc, rows.stride, d_len2, d_gk, d_gm, ms, n,
                           None if no_out else b["out"], None if no_out else d_off, b["olen"],
                           status=b["st"], slot=d_slot, n_slots=n_slots, release_mask=mask,
                           **opt(b))
    keep = [d_off, d_slot, d_k, d_maps, d_gk, d_gm]

    def check():
        for name, dt in (("st", np.uint8), ("olen", np.uint16), ("idx", np.uint8),
                         ("rlist", np.uint64), ("cnt", np.uint64), ("out", np.uint8)):
            same(name + " against revive_accumulated", host(a[name], dt), host(b[name], dt))
        same("acc_len against revive_accumulated", host(rows.d_len, np.uint16),
             host(d_len2, np.uint16))
        same("status", host(a["st"], np.uint8), want_st)
        same("out_len", host(a["olen"], np.uint16), want_olen)
        if optional:
            same("revived_idx", host(a["idx"], np.uint8), want_idx)
            same("revived_list", host(a["rlist"], np.uint64), want_list)
            same("counts", host(a["cnt"], np.uint64), counts)
        else:
            assert torch.all(a["idx"] == POISON) and torch.all(a["cnt"].view(torch.uint8) == POISON)
        same("out", host(a["out"], np.uint8), want_out)
        same("maps", host(d_maps, np.uint8).ravel(), maps.ravel())
        same("slot_k", host(d_k, np.uint8), slot_k)
        rows.check(want_len)
        rows.acc_len = want_len
        keep.clear()
        return want_st

    if sync:
        ctx.sync()
        return errs, check()
    return errs, check


def batch(rng, n, kset, ms, slot, n_slots, stride=48, fresh_every=5):
    ks = np.array([kset[i % len(kset)] for i in rng.permutation(n)], np.uint8)
    kinds = rng.integers(0, 3, n)
    fresh = set(range(2, n, fresh_every))
    named = np.arange(n) if slot is None else slot
    lens = rng.integers(1, min(stride, R.MAX_PACKET) + 1, n)
    rows = Rows(rng, n_slots, stride,
                {int(named[g]): 0 if g in fresh else int(lens[g]) for g in range(n)})
    slot_k, maps = by_slot(rng, n_slots, slot, ks, make_maps(rng, ks, kinds, ms), fresh)
    out_off, size = place(lens)
    return rows, slot_k, maps, kinds, fresh, out_off, size


# ---- 1. shapes: group counts, K edges, map strides, slots, fresh slots ---------------------------
@gpu
@pytest.mark.parametrize("mode", ["exact_identity", "wide_permuted"])
@pytest.mark.parametrize("n", [1, 7, 8, 9, 64, 65, 255, 256, 257, 1000])
def test_shapes(ctx, n, mode):
    rng = np.random.default_rng(2000 + n)
    if mode == "exact_identity":
        kset, ms, n_slots, slot = [1, 7, 8, 15], 2, n + 3, None
    else:
        kset, ms, n_slots = KSET, 32, n + n // 2 + 5
        slot = rng.permutation(n_slots)[:n].astype(np.uint32)
    rows, slot_k, maps, kinds, fresh, out_off, size = batch(rng, n, kset, ms, slot, n_slots)
    errs, st = run_tracked(ctx, rows, slot_k, maps, n, out_off, size, slot, mask=0b011)
    assert not errs.any()
    for g in range(n):  # fresh slots are unrevivable whatever their stale maps say
        assert st[g] == (R.UNREVIVABLE if g in fresh else kinds[g])


@gpu
def test_groups_beyond_one_scan_trip(ctx):
    """256 * 1024 + 1 groups of 16-B rows, K = 7 and one map byte by slot: the
    scan over the 1,025 tiles takes a second trip, and the last group, a
    revived one, gets its place in the list and the three counts from the base
    and the side sums the scan carried into it.  The expectation is
    test_hip_close_accumulated's vectorised one; qfec_revive_accumulated on the
    same inputs gives the same buffers."""
    rng = np.random.default_rng(2600)
    n, k = SCAN_WRAP, 7
    assert (n + TILE - 1) // TILE > SCAN_BLOCK, "the groups no longer make the scan take a second trip"
    maps = rng.integers(0, 256, (n + 1, 1), dtype=np.uint8)
    maps[rng.integers(0, n, n // 2), 0] |= 0x7F  # more complete groups than chance gives
    maps[n - 1, 0], maps[n, 0] = 0xFF & ~0x08, POISON  # the last group revived; the row nobody owns
    st, idx = classify_one_byte(maps[:n], k)
    edge = SCAN_BLOCK * TILE
    assert set(st[edge - TILE:edge].tolist()) == {0, 1, 2} and st[n - 1] == CR.REVIVED
    assert idx[n - 1] == 3
    acc = rng.integers(0, 256, n * 16, dtype=np.uint8)
    rev = np.flatnonzero(st == CR.REVIVED)
    want = dict(out=np.full(n * 16 + 32, PAD, np.uint8), st=st, idx=idx,
                olen=np.where(st == CR.REVIVED, 16, 0).astype(np.uint16),
                rlist=np.full(n, POISON64, np.uint64),
                cnt=np.array([(st == s).sum() for s in range(3)], np.uint64))
    want["out"][:n * 16].reshape(n, 16)[rev] = acc.reshape(n, 16)[rev]
    want["rlist"][:rev.size] = rev
    want_len = np.where(st != CR.UNREVIVABLE, 0, 16).astype(np.uint16)
    d_acc, d_off = dview(acc), dview(np.arange(n, dtype=np.uint64) * np.uint64(16))
    d_len, d_len2 = dview(np.full(n, 16, np.uint16)), dview(np.full(n, 16, np.uint16))
    d_k, d_maps = dview(np.full(n, k, np.uint8)), dview(maps)
    a, b = outputs(n, n * 16 + 32), outputs(n, n * 16 + 32)
    ctx.revive_tracked(d_acc, 16, d_len, d_maps, 1, d_k, n, a["out"], d_off, a["olen"],
                       status=a["st"], slot=None, n_slots=n, release_mask=0b011,
                       revived_idx=a["idx"], revived_list=a["rlist"], counts=a["cnt"])
    ctx.revive_accumulated(d_acc, 16, d_len2, d_k, d_maps, 1, n, b["out"], d_off, b["olen"],
                           status=b["st"], slot=None, n_slots=n, release_mask=0b011,
                           revived_idx=b["idx"], revived_list=b["rlist"], counts=b["cnt"])
    ctx.sync()
    for name, dt in (("st", np.uint8), ("olen", np.uint16), ("idx", np.uint8),
                     ("rlist", np.uint64), ("cnt", np.uint64), ("out", np.uint8)):
        same(name, host(a[name], dt), want[name])
        same(name + " against revive_accumulated", host(a[name], dt), host(b[name], dt))
    same("acc_len", host(d_len, np.uint16), want_len)
    same("acc_len against revive_accumulated", host(d_len, np.uint16), host(d_len2, np.uint16))
    same("acc", host(d_acc, np.uint8), acc)
    same("maps", host(d_maps, np.uint8).ravel(), maps.ravel())


# ---- 2. release masks ---------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("mask", [0, 0b001, 0b010, 0b011, 0b100, 0b111])
def test_release_masks(ctx, mask):
    rng = np.random.default_rng(2100 + mask)
    n, n_slots = 70, 140
    slot = rng.permutation(n_slots)[:n].astype(np.uint32)
    rows, slot_k, maps, kinds, fresh, out_off, size = batch(rng, n, [3, 9, 15, 20], 3, slot,
                                                            n_slots, stride=1536)
    before = rows.acc_len.copy()
    errs, st = run_tracked(ctx, rows, slot_k, maps, n, out_off, size, slot, mask=mask)
    assert not errs.any()
    for g in range(n):
        s = int(slot[g])
        assert rows.acc_len[s] == (0 if (mask >> int(st[g])) & 1 else before[s])


# ---- 3. no copy, no optional outputs ---------------------------------------------------------------
@gpu
def test_without_out(ctx):
    rng = np.random.default_rng(2200)
    n = 90
    for optional, mask in ((True, 0b011), (False, 0)):
        rows, slot_k, maps, kinds, fresh, out_off, size = batch(rng, n, KSET, 32, None, n,
                                                                stride=1452)
        out_off = np.full(n, POISON64, np.uint64)  # (never read)
        errs, _ = run_tracked(ctx, rows, slot_k, maps, n, out_off, 64, None, mask=mask,
                              no_out=True, optional=optional)
        assert not errs.any()


# ---- 4. latched errors -----------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("case,err", [
    ("slot_eq_n_slots", R.E_INDEX), ("k0", R.E_GROUP), ("k_over_map", R.E_GROUP),
    ("acc_len_over_lim", R.E_ROWLEN), ("acc_len_over_stride", R.E_ROWLEN)])
def test_latched_errors(ctx, case, err):
    rng = np.random.default_rng(2300)
    n, n_slots, bad = 33, 40, 12
    stride = 1350 if case == "acc_len_over_stride" else 1536
    slot = rng.permutation(n_slots)[:n].astype(np.uint32)
    ks = rng.integers(1, 16, n).astype(np.uint8)
    kinds = rng.integers(0, 3, n)
    kinds[bad] = 1
    lens = {int(s): int(rng.integers(1, 1351)) for s in slot}
    sb = int(slot[bad])
    if case == "slot_eq_n_slots":
        del lens[sb]
        slot[bad] = n_slots
    elif case == "acc_len_over_lim":
        lens[sb] = 1453
    elif case == "acc_len_over_stride":
        lens[sb] = 1351
    slot_k, maps = by_slot(rng, n_slots, slot, ks, make_maps(rng, ks, kinds, 2))
    if case == "k0":
        slot_k[sb] = 0
    elif case == "k_over_map":
        slot_k[sb] = 16
    rows = Rows(rng, n_slots, stride, lens)
    before = rows.acc_len.copy()
    out_off, size = place([1452] * n)
    errs, check = run_tracked(ctx, rows, slot_k, maps, n, out_off, size, slot, mask=0b111,
                              sync=False)
    assert errs[bad] == err and np.count_nonzero(errs) == 1
    with pytest.raises(qfec.InvalidFecData, match=MSG[err]) as e:
        ctx.sync()
    assert e.value.code == -5
    assert MSG[err] in ctx.lib.qfec_last_error(ctx.ctx).decode()
    assert ctx.sync() == qfec.QFEC_OK  # once
    st = check()  # every other group's outputs are right
    assert st[bad] == (R.REVIVED if err == R.E_ROWLEN else R.UNREVIVABLE)
    if case != "slot_eq_n_slots":  # the offender: not released
        assert rows.acc_len[sb] == before[sb]


# ---- 5. host refusals ------------------------------------------------------------------------------
@gpu
def test_host_refusals(ctx):
    rng = np.random.default_rng(2400)
    n, n_slots, stride = 9, 12, 1536
    slot = dview(rng.permutation(n_slots)[:n].astype(np.uint32))
    acc = torch.full((n_slots * stride,), POISON, dtype=torch.uint8, device=DEV)
    bufs = dict(acc_len=dview(np.full(n_slots, POISON16, np.uint16)),
                slot_k=dview(np.full(n_slots, POISON, np.uint8)),
                maps=dview(np.full(2 * n_slots, POISON, np.uint8)),
                out=torch.full((n * stride,), POISON, dtype=torch.uint8, device=DEV),
                out_len=dview(np.full(n, POISON16, np.uint16)),
                status=dview(np.full(n, POISON, np.uint8)), idx=dview(np.full(n, POISON, np.uint8)),
                rlist=dview(np.full(n, POISON64, np.uint64)),
                counts=dview(np.full(3, POISON64, np.uint64)))
    off = dview(np.arange(n, dtype=np.uint64) * np.uint64(stride))
    P = qfec._ptr
    ints = ("stride", "ms", "n_slots", "n", "mask", "flags")
    names = ["acc", "stride", "acc_len", "maps", "ms", "slot_k", "slot", "n_slots", "n", "out",
             "off", "out_len", "status", "idx", "rlist", "counts", "mask", "flags"]

    def revive(**kw):
        a = dict(bufs, acc=acc, slot=slot, off=off, stride=stride, n_slots=n_slots, ms=2, n=n,
                 mask=7, flags=0)
        a.update(kw)
        rc = ctx.lib.qfec_revive_tracked(ctx.ctx, *[a[x] if x in ints else P(a[x]) for x in names])
        return rc, ctx.lib.qfec_last_error(ctx.ctx).decode()

    def untouched():
        assert ctx.sync() == qfec.QFEC_OK
        assert torch.all(acc == POISON)
        for name, t in bufs.items():
            assert torch.all(t.view(torch.uint8) == POISON), name

    rc, msg = revive(stride=0)
    assert rc == -5 and "accumulator stride 0" in msg
    untouched()
    rc, msg = revive(ms=0)
    assert rc == -5 and "receive map stride 0" in msg
    untouched()
    for fl in (qfec.QFEC_PTR_HOST, qfec.QFEC_PTR_MAPPED, qfec.QFEC_ASYNC):
        rc, msg = revive(flags=fl)
        assert rc == -1 and "device pointers only" in msg and "QFEC_ASYNC" in msg
        untouched()
    for kw in (dict(n=1 << 32), dict(n_slots=1 << 32)):
        rc, msg = revive(**kw)
        assert rc == -1 and "2^32" in msg
        untouched()
    rc, msg = revive(slot=None, n_slots=n - 1)
    assert rc == -1 and "fewer slots than groups" in msg
    untouched()
    for name in ("acc", "acc_len", "slot_k", "maps", "off", "out_len", "status"):
        rc, msg = revive(**{name: None})
        assert rc == -1 and "null buffer" in msg, name
        untouched()
    for mask in (8, 0x10, 0xFFFFFFFF):
        rc, msg = revive(mask=mask)
        assert rc == -1 and "release_mask" in msg
        untouched()
    assert ctx.lib.qfec_debug_fail_launches(ctx.ctx, 1) == 0
    try:
        rc, msg = revive()
    finally:
        assert ctx.lib.qfec_debug_fail_launches(ctx.ctx, 0) == 0
    assert rc == -1 and "launch failure injected" in msg
    untouched()
    none = dict(acc=None, acc_len=None, slot=None, slot_k=None, maps=None, out=None, off=None,
                out_len=None, status=None, idx=None, rlist=None, n=0, n_slots=0)
    rc, msg = revive(counts=None, **none)
    assert rc == qfec.QFEC_OK, msg
    untouched()
    rc, msg = revive(**none)
    assert rc == qfec.QFEC_OK, msg
    assert ctx.sync() == qfec.QFEC_OK
    assert host(bufs["counts"], np.uint64).tolist() == [0, 0, 0]
