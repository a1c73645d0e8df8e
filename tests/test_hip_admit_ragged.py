"""qfec_admit_ragged on the GPU: filter a turn's candidates against the per-slot
running maps and the open call's ok flags, bit for bit against the rule of
tests/admit_rule.py (pinned by test_admit_rule.py).

Discipline, as in test_hip_accumulate_ragged.py: every index and offset is in
range, so a wrong kernel gives wrong bytes, not a fault.  Maps carry POISON
guard bytes beyond K / 8 + 1 (inside map_stride where it is wider, and one
guard row behind the last slot); slots no group names hold a POISON map, a
POISON K and a POISON length; the candidate tables carry one trailing entry
nobody owns; the output tables and verdict start as POISON, so entries from
grp_ptr_out[n_groups] on must stay that.  Whole buffers are compared.
"""
import numpy as np
import pytest
import torch

import accumulate_rule as AR
import admit_rule as R
from libquic_amd import qfec
from test_admit_rule import Batch, make_groups, scenario
from test_hip_accumulate_ragged import dview

gpu = pytest.mark.gpu
DEV = "cuda:0"
POISON = 0xA5
POISON16 = np.uint16(0xA5A5)
POISON32 = np.uint32(0xA5A5A5A5)
POISON64 = np.uint64(0xA5A5A5A5A5A5A5A5)
KSET = [1, 7, 8, 15, 16, 31, 32, 63, 64, 254, 255]
MSG = {R.E_GROUP: "FEC group with 0 or more than 255 packets",
       R.E_INDEX: "missing packet index >= FEC group size",
       R.E_ROWLEN: "Illegal FEC redundancy length",
       R.E_PKTLEN: "Illegal payload size"}
# the implementation's own boundaries: groups per decide / scatter workgroup,
# and tiles per pass of the one-workgroup scan
TILE, SCAN_BLOCK = 256, 1024


def host(t, dtype):
    return t.cpu().numpy().view(dtype)


def same(name, got, want):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{name}: {bad.size} differ, first at {bad[0]}: {got[bad[0]]} " \
                          f"want {want[bad[0]]}"


class Slots:
    """Per-slot state: K, the running map (one guard row behind the last slot)
    and the row length.  Everything POISON until a slot is set."""

    def __init__(self, n_slots, ms):
        self.n_slots, self.ms = n_slots, ms
        self.k = np.full(n_slots, POISON, np.uint8)
        self.maps = np.full((n_slots + 1, ms), POISON, np.uint8)
        self.len = np.full(n_slots, POISON16, np.uint16)

    def set(self, s, k, length, have=None, stale=None):
        """have: the packets the map shows (junk above bit K, POISON beyond the
        map's bytes); stale: the byte a fresh slot's old map is filled with"""
        self.k[s], self.len[s] = k, length
        nb = k // 8 + 1
        if stale is not None:
            self.maps[s, :nb] = stale
        if have is not None:
            bits = np.ones(8 * nb, bool)  # (junk above bit K)
            bits[:k + 1] = False
            bits[sorted(have)] = True
            self.maps[s, :nb] = np.packbits(bits, bitorder="little")

    def upload(self):
        self.d_k, self.d_maps, self.d_len = dview(self.k), dview(self.maps), dview(self.len)
        return self


class Tables:
    """Candidates as CSR tables without payloads (the call reads none): per
    group a list of (idx, len, ok); offsets are distinct random multiples of
    16.  One trailing entry nobody owns."""

    def __init__(self, rng, per_group, ptr_override=None):
        flat = [c for g in per_group for c in g]
        self.n, self.m = len(per_group), len(flat)
        self.ptr = np.zeros(self.n + 1, np.uint32)
        self.ptr[1:] = np.cumsum([len(g) for g in per_group])
        if ptr_override is not None:
            self.ptr = np.asarray(ptr_override, np.uint32)
        self.off = (rng.permutation(self.m + 1).astype(np.uint64) + np.uint64(1)) * np.uint64(16)
        self.idx = np.array([c[0] for c in flat] + [0], np.uint8)
        self.ln = np.array([c[1] for c in flat] + [0], np.uint16)
        self.ok = np.array([c[2] for c in flat] + [0], np.uint8)


def run_admit(ctx, t, st, stride, slot=None, use_ok=True, counts=True, sync=True, flags=0):
    """One admit against the rule, whole buffers; st (Slots) is uploaded here
    and carries the rule's maps afterwards.  Returns the rule's errors (sync =
    False: the caller syncs, then calls the returned check)."""
    m, n = t.m, t.n
    want_ptr = np.full(n + 1, POISON32, np.uint32)
    want_off, want_ln = np.full(m + 1, POISON64, np.uint64), np.full(m + 1, POISON16, np.uint16)
    want_v = np.full(m + 1, POISON, np.uint8)
    want_maps = st.maps.copy()
    errs, want_cnt = R.admit(t.off, t.ln, t.idx, t.ok if use_ok else None, t.ptr, st.k,
                             want_maps[:st.n_slots], st.len, stride, want_ptr, want_off, want_ln,
                             want_v, slot)
    st.upload()
    d = [dview(x) for x in (t.off, t.ln, t.idx, t.ok, t.ptr)]
    d_slot = None if slot is None else dview(np.asarray(slot, np.uint32))
    o_ptr, o_off, o_ln = (dview(np.full(n + 1, POISON32, np.uint32)),
                          dview(np.full(m + 1, POISON64, np.uint64)),
                          dview(np.full(m + 1, POISON16, np.uint16)))
    o_v, o_cnt = dview(np.full(m + 1, POISON, np.uint8)), dview(np.full(4, POISON64, np.uint64))
    ctx.admit_ragged(d[0], d[1], d[2], d[3] if use_ok else None, d[4], n, st.d_k, st.d_maps,
                     st.ms, st.d_len, stride, o_ptr, o_off, o_ln, o_v, slot=d_slot,
                     n_slots=st.n_slots, counts=o_cnt if counts else None, flags=flags)
    keep = [d, d_slot]  # (alive until the check: the call only queues)

    def check():
        same("verdict", host(o_v, np.uint8), want_v)
        same("grp_ptr_out", host(o_ptr, np.uint32), want_ptr)
        same("pkt_off_out", host(o_off, np.uint64), want_off)
        same("pkt_len_out", host(o_ln, np.uint16), want_ln)
        same("maps", host(st.d_maps, np.uint8).ravel(), want_maps.ravel())
        same("counts", host(o_cnt, np.uint64), want_cnt if counts else np.full(4, POISON64))
        same("acc_len", host(st.d_len, np.uint16), st.len)
        same("slot_k", host(st.d_k, np.uint8), st.k)
        st.maps = want_maps
        keep.clear()
        return want_v, want_ptr, want_cnt

    if sync:
        ctx.sync()
        return errs, check()
    return errs, check


def behaviours(rng, n, kset, st, named, lim):
    """Group g's behaviour is g % 8: 0 no candidates; 1 every candidate fails;
    2 every candidate a duplicate of the map; 3 a fresh slot whose stale map is
    all ones; 4 every packet of the group, all admitted; 5 copies within the
    call, the later ones at other offsets; 6, 7 a random mix on a used / fresh
    slot.  Sets the slots and returns the candidates."""
    per_group = []
    ks = [kset[i % len(kset)] for i in rng.permutation(n)]
    for g in range(n):
        k, s, b = int(ks[g]), int(named[g]), g % 8
        every = list(rng.permutation(k + 1)[:255])
        some = every[:max(1, min(len(every), int(rng.integers(1, 13))))]
        ln = lambda: int(rng.integers(1, lim + 1))  # noqa: E731
        if b == 0:
            st.set(s, k, int(rng.integers(0, 2)) * ln(), have=set(some))
            c = []
        elif b == 1:
            st.set(s, k, ln(), have=set())
            c = [(i, ln(), 0) for i in some]
        elif b == 2:
            st.set(s, k, ln(), have=set(some))
            c = [(i, ln(), 1) for i in some]
        elif b == 3:
            st.set(s, k, 0, stale=0xFF)
            c = [(i, ln(), 1) for i in some]
        elif b == 4:
            st.set(s, k, ln(), have=set())
            c = [(i, ln(), 1) for i in every]
        elif b == 5:
            st.set(s, k, ln(), have=set())
            c = [(i, ln(), 1) for i in some]
            c += [(c[int(j)][0], ln(), 1) for j in rng.integers(0, len(c), 3)]
        else:
            have = set(int(i) for i in every[:len(every) // 2])
            if b == 6:
                st.set(s, k, ln(), have=have)
            else:
                st.set(s, k, 0, have=have)
            c = [(int(rng.integers(0, k + 1)), ln(), int(rng.random() < 0.8))
                 for _ in range(int(rng.integers(1, 13)))]
        per_group.append(c)
    return per_group


# ---- 1. shapes: group counts, K edges, map strides, slots ------------------------------------
@gpu
@pytest.mark.parametrize("mode", ["exact_identity", "wide_permuted"])
@pytest.mark.parametrize("n", [1, 7, 8, 9, 64, 65, 255, 256, 257, 1000])
def test_shapes(ctx, n, mode):
    rng = np.random.default_rng(1000 + n)
    if mode == "exact_identity":  # map_stride exactly the largest map, slot == NULL
        kset, ms, n_slots, slot = [1, 7, 8, 15], 2, n + 3, None
    else:  # map_stride 32, a random permutation into more slots than groups
        kset, ms, n_slots = KSET, 32, n + n // 2 + 5
        slot = rng.permutation(n_slots)[:n].astype(np.uint32)
    named = np.arange(n) if slot is None else slot
    st = Slots(n_slots, ms)
    per_group = behaviours(rng, n, kset if n > 1 else kset[-1:], st, named, 1350)
    if n == 1:
        per_group[0] = [(i, 100 + i, 1) for i in range(kset[-1] + 1)][:255]  # (not "no candidates")
    t = Tables(rng, per_group)
    errs, (v, ptr_out, cnt) = run_admit(ctx, t, st, 1350, slot)
    assert not errs.any()
    for g in range(n):  # the behaviours are what they are meant to be
        got = v[int(t.ptr[g]):int(t.ptr[g + 1])]
        adm = int(ptr_out[g + 1]) - int(ptr_out[g])
        b = g % 8
        if n > 1 and b == 1:
            assert np.all(got == R.FAILED) and adm == 0
        elif n > 1 and b == 2:
            assert np.all(got == R.DUPLICATE) and adm == 0
        elif n > 1 and b in (3, 4):
            assert np.all(got == R.ADMITTED) and adm == got.size
        elif n > 1 and b == 5:
            assert np.all(got[-3:] == R.DUPLICATE) and adm == got.size - 3


@gpu
def test_without_ok_and_without_counts(ctx):
    rng = np.random.default_rng(1100)
    n = 65
    for use_ok, counts in ((False, True), (True, False), (False, False)):
        st = Slots(n + 4, 32)
        t = Tables(rng, behaviours(rng, n, KSET, st, np.arange(n), 1452))
        errs, (v, _, _) = run_admit(ctx, t, st, 1536, None, use_ok=use_ok, counts=counts)
        assert not errs.any()
        assert use_ok or not np.any(v[:t.m] == R.FAILED)


@gpu
def test_accepted_flags_change_nothing(ctx):
    rng = np.random.default_rng(1150)
    for fl in (qfec.QFEC_CACHED, qfec.QFEC_SMALL_GROUPS):
        st = Slots(40, 4)
        t = Tables(rng, behaviours(rng, 33, [1, 7, 8, 15, 16, 31], st, np.arange(33), 1350))
        assert not run_admit(ctx, t, st, 1350, None, flags=fl)[0].any()


# ---- 2. past the tile and the scan block -------------------------------------------------------
@gpu
def test_second_scan_block(ctx):
    """TILE * SCAN_BLOCK + 1 groups of one 16-B candidate: the scan kernel's
    second pass and a last tile of one group.  K = 7 and one map byte, so the
    expectation is vectorised; it is tied to the rule on the first 600 groups
    (the admitted packets of a prefix do not depend on what follows)."""
    rng = np.random.default_rng(1200)
    n, k = TILE * SCAN_BLOCK + 1, 7
    idx = rng.integers(0, k + 1, n + 1).astype(np.uint8)
    ok = (rng.random(n + 1) < 0.9).astype(np.uint8)
    fresh = rng.random(n) < 0.25
    maps = rng.integers(0, 256, (n + 1, 1), dtype=np.uint8)
    acc_len = np.where(fresh, 0, 16).astype(np.uint16)
    off = (rng.permutation(n + 1).astype(np.uint64) + np.uint64(1)) * np.uint64(16)
    ln = np.full(n + 1, 16, np.uint16)
    ln[n] = 0
    ptr = np.arange(n + 1, dtype=np.uint32)
    base = np.where(fresh, 0, maps[:n, 0])
    bit = (1 << idx[:n].astype(np.int64))
    v = np.where(ok[:n] == 0, R.FAILED, np.where(base & bit, R.DUPLICATE, R.ADMITTED))
    adm = v == R.ADMITTED
    want_v = np.append(v.astype(np.uint8), np.uint8(POISON))
    want_maps = maps.copy()
    want_maps[:n, 0] = np.where(adm, base | bit, maps[:n, 0])
    want_ptr = np.zeros(n + 1, np.uint32)
    want_ptr[1:] = np.cumsum(adm)
    na = int(adm.sum())
    want_off, want_ln = np.full(n + 1, POISON64, np.uint64), np.full(n + 1, POISON16, np.uint16)
    want_off[:na], want_ln[:na] = off[:n][adm], 16
    # the rule on a prefix
    h = 600
    r_ptr, r_off, r_ln = (np.zeros(h + 1, np.uint32), np.full(h + 1, POISON64, np.uint64),
                          np.full(h + 1, POISON16, np.uint16))
    r_v, r_maps = np.full(h + 1, POISON, np.uint8), maps[:h].copy()
    R.admit(off[:h + 1], ln[:h + 1], idx[:h + 1], ok[:h + 1], ptr[:h + 1], np.full(h, k, np.uint8),
            r_maps, acc_len[:h], 16, r_ptr, r_off, r_ln, r_v)
    nh = int(r_ptr[h])
    assert np.array_equal(r_v[:h], want_v[:h]) and np.array_equal(r_ptr, want_ptr[:h + 1])
    assert np.array_equal(r_off[:nh], want_off[:nh]) and np.array_equal(r_maps, want_maps[:h])
    d = [dview(x) for x in (off, ln, idx, ok, ptr, np.full(n, k, np.uint8), maps, acc_len)]
    o_ptr, o_off, o_ln = (dview(np.full(n + 1, POISON32, np.uint32)),
                          dview(np.full(n + 1, POISON64, np.uint64)),
                          dview(np.full(n + 1, POISON16, np.uint16)))
    o_v, o_cnt = dview(np.full(n + 1, POISON, np.uint8)), dview(np.full(4, POISON64, np.uint64))
    ctx.admit_ragged(d[0], d[1], d[2], d[3], d[4], n, d[5], d[6], 1, d[7], 16, o_ptr, o_off, o_ln,
                     o_v, counts=o_cnt)
    ctx.sync()
    same("verdict", host(o_v, np.uint8), want_v)
    same("grp_ptr_out", host(o_ptr, np.uint32), want_ptr)
    same("pkt_off_out", host(o_off, np.uint64), want_off)
    same("pkt_len_out", host(o_ln, np.uint16), want_ln)
    same("maps", host(d[6], np.uint8).ravel(), want_maps.ravel())
    assert host(o_cnt, np.uint64).tolist() == [int((v == c).sum()) for c in range(4)]


# ---- 3. latched errors -----------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("case,err", [
    ("kg_over_255", R.E_GROUP), ("slot_eq_n_slots", R.E_INDEX), ("k0", R.E_GROUP),
    ("k_over_map", R.E_GROUP), ("acc_len_over_lim", R.E_ROWLEN),
    ("acc_len_over_stride", R.E_ROWLEN), ("idx_over_k", R.E_INDEX), ("len0", R.E_PKTLEN),
    ("len_over_lim", R.E_PKTLEN), ("len_over_stride", R.E_PKTLEN)])
def test_latched_errors(ctx, case, err):
    rng = np.random.default_rng(1300)
    n, n_slots, bad = 33, 40, 13  # (13 % 8 == 5: candidates on a used slot)
    stride = 1350 if case in ("acc_len_over_stride", "len_over_stride") else 1536
    slot = rng.permutation(n_slots)[:n].astype(np.uint32)
    st = Slots(n_slots, 2)
    per_group = behaviours(rng, n, [1, 7, 8, 15], st, slot, 1350)
    sb = int(slot[bad])
    kb = int(st.k[sb])
    before = st.maps[sb].copy()
    if case == "kg_over_255":
        per_group[bad] = [(int(rng.integers(0, kb + 1)), 64, 1) for _ in range(256)]
    elif case == "slot_eq_n_slots":
        st.k[sb], st.len[sb], st.maps[sb] = POISON, POISON16, POISON
        slot[bad] = n_slots
    elif case == "k0":
        st.k[sb] = 0
    elif case == "k_over_map":
        st.k[sb] = 16
    elif case == "acc_len_over_lim":
        st.len[sb] = 1453
    elif case == "acc_len_over_stride":
        st.len[sb] = 1351
    elif case == "idx_over_k":
        per_group[bad][1] = (kb + 1, 64, 1)
    elif case == "len0":
        per_group[bad][1] = (per_group[bad][1][0], 0, 1)
    elif case == "len_over_lim":
        per_group[bad][1] = (per_group[bad][1][0], 1453, 1)
    elif case == "len_over_stride":
        per_group[bad][1] = (per_group[bad][1][0], 1351, 1)
    t = Tables(rng, per_group)
    errs, check = run_admit(ctx, t, st, stride, slot, sync=False)
    assert errs[bad] == err and np.count_nonzero(errs) == 1
    with pytest.raises(qfec.InvalidFecData, match=MSG[err]) as e:
        ctx.sync()
    assert e.value.code == -5
    assert MSG[err] in ctx.lib.qfec_last_error(ctx.ctx).decode()
    assert ctx.sync() == qfec.QFEC_OK  # once
    v, ptr_out, cnt = check()  # every other group's outputs are right
    got = v[int(t.ptr[bad]):int(t.ptr[bad + 1])]
    if case == "kg_over_255":
        assert np.all(got == POISON)
    elif case in ("idx_over_k", "len0", "len_over_lim", "len_over_stride"):
        assert got[1] == R.INVALID and np.count_nonzero(got == R.INVALID) == 1
    else:
        assert np.all(got == R.INVALID) and ptr_out[bad + 1] == ptr_out[bad]
        if case != "slot_eq_n_slots":
            assert np.array_equal(st.maps[sb], before)


@gpu
def test_oversized_group_in_one_tile(ctx):
    """Three scatter tiles: the middle one holds a group of 300 candidates and
    goes group by group (that group's verdicts are not written, so its packets
    cannot be ranked), its neighbours one lane per packet; the places of the
    third tile's packets follow both."""
    rng = np.random.default_rng(1350)
    n, bad = 2 * TILE + 88, TILE + 44
    st = Slots(n + 5, 2)
    per_group = behaviours(rng, n, [1, 7, 8, 15], st, np.arange(n), 1350)
    per_group[bad] = [(0, 64, 1)] * 300
    t = Tables(rng, per_group)
    errs, check = run_admit(ctx, t, st, 1350, None, sync=False)
    assert errs[bad] == R.E_GROUP and np.count_nonzero(errs) == 1
    with pytest.raises(qfec.InvalidFecData, match=MSG[R.E_GROUP]):
        ctx.sync()
    v, ptr_out, cnt = check()
    assert np.all(v[int(t.ptr[bad]):int(t.ptr[bad + 1])] == POISON)
    assert ptr_out[bad + 1] == ptr_out[bad] and ptr_out[n] > ptr_out[bad] > 0


# ---- 4. host refusals ------------------------------------------------------------------------------
@gpu
def test_host_refusals(ctx):
    rng = np.random.default_rng(1400)
    n, n_slots, m = 9, 12, 30
    slot = dview(rng.permutation(n_slots)[:n].astype(np.uint32))
    ptr = np.zeros(n + 1, np.uint32)
    ptr[1:] = np.sort(rng.integers(0, m + 1, n))
    ptr[n] = m
    keep = dict(off=dview(np.arange(m, dtype=np.uint64)), ln=dview(np.full(m, 64, np.uint16)),
                idx=dview(np.zeros(m, np.uint8)), ok=dview(np.ones(m, np.uint8)), ptr=dview(ptr),
                slot_k=dview(np.full(n_slots, 10, np.uint8)),
                acc_len=dview(np.full(n_slots, 100, np.uint16)))
    before = {k: host(v, np.uint8).copy() for k, v in keep.items()}
    bufs = dict(maps=dview(np.full(2 * n_slots, POISON, np.uint8)),
                ptr_out=dview(np.full(n + 1, POISON32, np.uint32)),
                off_out=dview(np.full(m, POISON64, np.uint64)),
                ln_out=dview(np.full(m, POISON16, np.uint16)),
                verdict=dview(np.full(m, POISON, np.uint8)),
                counts=dview(np.full(4, POISON64, np.uint64)))
    P = qfec._ptr
    ints = ("n", "n_slots", "ms", "stride", "flags")
    names = ["off", "ln", "idx", "ok", "ptr", "n", "slot", "n_slots", "slot_k", "maps", "ms",
             "acc_len", "stride", "ptr_out", "off_out", "ln_out", "verdict", "counts", "flags"]

    def admit(**kw):
        a = dict(bufs, **keep, slot=slot, n=n, n_slots=n_slots, ms=2, stride=1536, flags=0)
        a.update(kw)
        rc = ctx.lib.qfec_admit_ragged(ctx.ctx, *[a[x] if x in ints else P(a[x]) for x in names])
        return rc, ctx.lib.qfec_last_error(ctx.ctx).decode()

    def untouched():
        assert ctx.sync() == qfec.QFEC_OK
        for name, t in bufs.items():
            assert torch.all(t.view(torch.uint8) == POISON), name
        for name, t in keep.items():
            assert np.array_equal(host(t, np.uint8), before[name]), name

    rc, msg = admit(stride=0)
    assert rc == -5 and "accumulator stride 0" in msg
    untouched()
    rc, msg = admit(ms=0)
    assert rc == -5 and "receive map stride 0" in msg
    untouched()
    for fl in (qfec.QFEC_PTR_HOST, qfec.QFEC_PTR_MAPPED, qfec.QFEC_ASYNC):
        rc, msg = admit(flags=fl)
        assert rc == -1 and "device pointers only" in msg and "QFEC_ASYNC" in msg
        untouched()
    for name in ("off", "ln", "idx", "ptr", "slot_k", "maps", "acc_len", "ptr_out", "off_out",
                 "ln_out", "verdict"):
        rc, msg = admit(**{name: None})
        assert rc == -1 and "null buffer" in msg, name
        untouched()
    for kw in (dict(n=1 << 32), dict(n_slots=1 << 32)):
        rc, msg = admit(**kw)
        assert rc == -1 and "2^32" in msg
        untouched()
    rc, msg = admit(slot=None, n_slots=n - 1)
    assert rc == -1 and "fewer slots than groups" in msg
    untouched()
    assert ctx.lib.qfec_debug_fail_launches(ctx.ctx, 1) == 0
    try:
        rc, msg = admit()
    finally:
        assert ctx.lib.qfec_debug_fail_launches(ctx.ctx, 0) == 0
    assert rc == -1 and "launch failure injected" in msg
    untouched()
    # no groups: decided before the buffers are looked at
    none = dict((k, None) for k in names if k not in ints and k != "counts")
    rc, msg = admit(n=0, n_slots=0, counts=None, **none)
    assert rc == qfec.QFEC_OK, msg
    untouched()
    rc, msg = admit(n=0)
    assert rc == qfec.QFEC_OK, msg
    assert ctx.sync() == qfec.QFEC_OK
    assert host(bufs["counts"], np.uint64).tolist() == [0, 0, 0, 0]
    assert torch.all(bufs["ptr_out"].view(torch.uint8) == POISON)


# ---- 5. admit + accumulate, twice, no sync between -----------------------------------------------
def turn_pairs(ctx, seed):
    """Two admit + accumulate pairs queued back to back: the second pair sees
    the first's maps and lengths.  Fresh slots: stale maps of all ones, rows of
    garbage.  Returns after the one sync with everything compared."""
    rng = np.random.default_rng(seed)
    n, n_slots, ms, stride = 70, 90, 2, 1536
    groups = make_groups(rng, n)
    cands, kind, lost, verified, dup = scenario(rng, groups, turns=2)
    slot = rng.permutation(n_slots)[:n].astype(np.uint32)
    st = Slots(n_slots, ms)
    for g in range(n):
        st.set(int(slot[g]), len(groups[g]) - 1, 0, stale=0xFF)
    acc = np.full(n_slots * stride + 32, POISON, np.uint8)
    for s in slot:
        acc[s * stride:(s + 1) * stride] = rng.integers(0, 256, stride, dtype=np.uint8)
    st.upload()
    d_acc, d_slot = dview(acc), dview(slot)
    want_maps, want_len = st.maps.copy(), st.len.copy()
    checks, keep = [], []
    for per_group in cands:
        b = Batch(per_group)
        w_ptr, w_off, w_ln = (np.full(n + 1, POISON32, np.uint32),
                              np.full(b.m + 1, POISON64, np.uint64),
                              np.full(b.m + 1, POISON16, np.uint16))
        w_v = np.full(b.m + 1, POISON, np.uint8)
        errs, w_cnt = R.admit(b.off, b.ln, b.idx, b.ok, b.ptr, st.k, want_maps[:n_slots], want_len,
                              stride, w_ptr, w_off, w_ln, w_v, slot)
        assert not errs.any()
        f_off, f_ln = w_off.copy(), w_ln.copy()
        f_ln[int(w_ptr[n]):] = 0  # (entries nobody owns; the rule never reads them)
        assert not AR.accumulate(b.data, f_off, f_ln, w_ptr, acc, stride, want_len, slot).any()
        d = [dview(x) for x in (b.data, b.off, b.ln, b.idx, b.ok, b.ptr)]
        o_ptr, o_off, o_ln = (dview(np.full(n + 1, POISON32, np.uint32)),
                              dview(np.full(b.m + 1, POISON64, np.uint64)),
                              dview(np.full(b.m + 1, POISON16, np.uint16)))
        o_v, o_cnt = dview(np.full(b.m + 1, POISON, np.uint8)), dview(np.zeros(4, np.uint64))
        ctx.admit_ragged(d[1], d[2], d[3], d[4], d[5], n, st.d_k, st.d_maps, ms, st.d_len, stride,
                         o_ptr, o_off, o_ln, o_v, slot=d_slot, n_slots=n_slots, counts=o_cnt)
        ctx.accumulate_ragged(d[0], o_off, o_ln, o_ptr, n, d_acc, stride, st.d_len, slot=d_slot,
                              n_slots=n_slots)
        keep.append(d)
        checks.append((o_v, w_v, o_ptr, w_ptr, o_off, w_off, o_ln, w_ln, o_cnt, w_cnt))
    ctx.sync()
    for o_v, w_v, o_ptr, w_ptr, o_off, w_off, o_ln, w_ln, o_cnt, w_cnt in checks:
        same("verdict", host(o_v, np.uint8), w_v)
        same("grp_ptr_out", host(o_ptr, np.uint32), w_ptr)
        same("pkt_off_out", host(o_off, np.uint64), w_off)
        same("pkt_len_out", host(o_ln, np.uint16), w_ln)
        same("counts", host(o_cnt, np.uint64), w_cnt)
    assert np.any(checks[1][1] == R.DUPLICATE)  # the second pair saw the first's bits
    same("maps", host(st.d_maps, np.uint8).ravel(), want_maps.ravel())
    same("acc_len", host(st.d_len, np.uint16), want_len)
    same("acc", host(d_acc, np.uint8), acc)


@gpu
def test_two_pairs_without_a_sync(ctx):
    turn_pairs(ctx, 1500)


@gpu
def test_context_on_its_own_stream():
    torch.cuda.synchronize()
    with qfec.Context(0) as own:  # its own non-blocking stream: uploads are
        # synchronous copies from pageable memory, done before each call
        class Waited:
            def __getattr__(self, name):
                fn = getattr(own, name)

                def call(*a, **kw):
                    torch.cuda.synchronize()
                    return fn(*a, **kw)
                return call
        turn_pairs(Waited(), 1600)
