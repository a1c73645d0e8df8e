"""qfec_revive_batch on the GPU: classify every group of a device-resident
batch from its receive map and rebuild the lost packet of the revivable ones.

The reference for status, revived_idx, revived_list and counts is reference()
below, a few lines of NumPy stating the rule of include/qfec.h; the revived
bytes are checked against the C oracle's recover_fixed run on the revived
groups with their m (and, as a check of the test's own inputs, against the
packet that was erased).  Every output buffer starts as POISON; every lost slot
holds LOST and the parity row of every group without its FEC packet holds
NOFEC, so a stray read changes a result and a stray write shows.  All
comparisons are bit-exact.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import oracle_c as OC
from oracle import qfec_np as Q
from libquic_amd import qfec
from turn_sizes import SCAN_BLOCK, SCAN_WRAP, TILE

gpu = pytest.mark.gpu
DEV = "cuda:0"
POISON, LOST, NOFEC, PAD = 0xA5, 0x3C, 0xC3, 0x5A
POISON64 = np.uint64(0xA5A5A5A5A5A5A5A5)


# ---- the rule ---------------------------------------------------------------
def reference(data, fec):
    """data [n, k] bool, fec [n] bool -> status, revived_idx, revived_list, counts."""
    k = data.shape[1]
    miss = k - data.sum(axis=1)
    status = np.where(miss == 0, qfec.GROUP_COMPLETE,
                      np.where((miss == 1) & fec, qfec.GROUP_REVIVED,
                               qfec.GROUP_UNREVIVABLE)).astype(np.uint8)
    idx = np.where(status == qfec.GROUP_REVIVED, np.argmin(data, axis=1), 0xFF).astype(np.uint8)
    lst = np.flatnonzero(status == qfec.GROUP_REVIVED).astype(np.uint64)
    counts = np.bincount(status, minlength=3).astype(np.uint64)
    return status, idx, lst, counts


class Case:
    """A batch: complete rows, the receiver's view of them (lost slots and
    unreceived parity rows poisoned), the maps, and everything expected."""

    def __init__(self, data, fec, L, seed):
        data = np.ascontiguousarray(data, dtype=bool)
        fec = np.ascontiguousarray(fec, dtype=bool)
        n, k = data.shape
        rng = np.random.default_rng(seed)
        self.n, self.k, self.L, self.data, self.fec = n, k, L, data, fec
        self.complete = rng.integers(0, 256, (n, k, L), dtype=np.uint8)
        par = np.bitwise_xor.reduce(self.complete, axis=1)
        self.rows_in = self.complete.copy()
        self.rows_in[~data] = LOST
        self.par_in = par
        self.par_in[~fec] = NOFEC
        self.maps = qfec.pack_received(data, fec)
        self.status, self.idx, self.lst, self.counts = reference(data, fec)
        sel = self.lst.astype(np.int64)
        self.sel = sel
        if sel.size:
            rc, o = OC.recover_fixed(np.ascontiguousarray(self.rows_in[sel]).ravel(),
                                     np.ascontiguousarray(self.par_in[sel]).ravel(),
                                     self.idx[sel], k, L, sel.size)
            assert rc == 0
            self.revived = o.reshape(sel.size, L)
            # the test's own inputs: the oracle rebuilt exactly the erased packets
            assert np.array_equal(self.revived, self.complete[sel, self.idx[sel].astype(np.int64)])
        else:
            self.revived = np.zeros((0, L), dtype=np.uint8)
        self.want_out = np.full((n, L), POISON, dtype=np.uint8)
        self.want_out[sel] = self.revived
        self.want_rows = self.rows_in.copy()
        self.want_rows[sel, self.idx[sel].astype(np.int64)] = self.revived


class Outs:
    """Poisoned device outputs of one call."""

    def __init__(self, n, out_bytes=0):
        self.n = n
        self.status = torch.full((max(n, 1),), POISON, dtype=torch.uint8, device=DEV)
        self.idx = torch.full((max(n, 1),), POISON, dtype=torch.uint8, device=DEV)
        self.lst = torch.full((max(n, 1) * 8,), POISON, dtype=torch.uint8, device=DEV)
        self.counts = torch.full((24,), POISON, dtype=torch.uint8, device=DEV)
        self.out = torch.full((max(out_bytes, 1),), POISON, dtype=torch.uint8, device=DEV)

    def repoison(self):
        for t in (self.status, self.idx, self.lst, self.counts, self.out):
            t.fill_(POISON)

    def host(self):
        torch.cuda.synchronize()
        return dict(status=self.status.cpu().numpy()[:self.n], idx=self.idx.cpu().numpy()[:self.n],
                    lst=self.lst.cpu().numpy().view(np.uint64)[:self.n],
                    counts=self.counts.cpu().numpy().view(np.uint64),
                    out=self.out.cpu().numpy())


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def check_meta(h, case, what=("status", "idx", "lst", "counts")):
    """status / revived_idx / revived_list / counts of a call against the rule."""
    n = case.n
    if "status" in what:
        assert np.array_equal(h["status"], case.status)
    if "idx" in what:
        assert np.array_equal(h["idx"], case.idx)
    if "counts" in what:
        assert np.array_equal(h["counts"], case.counts)
        assert int(case.counts.sum()) == n
    if "lst" in what:
        c = case.lst.size
        assert np.array_equal(h["lst"][:c], case.lst)
        assert np.all(h["lst"][c:] == POISON64), "revived_list written past the count"


def run_dense(ctx, case, inplace, cached=False):
    """One dense call, out of place or in place, everything checked."""
    n, k, L = case.n, case.k, case.L
    rows, par, maps = dev(case.rows_in.ravel()), dev(case.par_in.ravel()), dev(case.maps.ravel())
    o = Outs(n, 0 if inplace else n * L)
    ctx.revive(rows, par, maps, k, L, n, None if inplace else o.out, status=o.status,
               revived_idx=o.idx, revived_list=o.lst, counts=o.counts, cached=cached)
    ctx.sync()
    h = o.host()
    check_meta(h, case)
    rows_h = rows.cpu().numpy().reshape(n, k, L)
    if inplace:
        # revived groups are whole again, every other byte is as it was --
        # the poisoned lost slots of unrevivable groups included
        assert np.array_equal(rows_h, case.want_rows)
        assert np.array_equal(rows_h[case.sel], case.complete[case.sel])
        assert np.all(h["out"] == POISON)
    else:
        assert np.array_equal(h["out"].reshape(n, L), case.want_out)
        assert np.array_equal(rows_h, case.rows_in)
    assert np.array_equal(par.cpu().numpy().reshape(n, L), case.par_in)
    assert np.array_equal(maps.cpu().numpy(), case.maps.ravel())


# ---- 1. every map, small k --------------------------------------------------
@functools.lru_cache(maxsize=4)
def every_map_case(k, L):
    n = 1 << (k + 1)
    bits = (np.arange(n)[:, None] >> np.arange(k + 1)[None, :]) & 1
    return Case(bits[:, :k] == 1, bits[:, k] == 1, L, 7000 + 10 * L + k)


@gpu
@pytest.mark.parametrize("inplace", [False, True])  # (the top one varies fastest)
@pytest.mark.parametrize("L", [1, 15, 16, 17, 100, 1350, 1452])
@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_every_map_small_k(ctx, k, L, inplace):
    case = every_map_case(k, L)
    assert sorted(set(case.status)) == [0, 1, 2]
    run_dense(ctx, case, inplace)


# ---- 2 / 3. every drop index, out of place and in place -----------------------
DROP_SHAPES = ([(k, L) for k in list(range(1, 18)) + [33, 64, 255] for L in (16, 1350)]
               + [(10, 1), (10, 1452)])
# (L = 1350 runs every templated k through the scalar-entry form of the revive
# kernel, L = 16 through the per-lane form; 7: all of it again with
# cached=True, so every compiled body of both cache policies is launched)


@functools.lru_cache(maxsize=2)
def drop_case(k, L):
    n = 3 * k + 2
    data = np.ones((n, k), dtype=bool)
    fec = np.ones(n, dtype=bool)
    for g in range(k):
        data[g, g] = False            # loses packet g, has its FEC packet: revived
        data[k + g, g] = False        # loses packet g, no FEC packet: unrevivable
        fec[k + g] = False
        data[2 * k + g, g] = False    # loses two packets, has its FEC packet
        if k > 1:
            data[2 * k + g, (g + 1 + g % (k - 1)) % k] = False
        else:
            fec[2 * k + g] = False    # k = 1: the only packet and the FEC packet
    fec[3 * k + 1] = False            # complete without its FEC packet (3k: with it)
    case = Case(data, fec, L, 9000 + 10 * L + k)
    assert case.counts.tolist() == [2, k, 2 * k]
    assert case.idx[:k].tolist() == list(range(k))
    return case


@gpu
@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("k,L", DROP_SHAPES)
def test_every_drop_index(ctx, k, L, inplace):
    run_dense(ctx, drop_case(k, L), inplace)


@gpu
@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("k,L", DROP_SHAPES)
def test_every_drop_index_cached(ctx, k, L, inplace):
    run_dense(ctx, drop_case(k, L), inplace, cached=True)


# ---- the scalar-entry form in every groups-per-workgroup class ----------------
# gpb = 256 // ceil(L / 16) from 8 down to 2 (L = 480: 8 groups of 30 lanes and
# 16 leftover lanes whose entry index is 8; 448 / 449 is the 9 <-> 8 switch to
# the per-lane form), group sizes on both sides of the templated range, more
# groups than a step so that every entry of the select chain is used
@gpu
@pytest.mark.parametrize("cached", [False, True])
@pytest.mark.parametrize("L", [448, 449, 480, 512, 513, 576, 577, 672, 673, 816, 817, 1024, 1025])
@pytest.mark.parametrize("k", [3, 12, 17])
def test_entry_load_classes(ctx, k, L, cached):
    gpb = 256 // ((L + 15) // 16)
    n = 7 * gpb + 3
    rng = np.random.default_rng(31 * L + k)
    kinds = (rng.random(n) < 0.8).astype(np.int64)
    kinds[rng.integers(0, n, 3)] = 2
    data, fec = maps_from_kinds(kinds, k, rng)
    case = Case(data, fec, L, 8000 + 10 * L + k)
    assert case.counts[1] > 4 * gpb
    run_dense(ctx, case, inplace=False, cached=cached)
    run_dense(ctx, case, inplace=True, cached=cached)


# the revive grid is 8 workgroups per CU: with more revived groups than
# 8 x CUs x gpb its workgroups take a second step of the list
@gpu
@pytest.mark.parametrize("k,L,n", [(7, 480, 20011), (17, 816, 12007)])
def test_revive_grid_loops(ctx, k, L, n):
    gpb = 256 // ((L + 15) // 16)
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    rng = np.random.default_rng(n + k)
    kinds = (rng.random(n) < 0.95).astype(np.int64)
    data, fec = maps_from_kinds(kinds, k, rng)
    case = Case(data, fec, L, 8100 + k)
    assert case.counts[1] > 8 * ncu * gpb, "the batch no longer makes the grid loop"
    run_dense(ctx, case, inplace=False)
    run_dense(ctx, case, inplace=True)


# ---- 4. list order across workgroup and scan-tile boundaries ------------------
def maps_from_kinds(kinds, k, rng):
    """data / fec for the wanted status per group (0 / 1 / 2), at random."""
    n = kinds.size
    data = np.ones((n, k), dtype=bool)
    fec = rng.random(n) < 0.5
    ar = np.arange(n)
    first = rng.integers(0, k, n)
    lose = kinds != 0
    data[ar[lose], first[lose]] = False
    fec[kinds == 1] = True
    two = (kinds == 2) & (rng.random(n) < 0.5) if k > 1 else np.zeros(n, dtype=bool)
    second = (first + 1 + rng.integers(0, max(k - 1, 1), n)) % k
    data[ar[two], second[two]] = False
    fec[(kinds == 2) & ~two] = False
    return data, fec


def order_kinds(pattern, n, rng):
    if pattern == "random":
        r = rng.random(n)
        return np.where(r < 0.3, 1, np.where(r < 0.8, 0, 2))
    if pattern == "late":
        return (np.arange(n) >= 70000).astype(np.int64)
    assert pattern == "alternating"
    return (np.arange(n) % 2 == 0).astype(np.int64)


@gpu
@pytest.mark.parametrize("n,pattern", [(100003, "random"), (100003, "late"),
                                       (100003, "alternating"), (1, "alternating"),
                                       (1, "random"), (257, "random"), (257, "alternating")])
def test_list_order(ctx, n, pattern):
    rng = np.random.default_rng(n + len(pattern))
    run_list_order(ctx, order_kinds(pattern, n, rng), 4, 32, rng)


@gpu
def test_groups_beyond_one_scan_trip(ctx):
    """256 * 1024 + 1 groups of the smallest rows: the scan over the 1,025 tiles
    takes a second trip, and the last group, a revived one, gets its place in
    the list and the three counts from the base and the side sums carried into
    it"""
    n = SCAN_WRAP
    assert (n + TILE - 1) // TILE > SCAN_BLOCK, "the groups no longer make the scan take a second trip"
    rng = np.random.default_rng(n)
    kinds = order_kinds("random", n, rng)
    kinds[n - 1] = 1
    edge = SCAN_BLOCK * TILE
    assert set(kinds[edge - TILE:edge].tolist()) == {0, 1, 2} == set(kinds[:TILE].tolist())
    run_list_order(ctx, kinds, 2, 16, rng)


def run_list_order(ctx, kinds, k, L, rng):
    n = kinds.size
    data, fec = maps_from_kinds(kinds, k, rng)
    case = Case(data, fec, L, 4242 + n)
    assert np.array_equal(case.status, kinds.astype(np.uint8))
    rows, par, maps = dev(case.rows_in.ravel()), dev(case.par_in.ravel()), dev(case.maps.ravel())
    o = Outs(n, n * L)
    ctx.revive(rows, par, maps, k, L, n, o.out, status=o.status, revived_idx=o.idx,
               revived_list=o.lst, counts=o.counts)
    ctx.sync()
    h = o.host()
    c = int(h["counts"][1])
    assert np.array_equal(h["lst"][:c], np.flatnonzero(h["status"] == 1).astype(np.uint64))
    assert np.all(h["lst"][c:] == POISON64)
    assert h["counts"].tolist() == [int((kinds == s).sum()) for s in (0, 1, 2)]
    check_meta(h, case)
    assert np.array_equal(h["out"].reshape(n, L), case.want_out)


# ---- 5. strides and alignment -------------------------------------------------
K5, L5 = 10, 1350
RS5, GS5, PS5, OS5, MS5 = 1360, 10 * 1360 + 48, 1376, 1408, 5


@functools.lru_cache(maxsize=1)
def stride_case():
    rng = np.random.default_rng(55)
    n = 61
    kinds = rng.integers(0, 3, n)
    kinds[:3] = (1, 0, 2)
    data, fec = maps_from_kinds(kinds, K5, rng)
    return Case(data, fec, L5, 5555)


def padded(a, stride, fill=PAD):
    """[n, w] -> flat [n * stride], row g at g * stride, the padding filled."""
    n, w = a.shape
    b = np.full((n, stride), fill, dtype=np.uint8)
    b[:, :w] = a
    return b.ravel()


def strided_inputs(case, ms):
    n, k, L = case.n, case.k, case.L
    r = np.full((n, k, RS5), PAD, dtype=np.uint8)
    r[:, :, :L] = case.rows_in
    rows = padded(r.reshape(n, k * RS5), GS5)
    return rows, padded(case.par_in, PS5), padded(case.maps, ms)


def want_strided_rows(case):
    n, k, L = case.n, case.k, case.L
    r = np.full((n, k, RS5), PAD, dtype=np.uint8)
    r[:, :, :L] = case.want_rows
    return padded(r.reshape(n, k * RS5), GS5)


@gpu
@pytest.mark.parametrize("cached", [False, True])
@pytest.mark.parametrize("inplace", [False, True])
def test_strides(ctx, inplace, cached):
    case = stride_case()
    n, k, L = case.n, case.k, case.L
    rows_h, par_h, maps_h = strided_inputs(case, MS5)
    rows, par, maps = dev(rows_h), dev(par_h), dev(maps_h)
    o = Outs(n, n * OS5)
    ctx.revive(rows, par, maps, k, L, n, None if inplace else o.out, status=o.status,
               revived_idx=o.idx, revived_list=o.lst, counts=o.counts, row_stride=RS5,
               group_stride=GS5, parity_stride=PS5, map_stride=MS5, out_stride=OS5, cached=cached)
    ctx.sync()
    h = o.host()
    check_meta(h, case)
    if inplace:
        assert np.array_equal(rows.cpu().numpy(), want_strided_rows(case))
        assert np.all(h["out"] == POISON)
    else:
        assert np.array_equal(h["out"], padded(case.want_out, OS5, POISON))
        assert np.array_equal(rows.cpu().numpy(), rows_h)
    assert np.array_equal(par.cpu().numpy(), par_h)
    assert np.array_equal(maps.cpu().numpy(), maps_h)


@gpu
@pytest.mark.parametrize("ms", [2, 5])
def test_map_base_alignment(ctx, ms):
    """The maps at every byte offset 0..7 from a 16-byte-aligned allocation."""
    case = stride_case()
    n, k, L = case.n, case.k, case.L
    rows, par = dev(case.rows_in.ravel()), dev(case.par_in.ravel())
    maps_h = padded(case.maps, ms)
    for shift in range(8):
        buf = torch.full((maps_h.size + 32,), 0xFF, dtype=torch.uint8, device=DEV)
        assert buf.data_ptr() % 16 == 0
        buf[shift:shift + maps_h.size] = dev(maps_h)
        maps = buf[shift:shift + maps_h.size]
        assert maps.data_ptr() % 16 == shift
        o = Outs(n, n * L)
        ctx.revive(rows, par, maps, k, L, n, o.out, status=o.status, revived_idx=o.idx,
                   revived_list=o.lst, counts=o.counts, map_stride=ms)
        ctx.sync()
        h = o.host()
        check_meta(h, case)
        assert np.array_equal(h["out"].reshape(n, L), case.want_out), shift
    assert np.array_equal(rows.cpu().numpy(), case.rows_in.ravel())


BASE, GUARD = 256, 64  # as tests/test_hip_fixed_variants.py: buffers start BASE bytes in


def strided_alloc(nbytes, shape, strides):
    big = torch.empty(BASE + nbytes, dtype=torch.uint8, device=DEV)
    L = shape[-1]
    used = big.as_strided(shape, strides, BASE)
    before = big.as_strided(shape[:-1] + (GUARD,), strides, BASE - GUARD)
    after = big.as_strided(shape[:-1] + (GUARD,), strides, BASE + L)
    before.fill_(PAD)
    after.fill_(PAD)
    return big[BASE:], used, (before, after)


def guards_intact(guards):
    return all(bool((g == PAD).all()) for g in guards)


@gpu
@pytest.mark.parametrize("inplace", [False, True])
def test_strides_beyond_32_bits(ctx, inplace):
    """g * group_stride, r * row_stride, g * parity_stride, g * out_stride and
    g * map_stride past 4 GiB (uninitialised allocations, a few rows touched)."""
    k, L, n = 3, 1350, 2
    rs = (1 << 31) + 64
    gs = 3 * rs
    st = (1 << 32) + 16
    data = np.array([[1, 0, 1], [1, 1, 0]], dtype=bool)
    fec = np.array([1, 1], dtype=bool)
    case = Case(data, fec, L, 3232)
    assert case.status.tolist() == [1, 1] and case.idx.tolist() == [1, 2]
    rows, r3, rg = strided_alloc(n * gs, (n, k, L), (gs, rs, 1))
    r3.copy_(dev(case.rows_in))
    par, p2, pg = strided_alloc(n * st, (n, L), (st, 1))
    p2.copy_(dev(case.par_in))
    out, o2, og = strided_alloc(n * st, (n, L), (st, 1))
    o2.fill_(POISON)
    nb = case.maps.shape[1]
    maps, m2, mg = strided_alloc(n * st, (n, nb), (st, 1))
    m2.copy_(dev(case.maps))
    o = Outs(n)
    ctx.revive(rows, par, maps, k, L, n, None if inplace else out, status=o.status,
               revived_idx=o.idx, revived_list=o.lst, counts=o.counts, row_stride=rs,
               group_stride=gs, parity_stride=st, map_stride=st, out_stride=st)
    ctx.sync()
    check_meta(o.host(), case)
    if inplace:
        assert np.array_equal(r3.cpu().numpy(), case.want_rows)
        assert bool((o2 == POISON).all())
    else:
        assert np.array_equal(o2.cpu().numpy(), case.want_out)
        assert np.array_equal(r3.cpu().numpy(), case.rows_in)
    assert np.array_equal(p2.cpu().numpy(), case.par_in)
    assert guards_intact(rg) and guards_intact(pg) and guards_intact(og) and guards_intact(mg)


# ---- 6. ignored bits ----------------------------------------------------------
@gpu
@pytest.mark.parametrize("k", [10, 3])
def test_bits_above_k_are_ignored(ctx, k):
    L, n = 100, 300
    rng = np.random.default_rng(600 + k)
    data, fec = maps_from_kinds(rng.integers(0, 3, n), k, rng)
    case = Case(data, fec, L, 660 + k)
    nb = case.maps.shape[1]
    high = (0xFF << ((k + 1) % 8)) & 0xFF if (k + 1) % 8 else 0
    assert high != 0
    noisy = case.maps.copy()
    noisy[:, nb - 1] |= rng.integers(0, 256, n).astype(np.uint8) & np.uint8(high)
    assert not np.array_equal(noisy, case.maps)
    rows, par, maps = dev(case.rows_in.ravel()), dev(case.par_in.ravel()), dev(noisy.ravel())
    o = Outs(n, n * L)
    ctx.revive(rows, par, maps, k, L, n, o.out, status=o.status, revived_idx=o.idx,
               revived_list=o.lst, counts=o.counts)
    ctx.sync()
    h = o.host()
    check_meta(h, case)
    assert np.array_equal(h["out"].reshape(n, L), case.want_out)


# ---- 8. optional outputs ------------------------------------------------------
@gpu
@pytest.mark.parametrize("absent", ["idx", "lst", "counts", "out", "all"])
def test_optional_outputs(ctx, absent):
    case = stride_case()
    n, k, L = case.n, case.k, case.L
    gone = {"idx", "lst", "counts", "out"} if absent == "all" else {absent}
    rows, par, maps = dev(case.rows_in.ravel()), dev(case.par_in.ravel()), dev(case.maps.ravel())
    o = Outs(n, n * L)
    ctx.revive(rows, par, maps, k, L, n, None if "out" in gone else o.out, status=o.status,
               revived_idx=None if "idx" in gone else o.idx,
               revived_list=None if "lst" in gone else o.lst,
               counts=None if "counts" in gone else o.counts)
    ctx.sync()
    h = o.host()
    check_meta(h, case, what={"status", "idx", "lst", "counts"} - gone)
    if "idx" in gone:
        assert np.all(h["idx"] == POISON)
    if "lst" in gone:
        assert np.all(h["lst"] == POISON64)
    if "counts" in gone:
        assert np.all(h["counts"] == POISON64)
    rows_h = rows.cpu().numpy().reshape(n, k, L)
    if "out" in gone:  # in place
        assert np.all(h["out"] == POISON)
        assert np.array_equal(rows_h, case.want_rows)
    else:
        assert np.array_equal(h["out"].reshape(n, L), case.want_out)
        assert np.array_equal(rows_h, case.rows_in)


@gpu
def test_zero_groups(ctx):
    o = Outs(0)
    ctx.revive(o.out, o.out, o.out, 10, 1350, 0, None, status=o.status, counts=o.counts)
    ctx.sync()
    h = o.host()
    assert h["counts"].tolist() == [0, 0, 0]
    assert bool((o.status == POISON).all())


# ---- 9. refusals --------------------------------------------------------------
@gpu
def test_refusals(ctx):
    case = stride_case()
    n, k, L = case.n, case.k, case.L
    rows, par, maps = dev(case.rows_in.ravel()), dev(case.par_in.ravel()), dev(case.maps.ravel())
    o = Outs(n, n * L)
    lib, P = ctx.lib, qfec._ptr
    INV, INT = qfec.QFEC_ERR_INVALID_FEC_DATA, qfec.QFEC_ERR_INTERNAL
    nb = k // 8 + 1

    def dense(k_=k, L_=L, rows_=rows, par_=par, maps_=maps, status_=o.status, flags=0):
        return lib.qfec_revive_batch(ctx.ctx, P(rows_), P(par_), P(maps_), k_, L_, n, P(o.out),
                                     P(status_), P(o.idx), P(o.lst), P(o.counts), flags)

    def strided(rs=L, gs=k * L, ps=L, ms=nb, os_=L):
        return lib.qfec_revive_batch_strided(ctx.ctx, P(rows), P(par), P(maps), k, L, rs, gs, ps,
                                             ms, n, P(o.out), os_, P(o.status), P(o.idx),
                                             P(o.lst), P(o.counts), 0)

    refused = [
        ("k = 0", lambda: dense(k_=0), INV),
        ("k = 256", lambda: dense(k_=256), INV),
        ("L = 0", lambda: dense(L_=0), INV),
        ("L = 1453", lambda: dense(L_=1453), INV),
        ("map_stride", lambda: strided(ms=nb - 1), INV),
        ("row_stride", lambda: strided(rs=L - 1), INV),
        ("group_stride", lambda: strided(gs=k * L - 1), INV),
        ("parity_stride", lambda: strided(ps=L - 1), INV),
        ("out_stride", lambda: strided(os_=L - 1), INV),
        ("rows NULL", lambda: dense(rows_=None), INT),
        ("received NULL", lambda: dense(maps_=None), INT),
        ("status NULL", lambda: dense(status_=None), INT),
        ("parity NULL", lambda: dense(par_=None), INT),
        ("host pointers", lambda: dense(flags=qfec.QFEC_PTR_HOST), INT),
        ("mapped pointers", lambda: dense(flags=qfec.QFEC_PTR_MAPPED), INT),
        ("async", lambda: dense(flags=qfec.QFEC_PTR_MAPPED | qfec.QFEC_ASYNC), INT),
    ]
    for name, call, code in refused:
        # a valid call's message first: the refusal must write its own
        assert strided() == qfec.QFEC_OK
        assert call() == code, name
        assert lib.qfec_last_error(ctx.ctx), name
        assert ctx.sync() == qfec.QFEC_OK
    # what a refused call leaves: nothing launched, nothing written
    o.repoison()
    for name, call, code in refused:
        assert call() == code, name
    ctx.sync()
    h = o.host()
    assert np.all(h["status"] == POISON) and np.all(h["idx"] == POISON)
    assert np.all(h["lst"] == POISON64) and np.all(h["counts"] == POISON64)
    assert np.all(h["out"] == POISON)
    assert np.array_equal(rows.cpu().numpy(), case.rows_in.ravel())
    # a following valid call on the same context succeeds
    assert dense() == qfec.QFEC_OK
    assert ctx.sync() == qfec.QFEC_OK
    h = o.host()
    check_meta(h, case)
    assert np.array_equal(h["out"].reshape(n, L), case.want_out)


@gpu
def test_refusal_messages_are_specific(ctx):
    o = Outs(4, 4 * 64)
    with pytest.raises(qfec.InvalidFecData, match="receive map stride"):
        ctx.revive(o.out, o.out, o.out, 10, 16, 4, None, status=o.status, map_stride=1)
    with pytest.raises(qfec.QfecError, match="device pointers only"):
        ctx._check(ctx.lib.qfec_revive_batch(ctx.ctx, 1, 1, 1, 10, 16, 4, None, 1, None, None,
                                             None, qfec.QFEC_PTR_HOST))
    assert ctx.sync() == qfec.QFEC_OK


# ---- 10. consistency with the dense recover -----------------------------------
@gpu
def test_matches_dense_recover(ctx):
    k, L, n = 10, 1350, 4099
    rows = torch.empty(n * k * L, dtype=torch.uint8, device=DEV)
    ctx.synth_fixed(rows, k, L, 0, n, Q.SEED_FIXED)
    par = torch.empty(n * L, dtype=torch.uint8, device=DEV)
    ctx.encode(rows, k, L, n, par)
    miss_np = Q.drop_index(Q.SEED_DROP, np.arange(n), k).astype(np.uint8)
    data = np.ones((n, k), dtype=bool)
    data[np.arange(n), miss_np.astype(np.int64)] = False
    ctx.sync()
    r3 = rows.view(n, k, L)
    erased = r3[torch.arange(n, device=DEV), dev(miss_np).long()].clone()
    r3[torch.arange(n, device=DEV), dev(miss_np).long()] = LOST
    maps = dev(qfec.pack_received(data, np.ones(n, dtype=bool)).ravel())
    miss = dev(miss_np)
    dense = torch.full((n * L,), POISON, dtype=torch.uint8, device=DEV)
    ctx.recover(rows, par, miss, k, L, n, dense)
    o = Outs(n, n * L)
    ctx.revive(rows, par, maps, k, L, n, o.out, status=o.status, revived_idx=o.idx,
               revived_list=o.lst, counts=o.counts)
    ctx.sync()
    h = o.host()
    assert torch.equal(o.out, dense)
    assert torch.equal(o.out.view(n, L), erased)
    assert np.all(h["status"] == qfec.GROUP_REVIVED)
    assert np.array_equal(h["idx"], miss_np)
    assert np.array_equal(h["lst"], np.arange(n, dtype=np.uint64))
    assert h["counts"].tolist() == [0, n, 0]


# ---- 11. moderate size --------------------------------------------------------
@gpu
@pytest.mark.parametrize("inplace", [False, True])
def test_moderate_batch(ctx, inplace):
    k, L, n = 10, 1350, 1 << 14
    rng = np.random.default_rng(1111)
    r = rng.random(n)
    kinds = np.where(r < 0.05, 1, np.where(r < 0.06, 2, 0))
    data, fec = maps_from_kinds(kinds, k, rng)
    status, idx, lst, counts = reference(data, fec)
    assert 600 < counts[1] < 1100 and 100 < counts[2] < 250
    rows = torch.empty(n * k * L, dtype=torch.uint8, device=DEV)
    ctx.synth_fixed(rows, k, L, 0, n, Q.SEED_FIXED)
    par0 = torch.empty(n * L, dtype=torch.uint8, device=DEV)
    ctx.encode(rows, k, L, n, par0)
    ctx.sync()
    r3 = rows.view(n, k, L)
    lost_g, lost_i = np.nonzero(~data)
    r3[dev(lost_g), dev(lost_i)] = LOST
    par = par0.clone()
    par.view(n, L)[dev(np.flatnonzero(~fec))] = NOFEC
    before = rows.clone()
    # the reference for the revived bytes: a torch XOR on the device
    sel = dev(lst.astype(np.int64))
    m = dev(idx[lst.astype(np.int64)].astype(np.int64))
    pick = r3[sel].clone()
    pick[torch.arange(sel.numel(), device=DEV), m] = par.view(n, L)[sel]
    want = pick[:, 0].clone()
    for i in range(1, k):
        want ^= pick[:, i]
    maps = dev(qfec.pack_received(data, fec).ravel())
    o = Outs(n, n * L)
    ctx.revive(rows, par, maps, k, L, n, None if inplace else o.out, status=o.status,
               revived_idx=o.idx, revived_list=o.lst, counts=o.counts)
    ctx.sync()
    h = o.host()
    assert np.array_equal(h["status"], status) and np.array_equal(h["idx"], idx)
    assert np.array_equal(h["counts"], counts)
    assert np.array_equal(h["lst"][:lst.size], lst) and np.all(h["lst"][lst.size:] == POISON64)
    if not inplace:
        expect = torch.full((n, L), POISON, dtype=torch.uint8, device=DEV)
        expect[sel] = want
        assert torch.equal(o.out.view(n, L), expect)
        assert torch.equal(rows, before)
        return
    expect = before.clone()
    expect.view(n, k, L)[sel, m] = want
    assert torch.equal(rows, expect)
    # an encode over the repaired rows: the original parity for every group
    # that is now complete
    par2 = torch.empty(n * L, dtype=torch.uint8, device=DEV)
    ctx.encode(rows, k, L, n, par2)
    ctx.sync()
    whole = dev(np.flatnonzero(status != qfec.GROUP_UNREVIVABLE))
    assert torch.equal(par2.view(n, L)[whole], par0.view(n, L)[whole])
