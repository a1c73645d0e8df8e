"""qfec_emit_accumulated / qfec_revive_accumulated on the GPU: close the running
rows of qfec_accumulate_ragged, bit for bit against the rules of
tests/close_rule.py (pinned to oracle/qfec_np.py by test_close_rule.py).

Discipline, as in test_hip_accumulate_ragged.py: every offset is in range, so a
wrong kernel gives wrong bytes, not a fault.  Slots no group names hold a
POISON row and a POISON length; out is PAD-filled with a tail behind the last
range; revived_list is POISON past the count.  Whole buffers are compared: acc,
acc_len, out, out_len, status, revived_idx, revived_list, counts.
"""
import numpy as np
import pytest
import torch

import close_rule as R
from oracle import oracle_c as OC
from libquic_amd import qfec
from test_hip_accumulate_ragged import Acc, Turn, arena_groups, dview, split3

gpu = pytest.mark.gpu
DEV = "cuda:0"
POISON, PAD = 0xA5, 0x5A
POISON16 = np.uint16(0xA5A5)
POISON64 = np.uint64(0xA5A5A5A5A5A5A5A5)
TAIL = 32
MSG = {R.ERR_SLOT: "missing packet index >= FEC group size",
       R.ERR_GROUP: "FEC group with 0 or more than 255 packets",
       R.ERR_ROWLEN: "Illegal FEC redundancy length"}


def host(t, dtype):
    return t.cpu().numpy().view(dtype)


class Rows:
    """Running rows as an accumulate left them.  lens: {slot: length}; a named
    slot's row is random over the whole stride (bytes at or beyond the length
    are garbage that must not travel), every other slot POISON.  base: the
    buffer starts that many bytes into its allocation."""

    def __init__(self, rng, n_slots, stride, lens, base=0):
        self.n_slots, self.stride, self.base = n_slots, stride, base
        self.acc = np.full(n_slots * stride + TAIL, POISON, np.uint8)
        self.acc_len = np.full(n_slots, POISON16, np.uint16)
        for s, ln in lens.items():
            self.acc[s * stride:(s + 1) * stride] = rng.integers(0, 256, stride, dtype=np.uint8)
            self.acc_len[s] = ln
        self.d_buf = dview(np.concatenate([np.full(base, POISON, np.uint8), self.acc]))
        self.d_acc = self.d_buf.data_ptr() + base
        self.d_len = dview(self.acc_len)

    def check(self, want_len):
        got = host(self.d_buf, np.uint8)
        assert np.all(got[:self.base] == POISON) and np.array_equal(got[self.base:], self.acc), \
            "acc bytes changed"
        got_len = host(self.d_len, np.uint16)
        bad = np.flatnonzero(got_len != want_len)
        assert bad.size == 0, f"acc_len differs at slots {bad[:8]}: {got_len[bad[:8]]} " \
                              f"want {want_len[bad[:8]]}"


def place(lens, mods=None, gap=3):
    """out_off for ranges of lens bytes: range g starts at mods[g] modulo 16
    (None: byte-packed with gaps).  Returns (out_off, out size with the tail)."""
    off, pos = np.zeros(len(lens), np.uint64), 0
    for g, ln in enumerate(lens):
        if mods is not None:
            pos = (pos + 15) // 16 * 16 + int(mods[g])
        off[g] = pos
        pos += int(ln) + gap
    return off, pos + TAIL


def same(name, got, want):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{name}: {bad.size} differ, first at {bad[0]}: {got[bad[0]]} " \
                          f"want {want[bad[0]]}"


def run_emit(ctx, rows, n, out_off, out_size, slot=None, release=False, sync=True):
    """One emit against the rule, whole buffers.  Returns the rule's errors
    (sync=False: the caller syncs, then calls the returned check)."""
    want_out = np.full(out_size, PAD, np.uint8)
    want_olen = np.full(n, POISON16, np.uint16)
    want_len = rows.acc_len.copy()
    errs = R.emit(rows.acc, rows.stride, want_len, n, want_out, out_off, want_olen, slot, release)
    d_out = torch.full((out_size,), PAD, dtype=torch.uint8, device=DEV)
    d_olen, d_off = dview(np.full(n, POISON16, np.uint16)), dview(out_off)
    d_slot = None if slot is None else dview(np.asarray(slot, np.uint32))
    ctx.emit_accumulated(rows.d_acc, rows.stride, rows.d_len, n, d_out, d_off, d_olen,
                         slot=d_slot, n_slots=rows.n_slots, release=release)
    keep = [d_off, d_slot]  # (alive until the check: the call only queues)

    def check():
        same("out_len", host(d_olen, np.uint16), want_olen)
        same("out", host(d_out, np.uint8), want_out)
        rows.check(want_len)
        rows.acc_len = want_len
        keep.clear()

    if sync:
        ctx.sync()
        check()
        return errs
    return errs, check


def run_revive(ctx, rows, gk, maps, out_off, out_size, slot=None, mask=0, no_out=False,
               optional=True, sync=True):
    """One revive against the rule, whole buffers."""
    n = len(gk)
    want_out = np.full(out_size, PAD, np.uint8)
    want_olen = np.full(n, POISON16, np.uint16)
    want_st, want_idx = np.full(n, POISON, np.uint8), np.full(n, POISON, np.uint8)
    want_len = rows.acc_len.copy()
    errs, rlist, counts = R.revive(rows.acc, rows.stride, want_len, gk, maps, n,
                                   None if no_out else want_out, out_off, want_olen, want_st,
                                   want_idx, slot, mask)
    want_list = np.full(n, POISON64, np.uint64)
    want_list[:rlist.size] = rlist
    d_out = torch.full((out_size,), PAD, dtype=torch.uint8, device=DEV)
    d_olen, d_off = dview(np.full(n, POISON16, np.uint16)), dview(out_off)
    d_st, d_idx = dview(np.full(n, POISON, np.uint8)), dview(np.full(n, POISON, np.uint8))
    d_list, d_cnt = dview(np.full(n, POISON64, np.uint64)), dview(np.full(3, POISON64, np.uint64))
    d_gk, d_maps = dview(np.asarray(gk, np.uint8)), dview(maps)
    d_slot = None if slot is None else dview(np.asarray(slot, np.uint32))
    ctx.revive_accumulated(rows.d_acc, rows.stride, rows.d_len, d_gk, d_maps, maps.shape[1], n,
                           None if no_out else d_out, None if no_out else d_off, d_olen,
                           status=d_st, slot=d_slot, n_slots=rows.n_slots,
                           revived_idx=d_idx if optional else None,
                           revived_list=d_list if optional else None,
                           counts=d_cnt if optional else None, release_mask=mask)
    keep = [d_off, d_gk, d_maps, d_slot]  # (alive until the check: the call only queues)

    def check():
        same("status", host(d_st, np.uint8), want_st)
        same("out_len", host(d_olen, np.uint16), want_olen)
        if optional:
            same("revived_idx", host(d_idx, np.uint8), want_idx)
            same("revived_list", host(d_list, np.uint64), want_list)
            same("counts", host(d_cnt, np.uint64), counts)
        same("out", host(d_out, np.uint8), want_out)
        rows.check(want_len)
        rows.acc_len = want_len
        keep.clear()

    if sync:
        ctx.sync()
        check()
        return errs
    return errs, check


def make_maps(rng, ks, kinds, map_stride=None, junk=True):
    """kinds per group: 0 complete, 1 revived, 2 unrevivable (one data packet
    and the FEC packet missing, or two data packets).  junk: bits above k set
    at random."""
    n = len(ks)
    ms = int(max(ks)) // 8 + 1 if map_stride is None else map_stride
    bits = rng.integers(0, 2, (n, 8 * ms)).astype(bool) if junk else np.zeros((n, 8 * ms), bool)
    for g, (k, kind) in enumerate(zip(ks, kinds)):
        k = int(k)
        bits[g, :k] = True
        if kind == 1:
            bits[g, int(rng.integers(0, k))] = False
            bits[g, k] = True
        elif kind == 2:
            if k >= 2 and rng.integers(0, 2):
                bits[g, rng.permutation(k)[:2]] = False
            else:
                bits[g, int(rng.integers(0, k))] = False
                bits[g, k] = False
    return np.packbits(bits, axis=1, bitorder="little")


# ---- 1. the gather's edges ----------------------------------------------------------------
EDGE_LENS = [1, 15, 16, 17, 31, 32, 33, 1023, 1024, 1025, 1040, 1451, 1452]
EDGE_MODS = [0, 1, 8, 15]


@gpu
@pytest.mark.parametrize("base", [0, 1])
@pytest.mark.parametrize("stride", [1536, 1452])
@pytest.mark.parametrize("call", ["emit", "revive"])
def test_gather_edges(ctx, call, stride, base):
    rng = np.random.default_rng(11)
    cases = [(ln, mod) for ln in EDGE_LENS + ([0] if call == "emit" else []) for mod in EDGE_MODS]
    cases = [cases[i] for i in rng.permutation(len(cases))]
    n = len(cases)
    slot = rng.permutation(n + 9)[:n].astype(np.uint32)
    rows = Rows(rng, n + 9, stride, {int(slot[g]): cases[g][0] for g in range(n)}, base)
    out_off, size = place([c[0] for c in cases], [c[1] for c in cases])
    if call == "emit":
        assert not run_emit(ctx, rows, n, out_off, size, slot, release=True).any()
        assert not rows.acc_len[slot].any()
    else:
        ks = rng.integers(1, 16, n).astype(np.uint8)
        maps = make_maps(rng, ks, [1] * n)
        assert not run_revive(ctx, rows, ks, maps, out_off, size, slot, mask=0b010).any()
        assert not rows.acc_len[slot].any()


# ---- 2. the classification's edges ----------------------------------------------------------
@gpu
@pytest.mark.parametrize("map_stride", [None, 40])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1025])
def test_classify_edges(ctx, n, map_stride):
    rng = np.random.default_rng(20 + n)
    kset = [1, 7, 8, 9, 31, 32, 33, 63, 64, 255]
    ks = np.array([kset[g % len(kset)] for g in rng.permutation(n)], np.uint8)
    if n == 1:
        ks[0] = 255
    kinds = rng.integers(0, 3, n)
    stride = 48
    lens = rng.integers(1, stride + 1, n)
    rows = Rows(rng, n, stride, {g: int(lens[g]) for g in range(n)})
    out_off, size = place(lens)
    maps = make_maps(rng, ks, kinds, map_stride)
    assert maps.shape[1] == (40 if map_stride else int(ks.max()) // 8 + 1)
    assert not run_revive(ctx, rows, ks, maps, out_off, size, None, mask=0b011).any()


@gpu
@pytest.mark.parametrize("kind", [0, 1])
def test_all_one_status(ctx, kind):
    rng = np.random.default_rng(31 + kind)
    n, stride = 300, 80
    ks = rng.integers(1, 256, n).astype(np.uint8)
    lens = rng.integers(1, stride + 1, n)
    rows = Rows(rng, n, stride, {g: int(lens[g]) for g in range(n)})
    out_off, size = place(lens)
    maps = make_maps(rng, ks, [kind] * n)
    assert not run_revive(ctx, rows, ks, maps, out_off, size, None, mask=0b111).any()
    assert not rows.acc_len.any()


def classify_one_byte(maps, k=7):
    """status and revived_idx of groups of k = 7 from their one map byte, over
    the whole array; tied to the rule on every 257th group and the last"""
    n = len(maps)
    data = maps[:, 0] & 0x7F
    miss = k - np.unpackbits(data[:, None], axis=1).sum(axis=1)
    fec = maps[:, 0] >> 7
    st = np.where(miss == 0, R.COMPLETE, np.where((miss == 1) & (fec == 1), R.REVIVED,
                                                  R.UNREVIVABLE)).astype(np.uint8)
    first = np.array([[i for i in range(8) if not (v >> i) & 1][0] if v != 0xFF else 0xFF
                      for v in range(256)], np.uint8)[data | 0x80]
    idx = np.where(st == R.REVIVED, first, 0xFF).astype(np.uint8)
    for g in list(range(0, n, 257)) + [n - 1]:
        assert R.classify(maps[g], k) == (int(st[g]), int(idx[g]))
    return st, idx


@gpu
def test_second_scan_tile(ctx):
    """256 * 1024 + 1 groups of 16-B rows: the scan kernel's second tile.  The
    expectation is vectorised (k = 7, one map byte) and tied to the rule on a
    sample."""
    rng = np.random.default_rng(41)
    n, k = 256 * 1024 + 1, 7
    maps = rng.integers(0, 256, (n, 1), dtype=np.uint8)
    maps[rng.integers(0, n, n // 2), 0] |= 0x7F  # more complete groups than chance gives
    st, idx = classify_one_byte(maps, k)
    acc = rng.integers(0, 256, n * 16, dtype=np.uint8)
    acc_len = np.full(n, 16, np.uint16)
    rev = np.flatnonzero(st == R.REVIVED)
    want_out = np.full(n * 16 + TAIL, PAD, np.uint8)
    want_out[:n * 16].reshape(n, 16)[rev] = acc.reshape(n, 16)[rev]
    want_olen = np.where(st == R.REVIVED, 16, 0).astype(np.uint16)
    want_len = np.where(st != R.UNREVIVABLE, 0, 16).astype(np.uint16)
    want_list = np.full(n, POISON64, np.uint64)
    want_list[:rev.size] = rev
    d_acc, d_len = dview(acc), dview(acc_len)
    d_out = torch.full((n * 16 + TAIL,), PAD, dtype=torch.uint8, device=DEV)
    d_off = dview(np.arange(n, dtype=np.uint64) * np.uint64(16))
    d_olen, d_st, d_idx = (dview(np.full(n, POISON16, np.uint16)),
                           dview(np.full(n, POISON, np.uint8)), dview(np.full(n, POISON, np.uint8)))
    d_list, d_cnt = dview(np.full(n, POISON64, np.uint64)), dview(np.full(3, POISON64, np.uint64))
    d_gk, d_maps = dview(np.full(n, k, np.uint8)), dview(maps)
    ctx.revive_accumulated(d_acc, 16, d_len, d_gk, d_maps, 1, n, d_out, d_off, d_olen,
                           status=d_st, revived_idx=d_idx, revived_list=d_list, counts=d_cnt,
                           release_mask=0b011)
    ctx.sync()
    same("status", host(d_st, np.uint8), st)
    same("revived_idx", host(d_idx, np.uint8), idx)
    same("revived_list", host(d_list, np.uint64), want_list)
    assert host(d_cnt, np.uint64).tolist() == [int((st == s).sum()) for s in range(3)]
    same("out_len", host(d_olen, np.uint16), want_olen)
    same("out", host(d_out, np.uint8), want_out)
    same("acc_len", host(d_len, np.uint16), want_len)
    same("acc", host(d_acc, np.uint8), acc)


# ---- 3. slots and release ------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("slots", ["identity", "permuted"])
@pytest.mark.parametrize("mask", [0, 0b010, 0b011, 0b111])
def test_revive_slots_and_release(ctx, slots, mask):
    rng = np.random.default_rng(50 + mask)
    n = 70
    n_slots = n if slots == "identity" else 2 * n
    slot = None if slots == "identity" else rng.permutation(n_slots)[:n].astype(np.uint32)
    named = np.arange(n) if slot is None else slot
    lens = rng.integers(1, 1453, n)
    rows = Rows(rng, n_slots, 1536, {int(named[g]): int(lens[g]) for g in range(n)})
    ks = rng.integers(1, 40, n).astype(np.uint8)
    kinds = rng.integers(0, 3, n)
    maps = make_maps(rng, ks, kinds)
    out_off, size = place(lens)
    assert not run_revive(ctx, rows, ks, maps, out_off, size, slot, mask=mask).any()
    for g in range(n):
        assert rows.acc_len[int(named[g])] == (0 if (mask >> int(kinds[g])) & 1 else lens[g])


@gpu
@pytest.mark.parametrize("slots", ["identity", "permuted"])
@pytest.mark.parametrize("release", [0, 1])
def test_emit_slots_and_release(ctx, slots, release):
    rng = np.random.default_rng(60 + release)
    n = 70
    n_slots = n + 3 if slots == "identity" else 2 * n
    slot = None if slots == "identity" else rng.permutation(n_slots)[:n].astype(np.uint32)
    named = np.arange(n) if slot is None else slot
    lens = rng.integers(0, 1453, n)
    rows = Rows(rng, n_slots, 1536, {int(named[g]): int(lens[g]) for g in range(n)})
    out_off, size = place(lens)
    assert not run_emit(ctx, rows, n, out_off, size, slot, release=bool(release)).any()
    assert np.array_equal(rows.acc_len[named], np.zeros(n) if release else lens)


@gpu
def test_revive_without_out(ctx):
    rng = np.random.default_rng(71)
    n = 90
    lens = rng.integers(1, 1453, n)
    rows = Rows(rng, n, 1536, {g: int(lens[g]) for g in range(n)})
    ks = rng.integers(1, 20, n).astype(np.uint8)
    maps = make_maps(rng, ks, rng.integers(0, 3, n))
    out_off = np.full(n, POISON64, np.uint64)  # (never read)
    assert not run_revive(ctx, rows, ks, maps, out_off, 64, None, mask=0b011, no_out=True).any()
    # the optional outputs absent as well
    rows = Rows(rng, n, 1536, {g: int(lens[g]) for g in range(n)})
    assert not run_revive(ctx, rows, ks, maps, out_off, 64, None, mask=0, no_out=True,
                          optional=False).any()


# ---- 4. stream order: two generations in the same slots, no sync between ---------------------
@gpu
def test_stream_order(ctx):
    rng = np.random.default_rng(81)
    n, stride = 40, 1536
    gen1, gen2 = arena_groups(rng, n), arena_groups(rng, n)
    st = Acc(n, stride, {g: 0 for g in range(n)}, rng)
    t1, t2 = Turn(gen1).upload(), Turn(gen2).upload()
    ks = np.array([len(g) for g in gen1], np.uint8)
    maps = make_maps(rng, ks, rng.integers(0, 3, n))
    d_gk, d_maps = dview(ks), dview(maps)
    d_st, d_olen = dview(np.zeros(n, np.uint8)), dview(np.zeros(n, np.uint16))
    poff = np.arange(n, dtype=np.uint64) * np.uint64(stride)
    d_off = dview(poff)
    out1 = torch.full((n * stride,), PAD, dtype=torch.uint8, device=DEV)
    out2 = torch.full((n * stride + TAIL,), PAD, dtype=torch.uint8, device=DEV)
    d_olen2 = dview(np.full(n, POISON16, np.uint16))
    ctx.accumulate_ragged(*t1.d, n, st.d_acc, stride, st.d_len)
    ctx.revive_accumulated(st.d_acc, stride, st.d_len, d_gk, d_maps, maps.shape[1], n, out1, d_off,
                           d_olen, status=d_st, release_mask=0b111)
    ctx.accumulate_ragged(*t2.d, n, st.d_acc, stride, st.d_len)
    ctx.emit_accumulated(st.d_acc, stride, st.d_len, n, out2, d_off, d_olen2, release=True)
    ctx.sync()
    rc, par, plen = OC.encode_ragged(t2.data, t2.off, t2.ln, t2.ptr, poff, n * stride + TAIL)
    assert rc == 0
    want = np.full(n * stride + TAIL, PAD, np.uint8)
    for g in range(n):
        lo, hi = g * stride, g * stride + int(plen[g])
        want[lo:hi] = par[lo:hi]
    same("out_len", host(d_olen2, np.uint16), plen)
    same("out", host(out2, np.uint8), want)
    assert not host(st.d_len, np.uint16).any()
    # and the first generation's revived rows were those of the first fold
    rc, par1, plen1 = OC.encode_ragged(t1.data, t1.off, t1.ln, t1.ptr, poff, n * stride)
    assert rc == 0
    status = host(d_st, np.uint8)
    want1 = np.full(n * stride, PAD, np.uint8)
    for g in np.flatnonzero(status == R.REVIVED):
        lo, hi = g * stride, g * stride + int(plen1[g])
        want1[lo:hi] = par1[lo:hi]
    same("first generation", host(out1, np.uint8), want1)
    same("first lengths", host(d_olen, np.uint16), np.where(status == R.REVIVED, plen1, 0))


# ---- 5. end to end against the oracle ---------------------------------------------------------
@gpu
def test_end_to_end_oracle(ctx):
    rng = np.random.default_rng(91)
    n, stride = 2048, 1536
    groups = arena_groups(rng, n)
    full = Turn(groups)
    poff = np.arange(n, dtype=np.uint64) * np.uint64(stride)
    rc, par, plen = OC.encode_ragged(full.data, full.off, full.ln, full.ptr, poff,
                                     n * stride + TAIL)
    assert rc == 0
    # sender: three turns, then the emit
    snd = Acc(n, stride, {g: 0 for g in range(n)}, rng)
    for t in split3(rng, groups):
        tt = Turn(t).upload()
        snd.keep.append(tt)
        ctx.accumulate_ragged(*tt.d, n, snd.d_acc, stride, snd.d_len)
    d_off = dview(poff)
    out = torch.full((n * stride + TAIL,), PAD, dtype=torch.uint8, device=DEV)
    d_olen = dview(np.full(n, POISON16, np.uint16))
    ctx.emit_accumulated(snd.d_acc, stride, snd.d_len, n, out, d_off, d_olen, release=True)
    ctx.sync()
    want = np.full(n * stride + TAIL, PAD, np.uint8)
    for g in range(n):
        want[g * stride:g * stride + int(plen[g])] = par[g * stride:g * stride + int(plen[g])]
    same("sender out_len", host(d_olen, np.uint16), plen)
    same("sender out", host(out, np.uint8), want)
    # receiver: a third complete, a third lacking the FEC packet or a second
    # data packet, the rest revivable; what arrived is folded in three turns
    kind = rng.permutation(n) % 3  # 0 complete, 1 revivable, 2 unrevivable
    lost = np.array([int(rng.integers(0, len(g))) for g in groups], np.uint8)
    rcv = np.ones(full.ln.size - 1, bool)
    fec = np.ones(n, bool)
    arrived = []
    for g in range(n):
        p0, k = int(full.ptr[g]), len(groups[g])
        if kind[g] >= 1:
            rcv[p0 + int(lost[g])] = False
        if kind[g] == 2:
            if rng.integers(0, 2):
                fec[g] = False
            else:
                rcv[p0 + (int(lost[g]) + 1 + int(rng.integers(0, k - 1))) % k] = False
        got = [groups[g][i] for i in range(k) if rcv[p0 + i]]
        if fec[g]:
            got.append(par[g * stride:g * stride + int(plen[g])].copy())
        arrived.append(got)
    rcv_data = full.data.copy()
    for p in np.flatnonzero(~rcv):
        rcv_data[int(full.off[p]):int(full.off[p]) + int(full.ln[p])] = 0x3C
    rc, rec = OC.recover_ragged(rcv_data, full.off, full.ln, full.ptr, par, poff, plen, lost, poff,
                                n * stride + TAIL)
    assert rc == 0
    rx = Acc(n, stride, {g: 0 for g in range(n)}, rng)
    for t in split3(rng, arrived):
        tt = Turn(t).upload()
        rx.keep.append(tt)
        ctx.accumulate_ragged(*tt.d, n, rx.d_acc, stride, rx.d_len)
    maps = qfec.pack_received_ragged(rcv, fec, full.ptr)
    ks = np.array([len(g) for g in groups], np.uint8)
    d_gk, d_maps = dview(ks), dview(maps)
    out = torch.full((n * stride + TAIL,), PAD, dtype=torch.uint8, device=DEV)
    d_olen, d_st = dview(np.full(n, POISON16, np.uint16)), dview(np.full(n, POISON, np.uint8))
    d_idx, d_cnt = dview(np.full(n, POISON, np.uint8)), dview(np.zeros(3, np.uint64))
    ctx.revive_accumulated(rx.d_acc, stride, rx.d_len, d_gk, d_maps, maps.shape[1], n, out, d_off,
                           d_olen, status=d_st, revived_idx=d_idx, counts=d_cnt,
                           release_mask=0b011)
    ctx.sync()
    same("status", host(d_st, np.uint8), kind.astype(np.uint8))
    same("revived_idx", host(d_idx, np.uint8), np.where(kind == 1, lost, 0xFF).astype(np.uint8))
    assert host(d_cnt, np.uint64).tolist() == [int((kind == s).sum()) for s in range(3)]
    want = np.full(n * stride + TAIL, PAD, np.uint8)
    for g in np.flatnonzero(kind == 1):
        want[g * stride:g * stride + int(plen[g])] = rec[g * stride:g * stride + int(plen[g])]
    same("receiver out_len", host(d_olen, np.uint16), np.where(kind == 1, plen, 0))
    same("receiver out", host(out, np.uint8), want)
    got_len = host(rx.d_len, np.uint16)
    assert not got_len[kind != 2].any() and np.all(got_len[kind == 2] > 0)


# ---- 6. latched errors --------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("case,err", [
    ("slot_eq_n_slots", R.ERR_SLOT), ("k0", R.ERR_GROUP), ("k_over_map", R.ERR_GROUP),
    ("acc_len_over_lim", R.ERR_ROWLEN), ("acc_len_over_stride", R.ERR_ROWLEN),
    ("revived_len0", R.ERR_ROWLEN)])
def test_revive_latched_errors(ctx, case, err):
    rng = np.random.default_rng(101)
    n, n_slots, bad = 33, 40, 12
    stride = 1350 if case == "acc_len_over_stride" else 1536
    slot = rng.permutation(n_slots)[:n].astype(np.uint32)
    lens = {int(s): int(rng.integers(1, 1351)) for s in slot}
    ks = rng.integers(1, 16, n).astype(np.uint8)  # (k <= 15: two map bytes)
    kinds = rng.integers(0, 3, n)
    kinds[bad] = 1
    if case == "slot_eq_n_slots":
        del lens[int(slot[bad])]
        slot[bad] = n_slots
    elif case == "acc_len_over_lim":
        lens[int(slot[bad])] = 1453
    elif case == "acc_len_over_stride":
        lens[int(slot[bad])] = 1351
    elif case == "revived_len0":
        lens[int(slot[bad])] = 0
    maps = make_maps(rng, ks, kinds, map_stride=2)
    if case == "k0":
        ks[bad] = 0
    elif case == "k_over_map":
        ks[bad] = 16
    rows = Rows(rng, n_slots, stride, lens)
    before = rows.acc_len.copy()
    out_off, size = place([1452] * n)
    errs, check = run_revive(ctx, rows, ks, maps, out_off, size, slot, mask=0b111, sync=False)
    assert errs[bad] == err and np.count_nonzero(errs) == 1
    with pytest.raises(qfec.InvalidFecData, match=MSG[err]) as e:
        ctx.sync()
    assert e.value.code == -5
    assert ctx.sync() == qfec.QFEC_OK  # once
    check()
    if case != "slot_eq_n_slots":  # the offender: not released
        assert rows.acc_len[int(slot[bad])] == before[int(slot[bad])]


@gpu
@pytest.mark.parametrize("case,err", [
    ("slot_eq_n_slots", R.ERR_SLOT), ("acc_len_over_lim", R.ERR_ROWLEN),
    ("acc_len_over_stride", R.ERR_ROWLEN)])
def test_emit_latched_errors(ctx, case, err):
    rng = np.random.default_rng(111)
    n, n_slots, bad = 33, 40, 20
    stride = 1350 if case == "acc_len_over_stride" else 1536
    slot = rng.permutation(n_slots)[:n].astype(np.uint32)
    lens = {int(s): int(rng.integers(0, 1351)) for s in slot}
    if case == "slot_eq_n_slots":
        del lens[int(slot[bad])]
        slot[bad] = n_slots
    else:
        lens[int(slot[bad])] = 1453 if case == "acc_len_over_lim" else 1351
    rows = Rows(rng, n_slots, stride, lens)
    before = rows.acc_len.copy()
    out_off, size = place([1452] * n)
    errs, check = run_emit(ctx, rows, n, out_off, size, slot, release=True, sync=False)
    assert errs[bad] == err and np.count_nonzero(errs) == 1
    with pytest.raises(qfec.InvalidFecData, match=MSG[err]) as e:
        ctx.sync()
    assert e.value.code == -5
    assert ctx.sync() == qfec.QFEC_OK
    check()
    if case != "slot_eq_n_slots":
        assert rows.acc_len[int(slot[bad])] == before[int(slot[bad])]


# ---- 7. host refusals ------------------------------------------------------------------------------
@gpu
def test_host_refusals(ctx):
    rng = np.random.default_rng(121)
    n, n_slots, stride = 9, 12, 1536
    slot = dview(rng.permutation(n_slots)[:n].astype(np.uint32))
    acc = torch.full((n_slots * stride,), POISON, dtype=torch.uint8, device=DEV)
    bufs = dict(acc_len=dview(np.full(n_slots, POISON16, np.uint16)),
                gk=dview(np.full(n, POISON, np.uint8)), maps=dview(np.full(2 * n, POISON, np.uint8)),
                out=torch.full((n * stride,), POISON, dtype=torch.uint8, device=DEV),
                off=dview(np.arange(n, dtype=np.uint64) * np.uint64(stride)),
                out_len=dview(np.full(n, POISON16, np.uint16)),
                status=dview(np.full(n, POISON, np.uint8)), idx=dview(np.full(n, POISON, np.uint8)),
                rlist=dview(np.full(n, POISON64, np.uint64)),
                counts=dview(np.full(3, POISON64, np.uint64)))
    off_before = host(bufs["off"], np.uint64).copy()
    P = qfec._ptr
    ints = ("stride", "n_slots", "ms", "n", "release", "mask", "flags")
    emit_names = ["acc", "stride", "acc_len", "slot", "n_slots", "n", "out", "off", "out_len",
                  "release", "flags"]
    revive_names = ["acc", "stride", "acc_len", "slot", "n_slots", "gk", "maps", "ms", "n", "out",
                    "off", "out_len", "status", "idx", "rlist", "counts", "mask", "flags"]

    def raw(fn, names, **kw):
        a = dict(bufs, acc=acc, slot=slot, stride=stride, n_slots=n_slots, ms=2, n=n, release=1,
                 mask=7, flags=0)
        a.update(kw)
        rc = fn(ctx.ctx, *[a[x] if x in ints else P(a[x]) for x in names])
        return rc, ctx.lib.qfec_last_error(ctx.ctx).decode()

    def emit(**kw):
        return raw(ctx.lib.qfec_emit_accumulated, emit_names, **kw)

    def revive(**kw):
        return raw(ctx.lib.qfec_revive_accumulated, revive_names, **kw)

    def untouched():
        assert ctx.sync() == qfec.QFEC_OK
        assert torch.all(acc == POISON)
        for name, t in bufs.items():
            if name == "off":
                assert np.array_equal(host(t, np.uint64), off_before)
            else:
                assert torch.all(t.view(torch.uint8) == POISON), name

    for call in (emit, revive):
        rc, msg = call(stride=0)
        assert rc == -5 and "accumulator stride 0" in msg
        untouched()
        for fl in (qfec.QFEC_PTR_HOST, qfec.QFEC_PTR_MAPPED, qfec.QFEC_ASYNC):
            rc, msg = call(flags=fl)
            assert rc == -1 and "device pointers only" in msg and "QFEC_ASYNC" in msg
            untouched()
        for kw in (dict(n=1 << 32), dict(n_slots=1 << 32)):
            rc, msg = call(**kw)
            assert rc == -1 and "2^32" in msg
            untouched()
        rc, msg = call(slot=None, n_slots=n - 1)
        assert rc == -1 and "fewer slots than groups" in msg
        untouched()
        assert ctx.lib.qfec_debug_fail_launches(ctx.ctx, 1) == 0
        try:
            rc, msg = call()
        finally:
            assert ctx.lib.qfec_debug_fail_launches(ctx.ctx, 0) == 0
        assert rc == -1 and "launch failure injected" in msg
        untouched()
    for name in ("acc", "acc_len", "out", "off", "out_len"):
        rc, msg = emit(**{name: None})
        assert rc == -1 and "null buffer" in msg, name
        untouched()
    for name in ("acc", "acc_len", "gk", "maps", "off", "out_len", "status"):
        rc, msg = revive(**{name: None})
        assert rc == -1 and "null buffer" in msg, name
        untouched()
    rc, msg = revive(ms=0)
    assert rc == -5 and "receive map stride 0" in msg
    untouched()
    for mask in (8, 0x10, 0xFFFFFFFF):
        rc, msg = revive(mask=mask)
        assert rc == -1 and "release_mask" in msg
        untouched()
    # no groups: decided before the buffers are looked at
    none = dict(acc=None, acc_len=None, slot=None, gk=None, maps=None, out=None, off=None,
                out_len=None, status=None, idx=None, rlist=None, n=0, n_slots=0)
    rc, msg = emit(**dict((k, v) for k, v in none.items() if k in emit_names))
    assert rc == qfec.QFEC_OK, msg
    rc, msg = revive(counts=None, **none)
    assert rc == qfec.QFEC_OK, msg
    untouched()
    rc, msg = revive(**none)
    assert rc == qfec.QFEC_OK, msg
    assert ctx.sync() == qfec.QFEC_OK
    assert host(bufs["counts"], np.uint64).tolist() == [0, 0, 0]


@gpu
def test_accepted_flags_change_nothing(ctx):
    rng = np.random.default_rng(131)
    n = 20
    lens = rng.integers(1, 1453, n)
    ks = rng.integers(1, 16, n).astype(np.uint8)
    maps = make_maps(rng, ks, rng.integers(0, 3, n))
    out_off, size = place(lens)
    for fl in (qfec.QFEC_CACHED, qfec.QFEC_SMALL_GROUPS):
        rows = Rows(rng, n, 1536, {g: int(lens[g]) for g in range(n)})
        want_out = np.full(size, PAD, np.uint8)
        want_olen = np.zeros(n, np.uint16)
        R.emit(rows.acc, 1536, rows.acc_len.copy(), n, want_out, out_off, want_olen)
        d_out = torch.full((size,), PAD, dtype=torch.uint8, device=DEV)
        d_off, d_olen = dview(out_off), dview(np.full(n, POISON16, np.uint16))
        ctx.emit_accumulated(rows.d_acc, 1536, rows.d_len, n, d_out, d_off, d_olen, flags=fl)
        d_out2 = torch.full((size,), PAD, dtype=torch.uint8, device=DEV)
        d_olen2, d_st = dview(np.full(n, POISON16, np.uint16)), dview(np.full(n, POISON, np.uint8))
        want_out2, want_olen2 = np.full(size, PAD, np.uint8), np.zeros(n, np.uint16)
        want_st = np.zeros(n, np.uint8)
        R.revive(rows.acc, 1536, rows.acc_len.copy(), ks, maps, n, want_out2, out_off, want_olen2,
                 want_st, np.zeros(n, np.uint8))
        d_gk, d_maps = dview(ks), dview(maps)
        ctx.revive_accumulated(rows.d_acc, 1536, rows.d_len, d_gk, d_maps, maps.shape[1], n, d_out2,
                               d_off, d_olen2, status=d_st, flags=fl)
        ctx.sync()
        same("emit out", host(d_out, np.uint8), want_out)
        same("emit out_len", host(d_olen, np.uint16), want_olen)
        same("revive out", host(d_out2, np.uint8), want_out2)
        same("revive out_len", host(d_olen2, np.uint16), want_olen2)
        same("status", host(d_st, np.uint8), want_st)
        rows.check(rows.acc_len)
