"""The rule of qfec_bin_arrivals (tests/bin_rule.py) on the CPU: against a
stable argsort of the slots, and, chained with the admit rule, against
admit_rule.admit over tables a host built by stable grouping -- per slot the
same verdicts, maps and admitted tables.  These pin the yardstick the GPU tests
compare with; the export test at the end needs the library to have the call.
"""
import ctypes
import os

import numpy as np
import pytest

import admit_rule as R
import bin_rule as B
from libquic_amd import qfec
from test_admit_rule import Batch, make_groups, scenario

STRIDE = 1536
POISON = 0xA5


def random_arrivals(rng, n, n_slots, p_none=0.1, n_bad=0):
    """n records in arrival order over n_slots slots (some slots unnamed)"""
    named = rng.permutation(n_slots)[:max(1, n_slots * 2 // 3)]
    slot = named[rng.integers(0, named.size, n)].astype(np.uint32)
    slot[rng.random(n) < p_none] = B.NO_SLOT
    for p in rng.permutation(n)[:n_bad]:
        slot[p] = rng.integers(n_slots, B.NO_SLOT)  # [n_slots, 0xFFFFFFFE]
    off = rng.integers(0, 1 << 63, n, dtype=np.uint64)
    ln = rng.integers(0, 1 << 16, n).astype(np.uint16)
    idx = rng.integers(0, 256, n).astype(np.uint8)
    ok = rng.integers(0, 2, n).astype(np.uint8)
    return slot, off, ln, idx, ok


@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("n,n_slots,n_bad", [(0, 5, 0), (1, 1, 0), (50, 7, 0), (2000, 300, 9),
                                             (500, 1000, 3)])
def test_rule_is_a_stable_argsort(seed, n, n_slots, n_bad):
    rng = np.random.default_rng(100 * seed + n)
    slot, off, ln, idx, ok = random_arrivals(rng, n, n_slots, n_bad=n_bad)
    ptr = np.full(n_slots + 1, 0xA5A5A5A5, np.uint32)
    o_off, o_ln = np.full(n + 1, 7, np.uint64), np.full(n + 1, 7, np.uint16)
    o_idx, o_ok, o_src = np.full(n + 1, 7, np.uint8), np.full(n + 1, 7, np.uint8), \
        np.full(n + 1, 7, np.uint32)
    errs, counts = B.bin_arrivals(slot, off, ln, idx, ok, n_slots, ptr, o_off, o_ln, o_idx, o_ok,
                                  o_src)
    order = np.argsort(slot, kind="stable")
    order = order[slot[order] < n_slots]  # in-range slots sort in front of everything else
    m = order.size
    assert counts.tolist() == [m, int((slot == B.NO_SLOT).sum()), n - m
                               - int((slot == B.NO_SLOT).sum())]
    assert counts[2] == n_bad and np.array_equal(errs != 0, (slot >= n_slots) & (slot != B.NO_SLOT))
    assert np.array_equal(ptr, np.searchsorted(slot[order], np.arange(n_slots + 1)))
    assert np.array_equal(o_src[:m], order)
    for got, src in ((o_off, off), (o_ln, ln), (o_idx, idx), (o_ok, ok)):
        assert np.array_equal(got[:m], src[order])
        assert np.all(got[m:] == 7)  # entries from ptr[n_slots] on: left alone
    assert np.all(o_src[m:] == 7)
    if n:  # without ok and src: the same tables, ok_out and src_out untouched
        ptr2, f_off, f_ln, f_idx = ptr.copy(), o_off.copy(), o_ln.copy(), o_idx.copy()
        ptr2[:], f_off[:], f_ln[:], f_idx[:] = 0, 7, 7, 7
        _, counts2 = B.bin_arrivals(slot, off, ln, idx, None, n_slots, ptr2, f_off, f_ln, f_idx)
        assert counts2.tolist() == counts.tolist()
        for a, b in ((ptr2, ptr), (f_off, o_off), (f_ln, o_ln), (f_idx, o_idx)):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("seed", range(3))
def test_admit_over_binned_tables_is_admit_over_host_grouped_tables(seed):
    """a turn's candidates shuffled into arrival order, binned in lockstep with
    the slots and admitted with slot=None, against the admit over the host's
    per-group tables with a slot list"""
    rng = np.random.default_rng(900 + seed)
    n, n_slots, ms = 60, 75, 2
    groups = make_groups(rng, n)
    cands, _, _, _, dup = scenario(rng, groups)
    assert len(dup) >= 10
    slot = rng.permutation(n_slots)[:n].astype(np.uint32)
    slot_k = np.full(n_slots, 1, np.uint8)  # (slots no group holds: K 1, never a candidate)
    slot_k[slot] = [len(g) - 1 for g in groups]
    maps_a = np.full((n_slots, ms), 0xFF, np.uint8)
    maps_b = maps_a.copy()
    len_a, len_b = np.zeros(n_slots, np.uint16), np.zeros(n_slots, np.uint16)
    for per_group in cands:
        b = Batch(per_group)
        m = b.m
        # (A) the host's tables, groups in batch order, slot list
        a_ptr, a_off, a_ln = np.zeros(n + 1, np.uint32), np.zeros(m + 1, np.uint64), \
            np.zeros(m + 1, np.uint16)
        a_v = np.full(m + 1, POISON, np.uint8)
        errs, a_cnt = R.admit(b.off, b.ln, b.idx, b.ok, b.ptr, slot_k, maps_a, len_a, STRIDE,
                              a_ptr, a_off, a_ln, a_v, slot)
        assert not errs.any()
        # (B) arrival order: a shuffle that keeps each group's own order is one
        # stable grouping's inverse; a plain shuffle changes which copy of a
        # duplicate comes first, so the host's tables (A) are regrouped from
        # the same shuffled arrivals
        perm = rng.permutation(m)
        grp_of = np.repeat(np.arange(n), np.diff(b.ptr).astype(np.int64))
        p_slot = slot[grp_of][perm].astype(np.uint32)
        p_off, p_ln, p_idx, p_ok = b.off[:m][perm], b.ln[:m][perm], b.idx[:m][perm], b.ok[:m][perm]
        # some arrivals belong to no open group
        extra = 7
        p_slot = np.concatenate([p_slot, np.full(extra, B.NO_SLOT, np.uint32)])
        p_off = np.concatenate([p_off, np.zeros(extra, np.uint64)])
        p_ln = np.concatenate([p_ln, np.zeros(extra, np.uint16)])
        p_idx = np.concatenate([p_idx, np.zeros(extra, np.uint8)])
        p_ok = np.concatenate([p_ok, np.zeros(extra, np.uint8)])
        mix = rng.permutation(m + extra)
        p_slot, p_off, p_ln, p_idx, p_ok = (x[mix] for x in (p_slot, p_off, p_ln, p_idx, p_ok))
        t_ptr = np.zeros(n_slots + 1, np.uint32)
        t_off, t_ln = np.zeros(m + extra + 1, np.uint64), np.zeros(m + extra + 1, np.uint16)
        t_idx, t_ok = np.zeros(m + extra + 1, np.uint8), np.zeros(m + extra + 1, np.uint8)
        t_src = np.zeros(m + extra + 1, np.uint32)
        errs, cnt = B.bin_arrivals(p_slot, p_off, p_ln, p_idx, p_ok, n_slots, t_ptr, t_off, t_ln,
                                   t_idx, t_ok, t_src)
        assert not errs.any() and cnt.tolist() == [m, extra, 0]
        # the host's stable grouping of the same arrivals, per group with a slot list
        h_order = np.concatenate([np.flatnonzero(p_slot == s) for s in slot])
        h_ptr = np.zeros(n + 1, np.uint32)
        h_ptr[1:] = np.cumsum([int((p_slot == s).sum()) for s in slot])
        h = [np.append(x[h_order], x[:1]) for x in (p_off, p_ln, p_idx, p_ok)]
        maps_h, len_h = maps_b.copy(), len_b.copy()
        h_ptr_out, h_off, h_ln = np.zeros(n + 1, np.uint32), np.zeros(m + 1, np.uint64), \
            np.zeros(m + 1, np.uint16)
        h_v = np.full(m + 1, POISON, np.uint8)
        errs, h_cnt = R.admit(h[0], h[1], h[2], h[3], h_ptr, slot_k, maps_h, len_h, STRIDE,
                              h_ptr_out, h_off, h_ln, h_v, slot)
        assert not errs.any()
        # the binned tables through the admit in lockstep with the slots
        b_ptr_out = np.zeros(n_slots + 1, np.uint32)
        b_off, b_ln = np.zeros(m + extra + 1, np.uint64), np.zeros(m + extra + 1, np.uint16)
        b_v = np.full(m + extra + 1, POISON, np.uint8)
        errs, b_cnt = R.admit(t_off, t_ln, t_idx, t_ok, t_ptr, slot_k, maps_b, len_b, STRIDE,
                              b_ptr_out, b_off, b_ln, b_v, None)
        assert not errs.any()
        assert b_cnt.tolist() == h_cnt.tolist()
        assert np.array_equal(maps_b, maps_h)
        for g in range(n):
            s = int(slot[g])
            hq, bq = slice(int(h_ptr[g]), int(h_ptr[g + 1])), slice(int(t_ptr[s]), int(t_ptr[s + 1]))
            assert np.array_equal(h_v[hq], b_v[bq]), g
            assert np.array_equal(h_order[hq], t_src[bq]), g  # verdicts map back to arrivals
            ho = slice(int(h_ptr_out[g]), int(h_ptr_out[g + 1]))
            bo = slice(int(b_ptr_out[s]), int(b_ptr_out[s + 1]))
            assert np.array_equal(h_off[ho], b_off[bo]) and np.array_equal(h_ln[ho], b_ln[bo]), g
        unnamed = np.setdiff1d(np.arange(n_slots), slot)
        assert not np.diff(t_ptr.astype(np.int64))[unnamed].any()
        # the distinct verified packets are the same set whatever the order
        # within a group, so turn (A)'s maps agree too
        assert np.array_equal(maps_a, maps_b) and a_cnt[R.FAILED] == b_cnt[R.FAILED]
        # the rows' lengths as the accumulate would leave them (the next turn's "fresh" test)
        for arr, ptr_o, ln_o, sl in ((len_a, a_ptr, a_ln, slot), (len_b, b_ptr_out, b_ln, None)):
            for g in range(len(ptr_o) - 1):
                s = g if sl is None else int(sl[g])
                seg = ln_o[int(ptr_o[g]):int(ptr_o[g + 1])]
                if seg.size:
                    arr[s] = max(int(arr[s]), int(seg.max()))
        assert np.array_equal(len_a, len_b)


def test_library_exports_the_call():
    sig = dict((s[0], s) for s in qfec.SIGNATURES)
    assert "qfec_bin_arrivals" in sig
    assert sig["qfec_bin_arrivals"][1] is ctypes.c_int and len(sig["qfec_bin_arrivals"][2]) == 16
    assert os.path.exists(qfec.LIB_PATH), "libqfec.so has not been built"
    # (symbol lookup only: nothing is called, no device is opened)
    lib = ctypes.CDLL(qfec.LIB_PATH)
    assert hasattr(lib, "qfec_bin_arrivals") and hasattr(qfec.Context, "bin_arrivals")
    assert qfec.QFEC_NO_SLOT == B.NO_SLOT
