"""The admit and tracked-revive rules (tests/admit_rule.py) against the rules
that exist and oracle/qfec_np.py, on the CPU: random ragged groups with losses
arrive over three turns in random order, with packets that failed to verify
(their bytes corrupted), duplicates within a turn and duplicates across turns;
admit -> accumulate_rule.accumulate -> tracked revive gives the oracle's
recovered packets and the receive maps of the distinct verified arrivals, and
without the admit a duplicated group's row is wrong.  These pin the yardstick
the GPU tests compare with; the export test at the end needs the library to
have the calls.
"""
import ctypes
import os

import numpy as np
import pytest

import accumulate_rule as A
import admit_rule as R
import close_rule as CR
from oracle import qfec_np as NP
from libquic_amd import qfec

STRIDE = 1536
POISON = 0xA5


def make_groups(rng, n, kmin=5, kmax=15, lmin=64, lmax=1350):
    """per group its K data payloads; item K of a group is its FEC redundancy"""
    groups = []
    for _ in range(n):
        k = int(rng.integers(kmin, kmax + 1))
        pays = [rng.integers(0, 256, int(x), dtype=np.uint8)
                for x in rng.integers(lmin, lmax + 1, k)]
        groups.append(pays + [NP.group_encode(pays)])
    return groups


def scenario(rng, groups, turns=3, quiet_last=()):
    """What arrives when.  Per group a kind (0 every data packet arrives, 1 one
    is lost, 2 beyond repair); every arrival lands in a random turn, then up to
    three injections: a copy that fails to verify (corrupted bytes, any index,
    the lost one included), a second copy later in the same turn, a copy in
    another turn.  quiet_last: groups whose traffic all lies before the last
    turn.  Returns (cands, kind, lost, verified, dup): cands[t][g] the turn's
    candidates of g in order, each (idx, bytes, good); verified[g] the indices
    that arrived verified at least once; dup the groups that saw a duplicate."""
    n = len(groups)
    cands = [[[] for _ in range(n)] for _ in range(turns)]
    kind, lost, verified, dup = np.zeros(n, np.int64), [], [], set()
    for g, items in enumerate(groups):
        k = len(items) - 1
        span = turns - 1 if g in quiet_last else turns
        kind[g] = rng.integers(0, 3)
        gone = set()
        if kind[g] >= 1:
            gone.add(int(rng.integers(0, k)))
        if kind[g] == 2:
            gone.add(k if rng.integers(0, 2) else
                     (min(gone) + 1 + int(rng.integers(0, k - 1))) % k)
        lost.append(gone)
        here = [i for i in range(k + 1) if i not in gone]
        verified.append(set(here))
        when = {i: int(rng.integers(0, span)) for i in here}
        for t in range(span):
            order = [i for i in here if when[i] == t]
            cands[t][g] = [(i, items[i], True) for i in rng.permutation(order)]
        if rng.random() < 0.4:  # fails to verify: never folded, sets no bit
            i, t = int(rng.integers(0, k + 1)), int(rng.integers(0, span))
            bad = items[i].copy()
            bad[rng.integers(0, bad.size, 3)] ^= 0x5A
            cands[t][g].insert(int(rng.integers(0, len(cands[t][g]) + 1)), (i, bad, False))
        if rng.random() < 0.4:  # twice in one turn
            i = here[int(rng.integers(0, len(here)))]
            lst = cands[when[i]][g]
            at = [j for j, c in enumerate(lst) if c[0] == i and c[2]][0]
            lst.insert(int(rng.integers(at + 1, len(lst) + 1)), (i, items[i].copy(), True))
            dup.add(g)
        if rng.random() < 0.4 and span > 1:  # again in another turn
            i = here[int(rng.integers(0, len(here)))]
            t = (when[i] + 1 + int(rng.integers(0, span - 1))) % span
            lst = cands[t][g]
            lst.insert(int(rng.integers(0, len(lst) + 1)), (i, items[i].copy(), True))
            dup.add(g)
    return cands, kind, lost, verified, dup


class Batch:
    """One turn's candidates as CSR tables, packets on 16-B boundaries, one
    trailing table entry nobody owns."""

    def __init__(self, per_group):
        flat = [c for g in per_group for c in g]
        self.n = len(per_group)
        self.ptr = np.zeros(self.n + 1, np.uint32)
        self.ptr[1:] = np.cumsum([len(g) for g in per_group])
        m = len(flat)
        self.off, self.ln = np.zeros(m + 1, np.uint64), np.zeros(m + 1, np.uint16)
        self.idx, self.ok = np.zeros(m + 1, np.uint8), np.zeros(m + 1, np.uint8)
        pos = 0
        for p, (i, b, good) in enumerate(flat):
            self.off[p], self.ln[p], self.idx[p], self.ok[p] = pos, b.size, i, good
            pos = (pos + b.size + 15) // 16 * 16
        self.data = np.full(pos + 32, 0x5A, np.uint8)
        for p, (i, b, good) in enumerate(flat):
            self.data[int(self.off[p]):int(self.off[p]) + b.size] = b
        self.m = m


def run_rules(rng, groups, cands, slot, n_slots, ms, use_admit=True):
    """admit -> accumulate per turn on host arrays that start as garbage (fresh
    slots: length 0, stale map and row).  Returns (acc, acc_len, maps)."""
    n = len(groups)
    acc = rng.integers(0, 256, n_slots * STRIDE, dtype=np.uint8)
    acc_len = np.zeros(n_slots, np.uint16)
    maps = np.full((n_slots, ms), 0xFF, np.uint8)
    slot_k = np.full(n_slots, POISON, np.uint8)
    slot_k[slot] = [len(g) - 1 for g in groups]
    for per_group in cands:
        b = Batch(per_group)
        if use_admit:
            ptr_out = np.zeros(n + 1, np.uint32)
            off_out, len_out = np.zeros(b.m + 1, np.uint64), np.zeros(b.m + 1, np.uint16)
            verdict = np.full(b.m + 1, POISON, np.uint8)
            errs, counts = R.admit(b.off, b.ln, b.idx, b.ok, b.ptr, slot_k, maps, acc_len, STRIDE,
                                   ptr_out, off_out, len_out, verdict, slot)
            assert not errs.any() and int(counts.sum()) == b.m
            assert counts[R.ADMITTED] == ptr_out[n] and verdict[b.m] == POISON
            for p in range(b.m):  # a verdict never contradicts the open call
                assert (verdict[p] == R.FAILED) == (b.ok[p] == 0)
            errs = A.accumulate(b.data, off_out, len_out, ptr_out, acc, STRIDE, acc_len, slot)
        else:
            errs = A.accumulate(b.data, b.off, b.ln, b.ptr, acc, STRIDE, acc_len, slot)
        assert not errs.any()
    return acc, acc_len, maps, slot_k


@pytest.mark.parametrize("seed", range(3))
def test_turns_with_failures_and_duplicates(seed):
    rng = np.random.default_rng(700 + seed)
    n, n_slots, ms = 60, 75, 2
    groups = make_groups(rng, n)
    cands, kind, lost, verified, dup = scenario(rng, groups)
    assert len(dup) >= 10
    slot = rng.permutation(n_slots)[:n].astype(np.uint32)
    acc, acc_len, maps, slot_k = run_rules(np.random.default_rng(seed), groups, cands, slot,
                                           n_slots, ms)
    # the maps are those of the distinct verified arrivals, whatever was injected
    ks = np.array([len(g) - 1 for g in groups])
    ptr = np.zeros(n + 1, np.uint32)
    ptr[1:] = np.cumsum(ks)
    rcv = np.concatenate([[i in verified[g] for i in range(ks[g])] for g in range(n)])
    fec = np.array([ks[g] in verified[g] for g in range(n)])
    want_maps = qfec.pack_received_ragged(rcv, fec, ptr, ms)
    for g in range(n):
        nb = ks[g] // 8 + 1
        assert np.array_equal(maps[slot[g], :nb], want_maps[g, :nb]), g
        assert np.all(maps[slot[g], nb:] == 0xFF)  # (bytes beyond the map: never written)
    unnamed = np.setdiff1d(np.arange(n_slots), slot)
    assert np.all(maps[unnamed] == 0xFF) and not acc_len[unnamed].any()
    # without the guard a duplicated packet cancels out of its row
    acc2, len2, _, _ = run_rules(np.random.default_rng(seed), groups, cands, slot, n_slots, ms,
                                 use_admit=False)
    wrong = [g for g in dup
             if not np.array_equal(acc2[slot[g] * STRIDE:slot[g] * STRIDE + int(len2[slot[g]])],
                                   acc[slot[g] * STRIDE:slot[g] * STRIDE + int(acc_len[slot[g]])])]
    assert wrong, "feeding every candidate to the accumulator changed no duplicated group's row"
    # the close: statuses by kind, revived packets the oracle's
    out_off = np.arange(n, dtype=np.uint64) * np.uint64(STRIDE)
    out = np.full(n * STRIDE, 0x5A, np.uint8)
    out_len = np.full(n, 0xA5A5, np.uint16)
    status, ridx = np.full(n, 9, np.uint8), np.full(n, 9, np.uint8)
    before = acc_len.copy()
    # ... and the same close through the existing rule on the gathered maps
    gk, gm = R.gather(maps, slot_k, acc_len, n, slot)
    out2, olen2 = out.copy(), out_len.copy()
    st2, ridx2, len_b = status.copy(), ridx.copy(), acc_len.copy()
    errs2, rlist2, counts2 = CR.revive(acc, STRIDE, len_b, gk, gm, n, out2, out_off, olen2, st2,
                                       ridx2, slot, 0b011)
    errs, rlist, counts = R.revive_tracked(acc, STRIDE, acc_len, maps, slot_k, n, out, out_off,
                                           out_len, status, ridx, slot, 0b011)
    assert not errs.any() and not errs2.any()
    assert np.array_equal(status, kind.astype(np.uint8))
    want = np.full(n * STRIDE, 0x5A, np.uint8)
    for g in np.flatnonzero(kind == 1):
        m = min(lost[g])
        assert ridx[g] == m
        rec = NP.group_recover(groups[g][:-1], groups[g][-1], m)
        assert out_len[g] == rec.size
        want[g * STRIDE:g * STRIDE + rec.size] = rec
        assert np.array_equal(rec[:groups[g][m].size], groups[g][m]) and not rec[groups[g][m].size:].any()
    assert np.array_equal(out, want)
    assert np.array_equal(out_len[kind != 1], np.zeros(int((kind != 1).sum()), np.uint16))
    assert not acc_len[slot[kind != 2]].any()
    assert np.array_equal(acc_len[slot[kind == 2]], before[slot[kind == 2]])
    for got, ref in ((out, out2), (out_len, olen2), (status, st2), (ridx, ridx2),
                     (acc_len, len_b), (rlist, rlist2), (counts, counts2)):
        assert np.array_equal(got, ref)


def test_tracked_revive_is_the_close_rule_on_gathered_maps():
    """every status, release mask and error class, fresh slots with stale maps among them"""
    rng = np.random.default_rng(800)
    n, n_slots, ms = 80, 90, 5
    slot = rng.permutation(n_slots)[:n].astype(np.uint32)
    slot[7] = n_slots  # out of range
    slot_k = rng.integers(1, 40, n_slots).astype(np.uint8)
    slot_k[slot[11]], slot_k[slot[12]] = 0, 40  # no packets; 40 // 8 + 1 = 6 bytes of map
    maps = rng.integers(0, 256, (n_slots, ms), dtype=np.uint8)
    for g in range(0, n, 3):  # enough complete and revivable groups
        if g != 7:
            k = int(slot_k[slot[g]])
            bits = np.ones(8 * ms, bool)
            if g % 2:
                bits[int(rng.integers(0, max(k, 1)))] = False
            maps[slot[g]] = np.packbits(bits, bitorder="little")
    acc_len0 = rng.integers(1, 1453, n_slots).astype(np.uint16)
    acc_len0[slot[[20, 21, 22, 23]]] = 0  # fresh slots, whatever their maps hold
    maps[slot[20]] = 0xFF
    acc_len0[slot[30]] = 1453
    maps[slot[30]], slot_k[slot[30]] = 0xFF, 9
    maps[slot[30], 0] = 0xFE  # revived, and its row too long
    acc = rng.integers(0, 256, n_slots * STRIDE, dtype=np.uint8)
    out_off = np.arange(n, dtype=np.uint64) * np.uint64(STRIDE)
    for mask in range(8):
        res = []
        for tracked in (True, False):
            out = np.full(n * STRIDE, 0x5A, np.uint8)
            out_len = np.full(n, 0xA5A5, np.uint16)
            status, ridx = np.full(n, 9, np.uint8), np.full(n, 9, np.uint8)
            acc_len = acc_len0.copy()
            if tracked:
                errs, rlist, counts = R.revive_tracked(acc, STRIDE, acc_len, maps, slot_k, n, out,
                                                       out_off, out_len, status, ridx, slot, mask)
                errs = [{0: 0, R.E_INDEX: CR.ERR_SLOT, R.E_GROUP: CR.ERR_GROUP,
                         R.E_ROWLEN: CR.ERR_ROWLEN}[int(e)] for e in errs]
            else:
                gk, gm = R.gather(maps, slot_k, acc_len, n, slot)
                errs, rlist, counts = CR.revive(acc, STRIDE, acc_len, gk, gm, n, out, out_off,
                                                out_len, status, ridx, slot, mask)
            res.append((out, out_len, status, ridx, acc_len, rlist, counts, np.array(errs)))
        for a, b in zip(*res):
            assert np.array_equal(a, b)
        status, errs = res[0][2], res[0][7]
        assert np.all(status[[20, 21, 22, 23]] == R.UNREVIVABLE) and not errs[20:24].any()
        assert errs[7] == CR.ERR_SLOT and errs[11] == CR.ERR_GROUP and errs[12] == CR.ERR_GROUP
        assert errs[30] == CR.ERR_ROWLEN and status[30] == R.REVIVED
        assert np.count_nonzero(errs) == 4
        assert set(status.tolist()) == {0, 1, 2}


def tiny(idx, ok=None, k=3, old=1, base=0, ln=None, ms=1, stride=64, slot=None, n_slots=1,
         ptr=None):
    """one call of the admit rule on a handful of candidates"""
    m = len(idx)
    ptr = np.array([0, m] if ptr is None else ptr, np.uint32)
    off = np.arange(m + 1, dtype=np.uint64) * np.uint64(16)
    ln = np.array((ln or [16] * m) + [0], np.uint16)
    maps = np.full((n_slots, ms + 1), POISON, np.uint8)
    maps[0, 0] = base
    ptr_out = np.full(len(ptr), 0xA5A5A5A5, np.uint32)
    off_out, len_out = np.full(m + 1, 7, np.uint64), np.full(m + 1, 7, np.uint16)
    verdict = np.full(m + 1, POISON, np.uint8)
    errs, counts = R.admit(off, ln, np.array(list(idx) + [0], np.uint8),
                           None if ok is None else np.array(list(ok) + [0], np.uint8), ptr,
                           np.full(n_slots, k, np.uint8), maps[:, :ms], np.full(n_slots, old, np.uint16),
                           stride, ptr_out, off_out, len_out, verdict, slot)
    assert verdict[m] == POISON and np.all(maps[:, ms] == POISON)
    return verdict[:m].tolist(), maps[0, 0], ptr_out.tolist(), off_out, counts.tolist(), errs


def test_admit_table():
    A_, F, D, I = R.ADMITTED, R.FAILED, R.DUPLICATE, R.INVALID
    v, mp, po, off_out, counts, errs = tiny([0, 2, 0, 3, 2], base=0b0100)
    assert v == [A_, D, D, A_, D] and mp == 0b1101 and po == [0, 2] and not errs.any()
    assert off_out.tolist() == [0, 48, 7, 7, 7, 7] and counts == [2, 0, 3, 0]
    # a fresh slot: the stale map counts as clear and its high bits go
    v, mp, po, _, _, _ = tiny([1, 1], old=0, base=0xFF)
    assert v == [A_, D] and mp == 0b0010 and po == [0, 1]
    # bits above K are ignored and leave with the first write
    v, mp, _, _, _, _ = tiny([3], base=0xF0)
    assert v == [A_] and mp == 0b1000
    # a failed copy sets no bit: the good copy behind it is admitted
    v, mp, _, off_out, counts, _ = tiny([1, 1, 1], ok=[0, 1, 1])
    assert v == [F, A_, D] and mp == 0b0010 and off_out[0] == 16 and counts == [1, 1, 1, 0]
    # nothing admitted: no byte of the map is written
    v, mp, po, _, _, _ = tiny([1, 2], ok=[0, 1], base=0xF4)
    assert v == [F, D] and mp == 0xF4 and po == [0, 0]
    v, mp, po, _, _, _ = tiny([], base=0xF4)
    assert mp == 0xF4 and po == [0, 0]
    # INVALID over FAILED over DUPLICATE; both packet errors latch
    v, mp, _, _, counts, errs = tiny([4, 1, 1, 2], ok=[0, 0, 1, 1], ln=[16, 0, 65, 64], base=0b10)
    assert v == [I, I, I, A_] and errs[0] == R.E_INDEX | R.E_PKTLEN and counts == [1, 0, 0, 3]
    # invalid groups: every packet INVALID, the map untouched
    for kw, e in ((dict(k=0), R.E_GROUP), (dict(k=8), R.E_GROUP), (dict(old=65), R.E_ROWLEN),
                  (dict(slot=np.array([1], np.uint32)), R.E_INDEX),
                  (dict(k=0, old=65), R.E_GROUP | R.E_ROWLEN)):
        v, mp, po, _, counts, errs = tiny([0, 1], base=0xF4, **kw)
        assert v == [I, I] and mp == 0xF4 and po == [0, 0] and errs[0] == e, kw
        assert counts == [0, 0, 0, 2]
    # more than 255 candidates: no verdict is written, nothing is counted
    v, mp, po, off_out, counts, errs = tiny([0, 1] + [0] * 298 + [2, 3], ptr=[0, 2, 300, 302],
                                            n_slots=3, old=0)
    assert errs.tolist() == [0, R.E_GROUP, 0] and counts == [4, 0, 0, 0]
    assert v[:2] == [A_, A_] and v[300:] == [A_, A_] and set(v[2:300]) == {POISON}
    assert po == [0, 2, 2, 4] and off_out[:5].tolist() == [0, 16, 4800, 4816, 7]


def test_library_exports_the_calls():
    sig = dict((s[0], s) for s in qfec.SIGNATURES)
    for name, nargs in (("qfec_admit_ragged", 20), ("qfec_revive_tracked", 19)):
        assert name in sig
        assert sig[name][1] is ctypes.c_int and len(sig[name][2]) == nargs
    assert os.path.exists(qfec.LIB_PATH), "libqfec.so has not been built"
    # (symbol lookup only: nothing is called, no device is opened)
    lib = ctypes.CDLL(qfec.LIB_PATH)
    assert hasattr(lib, "qfec_admit_ragged") and hasattr(lib, "qfec_revive_tracked")
    assert hasattr(qfec.Context, "admit_ragged") and hasattr(qfec.Context, "revive_tracked")
    assert (qfec.QFEC_PKT_ADMITTED, qfec.QFEC_PKT_FAILED, qfec.QFEC_PKT_DUPLICATE,
            qfec.QFEC_PKT_INVALID) == (R.ADMITTED, R.FAILED, R.DUPLICATE, R.INVALID)
