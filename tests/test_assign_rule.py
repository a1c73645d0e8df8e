"""The rule of qfec_assign_slots (tests/assign_rule.py) on the CPU: against an
independent restatement ("the r-th new key by first arrival gets free[r]"), and
chained with the other rules over three turns of arrivals, against the same
turns with the slots the host assigned: per KEY the same statuses, revived
indices and revived bytes.  These pin the yardstick the GPU tests compare
with; the export test at the end needs the header and the binding to have the
call.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import admit_rule as R
import assign_rule as AS
import assign_turns as T
from conftest import ROOT
from libquic_amd import qfec


def random_case(rng, n, n_slots, n_keys, p_open=0.5, p_none=0.1):
    """n packets over n_keys keys; some slots open under some of the keys (a
    few under the same key, a few under NO_KEY), the rest free with stale
    keys that arrive too"""
    pool = rng.integers(0, 1 << 64, n_keys, dtype=np.uint64)
    pool[pool == AS.NO_KEY] = 5
    acc_len = np.where(rng.random(n_slots) < p_open, rng.integers(1, 1400, n_slots), 0) \
        .astype(np.uint16)
    slot_key = pool[rng.integers(0, n_keys, n_slots)] if n_keys else np.zeros(n_slots, np.uint64)
    slot_key = slot_key.astype(np.uint64)
    slot_key[rng.random(n_slots) < 0.05] = AS.NO_KEY
    slot_k = rng.integers(0, 256, n_slots).astype(np.uint8)
    key = pool[rng.integers(0, n_keys, n)].astype(np.uint64)
    key[rng.random(n) < p_none] = AS.NO_KEY
    k = rng.integers(0, 256, n).astype(np.uint8)
    return key, k, slot_key, slot_k, acc_len


def restated(key, k, slot_key, slot_k, acc_len):
    """the rule by whole-array steps: returns (slot_out, slot_key, slot_k, counts)"""
    n_slots = len(acc_len)
    slot_key, slot_k = slot_key.copy(), slot_k.copy()
    is_open = acc_len > 0
    free = np.flatnonzero(~is_open)
    keyed = key != AS.NO_KEY
    out = np.full(len(key), AS.NO_SLOT, np.uint32)
    # the open groups: for every key the lowest open slot
    open_slots = np.flatnonzero(is_open & (slot_key != AS.NO_KEY))
    okeys, first_at = np.unique(slot_key[open_slots], return_index=True)  # (first = lowest)
    oslot = open_slots[first_at]
    at = np.searchsorted(okeys, key)
    at_c = np.minimum(at, max(len(okeys) - 1, 0))
    hit = keyed & (len(okeys) > 0) & (okeys[at_c] == key if len(okeys) else False)
    out[hit] = oslot[at_c[hit]]
    # the new keys, ranked by first arrival
    new = np.flatnonzero(keyed & ~hit)
    nkeys, nfirst = np.unique(key[new], return_index=True)
    firsts = new[nfirst]  # the first arrival of every new key
    order = np.argsort(firsts)
    rank = np.empty(len(nkeys), np.int64)
    rank[order] = np.arange(len(nkeys))
    got = rank < len(free)
    slot_of = np.where(got, free[np.minimum(rank, max(len(free) - 1, 0))] if len(free) else 0,
                       AS.NO_SLOT)
    slot_key[slot_of[got]] = nkeys[got]
    slot_k[slot_of[got]] = k[firsts[got]]
    which = np.searchsorted(nkeys, key[new])
    out[new] = slot_of[which]
    placed = out[new] != AS.NO_SLOT
    counts = [int(hit.sum()), int(placed.sum()), int((~keyed).sum()), int(got.sum()),
              int((~placed).sum())]
    assert n_slots == len(slot_key)
    return out, slot_key, slot_k, np.array(counts, np.uint64)


@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("n,n_slots,n_keys,p_open", [
    (0, 5, 3, 0.5), (1, 1, 1, 0.0), (1, 1, 1, 1.0), (50, 7, 20, 0.5), (2000, 300, 400, 0.3),
    (500, 1000, 100, 0.9), (300, 0, 40, 0.0), (300, 40, 200, 0.0), (300, 40, 30, 1.0)])
def test_rule_is_first_arrival_rank_into_free(seed, n, n_slots, n_keys, p_open):
    rng = np.random.default_rng(100 * seed + n + n_slots)
    key, k, slot_key, slot_k, acc_len = random_case(rng, n, n_slots, n_keys, p_open)
    w_out, w_key, w_k, w_cnt = restated(key, k, slot_key, slot_k, acc_len)
    g_key, g_k, g_len = slot_key.copy(), slot_k.copy(), acc_len.copy()
    g_out = np.full(n + 1, 7, np.uint32)
    g_cnt = AS.assign_slots(key, k, g_key, g_k, g_len, g_out)
    assert g_cnt.tolist() == w_cnt.tolist()
    assert int(g_cnt[[AS.OPEN, AS.NEW, AS.NONE, AS.AWAY]].sum()) == n
    assert np.array_equal(g_out[:n], w_out) and g_out[n] == 7
    assert np.array_equal(g_key, w_key) and np.array_equal(g_k, w_k)
    assert np.array_equal(g_len, acc_len)
    # written only where a group was opened, and those slots were free
    touched = np.flatnonzero((g_key != slot_key) | (g_k != slot_k))
    assert not acc_len[touched].any() and touched.size <= g_cnt[AS.OPENED]


def test_rule_table():
    """the cases of the header's rule, one each"""
    NK, NS = AS.NO_KEY, AS.NO_SLOT
    slot_key = np.array([7, 9, 7, NK, 9, 11], np.uint64)
    acc_len = np.array([0, 5, 5, 5, 5, 0], np.uint16)  # free: 0 and 5
    slot_k = np.array([1, 2, 3, 4, 5, 6], np.uint8)
    key = np.array([9, NK, 7, 13, 7, 11, 13, 9], np.uint64)
    k = np.array([20, 21, 22, 23, 24, 25, 26, 27], np.uint8)
    out = np.zeros(8, np.uint32)
    cnt = AS.assign_slots(key, k, slot_key, slot_k, acc_len, out)
    # 9: the lower of slots 1 and 4; 7: open in slot 2 (slot 0 is free, its key
    # stale); 13: new, takes free[0] = 0; 11: slot 5's key is stale, new, takes
    # free[1] = 5; the second 13 follows the first
    assert out.tolist() == [1, NS, 2, 0, 2, 5, 0, 1]
    assert slot_key.tolist() == [13, 9, 7, NK, 9, 11] and slot_k.tolist() == [23, 2, 3, 4, 5, 25]
    assert cnt.tolist() == [4, 3, 1, 2, 0]
    # nothing free: every new key is turned away, every time
    acc_len[:] = 5
    slot_key[:] = [1, 2, 3, 4, 5, 6]
    before = slot_key.copy(), slot_k.copy()
    cnt = AS.assign_slots(np.array([8, 1, 8], np.uint64), k, slot_key, slot_k, acc_len, out)
    assert out[:3].tolist() == [NS, 0, NS] and cnt.tolist() == [1, 0, 0, 0, 2]
    assert np.array_equal(slot_key, before[0]) and np.array_equal(slot_k, before[1])


@pytest.fixture(scope="module")
def host_turns():
    return T.host_turns(3200)


def test_turns_from_keys_are_the_turns_with_host_slots(host_turns):
    """per KEY the same statuses, revived indices and revived bytes"""
    state = T.KeyState(3201)
    reopened = revived = 0
    released = set()
    for t, d in enumerate(host_turns):
        r = T.key_turn(state, d)
        m = d["m"]
        assert r["a_cnt"][AS.AWAY] == 0 and r["a_cnt"][AS.NONE] == 0
        assert int(r["a_cnt"][AS.OPEN] + r["a_cnt"][AS.NEW]) == m == int(r["b_cnt"][0])
        holder = {}
        for s in np.flatnonzero(r["len_pre"]):
            assert int(r["slot_key"][s]) not in holder  # one open slot per key
            holder[int(r["slot_key"][s])] = int(s)
        for j, gid in enumerate(d["gid"]):
            key = int(T.key_of(int(gid)))
            if d["len_pre"][j] == 0:  # nothing folded: no group, and the host's slot is fresh
                assert key not in holder and d["st"][j] == R.UNREVIVABLE, (t, j)
                continue
            s = holder.pop(key)
            assert r["len_pre"][s] == d["len_pre"][j] and r["slot_k"][s] == d["k"][j], (t, j)
            assert (r["st"][s], r["ridx"][s], r["olen"][s]) == \
                (d["st"][j], d["ridx"][j], d["olen"][j]), (t, j)
            n = int(d["olen"][j])
            assert np.array_equal(r["out"][s * T.STRIDE:s * T.STRIDE + n],
                                  d["out"][j * T.STRIDE:j * T.STRIDE + n]), (t, j)
            revived += d["st"][j] == R.REVIVED
            reopened += key in released  # a late duplicate of a released group: open again
            if d["st"][j] != R.UNREVIVABLE:
                released.add(key)
        if t < 2:
            assert not holder  # every open slot belongs to a group of the turn
        else:  # (groups that left the third turn's batch may still hold a row)
            assert all(r["st"][s] == R.UNREVIVABLE for s in holder.values())
    assert revived >= 60 and reopened >= 1
    # the third turn's new groups sit in slots the first two turns released
    last, r_slots = host_turns[2], r["a_slot"][:host_turns[2]["m"]]
    new_keys = {int(T.key_of(int(g))) for g in last["gid"][-10:]}
    took = {int(s) for s, k in zip(r_slots, last["a_key"]) if int(k) in new_keys}
    assert len(took) == 10


def test_header_and_binding_declare_the_call():
    sig = dict((s[0], s) for s in qfec.SIGNATURES)
    assert "qfec_assign_slots" in sig and "qfec_debug_assign_probe" in sig
    assert sig["qfec_assign_slots"][1] is ctypes.c_int and len(sig["qfec_assign_slots"][2]) == 11
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qfec.h")).read(), flags=re.S)
    decl = re.search(r"\bint\s+qfec_assign_slots\s*\(([^)]*)\)\s*;", src)
    assert decl and len(decl.group(1).split(",")) == 11
    assert "#define QFEC_NO_KEY 0xFFFFFFFFFFFFFFFFull" in src
    assert os.path.exists(qfec.LIB_PATH), "libqfec.so has not been built"
    # (symbol lookup only: nothing is called, no device is opened)
    lib = ctypes.CDLL(qfec.LIB_PATH)
    assert hasattr(lib, "qfec_assign_slots") and hasattr(qfec.Context, "assign_slots")
    assert qfec.QFEC_NO_KEY == AS.NO_KEY and qfec.QFEC_NO_SLOT == AS.NO_SLOT
