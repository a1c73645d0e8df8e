"""The rule of qfec_retire_groups (tests/retire_rule.py) on the CPU: against an
independent whole-array restatement (np.unique per connection, the
max_groups-th largest by sorting), and against a packet-by-packet restatement
of the reference's group map (QuicFecReceiver::GetFecGroup and
CloseFecGroupsBefore: the closed set unbounded, evict the lowest, refuse below
the lowest when full) over single turns in which no group finishes.  These pin
the yardstick the GPU tests compare with; the export test at the end needs the
header and the binding to have the call.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import retire_rule as RR
from conftest import ROOT
from libquic_amd import qfec

NK = RR.NO_KEY


def make_keys(rng, n, n_conns, shift, width=24, p_bad=0.0, high=False):
    """n keys conn << shift | number over at most `width` numbers per
    connection (so numbers repeat), the numbers at the top of the field if
    `high`; about p_bad of them with connection n_conns, where the key has room
    for it"""
    field = 1 << shift
    conn_room = 1 << (64 - shift)
    conns = rng.integers(0, max(1, min(n_conns, conn_room)), n).astype(object)
    if p_bad and n_conns < conn_room:
        conns[rng.random(n) < p_bad] = n_conns
    base = max(0, field - width) if high else 0
    nums = base + rng.integers(0, min(width, field), n).astype(object)
    key = np.array([(int(c) << shift) | int(x) for c, x in zip(conns, nums)] + [0], np.uint64)[:n]
    key[key == NK] = np.uint64(NK - 1)
    return key


def random_case(rng, n, n_slots, n_conns, shift, max_groups, runs=False, p_bad=0.0, high=False):
    """dict of one call's inputs: packets and slots over the same small set of
    numbers per connection, about 60% of the slots open, a few slots and
    packets without a key, marks inside the numbers' range, up to five raises"""
    field = 1 << shift
    base = max(0, field - 24) if high else 0
    pkt_key = make_keys(rng, n, n_conns, shift, p_bad=p_bad, high=high)
    if runs:  # runs of one key, as a connection delivers a group
        pkt_key = np.repeat(pkt_key, rng.integers(1, 12, n))[:n]
    pkt_key[rng.random(n) < 0.1] = NK
    slot_key = make_keys(rng, n_slots, n_conns, shift, p_bad=p_bad, high=high)
    slot_key[rng.random(n_slots) < 0.05] = NK
    acc_len = np.where(rng.random(n_slots) < 0.6, rng.integers(1, 1400, n_slots), 0) \
        .astype(np.uint16)
    conn_mark = (base + rng.integers(0, min(12, field), n_conns)).astype(np.uint64)
    conn_mark[rng.random(n_conns) < 0.3] = 0
    n_raise = int(rng.integers(0, 6))
    # (no connection at all: every raise is out of range)
    raise_conn = rng.integers(0, max(1, n_conns + (1 if p_bad else 0)), n_raise).astype(np.uint32)
    raise_mark = (base + rng.integers(0, min(16, field), n_raise)).astype(np.uint64)
    return dict(pkt_key=pkt_key, slot_key=slot_key, acc_len=acc_len, conn_mark=conn_mark,
                key_shift=shift, max_groups=max_groups, raise_conn=raise_conn,
                raise_mark=raise_mark)


def apply_rule(c, in_place=False):
    """retire_rule over a case: (acc_len, conn_mark, pkt_key_out, closed, counts)"""
    acc_len, mark = c["acc_len"].copy(), c["conn_mark"].copy()
    pkt_key = c["pkt_key"].copy()
    out = pkt_key if in_place else np.full(len(pkt_key), 7, np.uint64)
    closed = np.full(len(acc_len), 0xA5A5A5A5, np.uint32)
    cnt = RR.retire_groups(pkt_key, c["slot_key"], acc_len, mark, c["key_shift"], c["max_groups"],
                           c["raise_conn"], c["raise_mark"], out, closed)
    return acc_len, mark, out, closed[:int(cnt[RR.CLOSED])], cnt


def restated(c):
    """the rule by whole-array steps: the same five results"""
    shift, G = np.uint64(c["key_shift"]), c["max_groups"]
    mask = np.uint64((1 << c["key_shift"]) - 1)
    mark = c["conn_mark"].copy()
    n_conns = len(mark)
    r_ok = c["raise_conn"] < n_conns
    np.maximum.at(mark, c["raise_conn"][r_ok], c["raise_mark"][r_ok])

    def parts(key, keyed):
        conn, num = key >> shift, key & mask
        known = keyed & (conn < np.uint64(n_conns))
        return np.where(known, conn, 0).astype(np.int64), num, known

    s_keyed = (c["acc_len"] > 0) & (c["slot_key"] != np.uint64(NK))
    s_conn, s_num, s_known = parts(c["slot_key"], s_keyed)
    p_keyed = c["pkt_key"] != np.uint64(NK)
    p_conn, p_num, p_known = parts(c["pkt_key"], p_keyed)
    if G > 0:
        for conn in range(n_conns):
            nums = np.unique(np.concatenate([s_num[s_known & (s_conn == conn)],
                                             p_num[p_known & (p_conn == conn)]]))
            nums = nums[nums >= mark[conn]]
            if nums.size > G:
                mark[conn] = np.sort(nums)[::-1][G - 1]
    markp = np.append(mark, np.uint64(0))  # (an entry to index where there is no connection)
    closing = s_known & (s_num < markp[s_conn])
    acc_len = np.where(closing, 0, c["acc_len"]).astype(np.uint16)
    refused = p_known & (p_num < markp[p_conn])
    passed = p_known & ~refused
    out = np.where(passed, c["pkt_key"], np.uint64(NK))
    bad = int((~r_ok).sum() + (s_keyed & ~s_known).sum() + (p_keyed & ~p_known).sum())
    counts = [int(closing.sum()), int(refused.sum()), int((~p_keyed).sum()), int(passed.sum()), bad]
    return acc_len, mark, out, np.flatnonzero(closing).astype(np.uint32), \
        np.array(counts, np.uint64)


def check_against_restated(c):
    got, want = apply_rule(c), restated(c)
    for name, g, w in zip(("acc_len", "conn_mark", "pkt_key_out", "closed_list", "counts"), got, want):
        assert np.array_equal(g, w), name
    cnt = got[4]
    assert int(cnt[[RR.REFUSED, RR.NONE, RR.PASSED]].sum()) + \
        int(((c["pkt_key"] != NK) & ((c["pkt_key"] >> np.uint64(c["key_shift"])) >=
                                     np.uint64(len(c["conn_mark"])))).sum()) == len(c["pkt_key"])
    # the mark never falls, and in place gives the same keys
    assert np.all(got[1] >= c["conn_mark"])
    assert np.array_equal(apply_rule(c, in_place=True)[2], got[2])


@pytest.mark.parametrize("seed", range(3))
@pytest.mark.parametrize("n,n_slots,n_conns,shift,max_groups", [
    (0, 40, 3, 40, 2), (60, 0, 3, 40, 2), (1, 1, 1, 1, 1), (300, 200, 1, 40, 0),
    (300, 200, 2, 40, 1), (2000, 500, 300, 40, 2), (800, 300, 7, 1, 1), (800, 300, 2, 63, 16),
    (800, 300, 5, 40, 16), (500, 700, 4, 20, 3), (0, 0, 2, 40, 2), (50, 50, 0, 40, 2)])
def test_rule_is_unique_and_sort_per_connection(seed, n, n_slots, n_conns, shift, max_groups):
    rng = np.random.default_rng(1000 * seed + 7 * n + n_slots + shift)
    check_against_restated(random_case(rng, n, n_slots, n_conns, shift, max_groups,
                                       runs=seed == 1, p_bad=0.05 if seed == 2 else 0.0,
                                       high=seed == 1))


def K(conn, number, shift=40):
    return np.uint64((conn << shift) | number)


def edge_cases():
    """(name, case, expected) with expected a dict of the outputs worth naming"""
    u64, u16, u32 = np.uint64, np.uint16, np.uint32
    none32, none64 = np.zeros(0, u32), np.zeros(0, u64)

    def case(pkt, slots, lens, marks, G, rc=none32, rm=none64, shift=40):
        return dict(pkt_key=np.array(pkt, u64), slot_key=np.array(slots, u64),
                    acc_len=np.array(lens, u16), conn_mark=np.array(marks, u64), key_shift=shift,
                    max_groups=G, raise_conn=np.array(rc, u32), raise_mark=np.array(rm, u64))

    yield "as many live numbers as max_groups: the mark stays", \
        case([K(0, 5), K(0, 9)], [K(0, 7), K(0, 5)], [3, 3], [2], 3), \
        dict(mark=[2], closed=[], out=[K(0, 5), K(0, 9)])
    yield "one more than max_groups: one eviction", \
        case([K(0, 5), K(0, 9), K(0, 11)], [K(0, 7), K(0, 5)], [3, 3], [2], 3), \
        dict(mark=[7], closed=[1], out=[NK, K(0, 9), K(0, 11)])
    yield "one number in a slot and in packets, and in two open slots: it counts once", \
        case([K(0, 5), K(0, 5), K(0, 6)], [K(0, 5), K(0, 5), K(0, 4)], [1, 1, 1], [0], 3), \
        dict(mark=[0], closed=[], out=[K(0, 5), K(0, 5), K(0, 6)])
    yield "two open slots under one key are both closed", \
        case([], [K(0, 5), K(0, 8), K(0, 5)], [1, 1, 1], [0], 0, [0], [6]), \
        dict(mark=[6], closed=[0, 2], out=[])
    yield "a number equal to the mark is kept, mark - 1 is not", \
        case([K(0, 10), K(0, 9)], [K(0, 9), K(0, 10)], [1, 1], [10], 0), \
        dict(mark=[10], closed=[0], out=[K(0, 10), NK])
    yield "free slots with stale keys below and above the mark", \
        case([K(0, 30)], [K(0, 3), K(0, 40), K(0, 41), K(0, 20)], [0, 0, 0, 5], [10], 2), \
        dict(mark=[10], closed=[], out=[K(0, 30)])
    yield "open slots holding QFEC_NO_KEY", \
        case([K(0, 1)], [NK, K(0, 1), NK], [4, 4, 0], [5], 1), \
        dict(mark=[5], closed=[1], out=[NK])
    yield "a connection raised three times, once below its mark", \
        case([K(1, 6), K(1, 8)], [K(1, 7), K(0, 1)], [1, 1], [0, 4], 0, [1, 1, 1], [8, 3, 6]), \
        dict(mark=[0, 8], closed=[0], out=[NK, K(1, 8)])
    yield "a raise and an eviction on one connection", \
        case([K(0, 12), K(0, 14), K(0, 3)], [K(0, 10), K(0, 4)], [1, 1], [0], 2, [0], [5]), \
        dict(mark=[12], closed=[0, 1], out=[K(0, 12), K(0, 14), NK])
    yield "numbers below the mark do not count towards max_groups", \
        case([K(0, 1), K(0, 2), K(0, 3), K(0, 20)], [K(0, 21)], [1], [10], 2), \
        dict(mark=[10], closed=[], out=[NK, NK, NK, K(0, 20)])
    yield "connections out of range in a packet, a slot and a raise", \
        case([K(2, 5), K(1, 5)], [K(7, 1), K(1, 1), K(9, 1)], [1, 1, 0], [0, 3], 0, [2, 1], [9, 4]), \
        dict(mark=[0, 4], closed=[1], out=[NK, K(1, 5)], counts=[1, 0, 0, 1, 3])
    yield "key_shift 1: numbers 0 and 1", \
        case([K(3, 0, 1), K(3, 1, 1), K(2, 0, 1)], [K(3, 0, 1)], [1], [0, 0, 0, 0], 1, shift=1), \
        dict(mark=[0, 0, 0, 1], closed=[0], out=[NK, K(3, 1, 1), K(2, 0, 1)])
    top = (1 << 63) - 1
    yield "key_shift 63: numbers up to 2^63 - 1", \
        case([K(0, top, 63), K(1, top - 1, 63), K(1, 5, 63)], [K(0, top - 1, 63)], [1], [0, 0], 1,
             shift=63), \
        dict(mark=[top, top - 1], closed=[0], out=[K(0, top, 63), K(1, top - 1, 63), NK])


EDGES = list(edge_cases())


@pytest.mark.parametrize("name,case,want", EDGES, ids=[e[0] for e in EDGES])
def test_rule_table(name, case, want):
    acc_len, mark, out, closed, cnt = apply_rule(case)
    assert mark.tolist() == want["mark"]
    assert closed.tolist() == want["closed"]
    assert [int(x) for x in out] == [int(x) for x in want["out"]]
    assert np.flatnonzero(acc_len != case["acc_len"]).tolist() == want["closed"]
    if "counts" in want:
        assert cnt.tolist() == want["counts"]
    check_against_restated(case)


class SequentialMap:
    """QuicFecReceiver's group map of one connection, a packet at a time: a
    group that was closed is never recreated (the closed set is unbounded and
    holds every number below the floor the turn started with); with max_groups
    open, a group older than all kept ones is refused, otherwise the lowest is
    dropped."""

    def __init__(self, open_numbers, floor, max_groups):
        self.map, self.closed, self.floor, self.max = set(open_numbers), set(), floor, max_groups

    def close_before(self, threshold):  # CloseFecGroupsBefore
        self.closed |= {x for x in self.map if x < threshold}
        self.map -= self.closed
        self.floor = max(self.floor, threshold)

    def get(self, x):  # GetFecGroup: is there a group for this packet afterwards?
        if x in self.map:
            return True
        if x in self.closed or x < self.floor:
            return False
        if self.max and len(self.map) >= self.max:
            if x < min(self.map):
                return False
            lowest = min(self.map)
            self.map.remove(lowest)
            self.closed.add(lowest)
        self.map.add(x)
        return True


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("max_groups", [0, 1, 2, 5, 16])
def test_rule_is_the_sequential_map_at_the_turns_end(seed, max_groups):
    """a single turn from a random open state in which no group finishes"""
    rng = np.random.default_rng(77 * seed + max_groups)
    n_conns, shift = 6, 40
    mark0 = rng.integers(0, 10, n_conns).astype(np.uint64)
    # the open state the reference could be in: per connection at most
    # max_groups groups, all at or above the floor, one slot each
    slot_key, maps = [], []
    for c in range(n_conns):
        count = int(rng.integers(0, (max_groups or 8) + 1))
        nums = rng.permutation(np.arange(int(mark0[c]), int(mark0[c]) + 30))[:count]
        maps.append(SequentialMap([int(x) for x in nums], int(mark0[c]), max_groups))
        slot_key += [K(c, int(x)) for x in nums]
    stale = [K(int(rng.integers(0, n_conns)), int(rng.integers(0, 40))) for _ in range(10)]
    order = rng.permutation(len(slot_key) + len(stale))
    acc_len = np.array([5] * len(slot_key) + [0] * len(stale), np.uint16)[order]
    slot_key = np.array(slot_key + stale, np.uint64)[order]
    n = 400
    p_conn, p_num = rng.integers(0, n_conns, n), rng.integers(0, 45, n)
    pkt_key = np.array([K(int(c), int(x)) for c, x in zip(p_conn, p_num)], np.uint64)
    raise_conn = rng.integers(0, n_conns, 3).astype(np.uint32)
    raise_mark = rng.integers(0, 25, 3).astype(np.uint64)
    case = dict(pkt_key=pkt_key, slot_key=slot_key, acc_len=acc_len, conn_mark=mark0,
                key_shift=shift, max_groups=max_groups, raise_conn=raise_conn,
                raise_mark=raise_mark)
    g_len, g_mark, g_out, _, _ = apply_rule(case)
    for c, m in zip(raise_conn, raise_mark):
        maps[int(c)].close_before(int(m))
    for c, x in zip(p_conn, p_num):
        maps[int(c)].get(int(x))
    for c in range(n_conns):
        left = {int(k) & ((1 << shift) - 1) for k, ln in zip(slot_key, g_len)
                if ln > 0 and int(k) >> shift == c}
        passed = {int(k) & ((1 << shift) - 1) for k in g_out if int(k) != NK and int(k) >> shift == c}
        assert left | passed == maps[c].map, c
    for p in range(n):
        assert (int(g_out[p]) == NK) == (int(p_num[p]) not in maps[int(p_conn[p])].map), p
    if max_groups:
        assert any(len(m.closed) for m in maps)


def test_header_and_binding_declare_the_call():
    sig = dict((s[0], s) for s in qfec.SIGNATURES)
    assert "qfec_retire_groups" in sig
    assert sig["qfec_retire_groups"][1] is ctypes.c_int and len(sig["qfec_retire_groups"][2]) == 17
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qfec.h")).read(), flags=re.S)
    decl = re.search(r"\bint\s+qfec_retire_groups\s*\(([^)]*)\)\s*;", src)
    assert decl and len(decl.group(1).split(",")) == 17
    assert "#define QFEC_ABI_VERSION 1" in src
    assert os.path.exists(qfec.LIB_PATH), "libqfec.so has not been built"
    # (symbol lookup only: nothing is called, no device is opened)
    lib = ctypes.CDLL(qfec.LIB_PATH)
    assert hasattr(lib, "qfec_retire_groups") and hasattr(qfec.Context, "retire_groups")
    assert qfec.QFEC_NO_KEY == RR.NO_KEY
