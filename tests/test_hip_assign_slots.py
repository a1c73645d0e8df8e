"""qfec_assign_slots on the GPU: every packet's group key resolved to the slot
of its open group or to a free slot it opens, bit for bit against the rule of
tests/assign_rule.py (pinned by test_assign_rule.py): pkt_slot_out, slot_key,
slot_k and counts, whole buffers.

Discipline, as in test_hip_bin_arrivals.py: every array, input and output,
carries one trailing entry nobody owns, POISON where the call could write, so a
write past the end shows as a difference, not a fault.  Every input runs twice:
with the call's hash, and under qfec_debug_assign_probe(1), where every key
starts probing at the table's last entry -- one chain through the wrap to entry
0, the longest probe there is.  The chain is as long as the distinct keys, so
an input holds at most 2,000 of them wherever it has more than 2,000 packets
and slots together.
"""
import numpy as np
import pytest
import torch

import accumulate_rule as AR
import assign_rule as AS
import bin_rule as B
from libquic_amd import qfec
from test_hip_accumulate_ragged import dview
from turn_sizes import GRID_PER_CU, grid_wrap, ncu

gpu = pytest.mark.gpu
DEV = "cuda:0"
POISON = 0xA5
POISON32 = np.uint32(0xA5A5A5A5)
POISON64 = np.uint64(0xA5A5A5A5A5A5A5A5)
# the implementation's own boundaries: packets and slots per tile, tiles per
# pass of the one-workgroup scan
TILE, SCAN_BLOCK = 256, 1024
BIG = SCAN_BLOCK * TILE + 1
MAX_KEYS = 2000
NK = AS.NO_KEY


def host(t, dtype):
    return t.cpu().numpy().view(dtype)


def same(name, got, want):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{name}: {bad.size} differ, first at {bad[0]}: {got[bad[0]]} " \
                          f"want {want[bad[0]]}"


class Case:
    """One call's inputs, each with its trailing entry, and the rule's outputs
    over them (computed once, shared by every run of the case)."""

    def __init__(self, key, k, slot_key, slot_k, acc_len, hash_only=False):
        self.n, self.n_slots = len(key), len(acc_len)
        self.key = np.append(np.asarray(key, np.uint64), POISON64)
        self.k = np.append(np.asarray(k, np.uint8), np.uint8(POISON))
        self.slot_key = np.append(np.asarray(slot_key, np.uint64), POISON64)
        self.slot_k = np.append(np.asarray(slot_k, np.uint8), np.uint8(POISON))
        self.acc_len = np.append(np.asarray(acc_len, np.uint16), np.uint16(0))
        assert len(slot_key) == len(slot_k) == self.n_slots and len(k) == self.n
        distinct = np.unique(np.concatenate([self.key[:self.n], self.slot_key[:self.n_slots]])).size
        # (hash_only: run without the one-chain probe, where the keys may be many)
        assert hash_only or distinct <= MAX_KEYS or self.n + self.n_slots <= MAX_KEYS
        self.w_slot_key, self.w_slot_k = self.slot_key.copy(), self.slot_k.copy()
        self.w_out = np.full(self.n + 1, POISON32, np.uint32)
        cnt = AS.assign_slots(self.key[:self.n], self.k, self.w_slot_key[:self.n_slots],
                              self.w_slot_k[:self.n_slots], self.acc_len[:self.n_slots], self.w_out)
        self.w_cnt = np.append(cnt, POISON64)


def launch(ctx, c, use_counts=True):
    d = dict(key=dview(c.key), k=dview(c.k), slot_key=dview(c.slot_key), slot_k=dview(c.slot_k),
             acc_len=dview(c.acc_len), out=dview(np.full(c.n + 1, POISON32, np.uint32)),
             cnt=dview(np.full(6, POISON64, np.uint64)))
    ctx.assign_slots(d["key"], d["k"], c.n, d["slot_key"], d["slot_k"], d["acc_len"], c.n_slots,
                     d["out"], counts=d["cnt"] if use_counts else None)
    return d


def compare(c, d, use_counts=True):
    same("pkt_slot_out", host(d["out"], np.uint32), c.w_out)
    same("slot_key", host(d["slot_key"], np.uint64), c.w_slot_key)
    same("slot_k", host(d["slot_k"], np.uint8), c.w_slot_k)
    same("counts", host(d["cnt"], np.uint64), c.w_cnt if use_counts else np.full(6, POISON64))
    same("acc_len", host(d["acc_len"], np.uint16), c.acc_len)
    same("pkt_key", host(d["key"], np.uint64), c.key)
    same("pkt_k", host(d["k"], np.uint8), c.k)


def run(ctx, c, modes=(0, 1), use_counts=True):
    """the case under the hash and under the one-chain probe"""
    try:
        for mode in modes:
            assert ctx.lib.qfec_debug_assign_probe(ctx.ctx, mode) == 0
            d = launch(ctx, c, use_counts)
            assert ctx.sync() == qfec.QFEC_OK
            compare(c, d, use_counts)
    finally:
        assert ctx.lib.qfec_debug_assign_probe(ctx.ctx, 0) == 0


def key_pool(rng, n_keys):
    pool = np.unique(rng.integers(0, 1 << 64, n_keys, dtype=np.uint64))
    return pool[pool != NK]


def random_case(rng, n, n_slots, p_open=0.5, p_none=0.1, bursts=False):
    """packets over a pool of keys; about p_open of the slots open under keys
    of the pool (so some keys sit in two open slots), the free ones with stale
    keys of the same pool; a few open slots hold QFEC_NO_KEY"""
    pool = key_pool(rng, min(MAX_KEYS - 1, (n + n_slots) // 3 + 2))
    acc_len = np.where(rng.random(n_slots) < p_open, rng.integers(1, 1400, n_slots), 0)
    slot_key = pool[rng.integers(0, pool.size, n_slots)]
    slot_key[rng.random(n_slots) < 0.05] = NK
    key = pool[rng.integers(0, pool.size, n)]
    if bursts:  # runs of one key, as a connection delivers a group
        key = np.repeat(key, rng.integers(1, 12, n))[:n]
    key[rng.random(n) < p_none] = NK
    return Case(key, rng.integers(0, 256, n), slot_key, rng.integers(0, 256, n_slots), acc_len)


@gpu
@pytest.mark.parametrize("n_slots", [1, 2, TILE - 1, TILE, TILE + 1, BIG])
@pytest.mark.parametrize("n", [1, 63, 64, 65, TILE - 1, TILE, TILE + 1, BIG])
def test_shapes(ctx, n, n_slots):
    rng = np.random.default_rng(7 * n + n_slots)
    run(ctx, random_case(rng, n, n_slots, bursts=n % 2 == 0))


@gpu
def test_openers_and_free_slots_beyond_one_scan_pass(ctx):
    """The random big shapes open nothing: with 2,000 keys over 262,145 slots
    every key is open already.  Here 1,500 new keys arrive first at positions
    spread over all 1,025 packet tiles, the last at the very last packet, and
    the free slots lie scattered up to the very last slot, a third of them in
    tiles past the scan's first pass of 1,024: both scans carry a base across
    passes, and fewer slots are free than keys are new."""
    rng = np.random.default_rng(4600)
    pool = key_pool(rng, MAX_KEYS - 2)
    old, new = pool[:400], pool[400:1900]
    acc_len = np.full(BIG, 3)
    free = np.unique(np.concatenate([rng.integers(0, BIG, 900),
                                     rng.integers(SCAN_BLOCK * TILE - 3000, BIG, 450),
                                     [BIG - 1, SCAN_BLOCK * TILE - 1, 0]]))
    acc_len[free] = 0
    slot_key = old[rng.integers(0, old.size, BIG)]
    slot_key[free] = new[rng.integers(0, new.size, free.size)]  # stale, and arriving
    key = old[rng.integers(0, old.size, BIG)]
    first = np.unique(np.concatenate([rng.integers(0, BIG, new.size - 3), [0, BIG - 2, BIG - 1]]))
    key[first] = new[:first.size]
    again = rng.integers(0, BIG, 5000)  # later copies of new keys, after their first arrival
    src = first[rng.integers(0, first.size, again.size)]
    later = (again > src) & ~np.isin(again, first)
    key[again[later]] = key[src[later]]
    c = Case(key, rng.integers(0, 256, BIG), slot_key, rng.integers(0, 256, BIG), acc_len)
    assert free.size < first.size and c.w_cnt[AS.OPENED] == free.size
    assert c.w_cnt[AS.AWAY] > 0 and c.w_slot_key[BIG - 1] != c.slot_key[BIG - 1]
    opened_at = np.flatnonzero(c.w_slot_key[:BIG] != c.slot_key[:BIG])
    assert (opened_at >= SCAN_BLOCK * TILE - 3000).sum() > 300
    run(ctx, c)


@gpu
def test_a_turn_of_new_groups_under_header_style_keys(ctx):
    """8,192 new groups of 5 to 15 packets in a random arrival order, keyed
    connection << 40 | number as the header suggests, every slot free: the
    shape at which tools/assign_rate.py first showed packets of key 0x1 in
    their lane neighbour's slot.  Many keys, so under the hash only."""
    rng = np.random.default_rng(4700)
    n_groups = 8192
    g = np.arange(n_groups, dtype=np.uint64)
    gkey = ((g % np.uint64(4096)) << np.uint64(40)) | (g // np.uint64(4096) + np.uint64(1))
    sizes = rng.integers(5, 16, n_groups)
    of = rng.permutation(np.repeat(np.arange(n_groups), sizes))
    c = Case(gkey[of], sizes[of], np.roll(gkey, 777), np.ones(n_groups), np.zeros(n_groups),
             hash_only=True)
    assert c.w_cnt[:5].tolist() == [0, of.size, 0, n_groups, 0]
    run(ctx, c, modes=(0,))


@gpu
def test_packets_beyond_one_grid(ctx):
    """one packet more than the probe and emit grids take in a trip, in a
    shuffled turn of 150,000 open groups and 100,000 new ones over 300,000
    slots, half of them free: the last packet is the only one of its group,
    which the first workgroup's second trip finds new and opens.  Many keys, so
    under the hash only."""
    n, n_slots = grid_wrap(), 300000
    grid = ncu() * GRID_PER_CU * TILE
    assert n > grid, "the packets no longer make the grid loop"
    rng = np.random.default_rng(4650)
    g = rng.permutation(250001).astype(np.uint64)
    gkey = ((g % np.uint64(4096)) << np.uint64(40)) | (g // np.uint64(4096) + np.uint64(1))
    open_keys, new_keys, lone = gkey[:150000], gkey[150000:250000], gkey[250000]
    acc_len = np.zeros(n_slots, np.int64)
    taken = rng.permutation(n_slots)[:150000]
    acc_len[taken] = rng.integers(1, 1400, 150000)
    slot_key = new_keys[rng.integers(0, new_keys.size, n_slots)]  # (the free slots': stale)
    slot_key[taken] = open_keys
    key = np.where(rng.random(n) < 0.5, open_keys[rng.integers(0, open_keys.size, n)],
                   new_keys[rng.integers(0, new_keys.size, n)])
    key[n - 1] = lone
    c = Case(key, rng.integers(0, 256, n), slot_key, rng.integers(0, 256, n_slots), acc_len,
             hash_only=True)
    assert c.w_cnt[AS.OPENED] > 90000 and c.w_cnt[AS.AWAY] == 0 and c.w_cnt[AS.OPEN] > grid // 3
    at = int(c.w_out[n - 1])
    assert at < n_slots and acc_len[at] == 0 and c.w_slot_key[at] == lone != c.slot_key[at]
    assert c.w_slot_k[at] == c.k[n - 1]
    run(ctx, c, modes=(0,))


def named_cases():
    rng = np.random.default_rng(4100)
    n, ns = 3 * TILE + 17, 2 * TILE + 9
    pool = key_pool(rng, 1500)
    some = pool[rng.integers(0, 400, n)]
    k = rng.integers(0, 256, n)
    sk = rng.integers(0, 256, ns)
    distinct_slot_keys = pool[400:400 + ns]
    yield "every slot open, its packets' keys among them", Case(
        distinct_slot_keys[rng.integers(0, ns, n)], k, distinct_slot_keys, sk, np.full(ns, 9))
    yield "every slot free", Case(some, k, pool[rng.integers(0, 400, ns)], sk, np.zeros(ns))
    yield "no slot free, most keys new", Case(some, k, pool[200:200 + ns], sk, np.full(ns, 1))
    # 100 new keys in tile 0, then only repeats until tile 1 brings new ones;
    # 100 free slots: the last opener accepted arrives at p = 99, the first
    # refused at p = 300
    cut_key = np.concatenate([pool[:100], pool[rng.integers(0, 100, 200)], pool[100:100 + n - 300]])
    cut_len = np.full(ns, 7)
    cut_len[rng.permutation(ns)[:100]] = 0
    yield "fewer free slots than new keys, the cut between two tiles", Case(
        cut_key, k, pool[900:900 + ns], sk, cut_len)
    yield "one key for every packet, new", Case(np.full(n, pool[3]), k, pool[10:10 + ns], sk,
                                                rng.integers(0, 2, ns) * 40)
    yield "one key for every packet, open", Case(np.full(n, pool[11]), k, pool[10:10 + ns], sk,
                                                 np.full(ns, 40))
    yield "every key distinct", Case(pool[:n], k, pool[300:300 + ns], sk,
                                     rng.integers(0, 2, ns) * 40)
    half = some.copy()
    half[rng.random(n) < 0.5] = NK
    yield "half the packets without a key", Case(half, k, pool[:ns], sk, rng.integers(0, 2, ns))
    yield "no packet with a key", Case(np.full(n, NK), k, pool[:ns], sk, rng.integers(0, 2, ns))
    # free slots whose stale keys are exactly the arriving keys: each opens anew
    # in the LOWEST free slot, not where its stale copy lies
    stale_len = np.zeros(ns)
    stale_len[:5] = 3
    yield "free slots with the arriving keys, stale", Case(
        pool[ns - 1 - rng.integers(0, 50, n)], k, pool[:ns], sk, stale_len)
    twice = pool[:ns].copy()
    twice[ns // 2:] = twice[:ns - ns // 2]
    yield "two open slots under one key", Case(pool[rng.integers(0, ns // 2, n)], k, twice, sk,
                                               np.full(ns, 2))
    nokey = pool[:ns].copy()
    nokey[::3] = NK
    nk_pkts = some.copy()
    nk_pkts[::4] = NK
    yield "open slots holding QFEC_NO_KEY", Case(nk_pkts, k, nokey, sk, rng.integers(0, 3, ns))
    edge = np.array([0, NK - 1], np.uint64)
    edge_slots = pool[:ns].copy()
    edge_slots[[4, 9]] = edge
    edge_len = rng.integers(0, 2, ns)
    edge_len[[4, 9]] = [5, 0]  # key 0 open in slot 4; 2^64 - 2 stale in slot 9: new
    yield "keys 0 and 2^64 - 2", Case(edge[rng.integers(0, 2, n)], k, edge_slots, sk, edge_len)
    low = np.uint64(0x00123456789ABC00)
    top8 = (np.arange(256, dtype=np.uint64) << np.uint64(56)) | low
    low8 = np.arange(256, dtype=np.uint64) | low
    fam = np.concatenate([top8, low8[1:]])  # (low8[0] is top8[0])
    fam_slots = fam[rng.integers(0, fam.size, ns)]
    yield "keys differing in their top 8 bits only, and in their low 8 bits only", Case(
        fam[rng.integers(0, fam.size, n)], k, fam_slots, sk, rng.integers(0, 2, ns))
    # Keys that share their low 32 bits, one of them with nothing above: what
    # connection << 40 | number gives for small numbers.  A run test that reads
    # a neighbour's high half in some lanes only sees zero for the others, and
    # takes key 7 for its neighbour's.  Two low words, so that neighbours differ
    # in either half, in both, or in none.
    conn = np.arange(300, dtype=np.uint64) << np.uint64(40)
    shared = np.concatenate([conn | np.uint64(7), conn | np.uint64(9)])
    sh_key = shared[rng.integers(0, shared.size, n)]
    sh_key[rng.random(n) < 0.3] = 7  # (the key whose high half is zero, often)
    yield "keys sharing their low 32 bits, one with a zero high half", Case(
        sh_key, k, shared[rng.integers(0, shared.size, ns)], sk, rng.integers(0, 2, ns) * 3)
    yield "pkt_k of 0 and 255 carried through", Case(
        pool[:n], np.where(np.arange(n) % 2, 255, 0), pool[600:600 + ns], sk, np.zeros(ns))


NAMED = list(named_cases())


@gpu
@pytest.mark.parametrize("name,case", NAMED, ids=[x[0] for x in NAMED])
def test_cases(ctx, name, case):
    if name.startswith("fewer free"):
        away = np.flatnonzero(case.w_out[:case.n] == AS.NO_SLOT)
        opened = np.flatnonzero(case.w_slot_key != case.slot_key)
        assert opened.size == 100 and away.min() == 300 and case.w_cnt[AS.AWAY] == away.size
    if name.startswith("pkt_k"):
        assert set(case.w_slot_k[:case.n_slots].tolist()) == {0, 255}
    if name.startswith("two open"):
        assert case.w_out[:case.n].max() < case.n_slots // 2 + 1
    run(ctx, case)


@gpu
def test_without_counts(ctx):
    run(ctx, random_case(np.random.default_rng(4200), 700, 300), use_counts=False)


@gpu
def test_no_slots_at_all(ctx):
    """n_slots == 0 with packets present: every keyed packet is turned away"""
    rng = np.random.default_rng(4300)
    key = key_pool(rng, 50)[rng.integers(0, 40, 300)]
    key[::7] = NK
    c = Case(key, rng.integers(0, 256, 300), [], [], [])
    assert c.w_cnt[:5].tolist() == [0, 0, 43, 0, 257]
    run(ctx, c)


@gpu
def test_five_calls_identical(ctx):
    """the atomics decide nothing that shows: the same call five times"""
    c = random_case(np.random.default_rng(4400), 40 * TILE + 3, 9 * TILE + 1, bursts=True)
    runs = [launch(ctx, c) for _ in range(5)]
    assert ctx.sync() == qfec.QFEC_OK
    for d in runs:
        compare(c, d)


@gpu
def test_two_turns_back_to_back(ctx):
    """assign -> bin -> accumulate, twice, one sync at the end: the second
    assign finds the groups the first one opened through the lengths the
    accumulate left, and opens its new ones in what is still free"""
    rng = np.random.default_rng(4500)
    n_slots, stride, n = 300, 64, 700
    pool = key_pool(rng, 400)
    acc = rng.integers(0, 256, n_slots * stride + 32, dtype=np.uint8)
    acc_len = np.zeros(n_slots + 1, np.uint16)
    acc_len[rng.permutation(n_slots)[:60]] = 10  # (open under keys nobody sends)
    slot_key = np.append(pool[rng.integers(0, 100, n_slots)], POISON64)
    slot_key[:n_slots][acc_len[:n_slots] > 0] = pool[399]
    slot_k = np.full(n_slots + 1, POISON, np.uint8)
    d_acc, d_len, d_key, d_k = dview(acc), dview(acc_len), dview(slot_key), dview(slot_k)
    keep, want = [], []
    for t in range(2):
        key = np.append(pool[rng.integers(60 * t, 60 * t + 150, n)], POISON64)
        key[:n][rng.random(n) < 0.1] = NK
        k = rng.integers(1, 256, n + 1).astype(np.uint8)
        ln = rng.integers(1, stride + 1, n + 1).astype(np.uint16)
        off = (np.arange(n + 1, dtype=np.uint64) * np.uint64(stride))
        idx = np.zeros(n + 1, np.uint8)
        data = rng.integers(0, 256, (n + 1) * stride + 32, dtype=np.uint8)
        w_slot = np.full(n + 1, POISON32, np.uint32)
        w_cnt = AS.assign_slots(key[:n], k, slot_key[:n_slots], slot_k[:n_slots], acc_len[:n_slots],
                                w_slot)
        t_ptr = np.full(n_slots + 1, POISON32, np.uint32)
        t_off, t_ln = np.full(n + 1, POISON64, np.uint64), np.full(n + 1, 0xA5A5, np.uint16)
        t_idx = np.full(n + 1, POISON, np.uint8)
        errs, _ = B.bin_arrivals(w_slot[:n], off, ln, idx, None, n_slots, t_ptr, t_off, t_ln, t_idx)
        assert not errs.any()
        assert not AR.accumulate(data, t_off, t_ln, t_ptr, acc, stride, acc_len[:n_slots], None).any()
        want.append(dict(slot=w_slot, cnt=w_cnt, key=slot_key.copy(), k=slot_k.copy()))
        d = dict(key=dview(key), k=dview(k), ln=dview(ln), off=dview(off), idx=dview(idx),
                 data=dview(data), slot=dview(np.full(n + 1, POISON32, np.uint32)),
                 cnt=dview(np.full(5, POISON64, np.uint64)),
                 t_ptr=dview(np.full(n_slots + 1, POISON32, np.uint32)),
                 t_off=dview(np.full(n + 1, POISON64, np.uint64)),
                 t_ln=dview(np.full(n + 1, 0xA5A5, np.uint16)),
                 t_idx=dview(np.full(n + 1, POISON, np.uint8)))
        ctx.assign_slots(d["key"], d["k"], n, d_key, d_k, d_len, n_slots, d["slot"],
                         counts=d["cnt"])
        ctx.bin_arrivals(d["slot"], d["off"], d["ln"], d["idx"], None, n, n_slots, d["t_ptr"],
                         d["t_off"], d["t_ln"], d["t_idx"])
        ctx.accumulate_ragged(d["data"], d["t_off"], d["t_ln"], d["t_ptr"], n_slots, d_acc, stride,
                              d_len, slot=None, n_slots=n_slots)
        keep.append(d)
    assert ctx.sync() == qfec.QFEC_OK  # the only one
    for t, (d, w) in enumerate(zip(keep, want)):
        same(f"pkt_slot_out, turn {t}", host(d["slot"], np.uint32), w["slot"])
        same(f"counts, turn {t}", host(d["cnt"], np.uint64), w["cnt"])
    assert want[1]["cnt"][AS.OPEN] > 100 and want[1]["cnt"][AS.OPENED] > 20
    same("slot_key", host(d_key, np.uint64), slot_key)
    same("slot_k", host(d_k, np.uint8), slot_k)
    same("acc_len", host(d_len, np.uint16), acc_len)
    same("acc", host(d_acc, np.uint8), acc)
