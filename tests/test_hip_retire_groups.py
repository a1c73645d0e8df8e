"""qfec_retire_groups on the GPU: the watermarks raised, the max_groups highest
groups of every connection kept, the open slots below their mark closed and
the packets below it masked, bit for bit against the rule of
tests/retire_rule.py (pinned by test_retire_rule.py): acc_len, conn_mark,
pkt_key_out, closed_list and counts, whole buffers.

Discipline, as in test_hip_assign_slots.py: every array, input and output,
carries one trailing entry nobody owns, POISON where the call could write, so a
write past the end shows as a difference, not a fault.  Inputs the call must
not write are compared unchanged: slot_key, pkt_key out of place, the raise
tables.
"""
import numpy as np
import pytest
import torch

import retire_rule as RR
from libquic_amd import qfec
from test_hip_accumulate_ragged import dview
from test_retire_rule import EDGES, K, make_keys, random_case
from turn_sizes import GRID_PER_CU, grid_wrap, ncu

gpu = pytest.mark.gpu
DEV = "cuda:0"
POISON16 = np.uint16(0xA5A5)
POISON32 = np.uint32(0xA5A5A5A5)
POISON64 = np.uint64(0xA5A5A5A5A5A5A5A5)
# the implementation's own boundaries: packets and slots per tile, tiles per
# pass of the one-workgroup scan
TILE, SCAN_BLOCK = 256, 1024
BIG = SCAN_BLOCK * TILE + 1
NK = RR.NO_KEY


def host(t, dtype):
    return t.cpu().numpy().view(dtype)


def same(name, got, want):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{name}: {bad.size} differ, first at {bad[0]}: {got[bad[0]]} " \
                          f"want {want[bad[0]]}"


def tail(a, dtype, poison):
    return np.append(np.asarray(a, dtype), poison)


class Case:
    """One call's inputs (a dict as test_retire_rule.random_case makes them),
    each with its trailing entry, and the rule's outputs over them (computed
    once, shared by every run of the case)."""

    def __init__(self, c):
        self.n, self.n_slots, self.n_conns = len(c["pkt_key"]), len(c["acc_len"]), len(c["conn_mark"])
        self.n_raise = len(c["raise_conn"])
        self.shift, self.max_groups = c["key_shift"], c["max_groups"]
        self.pkt_key = tail(c["pkt_key"], np.uint64, POISON64)
        self.slot_key = tail(c["slot_key"], np.uint64, POISON64)
        self.acc_len = tail(c["acc_len"], np.uint16, POISON16)
        self.conn_mark = tail(c["conn_mark"], np.uint64, POISON64)
        self.raise_conn = tail(c["raise_conn"], np.uint32, POISON32)
        self.raise_mark = tail(c["raise_mark"], np.uint64, POISON64)
        self.w_len, self.w_mark = self.acc_len.copy(), self.conn_mark.copy()
        self.w_out = np.full(self.n + 1, POISON64, np.uint64)
        self.w_closed = np.full(self.n_slots + 1, POISON32, np.uint32)
        cnt = RR.retire_groups(self.pkt_key[:self.n], self.slot_key[:self.n_slots],
                               self.w_len[:self.n_slots], self.w_mark[:self.n_conns], self.shift,
                               self.max_groups, self.raise_conn[:self.n_raise],
                               self.raise_mark[:self.n_raise], self.w_out, self.w_closed)
        self.w_cnt = np.append(cnt, POISON64)
        self.latches = bool(cnt[RR.BAD])


def launch(ctx, c, in_place=False, use_list=True, use_counts=True, null_raise=False):
    d = dict(pkt_key=dview(c.pkt_key), slot_key=dview(c.slot_key), acc_len=dview(c.acc_len),
             conn_mark=dview(c.conn_mark), raise_conn=dview(c.raise_conn),
             raise_mark=dview(c.raise_mark), closed=dview(np.full(c.n_slots + 1, POISON32)),
             cnt=dview(np.full(6, POISON64)))
    d["out"] = d["pkt_key"] if in_place else dview(np.full(c.n + 1, POISON64))
    assert not (null_raise and c.n_raise)
    ctx.retire_groups(d["pkt_key"], c.n, d["slot_key"], d["acc_len"], c.n_slots, d["conn_mark"],
                      c.n_conns, c.shift, c.max_groups, d["out"],
                      raise_conn=None if null_raise else d["raise_conn"],
                      raise_mark=None if null_raise else d["raise_mark"], n_raise=c.n_raise,
                      closed_list=d["closed"] if use_list else None,
                      counts=d["cnt"] if use_counts else None)
    return d


def compare(c, d, in_place=False, use_list=True, use_counts=True):
    same("acc_len", host(d["acc_len"], np.uint16), c.w_len)
    same("conn_mark", host(d["conn_mark"], np.uint64), c.w_mark)
    w_out = c.w_out.copy()
    if in_place:
        w_out[c.n] = c.pkt_key[c.n]  # (the trailing entry of the input it shares)
    same("pkt_key_out", host(d["out"], np.uint64), w_out)
    same("closed_list", host(d["closed"], np.uint32),
         c.w_closed if use_list else np.full(c.n_slots + 1, POISON32))
    same("counts", host(d["cnt"], np.uint64), c.w_cnt if use_counts else np.full(6, POISON64))
    same("slot_key", host(d["slot_key"], np.uint64), c.slot_key)
    if not in_place:
        same("pkt_key", host(d["pkt_key"], np.uint64), c.pkt_key)
    same("raise_conn", host(d["raise_conn"], np.uint32), c.raise_conn)
    same("raise_mark", host(d["raise_mark"], np.uint64), c.raise_mark)


def sync(ctx, c):
    """the sync after a case: -QUIC_INVALID_FEC_DATA once where a connection
    was out of range, then nothing"""
    if c.latches:
        with pytest.raises(qfec.InvalidFecData):
            ctx.sync()
    assert ctx.sync() == qfec.QFEC_OK


def run(ctx, c, **how):
    d = launch(ctx, c, **how)
    sync(ctx, c)
    how.pop("null_raise", None)
    compare(c, d, **how)


SIZES = [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1]
CONNS, GROUPS, SHIFTS = [1, 2, 300], [0, 1, 2, 16], [1, 40, 63]


@gpu
@pytest.mark.parametrize("n_slots", SIZES)
@pytest.mark.parametrize("n", SIZES)
def test_shapes(ctx, n, n_slots):
    """every pair of sizes, the other parameters taken in turn"""
    i = SIZES.index(n) * len(SIZES) + SIZES.index(n_slots)
    rng = np.random.default_rng(5000 + i)
    c = random_case(rng, n, n_slots, CONNS[i % 3], SHIFTS[(i // 3) % 3], GROUPS[(i // 9) % 4],
                    runs=i % 2 == 0)
    run(ctx, Case(c))


@gpu
@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("max_groups", GROUPS)
@pytest.mark.parametrize("n_conns", CONNS)
def test_parameters(ctx, n_conns, max_groups, shift):
    """every connection count, bound and key layout, over more than one tile
    of packets and of slots; numbers at the top of the key's field"""
    rng = np.random.default_rng(5100 + 100 * n_conns + 10 * max_groups + shift)
    c = Case(random_case(rng, 3 * TILE + 17, 2 * TILE + 9, n_conns, shift, max_groups,
                         runs=max_groups % 2 == 0, high=True))
    if max_groups in (1, 2) and n_conns < 300 and shift > 1:
        assert np.any(c.w_mark != c.conn_mark)  # (something was evicted)
    run(ctx, c)


@gpu
def test_packets_beyond_one_scan_pass(ctx):
    rng = np.random.default_rng(5200)
    run(ctx, Case(random_case(rng, BIG, 300, 300, 40, 2, runs=True)))


@gpu
def test_packets_beyond_one_grid(ctx):
    """one packet more than the filter's grid takes in a trip: the last packet
    is judged by the first workgroup's second trip and counted with its first"""
    n = grid_wrap()
    assert n > ncu() * GRID_PER_CU * TILE, "the packets no longer make the grid loop"
    c = Case(random_case(np.random.default_rng(5250), n, 300, 300, 40, 2, runs=True))
    assert (c.w_cnt[:5] > 0).sum() >= 3, c.w_cnt
    run(ctx, c)


@gpu
def test_slots_beyond_one_scan_pass(ctx):
    """the closed slots lie in all 1,025 tiles, the last one closed too: the
    scan carries its base into the second pass"""
    rng = np.random.default_rng(5300)
    c = random_case(rng, 300, BIG, 300, 40, 2)
    c["slot_key"][BIG - 1], c["acc_len"][BIG - 1] = K(3, 0), 9
    c["raise_conn"], c["raise_mark"] = np.array([3], np.uint32), np.array([1], np.uint64)
    c = Case(c)
    closed = c.w_closed[:int(c.w_cnt[RR.CLOSED])]
    assert closed[-1] == BIG - 1 and (closed >= SCAN_BLOCK * TILE - TILE).sum() > 10
    run(ctx, c)


@gpu
@pytest.mark.parametrize("name,case,want", EDGES, ids=[e[0] for e in EDGES])
def test_edges(ctx, name, case, want):
    run(ctx, Case(case))


def one_connection(n, numbers, max_groups, mark=0, shuffled=False, seed=0):
    rng = np.random.default_rng(seed)
    nums = np.asarray(numbers)[np.arange(n) % len(numbers)]
    nums = rng.permutation(nums) if shuffled else np.sort(nums)
    return dict(pkt_key=np.array([K(1, int(x)) for x in nums], np.uint64),
                slot_key=np.array([K(1, int(numbers[0])), K(0, 3)], np.uint64),
                acc_len=np.array([7, 7], np.uint16), conn_mark=np.array([0, mark], np.uint64),
                key_shift=40, max_groups=max_groups, raise_conn=np.zeros(0, np.uint32),
                raise_mark=np.zeros(0, np.uint64))


@gpu
@pytest.mark.parametrize("shuffled", [False, True], ids=["in runs", "shuffled"])
def test_many_packets_of_one_connection(ctx, shuffled):
    """70,000 packets of one connection: of one group, then of 17 groups with
    max_groups 16 -- every atomic of a round on one word"""
    c = Case(one_connection(70000, [100], 16, shuffled=shuffled))
    assert c.w_cnt[:5].tolist() == [0, 0, 0, 70000, 0] and c.w_mark[1] == 0
    run(ctx, c)
    numbers = list(range(500, 517))
    c = Case(one_connection(70000, numbers, 16, shuffled=shuffled, seed=1))
    per = [70000 // 17 + (1 if i < 70000 % 17 else 0) for i in range(17)]
    assert c.w_mark[1] == 501 and c.w_cnt[:5].tolist() == [1, per[0], 0, 70000 - per[0], 0]
    assert c.w_closed[0] == 0
    run(ctx, c)


@gpu
def test_runs_and_shuffled_arrivals_agree(ctx):
    """the same packets in runs and uniformly shuffled: the same marks, the
    same closed slots"""
    rng = np.random.default_rng(5400)
    c = random_case(rng, 20 * TILE + 3, 5 * TILE + 1, 40, 40, 2, runs=True)
    a = Case(c)
    perm = rng.permutation(len(c["pkt_key"]))
    b = Case(dict(c, pkt_key=c["pkt_key"][perm]))
    assert np.array_equal(a.w_mark, b.w_mark) and np.array_equal(a.w_closed, b.w_closed)
    assert np.array_equal(a.w_out[:a.n][perm], b.w_out[:b.n])
    run(ctx, a)
    run(ctx, b)


@gpu
def test_in_place(ctx):
    run(ctx, Case(random_case(np.random.default_rng(5500), 700, 300, 5, 40, 2)), in_place=True)


@gpu
def test_without_list_and_counts(ctx):
    c = Case(random_case(np.random.default_rng(5600), 700, 300, 5, 40, 2))
    assert c.w_cnt[RR.CLOSED] > 0
    run(ctx, c, use_list=False)
    run(ctx, c, use_counts=False)
    run(ctx, c, use_list=False, use_counts=False)


@gpu
def test_no_raises_and_null_tables(ctx):
    c = random_case(np.random.default_rng(5700), 300, 300, 5, 40, 1)
    c["raise_conn"], c["raise_mark"] = np.zeros(0, np.uint32), np.zeros(0, np.uint64)
    run(ctx, Case(c), null_raise=True)


@gpu
def test_raises_alone(ctx):
    """n_packets == 0: the pure CloseFecGroupsBefore; then no slot either"""
    c = random_case(np.random.default_rng(5800), 0, 600, 5, 40, 0)
    c["raise_conn"] = np.array([1, 4, 1, 1], np.uint32)
    c["raise_mark"] = np.array([9, 20, 15, 2], np.uint64)
    c = Case(c)
    assert c.w_cnt[RR.CLOSED] > 20 and c.w_mark[1] == 15
    run(ctx, c)
    only = random_case(np.random.default_rng(5801), 0, 0, 5, 40, 2)
    only["raise_conn"], only["raise_mark"] = np.array([2], np.uint32), np.array([1 << 50], np.uint64)
    run(ctx, Case(only))


@gpu
def test_nothing_at_all(ctx):
    """n_packets, n_slots and n_raise all 0: five zeroes, NULL buffers, and
    conn_mark untouched"""
    cnt = dview(np.full(6, POISON64))
    mark = dview(np.full(3, POISON64))
    ctx.retire_groups(None, 0, None, None, 0, mark, 2, 40, 2, None, counts=cnt)
    ctx.retire_groups(None, 0, None, None, 0, None, 0, 40, 2, None)
    assert ctx.sync() == qfec.QFEC_OK
    assert host(cnt, np.uint64).tolist() == [0] * 5 + [int(POISON64)]
    assert host(mark, np.uint64).tolist() == [int(POISON64)] * 3


@gpu
def test_connections_out_of_range(ctx):
    """in packets, open slots and raises, at every key layout with room for
    them: latched once, every other output right"""
    for i, shift in enumerate([1, 40, 62]):
        c = Case(random_case(np.random.default_rng(5900 + i), 700, 300, 2, shift, 2, p_bad=0.1))
        assert c.latches and c.w_cnt[RR.PASSED] > 0
        run(ctx, c)
    # no connection at all: every key is out of range, conn_mark may be NULL
    c = random_case(np.random.default_rng(5950), 300, 100, 0, 40, 2)
    c = Case(c)
    assert c.w_cnt[RR.BAD] > 300 and c.w_cnt[RR.CLOSED] == 0
    run(ctx, c)


@gpu
def test_three_launches_identical(ctx):
    """the atomics decide nothing that shows: the same shuffled case thrice"""
    c = Case(random_case(np.random.default_rng(6000), 40 * TILE + 3, 9 * TILE + 1, 7, 40, 2))
    runs = [launch(ctx, c) for _ in range(3)]
    sync(ctx, c)
    for d in runs:
        compare(c, d)
    for name in ("acc_len", "conn_mark", "out", "closed", "cnt"):
        assert torch.equal(runs[0][name], runs[1][name]) and torch.equal(runs[0][name], runs[2][name])


NAMES = ["pkt_key", "n", "slot_key", "acc_len", "n_slots", "conn_mark", "n_conns", "shift",
         "max_groups", "raise_conn", "raise_mark", "n_raise", "out", "closed", "cnt", "flags"]
REFUSALS = [
    ("QFEC_PTR_HOST", dict(flags=qfec.QFEC_PTR_HOST), "device pointers only"),
    ("QFEC_PTR_MAPPED", dict(flags=qfec.QFEC_PTR_MAPPED), "device pointers only"),
    ("QFEC_ASYNC", dict(flags=qfec.QFEC_ASYNC), "QFEC_ASYNC"),
    ("slot_key NULL", dict(slot_key=None), "null buffer"),
    ("acc_len NULL", dict(acc_len=None), "null buffer"),
    ("pkt_key NULL", dict(pkt_key=None), "null buffer"),
    ("pkt_key_out NULL", dict(out=None), "null buffer"),
    ("conn_mark NULL", dict(conn_mark=None), "null buffer"),
    ("raise_conn NULL", dict(raise_conn=None), "null buffer"),
    ("raise_mark NULL", dict(raise_mark=None), "null buffer"),
    ("key_shift 0", dict(shift=0), "key_shift"),
    ("key_shift 64", dict(shift=64), "key_shift"),
    ("max_groups 17", dict(max_groups=17), "max_groups"),
    ("2^32 packets", dict(n=1 << 32), "2^32"),
    ("2^32 slots", dict(n_slots=1 << 32), "2^32"),
    ("2^32 connections", dict(n_conns=1 << 32), "2^32"),
    ("2^32 raises", dict(n_raise=1 << 32), "2^32"),
    ("launch failure injected", dict(inject=True), "launch failure injected"),
]


@gpu
@pytest.mark.parametrize("name,fault,fragment", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refused_on_the_host(ctx, name, fault, fragment):
    """Every refusal leaves the poisoned outputs as they were.  Should a check
    go missing and the call launch: every buffer is sized for the good call,
    whose slots would close and whose packets would be refused."""
    n, n_slots, n_conns = 9, 12, 3
    bufs = dict(pkt_key=dview(np.full(n, K(1, 2), np.uint64)),
                slot_key=dview(np.full(n_slots, K(1, 2), np.uint64)),
                acc_len=dview(np.full(n_slots, POISON16)), conn_mark=dview(np.full(n_conns, POISON64)),
                raise_conn=dview(np.array([1, 2], np.uint32)),
                raise_mark=dview(np.array([5, 5], np.uint64)), out=dview(np.full(n, POISON64)),
                closed=dview(np.full(n_slots, POISON32)), cnt=dview(np.full(6, POISON64)))
    before = {key: t.cpu() for key, t in bufs.items()}
    a = dict(bufs, n=n, n_slots=n_slots, n_conns=n_conns, shift=40, max_groups=2, n_raise=2, flags=0)
    a.update(fault)
    inject = a.pop("inject", False)
    if inject:
        assert ctx.lib.qfec_debug_fail_launches(ctx.ctx, 1) == 0
    try:
        rc = ctx.lib.qfec_retire_groups(ctx.ctx, *[qfec._ptr(a[x]) for x in NAMES])
    finally:
        if inject:
            assert ctx.lib.qfec_debug_fail_launches(ctx.ctx, 0) == 0
    msg = ctx.lib.qfec_last_error(ctx.ctx).decode()
    assert rc == qfec.QFEC_ERR_INTERNAL and fragment in msg and "retire groups" in msg, (rc, msg)
    assert ctx.sync() == qfec.QFEC_OK
    for key, t in bufs.items():
        assert torch.equal(t.cpu(), before[key]), key


@gpu
def test_hint_flags_change_nothing(ctx):
    c = Case(random_case(np.random.default_rng(6100), 300, 300, 5, 40, 2))
    d = dict(pkt_key=dview(c.pkt_key), slot_key=dview(c.slot_key), acc_len=dview(c.acc_len),
             conn_mark=dview(c.conn_mark), raise_conn=dview(c.raise_conn),
             raise_mark=dview(c.raise_mark), closed=dview(np.full(c.n_slots + 1, POISON32)),
             cnt=dview(np.full(6, POISON64)), out=dview(np.full(c.n + 1, POISON64)))
    ctx.retire_groups(d["pkt_key"], c.n, d["slot_key"], d["acc_len"], c.n_slots, d["conn_mark"],
                      c.n_conns, c.shift, c.max_groups, d["out"], raise_conn=d["raise_conn"],
                      raise_mark=d["raise_mark"], n_raise=c.n_raise, closed_list=d["closed"],
                      counts=d["cnt"], flags=qfec.QFEC_CACHED | qfec.QFEC_SMALL_GROUPS)
    sync(ctx, c)
    compare(c, d)
