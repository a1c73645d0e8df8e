"""qfec_bin_arrivals on the GPU: a turn's per-packet records in arrival order
binned into the per-slot CSR tables the admit reads, bit for bit against the
rule of tests/bin_rule.py (pinned by test_bin_rule.py).

Discipline, as in test_hip_admit_ragged.py: every in-range index really is in
range, so a wrong kernel gives wrong bytes, not a fault (an out-of-range
pkt_slot is a case of its own, which the kernels skip).  Every table, input and
output, carries one trailing entry nobody owns; the outputs start as POISON, so
entries from grp_ptr_out[n_slots] on must stay that.  Whole buffers are
compared; the entries of a slot named by more than 255 packets, whose order is
unspecified, are compared after sorting both sides by src_out, and an input
holds at most two such slots.
"""
import numpy as np
import pytest

import bin_rule as B
from libquic_amd import qfec
from test_hip_accumulate_ragged import dview
from turn_sizes import GRID_PER_CU, grid_wrap, ncu

gpu = pytest.mark.gpu
POISON = 0xA5
POISON16 = np.uint16(0xA5A5)
POISON32 = np.uint32(0xA5A5A5A5)
POISON64 = np.uint64(0xA5A5A5A5A5A5A5A5)
MSG_SLOT = "missing packet index >= FEC group size"  # the accumulate's slot >= n_slots
# the implementation's own boundaries: packets per count / scatter workgroup
# step and slots per tile / ptr / order workgroup, and tiles per pass of the
# one-workgroup scan
TILE, SCAN_BLOCK = 256, 1024


def host(t, dtype):
    return t.cpu().numpy().view(dtype)


def same(name, got, want):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{name}: {bad.size} differ, first at {bad[0]}: {got[bad[0]]} " \
                          f"want {want[bad[0]]}"


class Arrivals:
    """n records in arrival order, one trailing entry nobody owns.  Offsets
    carry bits above 2^32 and up to 2^63 (never dereferenced); lengths and
    indices are arbitrary (carried, not judged)."""

    def __init__(self, rng, slot):
        n = len(slot)
        self.n = n
        self.slot = np.append(np.asarray(slot, np.uint32), np.uint32(0))
        self.off = rng.integers(0, 1 << 63, n + 1, dtype=np.uint64)
        self.off[::3] |= np.uint64(1 << 62)
        self.ln = rng.integers(0, 1 << 16, n + 1).astype(np.uint16)
        self.idx = rng.integers(0, 256, n + 1).astype(np.uint8)
        self.ok = rng.integers(0, 2, n + 1).astype(np.uint8)


def arrivals_of(rng, per_slot, n_none=0, bad=()):
    """a shuffled arrival order in which slot s is named per_slot[s] times,
    n_none packets have no slot and `bad` lists out-of-range slot values"""
    slot = np.concatenate([np.repeat(np.arange(len(per_slot), dtype=np.uint32),
                                     np.asarray(per_slot, np.int64)),
                           np.full(n_none, B.NO_SLOT, np.uint32), np.asarray(bad, np.uint32)])
    return Arrivals(rng, rng.permutation(slot))


class Expect:
    """the rule's outputs over POISON buffers, computed once per input"""

    def __init__(self, a, n_slots, use_ok=True):
        n = a.n
        self.ptr = np.full(n_slots + 2, POISON32, np.uint32)
        self.off, self.ln = np.full(n + 1, POISON64, np.uint64), np.full(n + 1, POISON16, np.uint16)
        self.idx, self.ok = np.full(n + 1, POISON, np.uint8), np.full(n + 1, POISON, np.uint8)
        self.src = np.full(n + 1, POISON32, np.uint32)
        self.errs, self.cnt = B.bin_arrivals(a.slot[:n], a.off, a.ln, a.idx,
                                             a.ok if use_ok else None, n_slots, self.ptr[:n_slots + 1],
                                             self.off, self.ln, self.idx, self.ok, self.src)
        sizes = np.diff(self.ptr[:n_slots + 1].astype(np.int64))
        self.long = np.flatnonzero(sizes > 255)
        assert self.long.size <= 2  # (a condition on the inputs: nearly everything compared exactly)


def launch(ctx, a, n_slots, use_ok=True, use_src=True, use_counts=True, flags=0):
    n = a.n
    d = [dview(x) for x in (a.slot, a.off, a.ln, a.idx, a.ok)]
    o = dict(ptr=dview(np.full(n_slots + 2, POISON32, np.uint32)),
             off=dview(np.full(n + 1, POISON64, np.uint64)),
             ln=dview(np.full(n + 1, POISON16, np.uint16)),
             idx=dview(np.full(n + 1, POISON, np.uint8)), ok=dview(np.full(n + 1, POISON, np.uint8)),
             src=dview(np.full(n + 1, POISON32, np.uint32)),
             cnt=dview(np.full(4, POISON64, np.uint64)), keep=d)
    ctx.bin_arrivals(d[0], d[1], d[2], d[3], d[4] if use_ok else None, n, n_slots, o["ptr"],
                     o["off"], o["ln"], o["idx"], pkt_ok_out=o["ok"] if use_ok else None,
                     src_out=o["src"] if use_src else None, counts=o["cnt"] if use_counts else None,
                     flags=flags)
    return o


def fetch(o):
    return dict(ptr=host(o["ptr"], np.uint32), off=host(o["off"], np.uint64),
                ln=host(o["ln"], np.uint16), idx=host(o["idx"], np.uint8),
                ok=host(o["ok"], np.uint8), src=host(o["src"], np.uint32),
                cnt=host(o["cnt"], np.uint64))


def compare(got, e, use_ok=True, use_src=True, use_counts=True):
    """whole buffers against the rule; a long slot's run after sorting both by src"""
    same("grp_ptr_out", got["ptr"], e.ptr)
    same("counts", got["cnt"], np.append(e.cnt, POISON64) if use_counts else np.full(4, POISON64))
    tables = [("pkt_off_out", "off"), ("pkt_len_out", "ln"), ("pkt_idx_out", "idx")]
    if use_ok:
        tables.append(("pkt_ok_out", "ok"))
    else:
        same("pkt_ok_out (not written)", got["ok"], np.full(got["ok"].size, POISON, np.uint8))
    if use_src:
        tables.append(("src_out", "src"))
    else:
        same("src_out (not written)", got["src"], np.full(got["src"].size, POISON32, np.uint32))
    g = {key: got[key].copy() for _, key in tables}
    for s in e.long:
        assert use_src, "a long slot's run is compared by its arrival indices"
        q = slice(int(e.ptr[s]), int(e.ptr[s + 1]))
        order = np.argsort(got["src"][q], kind="stable")
        for _, key in tables:  # the five tables consistent per entry: one permutation for all
            g[key][q] = got[key][q][order]
    for name, key in tables:
        same(name, g[key], getattr(e, key))


def run(ctx, a, n_slots, **kw):
    e = Expect(a, n_slots, kw.get("use_ok", True))
    o = launch(ctx, a, n_slots, **kw)
    ctx.sync()
    got = fetch(o)
    compare(got, e, kw.get("use_ok", True), kw.get("use_src", True), kw.get("use_counts", True))
    return got, e


# ---- 1. rule conformance -----------------------------------------------------------------------
_conf = {}


def conformance_input():
    """about 700 slots (no multiple of 256) with 0, 1, 2, 254 and 255 candidates
    and small random counts, a tenth of the arrivals without a slot"""
    if not _conf:
        rng = np.random.default_rng(4100)
        n_slots = 701
        per_slot = [(0, 1, 2, 254, 255, int(rng.integers(3, 21)), int(rng.integers(3, 21)))[s % 7]
                    for s in range(n_slots)]
        a = arrivals_of(rng, per_slot, n_none=sum(per_slot) // 10)
        _conf.update(a=a, n_slots=n_slots, e_ok=Expect(a, n_slots, True),
                     e_nook=Expect(a, n_slots, False))
    return _conf


@gpu
@pytest.mark.parametrize("use_ok,use_src,use_counts", [(True, True, True), (False, True, True),
                                                       (True, False, True), (True, True, False),
                                                       (False, False, False)])
def test_rule_conformance(ctx, use_ok, use_src, use_counts):
    c = conformance_input()
    e = c["e_ok"] if use_ok else c["e_nook"]
    assert e.long.size == 0 and not e.errs.any() and e.cnt[1] > 1000
    o = launch(ctx, c["a"], c["n_slots"], use_ok=use_ok, use_src=use_src, use_counts=use_counts,
               flags=qfec.QFEC_CACHED | qfec.QFEC_SMALL_GROUPS if use_counts else 0)
    ctx.sync()
    compare(fetch(o), e, use_ok, use_src, use_counts)


# ---- 2. the edges of the implementation's tiling ---------------------------------------------
@gpu
@pytest.mark.parametrize("n_slots", [1, TILE - 1, TILE, TILE + 1])
@pytest.mark.parametrize("n", [1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 4 * TILE - 1, 4 * TILE,
                               4 * TILE + 1])
def test_tiling_edges(ctx, n, n_slots):
    rng = np.random.default_rng(5000 + 7 * n + n_slots)
    slot = rng.integers(0, n_slots, n).astype(np.uint32)
    slot[rng.random(n) < 0.05] = B.NO_SLOT
    slot[0] = n_slots - 1  # the last slot is named
    got, e = run(ctx, Arrivals(rng, slot), n_slots)
    assert got["ptr"][n_slots] == e.cnt[0] and e.long.size == (1 if n_slots == 1 and n > 300 else 0)


@gpu
def test_more_tiles_than_one_scan_pass(ctx):
    rng = np.random.default_rng(5100)
    n_slots, n = TILE * SCAN_BLOCK + 1, 3000
    slot = rng.integers(0, n_slots, n).astype(np.uint32)
    slot[:5] = [0, n_slots - 1, TILE * SCAN_BLOCK - 1, TILE * SCAN_BLOCK, n_slots - 1]
    got, e = run(ctx, Arrivals(rng, slot), n_slots)
    assert got["ptr"][n_slots] == n and e.long.size == 0


@gpu
def test_packets_beyond_one_grid(ctx):
    """one packet more than the count and scatter grids take in a trip: the
    last packet is ranked and placed by the first workgroup's second trip, and
    leaves its slot behind the packets the first trip's workgroups brought"""
    n, n_slots = grid_wrap(), 16384
    grid = ncu() * GRID_PER_CU * TILE
    assert n > grid, "the packets no longer make the grid loop"
    rng = np.random.default_rng(5150)
    slot = rng.integers(0, n_slots, n).astype(np.uint32)
    slot[rng.random(n) < 0.05] = B.NO_SLOT
    bad = rng.integers(0, n - 1, 6)
    slot[bad] = [n_slots, n_slots + 1, 1 << 20, 1 << 31, 0xFFFFFFFE, n_slots]
    s = 4099
    slot[n - 1] = s
    a = Arrivals(rng, slot)
    e = Expect(a, n_slots)
    assert e.long.size == 0 and int(e.cnt[2]) == 6
    mine = e.src[int(e.ptr[s]):int(e.ptr[s + 1])]
    assert mine.size > 1 and mine[0] < grid <= mine[-1] == n - 1
    o = launch(ctx, a, n_slots)
    with pytest.raises(qfec.InvalidFecData):
        ctx.sync()
    compare(fetch(o), e)
    assert ctx.sync() == qfec.QFEC_OK


# ---- 3. stability across workgroups ----------------------------------------------------------
@gpu
def test_stable_across_workgroups(ctx):
    """one slot's 200 candidates spread evenly through 4,000 arrivals span many
    count / scatter workgroups: its run comes out in ascending arrival index"""
    rng = np.random.default_rng(5200)
    n, n_slots, s = 4000, 300, 137
    slot = rng.integers(0, n_slots - 1, n).astype(np.uint32)
    slot[slot >= s] += 1  # nobody else names s
    slot[np.arange(0, n, 20)] = s
    got, e = run(ctx, Arrivals(rng, slot), n_slots)
    q = slice(int(got["ptr"][s]), int(got["ptr"][s + 1]))
    assert q.stop - q.start == 200
    assert np.array_equal(got["src"][q], np.arange(0, n, 20))


@gpu
@pytest.mark.parametrize("grouped", [False, True])
def test_bursts(ctx, grouped):
    """Arrivals in bursts of one slot's packets (the count pass takes one
    provisional rank per run of neighbouring lanes): runs of 1..100 that cross
    lane 32, waves and workgroups, broken by packets without a slot, a slot
    coming back in a later burst; or the whole turn already grouped."""
    rng = np.random.default_rng(5250 + grouped)
    n_slots = 300
    if grouped:
        per_slot = rng.integers(0, 40, n_slots)
        slot = np.repeat(np.arange(n_slots, dtype=np.uint32), per_slot)
    else:
        runs = []
        for _ in range(400):
            s = B.NO_SLOT if rng.random() < 0.1 else int(rng.integers(0, n_slots))
            runs.append(np.full(int(rng.integers(1, 4 if s == B.NO_SLOT else 101)), s, np.uint32))
        slot = np.concatenate(runs)
        while np.bincount(slot[slot != B.NO_SLOT]).max() > 255:  # (no long slot here)
            s = int(np.bincount(slot[slot != B.NO_SLOT]).argmax())
            slot = np.delete(slot, np.flatnonzero(slot == s)[-50:])
    got, e = run(ctx, Arrivals(rng, slot), n_slots)
    assert e.long.size == 0 and e.cnt[0] > 3000


# ---- 4. long segments --------------------------------------------------------------------------
@gpu
def test_long_segments(ctx):
    rng = np.random.default_rng(5300)
    n_slots = 300
    per_slot = [int(x) for x in rng.integers(0, 13, n_slots)]
    per_slot[41], per_slot[255] = 256, 3001
    per_slot[40], per_slot[42], per_slot[256] = 255, 254, 7
    a = arrivals_of(rng, per_slot, n_none=50)
    got, e = run(ctx, a, n_slots)
    assert e.long.tolist() == [41, 255]
    for s in e.long:  # exactly its packets, each once
        q = slice(int(got["ptr"][s]), int(got["ptr"][s + 1]))
        assert np.array_equal(np.sort(got["src"][q]), np.flatnonzero(a.slot[:a.n] == s))


# ---- 5. out-of-range slots ---------------------------------------------------------------------
@gpu
def test_out_of_range_slots(ctx):
    rng = np.random.default_rng(5400)
    n_slots = 300
    per_slot = [int(x) for x in rng.integers(0, 13, n_slots)]
    bad = [n_slots, n_slots + 1, 1 << 20, 1 << 31, 0xFFFFFFFE, 0xFFFFFFFE, n_slots]
    a = arrivals_of(rng, per_slot, n_none=40, bad=bad)
    e = Expect(a, n_slots)
    assert int(e.cnt[2]) == len(bad) and np.count_nonzero(e.errs) == len(bad)
    o = launch(ctx, a, n_slots)
    with pytest.raises(qfec.InvalidFecData) as ei:
        ctx.sync()
    assert ei.value.code == -5 and MSG_SLOT in str(ei.value)
    got = fetch(o)
    compare(got, e)  # every other packet's outputs are right
    assert got["cnt"][2] == len(bad)
    # a following clean call syncs OK
    clean = arrivals_of(rng, per_slot, n_none=40)
    run(ctx, clean, n_slots)


# ---- 6. determinism ----------------------------------------------------------------------------
@gpu
def test_deterministic(ctx):
    """the same inputs twice into fresh POISON buffers: identical bytes (no long slot)"""
    rng = np.random.default_rng(5500)
    n_slots = 1000
    per_slot = [int(x) for x in rng.integers(0, 40, n_slots)]
    per_slot[500] = 255
    a = arrivals_of(rng, per_slot, n_none=500)
    first = launch(ctx, a, n_slots)
    second = launch(ctx, a, n_slots)
    ctx.sync()
    g1, g2 = fetch(first), fetch(second)
    for key in g1:
        assert g1[key].tobytes() == g2[key].tobytes(), key
    compare(g1, Expect(a, n_slots))


# ---- 7. no packets -----------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n_slots", [1, TILE + 1])
def test_no_packets(ctx, n_slots):
    """grp_ptr_out all zero (its trailing word untouched), counts zero, nothing else touched"""
    o = dict(ptr=dview(np.full(n_slots + 2, POISON32, np.uint32)),
             off=dview(np.full(1, POISON64, np.uint64)), ln=dview(np.full(1, POISON16, np.uint16)),
             idx=dview(np.full(1, POISON, np.uint8)), ok=dview(np.full(1, POISON, np.uint8)),
             src=dview(np.full(1, POISON32, np.uint32)), cnt=dview(np.full(4, POISON64, np.uint64)))
    # the input tables are not looked at
    ctx.bin_arrivals(None, None, None, None, None, 0, n_slots, o["ptr"], o["off"], o["ln"],
                     o["idx"], pkt_ok_out=o["ok"], src_out=o["src"], counts=o["cnt"])
    ctx.sync()
    got = fetch(o)
    assert got["ptr"].tolist() == [0] * (n_slots + 1) + [int(POISON32)]
    assert got["cnt"].tolist() == [0, 0, 0, int(POISON64)]
    assert got["off"][0] == POISON64 and got["ln"][0] == POISON16 and got["idx"][0] == POISON
    assert got["ok"][0] == POISON and got["src"][0] == POISON32
