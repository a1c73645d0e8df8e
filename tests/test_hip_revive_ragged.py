"""qfec_revive_ragged on the GPU: classify every group of a device-resident
ragged (CSR) batch from its receive map and rebuild the lost packet of the
revivable ones.

The reference for status, revived_idx, revived_list and counts is reference()
below, the rule of include/qfec.h per group with its own k; the revived bytes
come from the C oracle's recover_ragged run on the sub-CSR of the revived
groups with their m (and, as a check of the test's own inputs, must equal the
erased packet, zero padded).  Every output starts as POISON.  What the call
must never read is poisoned with values that are in bounds but would show:
lost payloads hold LOST, parity bytes of groups without their FEC packet NOFEC,
the pkt_len of a revived group's lost packet 0, 2000 or 16 and its pkt_off
another packet's, parity_len and every pkt_len of a complete or unrevivable group 0,
and the out_off of such a group points into a guard region behind the output
slots that must stay POISON.  No offset anywhere is out of range: a wrong
kernel gives wrong bytes, not a fault.  All comparisons are bit-exact.
"""
import numpy as np
import pytest
import torch

from oracle import oracle_c as OC
from libquic_amd import qfec
from turn_sizes import SCAN_BLOCK, SCAN_WRAP, TILE

gpu = pytest.mark.gpu
DEV = "cuda:0"
POISON, LOST, NOFEC, PAD = 0xA5, 0x3C, 0xC3, 0x5A
POISON64 = np.uint64(0xA5A5A5A5A5A5A5A5)
GUARD = 4096      # bytes behind the out slots; out_off of non-revived groups points here
NT, CAPW = 256, 16384  # the block body's limits per list step: received packets, windows
_SIGNED = {np.dtype(np.uint8): np.uint8, np.dtype(np.uint16): np.int16,
           np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}


def dview(a):
    """device copy of an index array (bits preserved; torch lacks wide unsigned types)"""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(_SIGNED[a.dtype]).copy()).to(DEV)


# ---- the rule ---------------------------------------------------------------
def reference(rcv, fec, ptr, map_stride):
    """rcv bool per packet, fec bool per group -> status, revived_idx, list, counts."""
    n = ptr.size - 1
    status = np.full(n, qfec.GROUP_UNREVIVABLE, np.uint8)
    idx = np.full(n, 0xFF, np.uint8)
    valid = np.zeros(n, bool)
    for g in range(n):
        k = int(ptr[g + 1]) - int(ptr[g])
        if not (1 <= k <= 255 and k // 8 + 1 <= map_stride):
            continue  # invalid: unrevivable, and kErrGroupSize is latched
        valid[g] = True
        lost = np.flatnonzero(~rcv[int(ptr[g]):int(ptr[g + 1])])
        if lost.size == 0:
            status[g] = qfec.GROUP_COMPLETE
        elif lost.size == 1 and fec[g]:
            status[g], idx[g] = qfec.GROUP_REVIVED, lost[0]
    lst = np.flatnonzero(status == qfec.GROUP_REVIVED).astype(np.uint64)
    return status, idx, lst, np.bincount(status, minlength=3).astype(np.uint64), valid


def loop_maps(rcv, fec, ptr, valid, stride, rng=None):
    """Bit by bit; rng: random garbage in every bit above k (and in the whole
    map of an invalid group, which is never read)."""
    n = ptr.size - 1
    maps = (rng.integers(0, 256, (n, stride), dtype=np.uint8) if rng is not None
            else np.zeros((n, stride), np.uint8))
    for g in np.flatnonzero(valid):
        bits = list(rcv[int(ptr[g]):int(ptr[g + 1])]) + [fec[g]]
        for i, b in enumerate(bits):
            maps[g, i // 8] = (int(maps[g, i // 8]) & ~(1 << (i % 8)) & 0xFF) | (int(b) << (i % 8))
    return maps


class Batch:
    """specs: per group (packet lengths, set of lost slots, FEC packet received).
    gap: PAD bytes between packets (and `lead` before the first: unaligned
    offsets); ptr_override: a grp_ptr to use instead (invalid-table cases)."""

    def __init__(self, specs, seed, *, map_stride=None, garbage=False, gap=0, lead=0,
                 out_guard=16, out_lead=0, ptr_override=None):
        rng = np.random.default_rng(seed)
        n = self.n = len(specs)
        ks = np.array([len(s[0]) for s in specs], np.int64)
        ptr = np.zeros(n + 1, np.uint32)
        ptr[1:] = np.cumsum(ks)
        ln = np.array([x for s in specs for x in s[0]], np.uint16)
        P = ln.size
        rcv = np.ones(P, bool)
        for g, s in enumerate(specs):
            for i in s[1]:
                rcv[int(ptr[g]) + i] = False
        fec = np.array([s[2] for s in specs], bool)
        if ptr_override is not None:
            ptr = np.asarray(ptr_override, np.uint32)
        self.ptr, self.rcv, self.fec = ptr, rcv, fec
        if map_stride is None:
            map_stride = max(1, int(ks[ks <= 255].max()) // 8 + 1)
        self.map_stride = map_stride
        self.status, self.idx, self.lst, self.counts, self.valid = reference(rcv, fec, ptr,
                                                                             map_stride)
        self.maps = loop_maps(rcv, fec, ptr, self.valid, map_stride, rng if garbage else None)
        if self.valid.all() and not garbage:
            assert np.array_equal(self.maps,
                                  qfec.pack_received_ragged(rcv, fec, ptr, map_stride))
        # payloads
        step = ln.astype(np.uint64) + np.uint64(gap)
        off = np.full(P, lead, np.uint64)
        off[1:] += np.cumsum(step[:-1])
        total = int(off[-1] + ln[-1]) + 16 if P else 16
        data = np.full(total, PAD, np.uint8)
        l64 = ln.astype(np.int64)
        pos = (np.repeat(off, l64) + (np.arange(int(l64.sum()))
                                      - np.repeat(np.cumsum(l64) - l64, l64)).astype(np.uint64))
        data[pos.astype(np.int64)] = rng.integers(0, 256, pos.size, dtype=np.uint8)
        self.off, self.ln, self.complete = off, ln, data
        # parity of the complete groups, one slot each
        plen = np.zeros(n, np.uint16)
        if self.valid.all():
            plen = np.maximum.reduceat(ln, ptr[:-1].astype(np.int64))
        else:
            for g in np.flatnonzero(self.valid):
                plen[g] = ln[int(ptr[g]):int(ptr[g + 1])].max()
        pslot = int(plen.max()) + 8
        poff = np.arange(n, dtype=np.uint64) * np.uint64(pslot) + np.uint64(lead)
        if self.valid.all():
            rc, par, plen2 = OC.encode_ragged(data, off, ln, ptr, poff, n * pslot + 16)
            assert rc == 0 and np.array_equal(plen2, plen)
        else:
            par = np.zeros(n * pslot + 16, np.uint8)
            for g in np.flatnonzero(self.valid):
                for p in range(int(ptr[g]), int(ptr[g + 1])):
                    o = int(poff[g])
                    par[o:o + int(ln[p])] ^= data[int(off[p]):int(off[p]) + int(ln[p])]
        self.plen, self.poff = plen, poff
        # the receiver's view
        rev = self.status == qfec.GROUP_REVIVED
        self.sel = sel = np.flatnonzero(rev)
        self.bytes_in = data.copy()
        lost_p = np.flatnonzero(~rcv)
        for p in lost_p:
            self.bytes_in[int(off[p]):int(off[p]) + int(ln[p])] = LOST
        self.par_in = par.copy()
        for g in np.flatnonzero(~fec & self.valid):
            self.par_in[int(poff[g]):int(poff[g]) + int(plen[g])] = NOFEC
        # out: a slot per group with guard bytes between, then the guard region
        oslot = int(plen.max()) + out_guard
        self.ooff = np.arange(n, dtype=np.uint64) * np.uint64(oslot) + np.uint64(out_lead)
        self.out_size = n * oslot + out_lead + GUARD
        guard0 = n * oslot + out_lead
        # expected bytes: the oracle on the sub-CSR of the revived groups
        self.want_out = np.full(self.out_size, POISON, np.uint8)
        if sel.size:
            pk = np.concatenate([np.arange(int(ptr[g]), int(ptr[g + 1])) for g in sel])
            sptr = np.zeros(sel.size + 1, np.uint32)
            sptr[1:] = np.cumsum(ptr[sel + 1].astype(np.int64) - ptr[sel].astype(np.int64))
            rc, o = OC.recover_ragged(self.bytes_in, off[pk], ln[pk], sptr, self.par_in,
                                      poff[sel], plen[sel], self.idx[sel], self.ooff[sel],
                                      self.out_size)
            assert rc == 0
            for g in sel:
                a, b = int(self.ooff[g]), int(self.ooff[g]) + int(plen[g])
                self.want_out[a:b] = o[a:b]
                # the test's own inputs: exactly the erased packet, zero padded
                p = int(ptr[g]) + int(self.idx[g])
                want = np.zeros(int(plen[g]), np.uint8)
                want[:int(ln[p])] = data[int(off[p]):int(off[p]) + int(ln[p])]
                assert np.array_equal(o[a:b], want)
        # tables the call must not read, poisoned in bounds
        self.ln_in, self.off_in = ln.copy(), off.copy()
        self.plen_in, self.ooff_in = plen.copy(), self.ooff.copy()
        for g in sel:
            p = int(ptr[g]) + int(self.idx[g])
            # (16: a legal length -- only wrong bytes can give a stray read away)
            self.ln_in[p] = (0, 2000, 16)[p % 3]
            self.off_in[p] = off[(p + 1) % P]
        for g in np.flatnonzero(~rev):
            self.plen_in[g] = 0
            self.ooff_in[g] = guard0 + (g * 37) % 2048
            if self.valid[g]:
                self.ln_in[int(ptr[g]):int(ptr[g + 1])] = 0

    def step_totals(self):
        """Per list step of 8 revived groups: received packets, 16-B windows,
        the shortest received packet and the shortest parity."""
        out = []
        for s in range(0, self.sel.size, 8):
            R = W = 0
            mn, mp = 1 << 20, 1 << 20
            for g in self.sel[s:s + 8]:
                for p in range(int(self.ptr[g]), int(self.ptr[g + 1])):
                    if self.rcv[p]:
                        R += 1
                        W += (int(self.ln[p]) + 15) // 16
                        mn = min(mn, int(self.ln[p]))
                mp = min(mp, int(self.plen[g]))
            out.append((R, W, mn, mp))
        return out


class Outs:
    def __init__(self, b):
        n = max(b.n, 1)
        self.n = b.n
        self.status = torch.full((n,), POISON, dtype=torch.uint8, device=DEV)
        self.idx = torch.full((n,), POISON, dtype=torch.uint8, device=DEV)
        self.lst = torch.full((n * 8,), POISON, dtype=torch.uint8, device=DEV)
        self.counts = torch.full((24,), POISON, dtype=torch.uint8, device=DEV)
        self.out = torch.full((b.out_size,), POISON, dtype=torch.uint8, device=DEV)

    def host(self):
        torch.cuda.synchronize()
        return dict(status=self.status.cpu().numpy()[:self.n], idx=self.idx.cpu().numpy()[:self.n],
                    lst=self.lst.cpu().numpy().view(np.uint64)[:self.n],
                    counts=self.counts.cpu().numpy().view(np.uint64), out=self.out.cpu().numpy())


def upload(b, map_lead=0):
    d = dict(bytes=dview(b.bytes_in), off=dview(b.off_in), ln=dview(b.ln_in), ptr=dview(b.ptr),
             par=dview(b.par_in), poff=dview(b.poff), plen=dview(b.plen_in), ooff=dview(b.ooff_in))
    m = torch.full((b.maps.size + map_lead + 1,), PAD, dtype=torch.uint8, device=DEV)
    m[map_lead:map_lead + b.maps.size] = torch.from_numpy(b.maps.ravel()).to(DEV)
    d["maps"] = m[map_lead:]
    return d


def call(ctx, b, d, o, skip=()):
    ctx.revive_ragged(d["bytes"], d["off"], d["ln"], d["ptr"], b.n, d["par"], d["poff"],
                      d["plen"], d["maps"], b.map_stride, o.out, d["ooff"], status=o.status,
                      revived_idx=None if "idx" in skip else o.idx,
                      revived_list=None if "lst" in skip else o.lst,
                      counts=None if "counts" in skip else o.counts)


def check(h, b, skip=(), bad=()):
    """Everything a call wrote against the rule and the oracle; bad: groups whose
    out bytes are unspecified (latched table errors)."""
    assert np.array_equal(h["status"], b.status)
    if "idx" in skip:
        assert np.all(h["idx"] == POISON)
    else:
        assert np.array_equal(h["idx"], b.idx)
    if "counts" in skip:
        assert np.all(h["counts"] == POISON64)
    else:
        assert np.array_equal(h["counts"], b.counts)
        assert int(b.counts.sum()) == b.n
    if "lst" in skip:
        assert np.all(h["lst"] == POISON64)
    else:
        c = b.lst.size
        assert np.array_equal(h["lst"][:c], b.lst)
        assert np.all(np.diff(h["lst"][:c].astype(np.int64)) > 0), "revived_list not ascending"
        assert np.all(h["lst"][c:] == POISON64), "revived_list written past the count"
    got, want = h["out"].copy(), b.want_out.copy()
    for g in bad:
        a, e = int(b.ooff[g]), int(b.ooff[g]) + int(b.plen[g])
        got[a:e] = want[a:e] = 0
    assert np.array_equal(got, want)


def run(ctx, b, map_lead=0, skip=()):
    d = upload(b, map_lead)
    o = Outs(b)
    call(ctx, b, d, o, skip)
    ctx.sync()  # OK: none of the poisoned table entries was read
    check(o.host(), b, skip)
    # inputs are inputs
    assert np.array_equal(d["bytes"].cpu().numpy(), b.bytes_in)
    assert np.array_equal(d["par"].cpu().numpy(), b.par_in)
    return o


def filler(i):
    """Groups between revived ones: complete, unrevivable (no FEC packet), two lost."""
    return [([20, 33], set(), i % 2 == 0), ([17, 40, 16], {1}, False),
            ([64, 16, 30], {0, 2}, True)][i % 3]


def spread(revived):
    """The revived groups with complete / unrevivable ones between them, so the
    entries of a list step come from non-adjacent groups."""
    specs = []
    for i, s in enumerate(revived):
        specs += [filler(i)] * (1 + i % 3) + [s]
    return specs + [filler(1)]


# ---- 1. every map -------------------------------------------------------------
@gpu
def test_every_map_small_k(ctx):
    rng = np.random.default_rng(11)
    specs = []
    for k in (1, 2, 3, 4):
        for bits in range(1 << (k + 1)):
            lens = [int(x) for x in rng.choice([1, 15, 16, 17, 100, 1452], k)]
            specs.append((lens, {i for i in range(k) if not (bits >> i) & 1}, bool(bits >> k & 1)))
    specs = [specs[i] for i in rng.permutation(len(specs))]
    b = Batch(specs, 12)
    assert b.n == 60 and b.counts.tolist() == [8, 1 + 2 + 3 + 4, 60 - 8 - 10]
    run(ctx, b)


# ---- 2. classify width classes --------------------------------------------------
def width_specs(ks, rng):
    specs = []
    for k in ks:
        lens = lambda: [int(x) for x in rng.integers(16, 49, k)]
        drops = range(k) if k in (9, 33, 65, 255) else [int(x) for x in rng.integers(0, k, 3)]
        for m in drops:
            specs.append((lens(), {m}, True))           # revived at every / a random index
        m = int(rng.integers(0, k))
        specs.append((lens(), {m}, False))              # FEC bit clear: unrevivable
        specs.append((lens(), set(), bool(k % 2)))      # complete
        specs.append((lens(), {0, k - 1} if k > 1 else {0}, k > 1))
    return specs


@gpu
@pytest.mark.parametrize("ks,stride", [((7, 8, 9, 31, 32, 33, 63, 64, 65, 254, 255), 32),
                                       ((7, 8, 9, 31, 32, 33, 63, 64, 65), 9)])
def test_classify_width_classes(ctx, ks, stride):
    rng = np.random.default_rng(21 + stride)
    b = Batch(width_specs(ks, rng), 22 + stride, map_stride=stride, garbage=True)
    assert stride == max(ks) // 8 + 1
    for k in (9, 33, 65) + ((255,) if 255 in ks else ()):
        sizes = b.ptr[b.sel + 1] - b.ptr[b.sel]
        assert sorted(b.idx[b.sel[sizes == k]].tolist()) == list(range(k))
    assert sorted(set(b.status)) == [0, 1, 2]
    run(ctx, b)


# ---- 3. list-step boundaries ------------------------------------------------------
def rev(lens, m):
    return (list(lens), {m}, True)


def step_of(nrecv_per_group, length, rng):
    """8 revived groups with the given received-packet counts, every packet `length` B."""
    out = []
    for r in nrecv_per_group:
        out.append(rev([length] * (r + 1), int(rng.integers(0, r + 1))))
    return out


@gpu
def test_list_step_boundaries(ctx):
    rng = np.random.default_rng(31)
    steps = [
        step_of([31] * 8, 48, rng),                       # 248 received packets
        step_of([31] * 7 + [32], 48, rng),                # 249
        step_of([32] * 8, 32, rng),                       # 256: the block body's table is full
        step_of([32] * 7 + [33], 32, rng),                # 257: falls back
        step_of([22] * 8, 1452, rng),                     # 176 x 91 = 16,016 windows
        step_of([23] * 8, 1452, rng),                     # 184 x 91 = 16,744: falls back
        step_of([3] * 8, 64, rng)[:7] + [rev([64, 9, 200, 30], 2)],   # a received packet < 16 B
        step_of([3] * 8, 64, rng)[:7] + [rev([12, 9, 15], 0)],        # a parity_len < 16
        [rev([int(rng.integers(16, 1453))], 0) for _ in range(8)],     # k = 1: out = the parity
        step_of([4, 1, 9], 100, rng),                     # a partial last step
    ]
    b = Batch(spread([s for st in steps for s in st]), 32)
    assert np.all(np.diff(b.sel) > 1), "revived groups are not adjacent"
    tot = b.step_totals()
    assert len(tot) == 10 and b.sel.size == 8 * 9 + 3
    R = [t[0] for t in tot]
    W = [t[1] for t in tot]
    assert {248, 249, 256, 257} <= set(R) and max(R) > NT >= 256
    assert {16016, 16744} <= set(W) and min(w for w in W if w > 16000) <= CAPW < max(W)
    assert sum(t[2] < 16 for t in tot) >= 1 and sum(t[3] < 16 for t in tot) == 1
    assert R[8] == 0 and W[8] == 0
    run(ctx, b)


@gpu
@pytest.mark.parametrize("count", [0, 1, 7, 8, 9])
def test_revived_count(ctx, count):
    rng = np.random.default_rng(40 + count)
    revived = [rev([int(x) for x in rng.integers(16, 300, 5)], int(rng.integers(0, 5)))
               for _ in range(count)]
    b = Batch(spread(revived) + [filler(0), filler(2)], 41 + count)
    assert b.counts[1] == count
    run(ctx, b)


# ---- 4. grid coverage -----------------------------------------------------------
def tiny_specs(n, kinds, rng):
    """k = 2, 16..64 B; kinds: 1 revived, 0 complete, 2 unrevivable."""
    lens = rng.integers(16, 65, (n, 2))
    m = rng.integers(0, 2, n)
    return [([int(lens[g, 0]), int(lens[g, 1])],
             {int(m[g])} if kinds[g] == 1 else (set() if kinds[g] == 0 else {0, 1}),
             True) for g in range(n)]


@gpu
def test_looping_grid(ctx):
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    n = 8 * 8 * ncu + 8 * 8 * 5 + 3  # more revived groups than the grid's blocks take in a step
    rng = np.random.default_rng(51)
    b = Batch(tiny_specs(n, np.ones(n, int), rng), 52)
    assert b.counts[1] == n > 8 * 8 * ncu
    run(ctx, b)


@gpu
@pytest.mark.parametrize("pattern", ["random", "late", "early"])
def test_large_batch(ctx, pattern):
    n = 100_003
    rng = np.random.default_rng(61)
    kinds = np.where(rng.random(n) < 0.5, 0, 2)
    if pattern == "random":
        kinds = np.where(rng.random(n) < 0.3, 1, kinds)
    elif pattern == "late":
        kinds[n - 5000:] = 1
    else:
        kinds[:5000] = 1
    b = Batch(tiny_specs(n, kinds, rng), 62)
    assert b.counts[1] == int((kinds == 1).sum()) >= 5000
    run(ctx, b)


@gpu
def test_groups_beyond_one_scan_trip(ctx):
    """256 * 1024 + 1 groups: the scan over the 1,025 tiles takes a second trip,
    and the last group, a revived one, gets its place in the list and the three
    counts from the base and the side sums carried into it"""
    n = SCAN_WRAP
    assert (n + TILE - 1) // TILE > SCAN_BLOCK, "the groups no longer make the scan take a second trip"
    rng = np.random.default_rng(63)
    # (few lost packets: the batch's per-packet loops on the host are what the test costs)
    kinds = np.where(rng.random(n) < 0.9, 0, 2)
    kinds = np.where(rng.random(n) < 0.04, 1, kinds)
    kinds[n - 1] = 1
    edge = SCAN_BLOCK * TILE
    assert set(kinds[edge - TILE:edge].tolist()) == {0, 1, 2} == set(kinds[:TILE].tolist())
    b = Batch(tiny_specs(n, kinds, rng), 64)
    assert b.counts[1] == int((kinds == 1).sum()) and b.lst[-1] == n - 1
    run(ctx, b)


# ---- 5. layout -------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("gap,lead,map_lead", [(0, 1, 1), (3, 5, 3), (29, 7, 0)])
def test_layout(ctx, gap, lead, map_lead):
    rng = np.random.default_rng(71 + gap)
    revived = [rev([int(x) for x in rng.integers(1, 1453, int(rng.integers(2, 16)))], 0)
               for _ in range(40)]
    for i, s in enumerate(revived):  # the lost slot anywhere in the group
        revived[i] = rev(s[0], int(rng.integers(0, len(s[0]))))
    b = Batch(spread(revived), 72 + gap, map_stride=5, garbage=True, gap=gap, lead=lead,
              out_guard=23, out_lead=lead)
    assert b.map_stride > 15 // 8 + 1 and int(b.off[1]) % 16 != 0
    run(ctx, b, map_lead=map_lead)


# ---- 6. optional outputs -----------------------------------------------------------
@gpu
@pytest.mark.parametrize("skip", [("idx",), ("lst",), ("counts",), ("idx", "lst", "counts")])
def test_optional_outputs(ctx, skip):
    rng = np.random.default_rng(81)
    revived = [rev([int(x) for x in rng.integers(16, 600, 6)], int(rng.integers(0, 6)))
               for _ in range(19)]
    run(ctx, Batch(spread(revived), 82), skip=skip)


@gpu
def test_no_groups(ctx):
    counts = torch.full((3,), -1, dtype=torch.int64, device=DEV)
    ctx.revive_ragged(None, None, None, None, 0, None, None, None, None, 2, None, None,
                      status=None, counts=counts)
    ctx.sync()
    assert counts.tolist() == [0, 0, 0]
    ctx.revive_ragged(None, None, None, None, 0, None, None, None, None, 2, None, None,
                      status=None)
    ctx.sync()


# ---- 7. errors -----------------------------------------------------------------------
def base_specs(rng, n=21):
    revived = [rev([int(x) for x in rng.integers(16, 400, 10)], int(rng.integers(0, 10)))
               for _ in range(n)]
    return spread(revived)


def expect_latched(ctx, b, d, message, bad=()):
    o = Outs(b)
    call(ctx, b, d, o)
    with pytest.raises(qfec.InvalidFecData, match=message) as e:
        ctx.sync()
    assert e.value.code == -5
    check(o.host(), b, bad=bad)
    # the error is cleared, and a clean call on the same context is clean
    ctx.sync()
    rng = np.random.default_rng(99)
    run(ctx, Batch(base_specs(rng, 9), 98))


@gpu
@pytest.mark.parametrize("case", ["k0", "k256", "stride", "not_monotone"])
def test_latched_group_size(ctx, case):
    rng = np.random.default_rng(91)
    specs = base_specs(rng)
    kw = {}
    if case == "k0":
        specs.insert(5, ([], set(), True))
    elif case == "k256":
        specs.insert(5, ([16] * 256, {3}, True))
    elif case == "stride":
        specs.insert(5, ([20] * 16, {3}, True))  # 17 bits in a stride of 2
        kw["map_stride"] = 2
    else:
        # groups 0 / 1 / 2 of 10 / 5 / 10 packets with grp_ptr[2] = 5: group 1 has
        # "-5" packets, group 2 packets 5 .. 24, all received (complete)
        # (group 0 is complete as well: group 2's poisoned lengths cover its packets)
        specs[0:0] = [([30] * 10, set(), True), ([30] * 5, set(), True), ([30] * 10, set(), True)]
        ks = np.cumsum([0] + [len(s[0]) for s in specs])
        ks[2] = 5
        kw["ptr_override"] = ks
        kw["map_stride"] = 3  # 20 + 1 bits
    b = Batch(specs, 92, garbage=True, **kw)
    g = 1 if case == "not_monotone" else 5
    assert not b.valid[g] and b.valid.sum() == b.n - 1
    assert b.status[g] == qfec.GROUP_UNREVIVABLE and b.idx[g] == 0xFF
    expect_latched(ctx, b, upload(b), "FEC group with 0 or more than 255 packets")


@gpu
@pytest.mark.parametrize("case,message", [
    ("plen0", "Illegal FEC redundancy length"), ("plen1453", "Illegal FEC redundancy length"),
    ("len0", "Illegal payload size"), ("len_above_parity", "Illegal payload size")])
def test_latched_table_errors(ctx, case, message):
    rng = np.random.default_rng(93)
    b = Batch(base_specs(rng), 94)
    g = int(b.sel[10])  # a revived group in the middle of a list step
    p = int(b.ptr[g]) + (int(b.idx[g]) + 1) % 10  # one of its received packets
    assert b.rcv[p]
    if case == "plen0":
        b.plen_in[g] = 0
    elif case == "plen1453":
        b.plen_in[g] = 1453
    elif case == "len0":
        b.ln_in[p] = 0
    else:
        b.ln_in[p] = b.plen[g] + 1
    # the status states the map: still REVIVED; its out bytes are unspecified
    assert b.status[g] == qfec.GROUP_REVIVED
    expect_latched(ctx, b, upload(b), message, bad=[g])


@gpu
def test_host_refusals(ctx):
    rng = np.random.default_rng(95)
    b = Batch(base_specs(rng, 9), 96)
    d = upload(b)
    o = Outs(b)
    P = qfec._ptr
    names = ["bytes", "off", "ln", "ptr", "n", "par", "poff", "plen", "maps", "stride", "out",
             "ooff", "status", "idx", "lst", "counts", "flags"]

    def raw(**kw):
        a = dict(bytes=d["bytes"], off=d["off"], ln=d["ln"], ptr=d["ptr"], n=b.n, par=d["par"],
                 poff=d["poff"], plen=d["plen"], maps=d["maps"], stride=b.map_stride, out=o.out,
                 ooff=d["ooff"], status=o.status, idx=o.idx, lst=o.lst, counts=o.counts, flags=0)
        a.update(kw)
        args = [a[x] if x in ("n", "stride", "flags") else P(a[x]) for x in names]
        rc = ctx.lib.qfec_revive_ragged(ctx.ctx, *args)
        return rc, ctx.lib.qfec_last_error(ctx.ctx).decode()

    def untouched():
        ctx.sync()
        h = o.host()
        for key in ("status", "idx", "out"):
            assert np.all(h[key] == POISON), key
        assert np.all(h["lst"] == POISON64) and np.all(h["counts"] == POISON64)

    rc, msg = raw(stride=0)
    assert rc == -5 and "receive map stride 0" in msg
    untouched()
    for fl in (qfec.QFEC_PTR_HOST, qfec.QFEC_PTR_MAPPED, qfec.QFEC_ASYNC):
        rc, msg = raw(flags=fl)
        assert rc == -1 and "device pointers only" in msg and "QFEC_ASYNC" in msg
    untouched()
    for name in ("bytes", "off", "ln", "ptr", "par", "poff", "plen", "maps", "out", "ooff",
                 "status"):
        rc, msg = raw(**{name: None})
        assert rc == -1 and "null buffer" in msg, name
    untouched()
    rc, msg = raw(n=1 << 32)
    assert rc == -1 and "2^32" in msg
    untouched()
    # the accepted flags change nothing
    for fl in (0, qfec.QFEC_CACHED, qfec.QFEC_SMALL_GROUPS):
        o = Outs(b)
        rc, msg = raw(flags=fl)
        assert rc == 0, msg
        ctx.sync()
        check(o.host(), b)


# ---- 8. against the dense call --------------------------------------------------------
@gpu
def test_against_recover_ragged(ctx):
    rng = np.random.default_rng(101)
    specs = []
    for _ in range(203):
        k = int(rng.integers(1, 21))
        specs.append(rev([int(x) for x in rng.integers(1, 1453, k)], int(rng.integers(0, k))))
    b = Batch(specs, 102)
    assert b.counts.tolist() == [0, b.n, 0]
    d = upload(b)
    o = run(ctx, b)
    dense = torch.full((b.out_size,), POISON, dtype=torch.uint8, device=DEV)
    ctx.recover_ragged(d["bytes"], d["off"], d["ln"], d["ptr"], b.n, d["par"], d["poff"],
                       d["plen"], o.idx, dense, d["ooff"])
    ctx.sync()
    assert torch.equal(dense, o.out)
