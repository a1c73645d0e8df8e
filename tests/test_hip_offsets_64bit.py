"""The uint64 offset tables of the CSR calls at and beyond 2^32: ad_off, in_off
and out_off of the protection calls, pkt_off, parity_off and out_off of the
ragged FEC calls, and s * acc_stride of qfec_accumulate_ragged.

One uninitialised device allocation of 2^32 + 8 MiB bytes serves as `bytes`
and as `out`.  Only its first and its last 8 MiB are used (and, for the
accumulator, a window around every row): half of a call's ranges lie below
2^32 and half at 2^32 + 48 + r and up.  For every range at a high address A
the range at A - 2^32 holds DIFFERENT data when it is an input, and a sentinel
that must come back unchanged when it is an output: an offset truncated to 32
bits reads wrong bytes or writes where the test looks, and cannot fault, since
both addresses lie inside the allocation.  Every output range has 64-byte 0xA5
guard bands on both sides, and both 8-MiB regions are compared whole.

None of these operations depends on position: the oracle (oracle/oracle_c.py,
tests/accumulate_rule.py) runs on a compact host copy with rebased offsets.
Each case runs with the high half in the inputs only, then in the outputs only.
"""
import numpy as np
import pytest
import torch

import accumulate_rule as R
import protect_cases as PC
from oracle import oracle_c as OC
from libquic_amd import qfec

from test_hip_revive_ragged import Batch, dview

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HI = 1 << 32
REGION = 8 << 20   # the bytes used at either end of the allocation
ZONE = 4 << 20     # of the low region: [0, ZONE) mirrors the high ranges, [ZONE, REGION) is used
GUARD, FILL, SENTINEL, LOST = 64, 0xA5, 0x3C, 0xC3
SIDES = ["inputs", "outputs"]


@pytest.fixture(scope="module")
def big():
    return torch.empty(HI + REGION, dtype=torch.uint8, device=DEV)


class Arena:
    """The images of the two regions (and of windows elsewhere), as they are
    before the call (init) and as they must be after it (want)."""

    def __init__(self, seed, start=48):
        rng = np.random.default_rng(seed)
        self.init = {0: rng.integers(0, 256, REGION, dtype=np.uint8),
                     HI: rng.integers(0, 256, REGION, dtype=np.uint8)}
        self.want = {k: v.copy() for k, v in self.init.items()}
        self.cur = {False: ZONE + start, True: start}

    def alloc(self, n, high, res=None):
        """n bytes (at res mod 16) with room for guard bands on both sides."""
        c = self.cur[high] + 2 * GUARD
        if res is not None:
            c += (int(res) - c) % 16
        self.cur[high] = c + n
        assert self.cur[high] + 2 * GUARD <= (ZONE if high else REGION)
        return HI + c if high else c

    def views(self, addr, n):
        """init and want bytes of [addr, addr + n): inside a region, or a window of its own."""
        for base, v in self.init.items():
            if base <= addr and addr + n <= base + v.size:
                s = slice(addr - base, addr - base + n)
                return v[s], self.want[base][s]
        assert all(addr + n <= base or base + v.size <= addr for base, v in self.init.items())
        assert addr + n <= HI
        self.init[addr], self.want[addr] = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        return self.init[addr], self.want[addr]

    def set(self, addr, data):
        for v in self.views(addr, len(data)):
            v[:] = data

    def input(self, data, high, res=None):
        """Place input bytes; below a high input lie different bytes."""
        data = np.asarray(data, np.uint8)
        a = self.alloc(data.size, high, res)
        self.set(a, data)
        if high:
            self.set(a - HI, data ^ 0xFF)
        return a

    def output(self, n, high, res=None):
        """An output range of FILL between FILL guard bands; below a high one a sentinel."""
        a = self.alloc(n, high, res)
        self.set(a - GUARD, np.full(n + 2 * GUARD, FILL, np.uint8))
        if high:
            self.set(a - HI - GUARD, np.full(n + 2 * GUARD, SENTINEL, np.uint8))
        return a

    def expect(self, addr, data):
        self.views(addr, len(data))[1][:] = data

    def upload(self, big):
        for a, v in self.init.items():
            big[a:a + v.size] = torch.from_numpy(v).to(DEV)

    def check(self, big):
        torch.cuda.synchronize()
        for a, w in self.want.items():
            got = big[a:a + w.size].cpu().numpy()
            bad = np.flatnonzero(got != w)
            assert bad.size == 0, f"{bad.size} bytes differ in the region at {a:#x}, first at " \
                                  f"{[hex(a + int(x)) for x in bad[:6]]}"


def spans(ar, data, off, lens, high, res=None):
    """Inputs: span i of the compact buffer to the arena; returns the addresses."""
    return np.array([ar.input(data[int(o):int(o) + int(l)], bool(h),
                              None if res is None else res[i])
                     for i, (o, l, h) in enumerate(zip(off, lens, high))], np.uint64)


def halves(addr):
    """Half of the ranges lie at or above 2^32 + 48, the others in the low region."""
    hi = int((addr >= np.uint64(HI + 48)).sum())
    return abs(2 * hi - addr.size) <= 1 and int((addr < np.uint64(REGION)).sum()) == addr.size - hi


# ---- packet protection: ad_off, in_off, out_off -----------------------------------------
@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("decrypt", [False, True], ids=["seal", "open"])
@pytest.mark.parametrize("cipher", PC.CIPHERS)
def test_protect(ctx, big, cipher, decrypt, side):
    """Three waves (two key-uniform with different keys, one mixed)."""
    n = 192
    p = np.arange(n)
    rng = np.random.default_rng(7)
    pn, path = PC.numbers(n, 8)
    plain = PC.Plain(p * 29 % 48, rng.choice(PC.LENGTHS, n), np.where(p >= 128, p % 2, p // 64),
                     pn, path, 2, 9)
    b = PC.open_batch(plain, cipher) if decrypt else PC.seal_batch(plain)
    if decrypt:
        w_out, w_ok = PC.oracle_open(cipher, b)
        assert w_ok.all()
    else:
        w_out = PC.oracle_seal(cipher, b)
    ar = Arena(10)
    ins, outs = side == "inputs", side == "outputs"
    ad = spans(ar, b.data, b.ad_off, b.ad_len, ins & (p % 2 == 1), p * 7 % 16)
    src = spans(ar, b.data, b.in_off, b.in_len, ins & (p // 2 % 2 == 1), p * 5 % 16)
    dst = np.array([ar.output(int(l), bool(h), r)
                    for l, h, r in zip(b.out_len, outs & (p % 2 == 1), p * 11 % 16)], np.uint64)
    assert (halves(ad) and halves(src)) if ins else halves(dst)
    for q in range(n):
        o = int(b.out_off[q])
        ar.expect(int(dst[q]), w_out[o:o + int(b.out_len[q])])
    ar.upload(big)
    ok = torch.full((n,), 7, dtype=torch.uint8, device=DEV)
    io = [big, dview(ad), dview(b.ad_len), dview(src), dview(b.in_len), n, big, dview(dst)]
    if decrypt:
        io.append(ok)
    if cipher == "null":
        (ctx.null_decrypt if decrypt else ctx.null_encrypt)(*io)
    else:
        keys, pre = plain.keys(cipher)
        getattr(ctx, cipher + ("_open" if decrypt else "_seal"))(
            dview(keys), dview(pre), dview(plain.kidx), dview(plain.pn), dview(plain.path), *io)
    ctx.sync()
    if decrypt:
        assert np.array_equal(ok.cpu().numpy(), w_ok)
    ar.check(big)


# ---- ragged FEC: pkt_off, parity_off, out_off ----------------------------------------------
def fec_batch(seed):
    """24 groups of 2..15 packets of 1..1452 bytes, compact, with the oracle's
    parity (a 1,452-byte slot per group) and a lost packet per group."""
    rng = np.random.default_rng(seed)
    n = 24
    ks = rng.integers(2, 16, n)
    ks[0], ks[1] = 2, 15
    ptr = np.zeros(n + 1, np.uint32)
    ptr[1:] = np.cumsum(ks)
    ln = rng.integers(16, 1453, int(ks.sum())).astype(np.uint16)
    ln[[0, 1, 2, 3]] = [1, 1452, 15, 16]
    ln[rng.integers(4, ln.size, 3)] = rng.integers(1, 16, 3)
    off = np.zeros(ln.size, np.uint64)
    off[1:] = np.cumsum(ln[:-1].astype(np.uint64))
    data = rng.integers(0, 256, int(ln.astype(np.int64).sum()), dtype=np.uint8)
    poff = np.arange(n, dtype=np.uint64) * np.uint64(1452)
    rc, par, plen = OC.encode_ragged(data, off, ln, ptr, poff, n * 1452)
    assert rc == 0
    miss = (rng.integers(0, 1 << 20, n) % ks).astype(np.uint8)
    rc, rec = OC.recover_ragged(data, off, ln, ptr, par, poff, plen, miss, poff, n * 1452)
    assert rc == 0
    return dict(n=n, ptr=ptr, ln=ln, off=off, data=data, poff=poff, par=par, plen=plen,
                miss=miss, rec=rec, grp=np.repeat(np.arange(n), ks))


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("small", [False, True], ids=["block", "small_groups"])
def test_encode_ragged(ctx, big, small, side):
    z = fec_batch(21)
    n, P = z["n"], z["ln"].size
    ar = Arena(22)
    pkt = spans(ar, z["data"], z["off"], z["ln"], (side == "inputs") & (np.arange(P) % 2 == 1),
                np.arange(P) * 5 % 16)
    par = np.array([ar.output(1452, side == "outputs" and g % 2 == 1, g * 7 % 16)
                    for g in range(n)], np.uint64)
    assert halves(pkt if side == "inputs" else par)
    for g in range(n):
        o = int(z["poff"][g])
        ar.expect(int(par[g]), z["par"][o:o + int(z["plen"][g])])
    ar.upload(big)
    plen = torch.zeros(n, dtype=torch.int16, device=DEV)
    ctx.encode_ragged(big, dview(pkt), dview(z["ln"]), dview(z["ptr"]), n, big, dview(par), plen,
                      small_groups=small)
    ctx.sync()
    assert np.array_equal(plen.cpu().numpy().view(np.uint16), z["plen"])
    ar.check(big)


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("small", [False, True], ids=["block", "small_groups"])
def test_recover_ragged(ctx, big, small, side):
    z = fec_batch(23)
    n, P = z["n"], z["ln"].size
    lost = z["ptr"][:-1].astype(np.int64) + z["miss"]
    data = z["data"].copy()
    for q in lost:  # never read
        data[int(z["off"][q]):int(z["off"][q]) + int(z["ln"][q])] = LOST
    ar = Arena(24)
    ins = side == "inputs"
    pkt = spans(ar, data, z["off"], z["ln"], ins & (np.arange(P) % 2 == 1), np.arange(P) * 5 % 16)
    par = spans(ar, z["par"], z["poff"], z["plen"], ins & (np.arange(n) % 2 == 0),
                np.arange(n) * 3 % 16)
    out = np.array([ar.output(1452, (not ins) and g % 2 == 1, g * 7 % 16) for g in range(n)],
                   np.uint64)
    assert (halves(pkt) and halves(par)) if ins else halves(out)
    for g in range(n):
        o = int(z["poff"][g])
        ar.expect(int(out[g]), z["rec"][o:o + int(z["plen"][g])])
    ar.upload(big)
    ctx.recover_ragged(big, dview(pkt), dview(z["ln"]), dview(z["ptr"]), n, big, dview(par),
                       dview(z["plen"]), dview(z["miss"]), big, dview(out), small_groups=small)
    ctx.sync()
    ar.check(big)


@pytest.mark.parametrize("side", SIDES)
def test_revive_ragged(ctx, big, side):
    """The tables of test_recover_ragged, every sixth group complete and every
    sixth unrevivable (their out ranges must stay as they were)."""
    rng = np.random.default_rng(31)
    specs = []
    for g in range(24):
        k = int(rng.integers(2, 16))
        lens = [int(x) for x in rng.integers(1, 1453, k)]
        lost = set() if g % 6 == 4 else {0, k - 1} if g % 6 == 5 else {int(rng.integers(0, k))}
        specs.append((lens, lost, g % 12 != 3))  # (group 3: its one loss without the FEC packet)
    b = Batch(specs, 32)
    n, P = b.n, b.ln.size
    assert b.counts.tolist() == [4, 14, 6]  # complete, revived, unrevivable
    ar = Arena(33)
    ins = side == "inputs"
    pkt = spans(ar, b.bytes_in, b.off, b.ln, ins & (np.arange(P) % 2 == 1), np.arange(P) * 5 % 16)
    par = spans(ar, b.par_in, b.poff, b.plen, ins & (np.arange(n) % 2 == 0),
                np.arange(n) * 3 % 16)
    out = np.array([ar.output(1452, (not ins) and g % 2 == 1, g * 7 % 16) for g in range(n)],
                   np.uint64)
    assert (halves(pkt) and halves(par)) if ins else halves(out)
    rev = b.status == qfec.GROUP_REVIVED
    assert rev[out >= np.uint64(HI)].sum() >= 5 or ins
    for g in np.flatnonzero(rev):
        o = int(b.ooff[g])
        ar.expect(int(out[g]), b.want_out[o:o + int(b.plen[g])])
    ar.upload(big)
    status = torch.full((n,), FILL, dtype=torch.uint8, device=DEV)
    idx = torch.full((n,), FILL, dtype=torch.uint8, device=DEV)
    lst = torch.full((n,), -1, dtype=torch.int64, device=DEV)
    counts = torch.full((3,), -1, dtype=torch.int64, device=DEV)
    ctx.revive_ragged(big, dview(pkt), dview(b.ln), dview(b.ptr), n, big, dview(par),
                      dview(b.plen), dview(b.maps), b.map_stride, big, dview(out), status=status,
                      revived_idx=idx, revived_list=lst, counts=counts)
    ctx.sync()
    assert np.array_equal(status.cpu().numpy(), b.status)
    assert np.array_equal(idx.cpu().numpy(), b.idx)
    assert np.array_equal(counts.cpu().numpy().view(np.uint64), b.counts)
    assert np.array_equal(lst.cpu().numpy().view(np.uint64)[:b.lst.size], b.lst)
    ar.check(big)


# ---- accumulate: s * acc_stride ----------------------------------------------------------------
ACC_STRIDE = (1 << 28) + 16
ACC_BASE = 4096   # acc = allocation + ACC_BASE: row 16 starts at 2^32 + 4352
N_SLOTS = 17
ROW = 1452


@pytest.mark.parametrize("side", SIDES)
def test_accumulate_ragged(ctx, big, side):
    """Rows acc_stride = 2^28 + 16 apart, 17 slots: s * acc_stride passes 2^32
    at slot 16.  Two turns: the high row is written, then read and written.
    inputs: the packets of both turns half above 2^32 (rows below it);
    outputs: slot 16 among the rows (packets below 2^32); where its offset
    truncated to 32 bits would land, inside slot 0's row, lie other bytes."""
    rng = np.random.default_rng(41)
    n = 12
    ins = side == "inputs"
    slot = (rng.permutation(np.arange(1, 16))[:n] if ins
            else np.concatenate([[16, 0, 15], rng.permutation(np.arange(1, 15))[:n - 3]]))
    slot = slot.astype(np.uint32)
    assert np.unique(slot).size == n and (ins or int(slot[0]) * ACC_STRIDE + ACC_BASE > HI)
    ks = rng.integers(2, 16, n)
    groups = [[rng.integers(0, 256, int(l), dtype=np.uint8) for l in rng.integers(1, ROW + 1, k)]
              for k in ks]
    groups[0][0] = rng.integers(0, 256, ROW, dtype=np.uint8)  # the high row at full length
    ar = Arena(42, start=2 * ACC_BASE)  # clear of rows 0 and 16 and what lies below row 16
    # the rule on a compact accumulator; the rows hold garbage, the named lengths 0
    acc = rng.integers(0, 256, N_SLOTS * 1536, dtype=np.uint8)
    acc_len = np.full(N_SLOTS, 0xA5A5, np.uint16)
    acc_len[slot] = 0
    rows = {}
    for s in slot:
        a = ACC_BASE + int(s) * ACC_STRIDE
        rows[int(s)] = a
        win = np.concatenate([np.full(GUARD, FILL, np.uint8), acc[int(s) * 1536:int(s) * 1536 + ROW],
                              np.full(GUARD, FILL, np.uint8)])
        if a >= HI:  # below the high row: other bytes, that must come back unchanged
            ar.set(a - HI - GUARD, np.full(win.size, SENTINEL, np.uint8))
        ar.set(a - GUARD, win)
    d_len = dview(acc_len)
    turns = []
    count = 0
    for t in range(2):
        part = [g[:len(g) // 2] if t == 0 else g[len(g) // 2:] for g in groups]
        flat = [q for g in part for q in g]
        ptr = np.zeros(n + 1, np.uint32)
        ptr[1:] = np.cumsum([len(g) for g in part])
        ln = np.array([q.size for q in flat], np.uint16)
        off = np.zeros(ln.size, np.uint64)
        off[1:] = np.cumsum(ln[:-1].astype(np.uint64))
        data = np.concatenate(flat)
        errs = R.accumulate(data, off, ln, ptr, acc, 1536, acc_len, slot)
        assert not errs.any()
        high = ins & ((np.arange(ln.size) + count) % 2 == 1)
        count += ln.size
        addr = spans(ar, data, off, ln, high, np.arange(ln.size) * 5 % 16)
        assert halves(addr) or not ins
        turns.append((dview(addr), dview(ln), dview(ptr)))
    for s, a in rows.items():
        ar.expect(a, acc[s * 1536:s * 1536 + int(acc_len[s])])
    ar.upload(big)
    d_slot = dview(slot)
    for addr, ln, ptr in turns:
        ctx.accumulate_ragged(big, addr, ln, ptr, n, big[ACC_BASE:], ACC_STRIDE, d_len,
                              slot=d_slot, n_slots=N_SLOTS)
    ctx.sync()
    assert np.array_equal(d_len.cpu().numpy().view(np.uint16), acc_len)
    ar.check(big)
