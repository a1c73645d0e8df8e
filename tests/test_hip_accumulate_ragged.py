"""qfec_accumulate_ragged on the GPU: fold a turn's packets into one running
row per open group, bit for bit against the rule of tests/accumulate_rule.py
(pinned to oracle/qfec_np.py by test_accumulate_rule.py).

Discipline, as in test_hip_revive_ragged.py: every offset is in range, so a
wrong kernel gives wrong bytes, not a fault.  Rows of slots in use hold random
garbage beyond their length before a call (the call must treat it as zero and
leave what lies beyond the new length alone); slots no group names hold a
POISON row and a POISON length; the tables carry one trailing entry that no
group owns, with a length of 0.  Whole buffers are compared, not just
[0, new) of the rows that were named.
"""
import numpy as np
import pytest
import torch

import accumulate_rule as R
from oracle import oracle_c as OC
from libquic_amd import qfec

gpu = pytest.mark.gpu
DEV = "cuda:0"
POISON, PAD, LOST = 0xA5, 0x5A, 0x3C
POISON16 = np.uint16(0xA5A5)
TAIL = 32  # bytes behind the last row / packet
_SIGNED = {np.dtype(np.uint8): np.uint8, np.dtype(np.uint16): np.int16,
           np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}
MSG = {R.ERR_GROUP: "FEC group with 0 or more than 255 packets",
       R.ERR_SLOT: "missing packet index >= FEC group size",
       R.ERR_ROWLEN: "Illegal FEC redundancy length",
       R.ERR_PKTLEN: "Illegal payload size"}


def dview(a):
    """device copy of an array (bits preserved; torch lacks wide unsigned types)"""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(_SIGNED[a.dtype]).copy()).to(DEV)


def pays(rng, lens):
    return [rng.integers(0, 256, int(x), dtype=np.uint8) for x in lens]


class Turn:
    """One call's CSR batch.  groups: per group the payload arrays to fold.
    align: packets start on multiples of it (0: byte-packed with `gap` PAD
    bytes between and `lead` before the first)."""

    def __init__(self, groups, *, align=16, lead=0, gap=0, ptr_override=None):
        flat = [p for g in groups for p in g]
        self.n = len(groups)
        ptr = np.zeros(self.n + 1, np.uint32)
        ptr[1:] = np.cumsum([len(g) for g in groups])
        ln = np.zeros(len(flat) + 1, np.uint16)  # (+ the entry nobody owns: length 0)
        off = np.zeros(len(flat) + 1, np.uint64)
        pos = lead
        for i, p in enumerate(flat):
            if align:
                pos = (pos + align - 1) // align * align
            off[i], ln[i] = pos, p.size
            pos += p.size + gap
        data = np.full(pos + TAIL, PAD, np.uint8)
        for i, p in enumerate(flat):
            data[int(off[i]):int(off[i]) + p.size] = p
        self.data, self.off, self.ln = data, off, ln
        self.ptr = ptr if ptr_override is None else np.asarray(ptr_override, np.uint32)

    def upload(self):
        self.d = [dview(x) for x in (self.data, self.off, self.ln, self.ptr)]
        return self


class Acc:
    """The accumulator buffer and its lengths: the expectation on the host, the
    buffer under test on the device.  used: {slot: old length}."""

    def __init__(self, n_slots, stride, used, rng):
        self.n_slots, self.stride, self.rng = n_slots, stride, rng
        self.want = np.full(n_slots * stride + TAIL, POISON, np.uint8)
        self.want_len = np.full(n_slots, POISON16, np.uint16)
        self.used = sorted(used)
        for s, old in used.items():
            self.want_len[s] = old
            self.want[s * stride:(s + 1) * stride] = rng.integers(0, 256, stride, dtype=np.uint8)
        self.keep = []
        self.push()

    def push(self):
        self.d_acc, self.d_len = dview(self.want), dview(self.want_len)

    def garbage(self):
        """fresh garbage beyond the length of every slot in use, on both sides"""
        for s in self.used:
            a, b = s * self.stride + int(self.want_len[s]), (s + 1) * self.stride
            if int(self.want_len[s]) <= self.stride:
                self.want[a:b] = self.rng.integers(0, 256, b - a, dtype=np.uint8)
        self.push()

    def call(self, ctx, t, slot=None, *, d_slot=None):
        """d_slot: the slots already on the device (a context on a stream of its
        own: the caller has waited for the upload)."""
        errs = R.accumulate(t.data, t.off, t.ln, t.ptr, self.want, self.stride,
                            self.want_len, slot)
        if not hasattr(t, "d"):
            t.upload()
        if slot is not None and d_slot is None:
            d_slot = dview(np.asarray(slot, np.uint32))
        self.keep += [t, d_slot]
        ctx.accumulate_ragged(t.d[0], t.d[1], t.d[2], t.d[3], t.n, self.d_acc, self.stride,
                              self.d_len, slot=d_slot, n_slots=self.n_slots)
        return errs

    def check(self):
        got = self.d_acc.cpu().numpy().view(np.uint8)
        got_len = self.d_len.cpu().numpy().view(np.uint16)
        bad = np.flatnonzero(got_len != self.want_len)
        assert bad.size == 0, f"lengths differ at slots {bad[:8]}: {got_len[bad[:8]]} " \
                              f"want {self.want_len[bad[:8]]}"
        bad = np.flatnonzero(got != self.want)
        assert bad.size == 0, f"{bad.size} bytes differ, first at slot {bad[0] // self.stride} " \
                              f"byte {bad[0] % self.stride}"
        self.keep.clear()


def arena_groups(rng, n, kmin=5, kmax=15, lmin=64, lmax=1350):
    return [pays(rng, rng.integers(lmin, lmax + 1, int(rng.integers(kmin, kmax + 1))))
            for _ in range(n)]


def split3(rng, groups):
    """each group's packets in three non-empty parts, in a random order"""
    turns = [[], [], []]
    for g in groups:
        order = rng.permutation(len(g))
        c1 = int(rng.integers(1, len(g) - 1))
        c2 = int(rng.integers(c1 + 1, len(g)))
        for t, idx in enumerate((order[:c1], order[c1:c2], order[c2:])):
            turns[t].append([g[i] for i in idx])
    return turns


# ---- 1. the block path over several turns -----------------------------------------------
@gpu
@pytest.mark.parametrize("mode", ["queued", "synced", "identity"])
def test_block_path_three_turns(ctx, mode):
    rng = np.random.default_rng(11)
    groups = arena_groups(rng, 64)
    slot = None if mode == "identity" else rng.permutation(80)[:64].astype(np.uint32)
    named = range(64) if slot is None else [int(s) for s in slot]
    st = Acc(80, 1536, {s: 0 for s in named}, rng)
    turns = [Turn(t).upload() for t in split3(rng, groups)]
    for t in turns:
        assert not st.call(ctx, t, slot).any()
        if mode == "synced":
            ctx.sync()
            st.check()
            st.garbage()
    ctx.sync()
    st.check()
    # and the rows are the groups' parities
    full = Turn(groups)
    poff = np.array(named, np.uint64) * np.uint64(1536)
    rc, par, plen = OC.encode_ragged(full.data, full.off, full.ln, full.ptr, poff, st.want.size)
    assert rc == 0
    for g, s in enumerate(named):
        assert st.want_len[s] == plen[g]
        assert np.array_equal(st.want[s * 1536:s * 1536 + int(plen[g])],
                              par[s * 1536:s * 1536 + int(plen[g])])


# ---- 2. group counts around the 8-group step ---------------------------------------------
@gpu
@pytest.mark.parametrize("n", [1, 7, 8, 9, 17])
def test_group_counts(ctx, n):
    rng = np.random.default_rng(20 + n)
    slot = rng.permutation(n + 5)[:n].astype(np.uint32)
    st = Acc(n + 5, 1536, {int(s): 0 for s in slot}, rng)
    for _ in range(2):  # fresh slots, then slots that hold a row
        assert not st.call(ctx, Turn(arena_groups(rng, n, 2, 6)), slot).any()
        ctx.sync()
        st.check()
        st.garbage()


# ---- 3. lengths ----------------------------------------------------------------------------
# (old length of the slot, this turn's packet lengths); block: a group the
# block path may take (old 0 or >= 16, every packet >= 16 B)
LENGTHS = [
    (0, [16]), (0, [17]), (0, [1350, 64]), (0, [1451]), (0, [1452]), (0, [700, 16, 1452]),
    (1452, [16, 700]), (1350, [1349]), (17, [16]), (16, [17]), (700, [1451]), (1451, [1452]),
    (1350, [1350, 20]), (16, [16]), (1452, [1452]), (31, [33, 47]),
    (0, [1]), (0, [15]), (0, [1, 15, 16, 17]), (7, [100, 30]), (15, [3]), (5, [5]), (1, [1]),
    (1, [1452]), (16, [1]), (1452, [1]), (0, [1200, 9, 800]), (900, [5, 1000]), (15, [16]),
]


@gpu
@pytest.mark.parametrize("order", ["grouped", "shuffled"])
@pytest.mark.parametrize("layout", ["aligned", "packed"])
def test_lengths(ctx, order, layout):
    rng = np.random.default_rng(31)
    cases = list(LENGTHS)
    assert any(o == 0 for o, _ in cases) and any(1 <= o <= 15 for o, _ in cases)
    assert any(o > max(l) for o, l in cases) and any(0 < o < max(l) for o, l in cases)
    assert any(o == max(l) for o, l in cases)
    if order == "shuffled":
        cases = [cases[i] for i in rng.permutation(len(cases))]
    stride = 1536 if layout == "aligned" else 1453
    kw = dict(align=16) if layout == "aligned" else dict(align=0, lead=3, gap=1)
    n = len(cases)
    slot = rng.permutation(n + 7)[:n].astype(np.uint32)
    st = Acc(n + 7, stride, {int(slot[g]): cases[g][0] for g in range(n)}, rng)
    t = Turn([pays(rng, lens) for _, lens in cases], **kw)
    assert not st.call(ctx, t, slot).any()
    ctx.sync()
    st.check()
    for g, (old, lens) in enumerate(cases):
        assert st.want_len[int(slot[g])] == max(old, max(lens))


# ---- 4. groups with nothing to fold ---------------------------------------------------------
@gpu
def test_empty_groups(ctx):
    rng = np.random.default_rng(41)
    groups, used = [], {}
    for g in range(19):
        empty = g % 3 == 1 or g in (8, 9, 10)
        groups.append([] if empty else pays(rng, rng.integers(16, 600, 4)))
        used[g] = (0, 500, 9)[g % 3] if g % 2 else 0
    st = Acc(19, 1536, used, rng)
    before, before_len = st.want.copy(), st.want_len.copy()
    assert not st.call(ctx, Turn(groups), None).any()
    for g in range(19):
        if not groups[g]:
            assert st.want_len[g] == before_len[g]
            assert np.array_equal(st.want[g * 1536:(g + 1) * 1536],
                                  before[g * 1536:(g + 1) * 1536])
    assert ctx.sync() == qfec.QFEC_OK
    st.check()


# ---- 5. wide groups --------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("case", ["k255", "second_chunk", "step_over_256"])
def test_wide_groups(ctx, case):
    rng = np.random.default_rng(51)
    ks = {"k255": [255, 3], "second_chunk": [65, 100, 130, 4, 64],
          "step_over_256": [40] * 8 + [5]}[case]
    groups = [pays(rng, rng.integers(16, 200, k)) for k in ks]
    if case == "step_over_256":
        assert sum(ks[:8]) > 256
    slot = rng.permutation(len(ks) + 3)[:len(ks)].astype(np.uint32)
    st = Acc(len(ks) + 3, 1536, {int(s): (0, 120)[i % 2] for i, s in enumerate(slot)}, rng)
    assert not st.call(ctx, Turn(groups), slot).any()
    ctx.sync()
    st.check()


# ---- 6. a receiver: the accumulator is the revived packet -----------------------------------
@gpu
@pytest.mark.parametrize("fec", ["first", "last"])
def test_receiver(ctx, fec):
    rng = np.random.default_rng(61)
    n, stride = 23, 1536
    groups = []
    for g in range(n):
        k = int(rng.integers(2, 13))
        lens = rng.integers(1, 1453, k) if g % 3 else rng.integers(16, 1351, k)
        groups.append(pays(rng, lens))
    lost = np.array([int(rng.integers(0, len(g))) for g in groups], np.uint8)
    full = Turn(groups, align=0)
    poff = np.arange(n, dtype=np.uint64) * np.uint64(stride)
    rc, par, plen = OC.encode_ragged(full.data, full.off, full.ln, full.ptr, poff,
                                     n * stride + TAIL)
    assert rc == 0
    # the receiver's copy: lost payloads never arrived
    rcv_data = full.data.copy()
    rcv = np.ones(full.ln.size - 1, bool)
    for g in range(n):
        p = int(full.ptr[g]) + int(lost[g])
        rcv[p] = False
        rcv_data[int(full.off[p]):int(full.off[p]) + int(full.ln[p])] = LOST
    rc, want = OC.recover_ragged(rcv_data, full.off, full.ln, full.ptr, par, poff, plen, lost,
                                 poff, n * stride + TAIL)
    assert rc == 0
    # two calls: the received data packets in two parts, the redundancy with one of them
    a, b = [], []
    for g in range(n):
        got = [groups[g][i] for i in rng.permutation(len(groups[g])) if i != lost[g]]
        cut = int(rng.integers(0, len(got) + 1))
        red = [par[int(poff[g]):int(poff[g]) + int(plen[g])].copy()]
        a.append((red if fec == "first" else []) + got[:cut])
        b.append(got[cut:] + (red if fec == "last" else []))
    st = Acc(n, stride, {g: 0 for g in range(n)}, rng)
    for t in (Turn(a), Turn(b)):
        assert not st.call(ctx, t, None).any()
    ctx.sync()
    st.check()
    for g in range(n):
        assert st.want_len[g] == plen[g]
        lo, hi = g * stride, g * stride + int(plen[g])
        assert np.array_equal(st.want[lo:hi], want[lo:hi])
    # qfec_revive_ragged from the matching receive maps, on the retained packets
    maps = qfec.pack_received_ragged(rcv, np.ones(n, bool), full.ptr)
    out = torch.full((n * stride + TAIL,), POISON, dtype=torch.uint8, device=DEV)
    status = torch.full((n,), POISON, dtype=torch.uint8, device=DEV)
    d = [dview(x) for x in (rcv_data, full.off, full.ln, full.ptr, par, poff, plen, maps)]
    ctx.revive_ragged(d[0], d[1], d[2], d[3], n, d[4], d[5], d[6], d[7], maps.shape[1], out, d[5],
                      status=status)
    ctx.sync()
    assert torch.all(status == qfec.GROUP_REVIVED)
    for g in range(n):
        lo, hi = g * stride, g * stride + int(plen[g])
        assert torch.equal(out[lo:hi], st.d_acc[lo:hi]), g


# ---- 7. latched errors -------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("case,err", [
    ("slot_eq_n_slots", R.ERR_SLOT), ("len0", R.ERR_PKTLEN), ("len1453", R.ERR_PKTLEN),
    ("len_above_stride", R.ERR_PKTLEN), ("acc_len1453", R.ERR_ROWLEN),
    ("not_monotone", R.ERR_GROUP)])
def test_latched_errors(ctx, case, err):
    rng = np.random.default_rng(71)
    n, n_slots, bad = 21, 30, 10
    stride = 1350 if case == "len_above_stride" else 1536
    groups = arena_groups(rng, n, 3, 8, 16, 1350)
    slot = rng.permutation(n_slots)[:n].astype(np.uint32)
    used = {int(s): (0, 300)[i % 2] for i, s in enumerate(slot)}
    ptr = None
    if case == "slot_eq_n_slots":
        del used[int(slot[bad])]
        slot[bad] = n_slots
    elif case == "acc_len1453":
        used[int(slot[bad])] = 1453
    elif case == "not_monotone":
        # groups 0 / 1 / 2 of 10 / 5 / 10 packets with grp_ptr[2] = 5: group 1 has "-5"
        # packets, group 2 packets 5 .. 24
        groups[0:3] = [pays(rng, [30] * 10), pays(rng, [30] * 5), pays(rng, [30] * 10)]
        ptr = np.cumsum([0] + [len(g) for g in groups])
        ptr[2] = 5
        bad = 1
    t = Turn(groups, ptr_override=ptr)
    p = int(t.ptr[bad]) + 1
    if case == "len0":
        t.ln[p] = 0
    elif case == "len1453":
        t.ln[p] = 1453  # (the bytes are there: the next packet's)
    elif case == "len_above_stride":
        t.ln[p] = 1351
    st = Acc(n_slots, stride, used, rng)
    before, before_len = st.want.copy(), st.want_len.copy()
    errs = st.call(ctx, t, slot)
    assert errs[bad] == err and np.count_nonzero(errs) == 1
    if case != "slot_eq_n_slots":  # the offending group's row and length: untouched
        s = int(slot[bad])
        assert st.want_len[s] == before_len[s]
        assert np.array_equal(st.want[s * stride:(s + 1) * stride],
                              before[s * stride:(s + 1) * stride])
    with pytest.raises(qfec.InvalidFecData, match=MSG[err]) as e:
        ctx.sync()
    assert e.value.code == -5
    assert ctx.sync() == qfec.QFEC_OK  # once
    st.check()


# ---- 8. host refusals ----------------------------------------------------------------------------
@gpu
def test_host_refusals(ctx):
    rng = np.random.default_rng(81)
    n, n_slots, stride = 9, 12, 1536
    t = Turn(arena_groups(rng, n)).upload()
    slot = rng.permutation(n_slots)[:n].astype(np.uint32)
    d_slot = dview(slot)
    acc = torch.full((n_slots * stride,), POISON, dtype=torch.uint8, device=DEV)
    acc_len = dview(np.full(n_slots, POISON16, np.uint16))
    P = qfec._ptr
    names = ["bytes", "off", "ln", "ptr", "n", "acc", "stride", "acc_len", "slot", "n_slots",
             "flags"]

    def raw(**kw):
        a = dict(bytes=t.d[0], off=t.d[1], ln=t.d[2], ptr=t.d[3], n=n, acc=acc, stride=stride,
                 acc_len=acc_len, slot=d_slot, n_slots=n_slots, flags=0)
        a.update(kw)
        args = [a[x] if x in ("n", "stride", "n_slots", "flags") else P(a[x]) for x in names]
        rc = ctx.lib.qfec_accumulate_ragged(ctx.ctx, *args)
        return rc, ctx.lib.qfec_last_error(ctx.ctx).decode()

    def untouched():
        assert ctx.sync() == qfec.QFEC_OK
        assert torch.all(acc == POISON)
        assert np.all(acc_len.cpu().numpy().view(np.uint16) == POISON16)

    rc, msg = raw(stride=0)
    assert rc == -5 and "accumulator stride 0" in msg
    untouched()
    for fl in (qfec.QFEC_PTR_HOST, qfec.QFEC_PTR_MAPPED, qfec.QFEC_ASYNC):
        rc, msg = raw(flags=fl)
        assert rc == -1 and "device pointers only" in msg and "QFEC_ASYNC" in msg
        untouched()
    for name in ("bytes", "off", "ln", "ptr", "acc", "acc_len"):
        rc, msg = raw(**{name: None})
        assert rc == -1 and "null buffer" in msg, name
        untouched()
    for kw in (dict(n=1 << 32), dict(n_slots=1 << 32)):
        rc, msg = raw(**kw)
        assert rc == -1 and "2^32" in msg
        untouched()
    rc, msg = raw(slot=None, n_slots=n - 1)
    assert rc == -1 and "fewer slots than groups" in msg
    untouched()
    assert ctx.lib.qfec_debug_fail_launches(ctx.ctx, 1) == 0
    try:
        rc, msg = raw()
    finally:
        assert ctx.lib.qfec_debug_fail_launches(ctx.ctx, 0) == 0
    assert rc == -1 and "launch failure injected" in msg
    untouched()
    # no groups: decided before the buffers are looked at
    rc, msg = raw(bytes=None, off=None, ln=None, ptr=None, n=0, acc=None, acc_len=None,
                  slot=None, n_slots=0)
    assert rc == qfec.QFEC_OK, msg
    untouched()
    # the accepted flags change nothing
    for fl in (0, qfec.QFEC_CACHED, qfec.QFEC_SMALL_GROUPS):
        st = Acc(n_slots, stride, {int(s): 0 for s in slot}, rng)
        R.accumulate(t.data, t.off, t.ln, t.ptr, st.want, stride, st.want_len, slot)
        rc, msg = raw(acc=st.d_acc, acc_len=st.d_len, flags=fl)
        assert rc == 0, msg
        ctx.sync()
        st.check()


# ---- 9. streams and contexts ------------------------------------------------------------------------
@gpu
def test_torch_stream(ctx):
    rng = np.random.default_rng(91)
    st = Acc(12, 1536, {g: 0 for g in range(12)}, rng)
    turns = [Turn(arena_groups(rng, 12, 2, 5)).upload() for _ in range(2)]
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    ctx.set_stream(s)
    try:
        for t in turns:
            assert not st.call(ctx, t, None).any()
        ctx.sync()
    finally:
        # back to the session's setting (conftest: torch's current stream), so later
        # tests' torch fills stay ordered with the context's launches
        ctx.set_stream(torch.cuda.current_stream())
    st.check()


@gpu
def test_two_contexts_one_buffer(ctx):
    rng = np.random.default_rng(92)
    n = 16
    slots = rng.permutation(2 * n + 3).astype(np.uint32)
    sa, sb = slots[:n], slots[n:2 * n]
    st = Acc(2 * n + 3, 1536, {int(s): (0, 200)[i % 2] for i, s in enumerate(slots[:2 * n])},
             rng)
    ta, tb = Turn(arena_groups(rng, n, 2, 6)).upload(), Turn(arena_groups(rng, n, 2, 6)).upload()
    da, db = dview(sa), dview(sb)
    torch.cuda.synchronize()  # the uploads (torch's stream) before launches on another stream
    with qfec.Context(0) as other:
        assert not st.call(ctx, ta, sa, d_slot=da).any()
        assert not st.call(other, tb, sb, d_slot=db).any()
        ctx.sync()
        other.sync()
    st.check()
