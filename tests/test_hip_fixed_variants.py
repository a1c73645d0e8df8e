"""Every compiled variant of the fixed-shape kernels against a reference.

fixed_xor_kernel and phase_xor_kernel (libquic_amd/csrc/qfec_kernels.hip)
ship as one compiled body per group size k, per operation (encode, recover,
in place), per cache policy and per lane geometry; on gfx950 one
instantiation's register allocation has given wrong bytes before (DESIGN.md
§4).  The other suites run the bench's shapes at full size; this one runs each
body once, at the smallest batch that reaches all of its code:

(a) the phased bodies of every k from 2 to 33, two phases with every LDS and
    every register-held step in use and a ragged last step;
(b) tiny and boundary batches of the phased kernel (one group, one step, the
    first register step alone);
(c) a lost-slot index >= k placed in chosen LDS and register steps;
(d) the one-pass kernel in every groups-per-workgroup class, both cache
    policies, with the lost-slot indices at every misalignment;
(e) row, parity and output strides beyond 32 bits.

The reference is never another HIP kernel: the expected parity is a torch XOR
over the k rows on the device (every group), the expected revived row is the
erased row itself, and the C oracle (oracle/qfec_oracle.c) runs on a sample
holding a group of every (phase, step) pair, or on every group of a small
batch.  Outputs are pre-filled with a poison byte.  qfec_debug_phase_min(1)
sends any batch through the phased kernel; every phased case asserts that it
did (qfec_last_fixed_phased, the grid, no abandoned meeting).

The geometry below mirrors phase_plan / phase_steps_for: C = ceil(L/16) lanes
per group, gpb = 256 // C groups per workgroup, G workgroups (one per CU), a
phase of up to 40 LDS steps plus, where k is templated for the operation, 32
register-held steps; group g is step (g mod (SP G gpb)) // (G gpb) of phase
g // (SP G gpb).
"""
import os
import re

import numpy as np
import pytest
import torch

from oracle import oracle_c as OC
from oracle import qfec_np as Q
from libquic_amd import qfec

gpu = pytest.mark.gpu
DEV = "cuda:0"
L0 = 1350  # gpb = 3, 255 live lanes, an overlapping last 16-byte window
LDS_STEPS, REG_STEPS = 40, 32  # kPhSteps, kPhRegSteps
POISON = 0xA5

# the sweeps of (a); test_sweeps_cover_every_templated_k pins them to the source
ENC_K = list(range(2, 34))
REC_K = list(range(2, 34))
INPL_K = list(range(2, 18)) + [20, 31]


def templated(op, k):
    """phase_k_templated: k has its own phased body (with register steps)."""
    return 2 <= k <= 16 or (op == "recover" and 17 <= k <= 25)


def ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count


class Plan:
    """The phased launch of n groups: phase_plan and phase_steps_for."""

    def __init__(self, op, k, L, n):
        self.G = ncu()
        self.gpb = 256 // ((L + 15) // 16)
        self.per = self.G * self.gpb  # groups per step
        self.steps = LDS_STEPS + (REG_STEPS if templated(op, k) else 0)
        self.nphase = -(-n // (self.per * self.steps))
        self.SP = -(-n // (self.per * self.nphase))
        self.n = n

    def where(self, g):
        span = self.SP * self.per
        return g // span, (g % span) // self.per

    def pairs(self):
        """Every (phase, step) that holds a group."""
        return {(p, i) for p in range(self.nphase) for i in range(self.SP)
                if (p * self.SP + i) * self.per < self.n}


def two_phase_n(op, k, L):
    """Two phases, every step of the body in use, the last one ragged."""
    pl = Plan(op, k, L, 1)
    return 2 * pl.per * pl.steps - 3


def oracle_groups(pl, rng, per_step=2):
    """Groups for the C oracle: all of a small batch, else some of every
    (phase, step) pair plus the first and the last group."""
    n = pl.n
    if n <= 4096:
        return np.arange(n)
    idx = [0, n - 1]
    for (p, i) in sorted(pl.pairs()):
        for r in rng.integers(0, pl.per, per_step):
            idx.append(min((p * pl.SP + i) * pl.per + int(r), n - 1))
    idx = np.unique(np.array(idx, dtype=np.int64))
    assert {pl.where(int(g)) for g in idx} == pl.pairs()  # no step left out
    return idx


def oracle_check(rows_s, miss_s, k, L, par_s=None, out_s=None):
    """rows_s: [S][k][L] device rows of the sampled groups; par_s / out_s: the
    kernels' [S][L] parity / revived rows of the same groups."""
    S = rows_s.shape[0]
    rr = np.ascontiguousarray(rows_s.cpu().numpy()).ravel()
    rc, wp = OC.encode_fixed(rr, k, L, S)
    assert rc == 0
    if par_s is not None:
        assert np.array_equal(par_s.cpu().numpy().ravel(), wp), "parity != oracle"
    if out_s is not None:
        rc, wo = OC.recover_fixed(rr, wp, miss_s, k, L, S)
        assert rc == 0
        assert np.array_equal(out_s.cpu().numpy().ravel(), wo), "revived != oracle"


def make_inputs(ctx, k, L, n):
    """Synthetic rows (pinned to the oracle), drop indices, and the reference
    parity: a torch XOR over the k rows of every group."""
    assert n <= 1 << 24
    rows = torch.empty(n * k * L, dtype=torch.uint8, device=DEV)
    ctx.synth_fixed(rows, k, L, 0, n, Q.SEED_FIXED)
    ctx.sync()
    miss_np = Q.drop_index(Q.SEED_DROP, np.arange(n), k).astype(np.uint8)
    r3 = rows.view(n, k, L)
    par = r3[:, 0].clone()
    for i in range(1, k):
        par ^= r3[:, i]
    return rows, miss_np, par


def poisoned(nbytes):
    return torch.full((nbytes,), POISON, dtype=torch.uint8, device=DEV)


def call(ctx, op, how, k, L, n, rows, miss=None, par=None, out=None, **strides):
    """One library call; how: "phased" (forced by qfec_debug_phase_min(1) and
    asserted), "one_pass" or "cached" (QFEC_ONE_PASS, with QFEC_CACHED)."""
    flags = dict(one_pass=how != "phased", cached=how == "cached")
    if how == "phased":
        ctx.debug_phase_min(1)
    try:
        if op == "encode":
            ctx.encode(rows, k, L, n, out, **flags, **strides)
        elif op == "recover":
            ctx.recover(rows, par, miss, k, L, n, out, **flags, **strides)
        elif op == "inslot":
            ctx.recover_inslot(rows, miss, k, L, n, out, **flags, **strides)
        else:
            assert op == "inplace" and out is None
            ctx.recover_inslot(rows, miss, k, L, n, None, **flags, **strides)
    finally:
        if how == "phased":
            ctx.debug_phase_min(0)
    if how == "phased":  # a silent fall-back to one-pass fails here
        assert ctx.last_fixed_phased() == 1
        assert ctx.last_phase_grid() == ncu()
    else:
        assert ctx.last_fixed_phased() == 0


def finish(ctx, abandons, invalid=False):
    """sync(); with a bad lost-slot index in the batch it raises exactly once."""
    if invalid:
        with pytest.raises(qfec.InvalidFecData):
            ctx.sync()
    ctx.sync()
    torch.cuda.synchronize()
    assert ctx.phase_abandons() == abandons


def bad_slots(pl, op, k, keep, rng):
    """{group: index >= k}: three groups (k, k + 1, 255) in the first and the
    last LDS step and, for a templated k, the first and the last register
    step, of both phases; none of the oracle's sample `keep`."""
    steps = [0, LDS_STEPS - 1]
    if templated(op, k):
        steps += [LDS_STEPS, LDS_STEPS + REG_STEPS - 1]
    assert pl.nphase == 2 and pl.SP == pl.steps
    bad = {}
    for p in range(2):
        for s in steps:
            start = (p * pl.SP + s) * pl.per
            cand = np.setdiff1d(np.arange(start, min(start + pl.per, pl.n)), keep)
            for g, v in zip(rng.choice(cand, 3, replace=False), (k, k + 1, 255)):
                bad[int(g)] = v
    assert {pl.where(g) for g in bad} == {(p, s) for p in range(2) for s in steps}
    return bad


def run_phased(ctx, op, k, L, n, with_bad=False):
    """One operation through the phased kernel against the torch reference on
    every group and the C oracle on the sample."""
    pl = Plan(op, k, L, n)
    rng = np.random.default_rng(1000 * k + n % 997)
    ctx.debug_phase(0, reset_backoff=True)  # an earlier abandoned launch: no backoff here
    rows, miss_np, want_par = make_inputs(ctx, k, L, n)
    idx = oracle_groups(pl, rng)
    bad = bad_slots(pl, op, k, idx, rng) if with_bad else {}
    for g, v in bad.items():
        miss_np[g] = v
    miss = torch.from_numpy(miss_np).to(DEV)
    good = torch.ones(n, dtype=torch.bool, device=DEV)
    if bad:
        good[torch.tensor(sorted(bad), device=DEV)] = False
    ar = torch.arange(n, device=DEV)
    m_ok = miss.long().clamp(max=k - 1)  # (a bad group's slot is never used)
    it = torch.from_numpy(idx).to(DEV)
    r3 = rows.view(n, k, L)
    abandons = ctx.phase_abandons()
    if op == "encode":
        out = poisoned(n * L)
        call(ctx, op, "phased", k, L, n, rows, out=out)
        finish(ctx, abandons)
        assert torch.equal(out.view(n, L), want_par)
        oracle_check(r3[it], miss_np[idx], k, L, par_s=out.view(n, L)[it])
    elif op == "recover":
        out = poisoned(n * L)
        call(ctx, op, "phased", k, L, n, rows, miss=miss, par=want_par.view(-1), out=out)
        finish(ctx, abandons, invalid=bool(bad))
        want = r3[ar, m_ok]
        want[~good] = POISON  # a bad group's output is not written
        assert torch.equal(out.view(n, L), want)
        oracle_check(r3[it], miss_np[idx], k, L, out_s=out.view(n, L)[it])
    else:
        assert op == "inplace"
        orig = rows.clone()
        gi = ar[good]
        r3[gi, m_ok[gi]] = want_par[gi]  # the redundancy in the lost packet's row
        ins = rows.clone()
        call(ctx, op, "phased", k, L, n, rows, miss=miss)
        finish(ctx, abandons, invalid=bool(bad))
        # row missing[g] holds the lost packet, every other row (and every
        # row of a bad group) is unchanged
        assert torch.equal(rows, orig)
        oracle_check(orig.view(n, k, L)[it], miss_np[idx], k, L, out_s=r3[it, m_ok[it]])
        call(ctx, op, "phased", k, L, n, rows, miss=miss)  # twice: the redundancy again
        finish(ctx, abandons, invalid=bool(bad))
        assert torch.equal(rows, ins)


# ---- (a) every phased body, k = 2 .. 33 -----------------------------------
@gpu
@pytest.mark.parametrize("k", ENC_K)
def test_phased_encode_every_k(ctx, k):
    run_phased(ctx, "encode", k, L0, two_phase_n("encode", k, L0))


@gpu
@pytest.mark.parametrize("k", REC_K)
def test_phased_recover_every_k(ctx, k):
    run_phased(ctx, "recover", k, L0, two_phase_n("recover", k, L0))


@gpu
@pytest.mark.parametrize("k", INPL_K)
def test_phased_in_place_every_k(ctx, k):
    run_phased(ctx, "inplace", k, L0, two_phase_n("inplace", k, L0))


# ---- (b) tiny and boundary batches ----------------------------------------
TINY_SHAPES = ([(op, k) for k in (2, 10, 16) for op in ("encode", "recover", "inplace")]
               + [("recover", 25)]
               + [(op, 26) for op in ("encode", "recover", "inplace")])
TINY_N = {
    "one_group": lambda G, gpb: 1,
    "gpb-1": lambda G, gpb: gpb - 1,
    "one_step": lambda G, gpb: G * gpb - 1,  # SP = 1
    "lds_steps": lambda G, gpb: G * gpb * 40 - 1,
    "first_reg_step": lambda G, gpb: G * gpb * 41 - 3,
    "two_phases_of_41": lambda G, gpb: G * gpb * 82 - 3,
}


@gpu
@pytest.mark.parametrize("size", list(TINY_N))
@pytest.mark.parametrize("op,k", TINY_SHAPES)
def test_phased_tiny_batches(ctx, op, k, size):
    pl = Plan(op, k, L0, 1)
    run_phased(ctx, op, k, L0, TINY_N[size](pl.G, pl.gpb))


# ---- (c) a bad lost-slot index in each step class -------------------------
@gpu
@pytest.mark.parametrize("op,k", [("recover", k) for k in (2, 10, 16, 17, 25, 26, 33)]
                         + [("inplace", 10), ("inplace", 20)])
def test_phased_bad_index_in_chosen_steps(ctx, op, k):
    run_phased(ctx, op, k, L0, two_phase_n(op, k, L0), with_bad=True)


# ---- (d) the one-pass kernel's lane-geometry classes ----------------------
# both sides of every groups-per-workgroup boundary from 256 down to 2 (9 <-> 8
# at L 448 <-> 449 switches recover to scalar-loaded lost-slot words), and
# three packet sizes inside a class
ONE_PASS_L = [16, 17, 32, 33, 448, 449, 512, 513, 576, 577, 672, 673, 816, 817, 1024, 1025,
              1360, 1361, 1452, 500, 1001, 1350]


def missing_shifts(L):
    """Three misalignments 1..7 of the lost-slot array; all seven over the list."""
    i = ONE_PASS_L.index(L)
    return [(3 * i + j) % 7 + 1 for j in range(3)]


def shifted(miss_np, shift):
    """The lost-slot indices `shift` bytes into their allocation, bytes that
    are no valid index around them."""
    n = miss_np.size
    buf = torch.full((n + 16,), 0xFF, dtype=torch.uint8, device=DEV)
    buf[shift:shift + n] = torch.from_numpy(miss_np).to(DEV)
    t = buf[shift:shift + n]
    assert t.data_ptr() % 8 == shift % 8
    return t


@gpu
@pytest.mark.parametrize("cached", [False, True])
@pytest.mark.parametrize("k", [10, 14, 20])
@pytest.mark.parametrize("L", ONE_PASS_L)
def test_one_pass_lane_classes(ctx, L, k, cached):
    gpb = 256 // ((L + 15) // 16)
    n = 5 * gpb + 1
    how = "cached" if cached else "one_pass"
    rows = torch.empty(n * k * L, dtype=torch.uint8, device=DEV)
    ctx.synth_fixed(rows, k, L, 0, n, Q.SEED_FIXED)
    ctx.sync()
    torch.cuda.synchronize()
    rows_h = rows.cpu().numpy()
    miss_np = Q.drop_index(Q.SEED_DROP, np.arange(n), k).astype(np.uint8)
    rc, want_p = OC.encode_fixed(rows_h, k, L, n)
    assert rc == 0
    rc, want_o = OC.recover_fixed(rows_h, want_p, miss_np, k, L, n)
    assert rc == 0
    ins_h = rows_h.reshape(n, k, L).copy()
    ins_h[np.arange(n), miss_np.astype(np.int64)] = want_p.reshape(n, L)
    ins_h = ins_h.ravel()
    abandons = ctx.phase_abandons()

    out = poisoned(n * L)
    call(ctx, "encode", how, k, L, n, rows, out=out)
    finish(ctx, abandons)
    assert np.array_equal(out.cpu().numpy(), want_p), "encode"

    ins = torch.from_numpy(ins_h).to(DEV)
    out = poisoned(n * L)
    call(ctx, "inslot", how, k, L, n, ins, out=out)
    finish(ctx, abandons)
    assert np.array_equal(out.cpu().numpy(), want_o), "in-slot, out of place"

    par = torch.from_numpy(want_p).to(DEV)
    for shift in [0] + missing_shifts(L):
        miss = shifted(miss_np, shift)
        out = poisoned(n * L)
        call(ctx, "recover", how, k, L, n, rows, miss=miss, par=par, out=out)
        finish(ctx, abandons)
        assert np.array_equal(out.cpu().numpy(), want_o), f"recover, missing + {shift}"
        ins = torch.from_numpy(ins_h).to(DEV)
        call(ctx, "inplace", how, k, L, n, ins, miss=miss)
        finish(ctx, abandons)
        assert np.array_equal(ins.cpu().numpy(), rows_h), f"in place, missing + {shift}"


def test_missing_shifts_cover_every_misalignment():
    assert {s for L in ONE_PASS_L for s in missing_shifts(L)} == set(range(1, 8))


# ---- (e) strides beyond 32 bits -------------------------------------------
BASE, GUARD = 256, 64  # the buffers start BASE bytes into their allocation


def strided(nbytes_stride, shape, strides):
    """An uninitialised allocation of BASE + n * stride bytes and three views
    of it: the rows / slots in use, and the GUARD bytes before and after each
    (poisoned here, checked by guards_intact)."""
    big = torch.empty(BASE + nbytes_stride, dtype=torch.uint8, device=DEV)
    L = shape[-1]
    used = big.as_strided(shape, strides, BASE)
    before = big.as_strided(shape[:-1] + (GUARD,), strides, BASE - GUARD)
    after = big.as_strided(shape[:-1] + (GUARD,), strides, BASE + L)
    before.fill_(POISON ^ 0xFF)
    after.fill_(POISON ^ 0xFF)
    return big[BASE:], used, (before, after)


def guards_intact(guards):
    return all(bool((g == (POISON ^ 0xFF)).all()) for g in guards)


@gpu
@pytest.mark.parametrize("how", ["one_pass", "phased"])
@pytest.mark.parametrize("op", ["encode", "recover", "inplace"])
def test_row_stride_beyond_32_bits(ctx, op, how):
    """r * row_stride and g * group_stride past 4 GiB (about 13 GiB allocated,
    six rows of it touched)."""
    k, L, n = 3, L0, 2
    rs = (1 << 31) + 64
    gs = 3 * rs
    ctx.debug_phase(0, reset_backoff=True)
    dense, miss_np, want_par = make_inputs(ctx, k, L, n)
    d3 = dense.view(n, k, L)
    miss = torch.from_numpy(miss_np).to(DEV)
    ar = torch.arange(n, device=DEV)
    rows, r3, guards = strided(n * gs, (n, k, L), (gs, rs, 1))
    r3.copy_(d3)
    kw = dict(row_stride=rs, group_stride=gs)
    abandons = ctx.phase_abandons()
    host_rows = d3.cpu().numpy().ravel()
    _, op_par = OC.encode_fixed(host_rows, k, L, n)
    _, op_out = OC.recover_fixed(host_rows, op_par, miss_np, k, L, n)
    if op == "inplace":
        for g in range(n):
            r3[g, int(miss_np[g])] = want_par[g]  # the redundancy in the lost packet's row
        call(ctx, op, how, k, L, n, rows, miss=miss, **kw)
        finish(ctx, abandons)
        assert torch.equal(r3, d3)
        assert np.array_equal(r3.cpu().numpy()[np.arange(n), miss_np].ravel(), op_out)
        call(ctx, op, how, k, L, n, rows, miss=miss, **kw)
        finish(ctx, abandons)
        for g in range(n):
            assert torch.equal(r3[g, int(miss_np[g])], want_par[g])
    else:
        out = poisoned(n * L)
        if op == "encode":
            call(ctx, op, how, k, L, n, rows, out=out, **kw)
        else:
            call(ctx, op, how, k, L, n, rows, miss=miss, par=want_par.view(-1), out=out, **kw)
        finish(ctx, abandons)
        assert torch.equal(out.view(n, L), want_par if op == "encode" else d3[ar, miss.long()])
        assert np.array_equal(out.cpu().numpy(), op_par if op == "encode" else op_out)
        assert torch.equal(r3, d3)
    assert guards_intact(guards)


@gpu
@pytest.mark.parametrize("how", ["one_pass", "phased"])
@pytest.mark.parametrize("op", ["encode", "recover"])
def test_parity_and_out_stride_beyond_32_bits(ctx, op, how):
    """g * parity_stride and g * out_stride past 4 GiB, dense rows."""
    k, L, n = 10, L0, 2
    st = (1 << 32) + 16
    ctx.debug_phase(0, reset_backoff=True)
    rows, miss_np, want_par = make_inputs(ctx, k, L, n)
    r3 = rows.view(n, k, L)
    miss = torch.from_numpy(miss_np).to(DEV)
    host_rows = r3.cpu().numpy().ravel()
    _, op_par = OC.encode_fixed(host_rows, k, L, n)
    _, op_out = OC.recover_fixed(host_rows, op_par, miss_np, k, L, n)
    out, o2, guards = strided(n * st, (n, L), (st, 1))
    o2.fill_(POISON)
    abandons = ctx.phase_abandons()
    if op == "encode":
        call(ctx, op, how, k, L, n, rows, out=out, parity_stride=st)
        finish(ctx, abandons)
        assert torch.equal(o2, want_par)
        assert np.array_equal(o2.cpu().numpy().ravel(), op_par)
    else:
        par, p2, pguards = strided(n * st, (n, L), (st, 1))
        p2.copy_(want_par)
        call(ctx, op, how, k, L, n, rows, miss=miss, par=par, out=out, parity_stride=st,
             out_stride=st)
        finish(ctx, abandons)
        assert torch.equal(o2, r3[torch.arange(n, device=DEV), miss.long()])
        assert np.array_equal(o2.cpu().numpy().ravel(), op_out)
        assert torch.equal(p2, want_par) and guards_intact(pguards)
    assert guards_intact(guards)


# ---- the sweeps follow the source (no GPU) --------------------------------
def test_sweeps_cover_every_templated_k():
    """A group size newly added to the templated lists of qfec_kernels.hip is
    in no sweep above until someone adds it: this fails first."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                        "libquic_amd", "csrc", "qfec_kernels.hip")
    with open(path) as f:
        src = f.read()

    def klist(name):
        m = re.search(r"#define[ \t]+%s\(X\)((?:[ \t]*\\\n|[ \t]*X\(\d+\))+)" % name, src)
        assert m, name
        ks = [int(x) for x in re.findall(r"X\((\d+)\)", m.group(1))]
        assert ks, name
        return ks

    k_all = klist("QFEC_K_ALL")
    k_rec = klist("QFEC_K_PHASE_RECOVER")
    assert set(k_all) | {max(k_all) + 1} <= set(ENC_K)
    assert set(k_all) | {max(k_all) + 1} <= set(INPL_K)
    assert set(k_all) | set(k_rec) | {max(k_all + k_rec) + 1} <= set(REC_K)
    # the mirror of phase_k_templated used for the geometry above
    for k in range(1, 64):
        assert templated("encode", k) == templated("inplace", k) == (k in k_all)
        assert templated("recover", k) == (k in k_all or k in k_rec)
