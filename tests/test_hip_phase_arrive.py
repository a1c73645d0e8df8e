"""GPU tests of the phased kernel's split meeting (phase_arrive / phase_wait,
libquic_amd/csrc/qfec_kernels.hip): a workgroup arrives E = kPhEarly steps
before a phase's last step, step max(SP - E, 0) of the launch's SP steps per
phase, and only polls at the phase's end.

Every case forces the phased kernel with qfec_debug_phase_min(1), so small
batches phase; the launch then has ceil(n / (W x gpb x T)) phases of
SP = ceil(n / (W x gpb x phases)) steps, W the launch's workgroups (read back
through qfec_debug_last_phase_grid), gpb = floor(256 / ceil(L / 16)) groups
per step and T = 72 steps (templated k: 40 in LDS + 32 in registers) or 40
(runtime k).  The shapes put the arrival at every place it can fall: at or
before the first step, just after it, on either side of the LDS / register
edge (SP = 40, 41), inside the register steps (SP = 72), inside the LDS loop
of the runtime-k body, and across two and three phases (the epoch
arithmetic).  Each case asserts that the call ran phased, compares parity and
revived rows byte for byte with the same call under QFEC_ONE_PASS and with the
oracle on sampled groups, and asserts that no launch abandoned its meetings.
"""
import numpy as np
import pytest
import torch

from oracle import oracle_c as OC
from oracle import qfec_np as Q

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E = 4  # kPhEarly
LDS_STEPS, REG_STEPS = 40, 32


def gpb(L):
    return 256 // ((L + 15) // 16)


@pytest.fixture(scope="module")
def grid(ctx):
    """Workgroups of a phased launch on this context (one per CU, less the
    CUs left to other contexts' resident workers)."""
    k, L, n = 10, 1350, 64
    rows = torch.zeros(n * k * L, dtype=torch.uint8, device=DEV)
    par = torch.empty(n * L, dtype=torch.uint8, device=DEV)
    ctx.debug_phase(0, reset_backoff=True)
    ctx.debug_phase_min(1)
    try:
        ctx.encode(rows, k, L, n, par)
        assert ctx.last_fixed_phased() == 1
        w = ctx.last_phase_grid()
        ctx.sync()
    finally:
        ctx.debug_phase_min(0)
    assert w > 0
    return w


def make_rows(ctx, k, L, n):
    rows = torch.empty(n * k * L, dtype=torch.uint8, device=DEV)
    ctx.synth_fixed(rows, k, L, 0, n, Q.SEED_FIXED)
    miss_np = Q.drop_index(Q.SEED_DROP, np.arange(n), k).astype(np.uint8)
    return rows, miss_np, torch.from_numpy(miss_np).to(DEV)


def sample_vs_oracle(rows3, par, out, miss_np, k, L, n, count=14):
    rng = np.random.default_rng(n + k + L)
    for g in list(rng.choice(n, min(count, n), replace=False)) + [0, n - 1]:
        g = int(g)
        rr = np.ascontiguousarray(rows3[g].cpu().numpy()).ravel()
        _, pp = OC.encode_fixed(rr, k, L, 1)
        assert np.array_equal(par[g].cpu().numpy(), pp), g
        assert np.array_equal(out[g].cpu().numpy(), rr.reshape(k, L)[int(miss_np[g])]), g


def encode_recover_checked(ctx, k, L, n):
    """Encode and recover, phased (forced) and one-pass: byte-equal, the round
    trip exact on every group, the oracle on sampled groups, nothing abandoned."""
    rows, miss_np, miss = make_rows(ctx, k, L, n)
    before = ctx.phase_abandons()
    res = {}
    ctx.debug_phase_min(1)
    try:
        for one_pass in (False, True):
            par = torch.full((n * L,), 0xA5, dtype=torch.uint8, device=DEV)
            out = torch.full((n * L,), 0x5A, dtype=torch.uint8, device=DEV)
            ctx.encode(rows, k, L, n, par, one_pass=one_pass)
            assert ctx.last_fixed_phased() == (0 if one_pass else 1)
            ctx.recover(rows, par, miss, k, L, n, out, one_pass=one_pass)
            assert ctx.last_fixed_phased() == (0 if one_pass else 1)
            ctx.sync()
            torch.cuda.synchronize()
            res[one_pass] = (par, out)
    finally:
        ctx.debug_phase_min(0)
    assert ctx.phase_abandons() == before
    (pp, po), (op, oo) = res[False], res[True]
    assert torch.equal(pp, op), "phased parity != one-pass parity"
    assert torch.equal(po, oo), "phased revived != one-pass revived"
    r3 = rows.view(n, k, L)
    assert torch.equal(r3[torch.arange(n, device=DEV), miss.long()], po.view(n, L))
    sample_vs_oracle(r3, pp.view(n, L), po.view(n, L), miss_np, k, L, n)


@pytest.mark.parametrize("sp", [1, E, E + 1])
def test_one_phase_arrival_at_the_first_steps(ctx, grid, sp):
    """SP = 1 and E: the arrival at step max(SP - E, 0) = 0 (SP = 1: the top
    counter's add left to the wait); SP = E + 1: at step 1."""
    k, L = 10, 1350
    n = sp * grid * gpb(L) - 5  # one phase of sp steps, the last step ragged
    assert n > (sp - 1) * grid * gpb(L)
    encode_recover_checked(ctx, k, L, n)


@pytest.mark.parametrize("k", [10, 5])
@pytest.mark.parametrize("sp", [LDS_STEPS, LDS_STEPS + 1])
def test_one_phase_at_the_lds_register_edge(ctx, grid, k, sp):
    """SP = 40: every step in the LDS loop; SP = 41: one register step, the
    arrival in the LDS loop and its return value looked at there too."""
    L = 1350
    n = sp * grid * gpb(L) - 5
    encode_recover_checked(ctx, k, L, n)


@pytest.mark.parametrize("phases,tail", [(1, 777), (2, 777), (2, -777), (3, -777)])
def test_phases_of_register_steps(ctx, grid, phases, tail):
    """k = 10, L = 1350: `phases` full phases of 72 steps and 777 groups more
    (one more phase, the steps spread evenly: 2 x 37, 3 x 49), or 777 fewer (2
    and 3 phases of 72 steps, the arrival in the register steps, a ragged
    tail): the epoch arithmetic over several meetings."""
    k, L = 10, 1350
    n = phases * grid * gpb(L) * (LDS_STEPS + REG_STEPS) + tail
    encode_recover_checked(ctx, k, L, n)


@pytest.mark.parametrize("k,L,steps", [(33, 1350, LDS_STEPS),              # runtime body, RS = 0
                                       (17, 1350, LDS_STEPS + REG_STEPS),  # recover templated
                                       (10, 16, LDS_STEPS + REG_STEPS),    # gpb = 256
                                       (10, 1452, LDS_STEPS + REG_STEPS)])  # gpb = 2
def test_two_phases_other_bodies(ctx, grid, k, L, steps):
    """Two phases of `steps` steps, the last one ragged.  k = 33: encode and
    recover in the runtime-k body, the arrival in its LDS loop; k = 17: the
    recover templated with 32 register steps (its encode, runtime k, takes
    four phases of 40)."""
    n = 2 * grid * gpb(L) * steps - 777
    encode_recover_checked(ctx, k, L, n)


@pytest.mark.parametrize("in_place", [False, True])
def test_two_phases_inslot(ctx, grid, in_place):
    """The in-slot recover (the lost slot holds the redundancy), out of place
    and written in place, two phases of 72 steps."""
    k, L = 10, 1350
    n = 2 * grid * gpb(L) * (LDS_STEPS + REG_STEPS) - 777
    rows, miss_np, miss = make_rows(ctx, k, L, n)
    r3 = rows.view(n, k, L)
    idx = torch.arange(n, device=DEV)
    lost = r3[idx, miss.long()].clone()
    par = torch.empty(n * L, dtype=torch.uint8, device=DEV)
    ctx.encode(rows, k, L, n, par, one_pass=True)
    before = ctx.phase_abandons()
    got = {}
    ctx.debug_phase_min(1)
    try:
        for one_pass in (False, True):
            r3[idx, miss.long()] = par.view(n, L)  # the redundancy into the lost slot
            out = None if in_place else torch.full((n * L,), 0x5A, dtype=torch.uint8, device=DEV)
            ctx.recover_inslot(rows, miss, k, L, n, out, one_pass=one_pass)
            assert ctx.last_fixed_phased() == (0 if one_pass else 1)
            ctx.sync()
            torch.cuda.synchronize()
            got[one_pass] = r3[idx, miss.long()].clone() if in_place else out.view(n, L)
    finally:
        ctx.debug_phase_min(0)
    assert ctx.phase_abandons() == before
    assert torch.equal(got[False], got[True]), "phased in-slot != one-pass in-slot"
    assert torch.equal(got[False], lost)
    if in_place:  # every other row untouched: the original rows are back
        fresh, _, _ = make_rows(ctx, k, L, n)
        assert torch.equal(rows, fresh)
    rng = np.random.default_rng(n)
    for g in [0, n - 1] + [int(x) for x in rng.choice(n, 14, replace=False)]:
        rr = OC.synth_fixed(Q.SEED_FIXED, g, 1, k, L)
        assert np.array_equal(got[False][g].cpu().numpy(), rr.reshape(k, L)[int(miss_np[g])]), g


def test_twenty_launches_back_to_back(ctx, grid):
    """Encode, recover and in-slot alternating on one stream, three phases
    each: every launch finds the sync words reset by the one before it (no
    launch abandons), and the last launch of each kind wrote the right bytes."""
    k, L = 10, 1350
    n = 3 * grid * gpb(L) * (LDS_STEPS + REG_STEPS) - 777
    rows, miss_np, miss = make_rows(ctx, k, L, n)
    want_par = torch.empty(n * L, dtype=torch.uint8, device=DEV)
    want_out = torch.empty(n * L, dtype=torch.uint8, device=DEV)
    ctx.encode(rows, k, L, n, want_par, one_pass=True)
    ctx.recover(rows, want_par, miss, k, L, n, want_out, one_pass=True)
    ctx.sync()
    par = torch.zeros(n * L, dtype=torch.uint8, device=DEV)
    out = torch.zeros(n * L, dtype=torch.uint8, device=DEV)
    ins = torch.zeros(n * L, dtype=torch.uint8, device=DEV)
    before = ctx.phase_abandons()
    ctx.debug_phase_min(1)
    try:
        for i in range(20):
            if i == 17:  # the last launch of each kind writes over zeroes
                torch.cuda.synchronize()
                par.zero_(), out.zero_(), ins.zero_()
            if i % 3 == 0:
                ctx.encode(rows, k, L, n, par)
            elif i % 3 == 1:
                ctx.recover(rows, want_par, miss, k, L, n, out)
            else:  # out of place: the XOR of the k rows as they are, the parity
                ctx.recover_inslot(rows, miss, k, L, n, ins)
            assert ctx.last_fixed_phased() == 1
        ctx.sync()
        torch.cuda.synchronize()
    finally:
        ctx.debug_phase_min(0)
    assert ctx.phase_abandons() == before
    assert torch.equal(out, want_out)  # launch 20
    assert torch.equal(par, want_par) and torch.equal(ins, want_par)
    r3 = rows.view(n, k, L)
    sample_vs_oracle(r3, par.view(n, L), out.view(n, L), miss_np, k, L, n)


def test_abandon_path(ctx):
    """One workgroup beyond the CUs (qfec_debug_phase): it is not resident
    until another exits, the first wait times out and the launch abandons its
    meetings -- the workgroups that have seen the flag neither arrive nor wait
    again.  Same bytes as one-pass, one abandon counted per launch, and the
    next normal launch meets without abandoning."""
    k, L, n = 10, 1350, 1 << 18
    rows, miss_np, miss = make_rows(ctx, k, L, n)
    want_par = torch.empty(n * L, dtype=torch.uint8, device=DEV)
    want_out = torch.empty(n * L, dtype=torch.uint8, device=DEV)
    ctx.encode(rows, k, L, n, want_par, one_pass=True)
    ctx.recover(rows, want_par, miss, k, L, n, want_out, one_pass=True)
    par = torch.zeros(n * L, dtype=torch.uint8, device=DEV)
    out = torch.zeros(n * L, dtype=torch.uint8, device=DEV)
    ctx.debug_phase(0, reset_backoff=True)
    a0 = ctx.phase_abandons()
    try:
        ctx.debug_phase(1, reset_backoff=False)
        ctx.encode(rows, k, L, n, par)
        assert ctx.last_fixed_phased() == 1
        ctx.recover(rows, want_par, miss, k, L, n, out)
        assert ctx.last_fixed_phased() == 1
        ctx.sync()
        torch.cuda.synchronize()
        assert ctx.phase_abandons() == a0 + 2
        assert torch.equal(par, want_par)
        assert torch.equal(out, want_out)
    finally:
        ctx.debug_phase(0, reset_backoff=True)  # the hook off, the backoff cleared
    par.zero_()
    out.zero_()
    ctx.encode(rows, k, L, n, par)
    assert ctx.last_fixed_phased() == 1
    ctx.recover(rows, want_par, miss, k, L, n, out)
    assert ctx.last_fixed_phased() == 1
    ctx.sync()
    torch.cuda.synchronize()
    assert ctx.phase_abandons() == a0 + 2
    assert ctx.phase_backoff() == 0
    assert torch.equal(par, want_par)
    assert torch.equal(out, want_out)
    r3 = rows.view(n, k, L)
    sample_vs_oracle(r3, par.view(n, L), out.view(n, L), miss_np, k, L, n)
