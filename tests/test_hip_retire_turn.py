"""The receiver's turn with retention on the device, end to end on the GPU:
qfec_retire_groups -> qfec_assign_slots -> qfec_bin_arrivals ->
qfec_admit_ragged -> qfec_accumulate_ragged -> qfec_revive_tracked, three turns
queued on one stream with ONE qfec_sync at each turn's end, everything equal to
the rules chained: retire_rule -> assign_rule -> bin_rule -> admit_rule ->
accumulate_rule -> admit_rule.revive_tracked.

The turns are tests/assign_turns.py's (about 300 groups), keyed two groups to a
connection (connection = group // 2) so that a bound of two open groups holds
until the test breaks it, with arrivals added:
  turn 2: a late duplicate of a group turn 1 released, its connection's mark
          raised past it -- not reopened (without the retire it is); a mark
          raised over an unrevivable group that release_mask 0b011 left open --
          its slot closes and the same turn's assign hands it to a new group,
          which is revived there with nothing cleared;
  turn 3: two new groups on a connection that holds two already, max_groups 2:
          the older two are evicted, their slots closed, their packets
          refused, and the new ones revived.
"""
import types

import numpy as np
import pytest
import torch

import admit_rule as R
import assign_rule as AS
import assign_turns as T
import retire_rule as RR
from libquic_amd import qfec
from test_admit_rule import make_groups
from test_hip_accumulate_ragged import dview
from test_hip_tracked_turn import MS, PAD, POISON, STRIDE, host

gpu = pytest.mark.gpu
DEV = "cuda:0"
SHIFT, N_CONNS = 40, 700
MASK = (1 << SHIFT) - 1
NK = RR.NO_KEY
P32, P64 = np.uint32(0xA5A5A5A5), np.uint64(0xA5A5A5A5A5A5A5A5)


def key_of(gid):
    """two groups to a connection, the number as assign_turns gives it"""
    return np.uint64(((gid // 2) << SHIFT) | (1000 + 3 * gid))


def rekeyed(d):
    """the turn with its arrivals under key_of"""
    m = d["m"]
    gid = ((d["a_key"][:m] & np.uint64(MASK)).astype(np.int64) - 1000) // 3
    key = np.append([key_of(int(g)) for g in gid], np.uint64(0)).astype(np.uint64)
    assert np.array_equal(key[:m] & np.uint64(MASK), d["a_key"][:m] & np.uint64(MASK))
    return dict(d, a_key=key)


def extended(d, recs, front=False):
    """the turn with the arrivals recs = [(key, K, idx, bytes)] in front of or
    behind its own, their plaintexts behind the turn's"""
    m, plain = d["m"], d["w"].plain
    pos = (plain.size + 15) // 16 * 16
    offs = []
    for _, _, _, b in recs:
        offs.append(pos)
        pos = (pos + b.size + 15) // 16 * 16
    new_plain = np.full(pos + 32, PAD, np.uint8)
    new_plain[:plain.size] = plain
    for off, (_, _, _, b) in zip(offs, recs):
        new_plain[off:off + b.size] = b

    def table(name, vals):
        x = d[name]
        vals = np.array(vals, x.dtype)
        parts = [vals, x[:m]] if front else [x[:m], vals]
        return np.concatenate(parts + [x[m:m + 1]])

    return dict(d, m=m + len(recs), w=types.SimpleNamespace(plain=new_plain),
                a_key=table("a_key", [r[0] for r in recs]), a_k=table("a_k", [r[1] for r in recs]),
                a_idx=table("a_idx", [r[2] for r in recs]),
                a_ln=table("a_ln", [r[3].size for r in recs]), a_pt_off=table("a_pt_off", offs),
                a_good=table("a_good", [1] * len(recs)))


def fresh_group(rng, key):
    """a small group of which everything but one data packet arrives: (recs,
    the packet the close must revive, zero-padded to the redundancy's length)"""
    items = make_groups(rng, 1, kmin=2, kmax=4, lmin=64, lmax=300)[0]
    k = len(items) - 1
    lost = int(rng.integers(0, k))
    recs = [(key, k, int(i), items[int(i)]) for i in rng.permutation(k + 1) if i != lost]
    want = np.zeros(items[k].size, np.uint8)
    want[:items[lost].size] = items[lost]
    return recs, want


def rule_turn(state, d, marks, raises, max_groups, retire):
    """one turn by the rules; state and marks are modified in place"""
    n_slots, m = state.n_slots, d["m"]
    key_out = np.full(m + 1, P64, np.uint64)
    closed = np.full(n_slots + 1, P32, np.uint32)
    cnt = np.zeros(5, np.uint64)
    if retire:
        cnt = RR.retire_groups(d["a_key"][:m], state.slot_key[:n_slots], state.acc_len[:n_slots],
                               marks[:N_CONNS], SHIFT, max_groups,
                               np.array([c for c, _ in raises], np.uint32),
                               np.array([x for _, x in raises], np.uint64), key_out, closed)
        assert cnt[RR.BAD] == 0
    else:
        key_out = d["a_key"].copy()
    len_retired = state.acc_len.copy()
    r = T.key_turn(state, dict(d, a_key=key_out))
    r.update(key_out=key_out, closed=closed, r_cnt=cnt, len_retired=len_retired,
             marks=marks.copy())
    return r


class Device:
    """the receiver's state on the device, and the turn's seven calls"""

    def __init__(self, ctx, state, marks):
        self.ctx, self.n_slots = ctx, state.n_slots
        self.acc, self.len, self.maps = dview(state.acc), dview(state.acc_len), dview(state.maps)
        self.key, self.k = dview(state.slot_key), dview(state.slot_k)
        self.out_off, self.marks = dview(state.out_off), dview(marks)

    def turn(self, h, raises, max_groups, retire):
        ctx, n_slots, m = self.ctx, self.n_slots, h["m"]
        d = dict(key=dview(h["a_key"]), k=dview(h["a_k"]), pt_off=dview(h["a_pt_off"]),
                 ln=dview(h["a_ln"]), idx=dview(h["a_idx"]), ok=dview(h["a_good"]),
                 plain=dview(h["w"].plain),
                 rc=dview(np.array([c for c, _ in raises] + [0], np.uint32)),
                 rm=dview(np.array([x for _, x in raises] + [0], np.uint64)),
                 key_out=dview(np.full(m + 1, P64, np.uint64)),
                 closed=dview(np.full(n_slots + 1, P32, np.uint32)),
                 r_cnt=dview(np.zeros(5, np.uint64)),
                 a_slot=dview(np.full(m + 1, POISON, np.uint32)),
                 a_cnt=dview(np.zeros(5, np.uint64)),
                 t_ptr=dview(np.full(n_slots + 1, POISON, np.uint32)),
                 t_off=dview(np.full(m + 1, POISON, np.uint64)),
                 t_ln=dview(np.full(m + 1, POISON, np.uint16)),
                 t_idx=dview(np.full(m + 1, POISON, np.uint8)),
                 t_ok=dview(np.full(m + 1, POISON, np.uint8)),
                 t_src=dview(np.full(m + 1, POISON, np.uint32)),
                 b_cnt=dview(np.zeros(3, np.uint64)),
                 o_ptr=dview(np.full(n_slots + 1, POISON, np.uint32)),
                 o_off=dview(np.zeros(m + 1, np.uint64)), o_ln=dview(np.zeros(m + 1, np.uint16)),
                 v=dview(np.full(m + 1, POISON, np.uint8)), cnt=dview(np.zeros(4, np.uint64)),
                 out=torch.full((n_slots * STRIDE + 32,), PAD, dtype=torch.uint8, device=DEV),
                 olen=dview(np.zeros(n_slots, np.uint16)),
                 st=dview(np.zeros(n_slots, np.uint8)), ridx=dview(np.zeros(n_slots, np.uint8)),
                 rlist=dview(np.full(n_slots, P64, np.uint64)), counts=dview(np.zeros(3, np.uint64)),
                 # (read back at the turn's end: the lengths the retire left, the
                 # slot tables the assign left)
                 len_retired=torch.empty(n_slots + 1, dtype=torch.int16, device=DEV),
                 slot_key=torch.empty(n_slots + 1, dtype=torch.int64, device=DEV),
                 slot_k=torch.empty(n_slots + 1, dtype=torch.uint8, device=DEV))
        keys = d["key"]
        if retire:
            ctx.retire_groups(d["key"], m, self.key, self.len, n_slots, self.marks, N_CONNS, SHIFT,
                              max_groups, d["key_out"], raise_conn=d["rc"], raise_mark=d["rm"],
                              n_raise=len(raises), closed_list=d["closed"], counts=d["r_cnt"])
            keys = d["key_out"]
        d["len_retired"].copy_(self.len)  # (device to device on the same stream: no sync)
        ctx.assign_slots(keys, d["k"], m, self.key, self.k, self.len, n_slots, d["a_slot"],
                         counts=d["a_cnt"])
        d["slot_key"].copy_(self.key)
        d["slot_k"].copy_(self.k)
        ctx.bin_arrivals(d["a_slot"], d["pt_off"], d["ln"], d["idx"], d["ok"], m, n_slots,
                         d["t_ptr"], d["t_off"], d["t_ln"], d["t_idx"], pkt_ok_out=d["t_ok"],
                         src_out=d["t_src"], counts=d["b_cnt"])
        ctx.admit_ragged(d["t_off"], d["t_ln"], d["t_idx"], d["t_ok"], d["t_ptr"], n_slots,
                         self.k, self.maps, MS, self.len, STRIDE, d["o_ptr"], d["o_off"], d["o_ln"],
                         d["v"], slot=None, n_slots=n_slots, counts=d["cnt"])
        ctx.accumulate_ragged(d["plain"], d["o_off"], d["o_ln"], d["o_ptr"], n_slots, self.acc,
                              STRIDE, self.len, slot=None, n_slots=n_slots)
        ctx.revive_tracked(self.acc, STRIDE, self.len, self.maps, MS, self.k, n_slots, d["out"],
                           self.out_off, d["olen"], status=d["st"], slot=None, n_slots=n_slots,
                           revived_idx=d["ridx"], revived_list=d["rlist"], counts=d["counts"],
                           release_mask=T.MASK)
        assert ctx.sync() == qfec.QFEC_OK  # the turn's only one
        return d


def check_turn(t, d, r, retire, state, dev, marks):
    """every table of the turn, and the state it leaves, against the rules"""
    for key, dt in (("a_slot", np.uint32), ("t_ptr", np.uint32), ("t_off", np.uint64),
                    ("t_ln", np.uint16), ("t_idx", np.uint8), ("t_ok", np.uint8),
                    ("t_src", np.uint32), ("o_ptr", np.uint32), ("v", np.uint8), ("st", np.uint8),
                    ("ridx", np.uint8), ("olen", np.uint16), ("out", np.uint8),
                    ("slot_key", np.uint64), ("slot_k", np.uint8), ("len_retired", np.uint16)):
        assert np.array_equal(host(d[key], dt), r[key]), (t, key)
    if retire:
        assert np.array_equal(host(d["key_out"], np.uint64), r["key_out"]), t
        assert np.array_equal(host(d["closed"], np.uint32), r["closed"]), t
    for key in ("r_cnt", "a_cnt", "b_cnt", "cnt", "counts"):
        assert host(d[key], np.uint64).tolist() == r[key].tolist(), (t, key)
    nrev = int(r["counts"][R.REVIVED])
    assert np.array_equal(host(d["rlist"], np.uint64)[:nrev], r["rlist"]), t
    assert np.array_equal(host(dev.marks, np.uint64), marks), t
    assert np.array_equal(host(dev.len, np.uint16), state.acc_len), t
    assert np.array_equal(host(dev.maps, np.uint8).ravel(), state.maps.ravel()), t
    assert np.array_equal(host(dev.acc, np.uint8), state.acc), t
    assert np.array_equal(host(dev.key, np.uint64), state.slot_key), t
    assert np.array_equal(host(dev.k, np.uint8), state.slot_k), t


def conn_num(key):
    return int(key) >> SHIFT, int(key) & MASK


@gpu
@pytest.mark.parametrize("retire", [True, False], ids=["retire", "no retire"])
def test_three_turns_with_retention(ctx, retire):
    turns = [rekeyed(h) for h in T.host_turns(3400)]
    state = T.KeyState(3401)
    n_slots = state.n_slots
    rng = np.random.default_rng(3402)
    marks = np.append(np.zeros(N_CONNS, np.uint64), P64)
    dev = Device(ctx, state, marks)

    # ---- turn 1: nothing to retire
    r0 = rule_turn(state, turns[0], marks, [], 0, retire)
    check_turn(0, dev.turn(turns[0], [], 0, retire), r0, retire, state, dev, marks)
    assert r0["r_cnt"][RR.CLOSED] == 0 and not marks[:N_CONNS].any()

    # ---- turn 2: a late duplicate of a released group, and an unrevivable
    # group left open, each with its connection's mark raised past it
    was_open = r0["len_pre"] > 0
    released = np.flatnonzero(was_open & (r0["st"] != R.UNREVIVABLE))
    stuck = np.flatnonzero(was_open & (r0["st"] == R.UNREVIVABLE) & (state.acc_len[:n_slots] > 0))
    s_dup, s_u = int(released[0]), int(stuck[0])
    key_dup, key_u = state.slot_key[s_dup], state.slot_key[s_u]
    (c_dup, x_dup), (c_u, x_u) = conn_num(key_dup), conn_num(key_u)
    assert c_dup != c_u
    raises = [(c_dup, x_dup + 1), (c_u, x_u + 1), (c_u, x_u)]
    # as many new groups, first in the turn, as there will be free slots up to
    # the stuck group's: the last of them takes that slot
    after = state.acc_len.copy()
    RR.retire_groups([], state.slot_key[:n_slots], after[:n_slots], marks[:N_CONNS].copy(), SHIFT, 0,
                     [c for c, _ in raises], [x for _, x in raises], [])
    assert after[s_u] == 0
    n_new = int((after[:s_u + 1] == 0).sum())
    new, new_want = [], []
    for j in range(n_new):
        recs, want = fresh_group(rng, np.uint64(((400 + j) << SHIFT) | 10))
        new += recs
        new_want.append(want)
    h1 = extended(turns[1], new, front=True)
    h1 = extended(h1, [(key_dup, int(state.slot_k[s_dup]), 0,
                        rng.integers(0, 256, 100, dtype=np.uint8))])
    r1 = rule_turn(state, h1, marks, raises if retire else [], 0, retire)
    check_turn(1, dev.turn(h1, raises if retire else [], 0, retire), r1, retire, state, dev, marks)
    last = h1["m"] - 1
    holders = [s for s in np.flatnonzero(r1["len_pre"]) if r1["slot_key"][s] == key_dup]
    if not retire:  # the policy the host would have had to keep: it is open again
        assert r1["a_slot"][last] != AS.NO_SLOT and holders == [int(r1["a_slot"][last])]
        return
    assert r1["key_out"][last] == NK and r1["a_slot"][last] == AS.NO_SLOT and not holders
    assert marks[c_dup] == x_dup + 1 and marks[c_u] == x_u + 1
    n_closed = int(r1["r_cnt"][RR.CLOSED])
    assert s_u in r1["closed"][:n_closed].tolist() and r1["len_retired"][s_u] == 0
    # the stuck group's slot went to the last of the new groups, whose lost
    # packet is revived there: its key, map and row were never cleared
    assert r1["slot_key"][s_u] == new[-1][0] and r1["a_slot"][len(new) - 1] == s_u
    assert r1["a_cnt"][AS.OPENED] >= n_new
    assert r1["st"][s_u] == R.REVIVED and r1["olen"][s_u] == new_want[-1].size
    assert np.array_equal(r1["out"][s_u * STRIDE:s_u * STRIDE + new_want[-1].size], new_want[-1])

    # ---- turn 3: two new groups on a connection that holds two, max_groups 2
    h2 = turns[2]
    arriving = {}
    for key in h2["a_key"][:h2["m"]]:
        c, x = conn_num(key)
        if x >= marks[c]:
            arriving.setdefault(c, set()).add(x)
    open_now = {}
    for s in np.flatnonzero(state.acc_len[:n_slots]):
        c, x = conn_num(state.slot_key[s])
        open_now.setdefault(c, {})[x] = int(s)
    c_full = next(c for c in sorted(open_now) if c in arriving and c < 150 and
                  len(set(open_now[c]) | arriving[c]) == 2)
    extra, extra_want = [], []
    for j in range(2):
        recs, want = fresh_group(rng, np.uint64((c_full << SHIFT) | (5000 + 3 * j)))
        extra += recs
        extra_want.append(want)
    h2 = extended(h2, extra)
    before = marks.copy()
    r2 = rule_turn(state, h2, marks, [], 2, True)
    check_turn(2, dev.turn(h2, [], 2, True), r2, True, state, dev, marks)
    assert np.flatnonzero(marks != before).tolist() == [c_full] and marks[c_full] == 5000
    n_closed = int(r2["r_cnt"][RR.CLOSED])
    assert sorted(r2["closed"][:n_closed].tolist()) == sorted(open_now[c_full].values())
    old = np.flatnonzero([conn_num(k)[0] == c_full and conn_num(k)[1] < 5000
                          for k in h2["a_key"][:h2["m"]]])
    # (late packets of the two groups turn 2 raised a mark past are refused too)
    below = [conn_num(k)[1] < marks[conn_num(k)[0]] for k in h2["a_key"][:h2["m"]]]
    assert old.size > 0 and np.all(np.array(below)[old]) and r2["r_cnt"][RR.REFUSED] == sum(below)
    assert np.all(r2["key_out"][old] == NK) and np.all(r2["a_slot"][old] == AS.NO_SLOT)
    for j in range(2):  # the survivors
        key = np.uint64((c_full << SHIFT) | (5000 + 3 * j))
        s = int(r2["a_slot"][h2["m"] - len(extra) + [r[0] for r in extra].index(key)])
        assert r2["slot_key"][s] == key and r2["st"][s] == R.REVIVED
        assert np.array_equal(r2["out"][s * STRIDE:s * STRIDE + extra_want[j].size], extra_want[j])
