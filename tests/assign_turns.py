"""Three receiver turns in arrival order, for test_assign_rule.py and
test_hip_assign_turn.py: the scenario and the wire of test_hip_bin_turn.py
(about 300 arena groups; arrivals corrupted on the wire, duplicated within a
turn and across turns; in the third turn new groups arrive after the first two
turns released slots), built once with the slots the HOST assigned, as that
test does, and then run again from the packets' group KEYS alone through the
rules chained: assign_rule -> bin_rule -> admit_rule -> accumulate_rule ->
admit_rule.revive_tracked.  Not a test module.
"""
import numpy as np

import accumulate_rule as AR
import admit_rule as R
import assign_rule as AS
import bin_rule as B
from test_admit_rule import make_groups, scenario
from test_hip_tracked_turn import MS, PAD, POISON, STRIDE, Wire

N, N_SLOTS, N_QUIET = 300, 330, 80
MASK = 0b011  # COMPLETE and REVIVED release their slot


def key_of(gid):
    """connection index << 40 | group number, as include/qfec.h suggests"""
    return np.uint64(((gid % 11) << 40) | (1000 + 3 * gid))


def host_turns(seed):
    """The three turns with host-assigned slots.  Per turn a dict: w (the
    Wire), m, the arrival-order tables a_* (one trailing entry nobody owns;
    a_key and a_k are what the key-driven turn gets instead of a_slot), gid and
    K per group of the turn, and what the close said per group: st, ridx, olen,
    out (group j at j * STRIDE), len_pre (the row lengths in front of the
    close, by group)."""
    rng = np.random.default_rng(seed)
    n, n_slots = N, N_SLOTS
    groups = make_groups(rng, n)
    cands, _, _, _, _ = scenario(rng, groups, quiet_last=set(range(N_QUIET)))
    slot = rng.permutation(n_slots)[:n].astype(np.uint32)
    acc = rng.integers(0, 256, n_slots * STRIDE + 32, dtype=np.uint8)
    acc_len = np.zeros(n_slots, np.uint16)
    maps = np.full((n_slots, MS), 0xFF, np.uint8)
    slot_k = np.full(n_slots, 1, np.uint8)
    slot_k[slot] = [len(g) - 1 for g in groups]
    out_off = np.arange(n, dtype=np.uint64) * np.uint64(STRIDE)
    turn_groups, turn_slot, turn_gid = list(groups), slot, np.arange(n)
    turns = []
    for t in range(3):
        per_group = cands[t]
        if t == 2:
            gone = [g for g in range(N_QUIET) if acc_len[slot[g]] == 0][:20]
            assert len(gone) >= 10
            fresh = make_groups(rng, len(gone))
            stay = [g for g in range(n) if g not in gone]
            turn_groups = [groups[g] for g in stay] + fresh
            turn_slot = np.concatenate([slot[stay], slot[gone]]).astype(np.uint32)
            turn_gid = np.concatenate([stay, n + np.arange(len(gone))])
            per_group = [cands[2][g] for g in stay]
            for f in fresh:  # everything but one data packet, at once
                lost = int(rng.integers(0, len(f) - 1))
                per_group.append([(int(i), f[int(i)], True) for i in rng.permutation(len(f))
                                  if i != lost])
            slot_k = slot_k.copy()
            slot_k[slot[gone]] = [len(f) - 1 for f in fresh]
        w = Wire(rng, per_group)
        m = w.m
        perm = rng.permutation(m)
        grp_of = np.repeat(np.arange(len(per_group)), np.diff(w.ptr).astype(np.int64))[perm]

        def arr(x):  # a per-candidate table in arrival order, its trailing entry kept
            return np.append(x[:m][perm], x[m:m + 1])

        k_of = np.array([len(g) - 1 for g in turn_groups], np.uint8)
        d = dict(w=w, m=m, gid=turn_gid.copy(), k=k_of,
                 a_slot=np.append(turn_slot[grp_of], np.uint32(0)).astype(np.uint32),
                 a_key=np.append([key_of(int(turn_gid[g])) for g in grp_of],
                                 np.uint64(0)).astype(np.uint64),
                 a_k=np.append(k_of[grp_of], np.uint8(0)).astype(np.uint8),
                 a_ad_off=arr(w.ad_off), a_ct_off=arr(w.ct_off), a_ct_len=arr(w.ct_len),
                 a_pt_off=arr(w.pt_off), a_ln=arr(w.ln), a_idx=arr(w.idx), a_good=arr(w.good))
        t_ptr = np.zeros(n_slots + 1, np.uint32)
        t_off, t_ln = np.zeros(m + 1, np.uint64), np.zeros(m + 1, np.uint16)
        t_idx, t_ok = np.zeros(m + 1, np.uint8), np.zeros(m + 1, np.uint8)
        errs, _ = B.bin_arrivals(d["a_slot"][:m], d["a_pt_off"], d["a_ln"], d["a_idx"], d["a_good"],
                                 n_slots, t_ptr, t_off, t_ln, t_idx, t_ok)
        assert not errs.any()
        r_ptr, r_off, r_ln = (np.zeros(n_slots + 1, np.uint32), np.zeros(m + 1, np.uint64),
                              np.zeros(m + 1, np.uint16))
        errs, _ = R.admit(t_off, t_ln, t_idx, t_ok, t_ptr, slot_k, maps, acc_len, STRIDE, r_ptr,
                          r_off, r_ln, np.zeros(m + 1, np.uint8), None)
        assert not errs.any()
        assert not AR.accumulate(w.plain, r_off, r_ln, r_ptr, acc, STRIDE, acc_len, None).any()
        d["len_pre"] = acc_len[turn_slot].copy()
        d["out"] = np.full(n * STRIDE + 32, PAD, np.uint8)
        d["olen"], d["st"], d["ridx"] = (np.zeros(n, np.uint16), np.zeros(n, np.uint8),
                                         np.zeros(n, np.uint8))
        errs, _, _ = R.revive_tracked(acc, STRIDE, acc_len, maps, slot_k, n, d["out"], out_off,
                                      d["olen"], d["st"], d["ridx"], turn_slot, MASK)
        assert not errs.any()
        turns.append(d)
    return turns


class KeyState:
    """What the key-driven receiver keeps between turns, as the tests start
    it: every slot free with a stale key, a stale map and a garbage row, and a
    legal K (the admit judges every slot of the lockstep tables)."""

    def __init__(self, seed, n_slots=N_SLOTS):
        rng = np.random.default_rng(seed)
        self.n_slots = n_slots
        self.acc = np.full(n_slots * STRIDE + 32, POISON, np.uint8)
        self.acc[:n_slots * STRIDE] = rng.integers(0, 256, n_slots * STRIDE, dtype=np.uint8)
        self.acc_len = np.zeros(n_slots + 1, np.uint16)
        self.maps = np.full((n_slots + 1, MS), 0xFF, np.uint8)
        self.slot_k = np.full(n_slots + 1, 1, np.uint8)
        # stale keys: those of the first groups to arrive, in slots that are free
        self.slot_key = np.array([key_of(g) for g in range(n_slots + 1)], np.uint64)
        self.out_off = np.arange(n_slots, dtype=np.uint64) * np.uint64(STRIDE)


def key_turn(state, d):
    """One turn from keys alone on host arrays, the rules chained; state is
    modified in place.  Returns every table the device produces, by name."""
    n_slots, m = state.n_slots, d["m"]
    r = dict(a_slot=np.full(m + 1, POISON, np.uint32))
    r["a_cnt"] = AS.assign_slots(d["a_key"][:m], d["a_k"], state.slot_key[:n_slots],
                                 state.slot_k[:n_slots], state.acc_len[:n_slots], r["a_slot"])
    r["slot_key"], r["slot_k"] = state.slot_key.copy(), state.slot_k.copy()
    r["t_ptr"] = np.full(n_slots + 1, POISON, np.uint32)
    r["t_off"], r["t_ln"] = np.full(m + 1, POISON, np.uint64), np.full(m + 1, POISON, np.uint16)
    r["t_idx"], r["t_ok"] = np.full(m + 1, POISON, np.uint8), np.full(m + 1, POISON, np.uint8)
    r["t_src"] = np.full(m + 1, POISON, np.uint32)
    errs, r["b_cnt"] = B.bin_arrivals(r["a_slot"][:m], d["a_pt_off"], d["a_ln"], d["a_idx"],
                                      d["a_good"], n_slots, r["t_ptr"], r["t_off"], r["t_ln"],
                                      r["t_idx"], r["t_ok"], r["t_src"])
    assert not errs.any()
    r["o_ptr"] = np.full(n_slots + 1, POISON, np.uint32)
    r["o_off"], r["o_ln"] = np.zeros(m + 1, np.uint64), np.zeros(m + 1, np.uint16)
    r["v"] = np.full(m + 1, POISON, np.uint8)
    errs, r["cnt"] = R.admit(r["t_off"], r["t_ln"], r["t_idx"], r["t_ok"], r["t_ptr"],
                             state.slot_k[:n_slots], state.maps[:n_slots], state.acc_len[:n_slots],
                             STRIDE, r["o_ptr"], r["o_off"], r["o_ln"], r["v"], None)
    assert not errs.any()
    assert not AR.accumulate(d["w"].plain, r["o_off"], r["o_ln"], r["o_ptr"], state.acc, STRIDE,
                             state.acc_len[:n_slots], None).any()
    r["len_pre"] = state.acc_len[:n_slots].copy()
    r["out"] = np.full(n_slots * STRIDE + 32, PAD, np.uint8)
    r["olen"], r["st"], r["ridx"] = (np.zeros(n_slots, np.uint16), np.zeros(n_slots, np.uint8),
                                     np.zeros(n_slots, np.uint8))
    errs, r["rlist"], r["counts"] = R.revive_tracked(
        state.acc, STRIDE, state.acc_len[:n_slots], state.maps[:n_slots], state.slot_k[:n_slots],
        n_slots, r["out"], state.out_off, r["olen"], r["st"], r["ridx"], None, MASK)
    assert not errs.any()
    r["len_after"] = state.acc_len.copy()
    return r
