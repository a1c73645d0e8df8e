"""The receiver's turn from ARRIVAL order, end to end on the GPU:
qfec_null_decrypt_batch opens the turn's packets as the sockets delivered them,
qfec_bin_arrivals bins the per-packet records by slot, qfec_admit_ragged
filters the binned tables in lockstep with the slots (slot == NULL, n_groups ==
n_slots), qfec_accumulate_ragged folds what was admitted and
qfec_revive_tracked closes -- three turns queued on one stream with ONE
qfec_sync at the very end.  The scenario and the wire are those of
test_hip_tracked_turn.py (about 300 arena groups; arrivals corrupted on the
wire, duplicated within a turn and across turns; in the third turn new groups
take slots the first two turns released, with no map clearing); each turn's
candidates are shuffled, so which copy of a duplicate comes first is decided by
the arrival order.  Everything equals the NumPy rules chained: bin_rule ->
admit_rule -> accumulate_rule -> admit_rule.revive_tracked.

A slot no group holds still has a group in the lockstep tables, an empty one:
the admit judges its slot_k like any other, so unnamed slots carry a legal K.
"""
import numpy as np
import pytest
import torch

import accumulate_rule as AR
import admit_rule as R
import bin_rule as B
from oracle import oracle_c as OC
from libquic_amd import qfec
from test_admit_rule import make_groups, scenario
from test_hip_accumulate_ragged import dview
from test_hip_tracked_turn import AD, MS, PAD, POISON, STRIDE, Wire, host

gpu = pytest.mark.gpu
DEV = "cuda:0"


@gpu
def test_three_turns_from_arrival_order_one_sync(ctx):
    rng = np.random.default_rng(3100)
    n, n_slots, n_quiet = 300, 330, 80
    groups = make_groups(rng, n)
    cands, kind, lost, verified, dup = scenario(rng, groups, quiet_last=set(range(n_quiet)))
    slot = rng.permutation(n_slots)[:n].astype(np.uint32)
    acc = np.full(n_slots * STRIDE + 32, POISON, np.uint8)
    acc[:n_slots * STRIDE] = rng.integers(0, 256, n_slots * STRIDE, dtype=np.uint8)
    acc_len = np.zeros(n_slots, np.uint16)
    maps = np.full((n_slots + 1, MS), 0xFF, np.uint8)  # stale: all ones
    slot_k = np.full(n_slots, 1, np.uint8)  # (unnamed slots: a legal K, never a candidate)
    slot_k[slot] = [len(g) - 1 for g in groups]
    d_acc, d_len, d_maps = dview(acc), dview(acc_len), dview(maps)
    out_off = np.arange(n, dtype=np.uint64) * np.uint64(STRIDE)
    d_out_off = dview(out_off)
    turn_groups, turn_slot = list(groups), slot
    keep, results = [], []
    for t in range(3):
        per_group = cands[t]
        if t == 2:
            # new groups in slots the first two turns released (see test_hip_tracked_turn.py)
            gone = [g for g in range(n_quiet) if acc_len[slot[g]] == 0][:20]
            assert len(gone) >= 10
            fresh = make_groups(rng, len(gone))
            stay = [g for g in range(n) if g not in gone]
            turn_groups = [groups[g] for g in stay] + fresh
            turn_slot = np.concatenate([slot[stay], slot[gone]]).astype(np.uint32)
            per_group = [cands[2][g] for g in stay]
            fresh_lost = [int(rng.integers(0, len(f) - 1)) for f in fresh]
            for f, m in zip(fresh, fresh_lost):  # everything but one data packet, at once
                per_group.append([(int(i), f[int(i)], True) for i in rng.permutation(len(f))
                                  if i != m])
            slot_k = slot_k.copy()
            slot_k[slot[gone]] = [len(f) - 1 for f in fresh]
        w = Wire(rng, per_group)
        m = w.m
        # arrival order: the turn's packets shuffled; the wire image stays as it is
        perm = rng.permutation(m)
        grp_of = np.repeat(np.arange(len(per_group)), np.diff(w.ptr).astype(np.int64))

        def arr(x):  # a per-candidate table in arrival order, its trailing entry kept
            return np.append(x[:m][perm], x[m:m + 1])

        a_slot = np.append(turn_slot[grp_of][perm], np.uint32(0)).astype(np.uint32)
        a_ad_off, a_ct_off, a_ct_len, a_pt_off = (arr(w.ad_off), arr(w.ct_off), arr(w.ct_len),
                                                  arr(w.pt_off))
        a_ln, a_idx, a_good = arr(w.ln), arr(w.idx), arr(w.good)
        # the rules on the host, chained
        t_ptr = np.full(n_slots + 1, POISON, np.uint32)
        t_off, t_ln = np.full(m + 1, POISON, np.uint64), np.full(m + 1, POISON, np.uint16)
        t_idx, t_ok = np.full(m + 1, POISON, np.uint8), np.full(m + 1, POISON, np.uint8)
        t_src = np.full(m + 1, POISON, np.uint32)
        errs, b_cnt = B.bin_arrivals(a_slot[:m], a_pt_off, a_ln, a_idx, a_good, n_slots, t_ptr,
                                     t_off, t_ln, t_idx, t_ok, t_src)
        assert not errs.any() and b_cnt.tolist() == [m, 0, 0]
        r_ptr, r_off, r_ln = (np.full(n_slots + 1, POISON, np.uint32), np.zeros(m + 1, np.uint64),
                              np.zeros(m + 1, np.uint16))
        r_v = np.full(m + 1, POISON, np.uint8)
        errs, r_cnt = R.admit(t_off, t_ln, t_idx, t_ok, t_ptr, slot_k, maps[:n_slots], acc_len,
                              STRIDE, r_ptr, r_off, r_ln, r_v, None)
        assert not errs.any()
        assert not AR.accumulate(w.plain, r_off, r_ln, r_ptr, acc, STRIDE, acc_len, None).any()
        r_out = np.full(n * STRIDE + 32, PAD, np.uint8)
        r_olen, r_st, r_idx = (np.zeros(n, np.uint16), np.zeros(n, np.uint8),
                               np.zeros(n, np.uint8))
        errs, r_list, r_counts = R.revive_tracked(acc, STRIDE, acc_len, maps[:n_slots], slot_k, n,
                                                  r_out, out_off, r_olen, r_st, r_idx, turn_slot,
                                                  0b011)
        assert not errs.any()
        # the same turn queued on the device
        d = dict(wire=dview(w.wire), ad_off=dview(a_ad_off), ad_len=dview(w.ad_len),
                 ct_off=dview(a_ct_off), ct_len=dview(a_ct_len), pt_off=dview(a_pt_off),
                 ln=dview(a_ln), idx=dview(a_idx), a_slot=dview(a_slot), slot=dview(turn_slot),
                 slot_k=dview(slot_k),
                 plain=torch.full((w.plain.size,), PAD, dtype=torch.uint8, device=DEV),
                 ok=dview(np.full(m + 1, POISON, np.uint8)),
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
                 out=torch.full((n * STRIDE + 32,), PAD, dtype=torch.uint8, device=DEV),
                 olen=dview(np.full(n, 0xA5A5, np.uint16)), st=dview(np.full(n, POISON, np.uint8)),
                 ridx=dview(np.full(n, POISON, np.uint8)),
                 rlist=dview(np.full(n, 0xA5A5A5A5A5A5A5A5, np.uint64)),
                 counts=dview(np.zeros(3, np.uint64)))
        ctx.null_decrypt(d["wire"], d["ad_off"], d["ad_len"], d["ct_off"], d["ct_len"], m,
                         d["plain"], d["pt_off"], d["ok"])
        ctx.bin_arrivals(d["a_slot"], d["pt_off"], d["ln"], d["idx"], d["ok"], m, n_slots,
                         d["t_ptr"], d["t_off"], d["t_ln"], d["t_idx"], pkt_ok_out=d["t_ok"],
                         src_out=d["t_src"], counts=d["b_cnt"])
        ctx.admit_ragged(d["t_off"], d["t_ln"], d["t_idx"], d["t_ok"], d["t_ptr"], n_slots,
                         d["slot_k"], d_maps, MS, d_len, STRIDE, d["o_ptr"], d["o_off"], d["o_ln"],
                         d["v"], slot=None, n_slots=n_slots, counts=d["cnt"])
        ctx.accumulate_ragged(d["plain"], d["o_off"], d["o_ln"], d["o_ptr"], n_slots, d_acc,
                              STRIDE, d_len, slot=None, n_slots=n_slots)
        ctx.revive_tracked(d_acc, STRIDE, d_len, d_maps, MS, d["slot_k"], n, d["out"], d_out_off,
                           d["olen"], status=d["st"], slot=d["slot"], n_slots=n_slots,
                           revived_idx=d["ridx"], revived_list=d["rlist"], counts=d["counts"],
                           release_mask=0b011)
        keep.append(d)
        results.append(dict(w=w, m=m, good=a_good, t=(t_ptr, t_off, t_ln, t_idx, t_ok, t_src),
                            b_cnt=b_cnt, r_ptr=r_ptr, v=r_v, cnt=r_cnt, st=r_st.copy(),
                            idx=r_idx.copy(), olen=r_olen.copy(), out=r_out, rlist=r_list,
                            counts=r_counts, groups=turn_groups, slot=turn_slot.copy(),
                            len_after=acc_len.copy()))
    ctx.sync()  # the only one
    revived_total = 0
    for t, (d, r) in enumerate(zip(keep, results)):
        m = r["m"]
        assert np.array_equal(host(d["ok"], np.uint8)[:m], r["good"][:m]), t
        # the binned tables, whole buffers
        for key, dt, want in zip(("t_ptr", "t_off", "t_ln", "t_idx", "t_ok", "t_src"),
                                 (np.uint32, np.uint64, np.uint16, np.uint8, np.uint8, np.uint32),
                                 r["t"]):
            assert np.array_equal(host(d[key], dt), want), (t, key)
        assert host(d["b_cnt"], np.uint64).tolist() == r["b_cnt"].tolist()
        # the admit's verdicts, in table order and mapped back to the arrivals
        got_v, src = host(d["v"], np.uint8), host(d["t_src"], np.uint32)[:m]
        assert np.array_equal(got_v, r["v"]), t
        by_arrival, want_by_arrival = np.full(m, POISON, np.uint8), np.full(m, POISON, np.uint8)
        by_arrival[src] = got_v[:m]
        want_by_arrival[r["t"][5][:m]] = r["v"][:m]
        assert np.array_equal(by_arrival, want_by_arrival), t
        assert np.array_equal(by_arrival == R.FAILED, r["good"][:m] == 0), t
        assert np.array_equal(host(d["o_ptr"], np.uint32), r["r_ptr"]), t
        assert host(d["cnt"], np.uint64).tolist() == r["cnt"].tolist()
        # the close
        assert np.array_equal(host(d["st"], np.uint8), r["st"]), t
        assert np.array_equal(host(d["ridx"], np.uint8), r["idx"]), t
        assert np.array_equal(host(d["olen"], np.uint16), r["olen"]), t
        assert host(d["counts"], np.uint64).tolist() == r["counts"].tolist()
        nrev = int(r["counts"][R.REVIVED])
        assert np.array_equal(host(d["rlist"], np.uint64)[:nrev], r["rlist"]), t
        assert np.array_equal(host(d["out"], np.uint8), r["out"]), t
        # the revived packets are the oracle's recover over the groups' clean payloads
        rev = np.flatnonzero(r["st"] == R.REVIVED)
        revived_total += rev.size
        if rev.size == 0:
            continue
        full = [r["groups"][g] for g in rev]
        flat = [p for items in full for p in items[:-1]]
        ln = np.array([p.size for p in flat], np.uint16)
        off = np.zeros(ln.size, np.uint64)
        off[1:] = np.cumsum((ln[:-1].astype(np.int64) + 15) // 16 * 16)
        data = np.zeros(int(off[-1]) + int(ln[-1]) + 32, np.uint8)
        for o, p in zip(off, flat):
            data[int(o):int(o) + p.size] = p
        ptr = np.zeros(rev.size + 1, np.uint32)
        ptr[1:] = np.cumsum([len(items) - 1 for items in full])
        poff = np.arange(rev.size, dtype=np.uint64) * np.uint64(STRIDE)
        par = np.zeros(rev.size * STRIDE, np.uint8)
        for j, items in enumerate(full):
            par[j * STRIDE:j * STRIDE + items[-1].size] = items[-1]
        plen = np.array([items[-1].size for items in full], np.uint16)
        rc, rec = OC.recover_ragged(data, off, ln, ptr, par, poff, plen, r["idx"][rev], poff,
                                    rev.size * STRIDE)
        assert rc == 0
        got = host(d["out"], np.uint8)
        for j, g in enumerate(rev):
            assert r["olen"][g] == plen[j]
            assert np.array_equal(got[g * STRIDE:g * STRIDE + int(plen[j])],
                                  rec[j * STRIDE:j * STRIDE + int(plen[j])]), (t, g)
            lost_pkt = full[j][int(r["idx"][g])]
            assert np.array_equal(rec[j * STRIDE:j * STRIDE + lost_pkt.size], lost_pkt)
        # released slots are fresh again
        done = r["st"] != R.UNREVIVABLE
        assert not r["len_after"][r["slot"][done]].any()
    assert revived_total >= 60
    last = results[2]
    assert np.all(last["st"][-10:] == R.REVIVED)  # the reused slots, never cleared
    assert np.array_equal(host(d_len, np.uint16), acc_len)
    assert np.array_equal(host(d_maps, np.uint8).ravel(), maps.ravel())
    assert np.array_equal(host(d_acc, np.uint8), acc)
