"""The receiver's turn from group KEYS alone, end to end on the GPU:
qfec_null_decrypt_batch opens the turn's packets in arrival order,
qfec_assign_slots finds or opens every packet's group, qfec_bin_arrivals bins
the records by the slots it wrote, qfec_admit_ragged filters the binned tables
in lockstep with the slots, qfec_accumulate_ragged folds what was admitted and
qfec_revive_tracked closes every slot -- three turns queued on one stream with
ONE qfec_sync at the very end.  The turns are test_hip_bin_turn.py's
(tests/assign_turns.py builds them): the host knows no slot, keeps no free
list and clears nothing.  In the third turn new keys take slots the first two
turns released; a late duplicate of a released group opens it again under its
key, which is the policy the host is told to filter with QFEC_NO_KEY.
Everything equals the rules chained: assign_rule -> bin_rule -> admit_rule ->
accumulate_rule -> admit_rule.revive_tracked.

The close runs over all slots in lockstep (slot == NULL): a free slot is a
fresh group, UNREVIVABLE and not released, so every slot keeps a legal K.
"""
import numpy as np
import pytest
import torch

import admit_rule as R
import assign_rule as AS
import assign_turns as T
from libquic_amd import qfec
from test_hip_accumulate_ragged import dview
from test_hip_tracked_turn import MS, PAD, POISON, STRIDE, host

gpu = pytest.mark.gpu
DEV = "cuda:0"


@gpu
def test_three_turns_from_keys_one_sync(ctx):
    turns = T.host_turns(3300)
    state = T.KeyState(3301)
    n_slots = state.n_slots
    d_acc, d_len, d_maps = dview(state.acc), dview(state.acc_len), dview(state.maps)
    d_key, d_k, d_out_off = dview(state.slot_key), dview(state.slot_k), dview(state.out_off)
    keep, results = [], []
    for t, h in enumerate(turns):
        w, m = h["w"], h["m"]
        r = T.key_turn(state, h)
        assert r["a_cnt"][AS.AWAY] == 0
        d = dict(wire=dview(w.wire), ad_off=dview(h["a_ad_off"]), ad_len=dview(w.ad_len),
                 ct_off=dview(h["a_ct_off"]), ct_len=dview(h["a_ct_len"]),
                 pt_off=dview(h["a_pt_off"]), ln=dview(h["a_ln"]), idx=dview(h["a_idx"]),
                 key=dview(h["a_key"]), k=dview(h["a_k"]),
                 plain=torch.full((w.plain.size,), PAD, dtype=torch.uint8, device=DEV),
                 ok=dview(np.full(m + 1, POISON, np.uint8)),
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
                 olen=dview(np.full(n_slots, 0xA5A5, np.uint16)),
                 st=dview(np.full(n_slots, POISON, np.uint8)),
                 ridx=dview(np.full(n_slots, POISON, np.uint8)),
                 rlist=dview(np.full(n_slots, 0xA5A5A5A5A5A5A5A5, np.uint64)),
                 counts=dview(np.zeros(3, np.uint64)),
                 # (read back at the end: what the slot tables held after this turn's assign)
                 key_after=torch.empty(n_slots + 1, dtype=torch.int64, device=DEV),
                 k_after=torch.empty(n_slots + 1, dtype=torch.uint8, device=DEV))
        ctx.null_decrypt(d["wire"], d["ad_off"], d["ad_len"], d["ct_off"], d["ct_len"], m,
                         d["plain"], d["pt_off"], d["ok"])
        ctx.assign_slots(d["key"], d["k"], m, d_key, d_k, d_len, n_slots, d["a_slot"],
                         counts=d["a_cnt"])
        d["key_after"].copy_(d_key)  # (device to device on the same stream: no sync)
        d["k_after"].copy_(d_k)
        ctx.bin_arrivals(d["a_slot"], d["pt_off"], d["ln"], d["idx"], d["ok"], m, n_slots,
                         d["t_ptr"], d["t_off"], d["t_ln"], d["t_idx"], pkt_ok_out=d["t_ok"],
                         src_out=d["t_src"], counts=d["b_cnt"])
        ctx.admit_ragged(d["t_off"], d["t_ln"], d["t_idx"], d["t_ok"], d["t_ptr"], n_slots,
                         d_k, d_maps, MS, d_len, STRIDE, d["o_ptr"], d["o_off"], d["o_ln"],
                         d["v"], slot=None, n_slots=n_slots, counts=d["cnt"])
        ctx.accumulate_ragged(d["plain"], d["o_off"], d["o_ln"], d["o_ptr"], n_slots, d_acc,
                              STRIDE, d_len, slot=None, n_slots=n_slots)
        ctx.revive_tracked(d_acc, STRIDE, d_len, d_maps, MS, d_k, n_slots, d["out"], d_out_off,
                           d["olen"], status=d["st"], slot=None, n_slots=n_slots,
                           revived_idx=d["ridx"], revived_list=d["rlist"], counts=d["counts"],
                           release_mask=T.MASK)
        keep.append(d)
        results.append(r)
    ctx.sync()  # the only one
    revived = reopened = 0
    released = set()
    for t, (d, r, h) in enumerate(zip(keep, results, turns)):
        m = h["m"]
        assert np.array_equal(host(d["ok"], np.uint8)[:m], h["a_good"][:m]), t
        for key, dt in (("a_slot", np.uint32), ("t_ptr", np.uint32), ("t_off", np.uint64),
                        ("t_ln", np.uint16), ("t_idx", np.uint8), ("t_ok", np.uint8),
                        ("t_src", np.uint32), ("o_ptr", np.uint32), ("v", np.uint8),
                        ("st", np.uint8), ("ridx", np.uint8), ("olen", np.uint16),
                        ("out", np.uint8)):
            assert np.array_equal(host(d[key], dt), r[key]), (t, key)
        assert np.array_equal(host(d["key_after"], np.uint64), r["slot_key"]), t
        assert np.array_equal(host(d["k_after"], np.uint8), r["slot_k"]), t
        for key in ("a_cnt", "b_cnt", "cnt", "counts"):
            assert host(d[key], np.uint64).tolist() == r[key].tolist(), (t, key)
        nrev = int(r["counts"][R.REVIVED])
        assert np.array_equal(host(d["rlist"], np.uint64)[:nrev], r["rlist"]), t
        # what happened to whom, by key
        open_now = np.flatnonzero(r["len_pre"])
        for s in open_now:
            key = int(r["slot_key"][s])
            reopened += key in released
            if r["st"][s] != R.UNREVIVABLE:
                released.add(key)
        revived += nrev
        assert not r["len_after"][:n_slots][r["st"] != R.UNREVIVABLE].any()
    assert revived >= 60 and reopened >= 1
    # the third turn's new keys sit in slots the first two turns released, and
    # are revived there: no key, map or row was ever cleared
    last, r = turns[2], results[2]
    new_keys = {int(T.key_of(int(g))) for g in last["gid"][-10:]}
    took = sorted({int(s) for s, k in zip(r["a_slot"][:last["m"]], last["a_key"])
                   if int(k) in new_keys})
    assert len(took) == 10 and np.all(r["st"][took] == R.REVIVED)
    assert all(results[0]["len_pre"][s] or results[1]["len_pre"][s] for s in took)
    assert np.array_equal(host(d_len, np.uint16), state.acc_len)
    assert np.array_equal(host(d_maps, np.uint8).ravel(), state.maps.ravel())
    assert np.array_equal(host(d_acc, np.uint8), state.acc)
    assert np.array_equal(host(d_key, np.uint64), state.slot_key)
    assert np.array_equal(host(d_k, np.uint8), state.slot_k)
