"""The receiver's turn end to end on the GPU: qfec_null_decrypt_batch opens the
arrivals, qfec_admit_ragged filters them with the open call's ok flags and the
per-slot maps, qfec_accumulate_ragged folds what was admitted and
qfec_revive_tracked closes -- three turns queued on one stream with ONE
qfec_sync at the very end.  About 300 arena groups (k 5-15, 64-1350 B); some
arrivals are corrupted on the wire, some duplicated within a turn, some across
turns; in the third turn new groups take slots the first two turns released,
with no map clearing.
"""
import numpy as np
import pytest
import torch

import accumulate_rule as AR
import admit_rule as R
from oracle import oracle_c as OC
from libquic_amd import qfec
from test_admit_rule import make_groups, scenario
from test_hip_accumulate_ragged import dview

gpu = pytest.mark.gpu
DEV = "cuda:0"
POISON, PAD = 0xA5, 0x5A
STRIDE, MS, AD, TAG = 1536, 2, 8, 12


def host(t, dtype):
    return t.cpu().numpy().view(dtype)


class Wire:
    """One turn on the wire: per candidate an 8-byte header (the associated
    data) and the NULL-protected payload; a candidate that is not `good` has a
    payload byte flipped after protection.  plain: where the open call puts
    the plaintexts (16-B aligned, PAD elsewhere), with the clean bytes of the
    verified candidates -- what the rule folds."""

    def __init__(self, rng, per_group):
        flat = [c for g in per_group for c in g]
        self.n, self.m = len(per_group), len(flat)
        m = self.m
        self.ptr = np.zeros(self.n + 1, np.uint32)
        self.ptr[1:] = np.cumsum([len(g) for g in per_group])
        self.idx = np.array([c[0] for c in flat] + [0], np.uint8)
        self.ln = np.array([c[1].size for c in flat] + [0], np.uint16)
        self.good = np.array([c[2] for c in flat] + [0], np.uint8)
        sizes = self.ln[:m].astype(np.int64)
        self.ad_off = np.zeros(m + 1, np.uint64)
        self.ad_off[:m] = np.cumsum(np.append(0, (sizes + AD + TAG)[:-1]))
        self.ad_len = np.full(m + 1, AD, np.uint16)
        self.ct_off = self.ad_off + np.uint64(AD)
        self.ct_len = (self.ln + np.uint16(TAG)).astype(np.uint16)
        self.pt_off = np.zeros(m + 1, np.uint64)
        self.pt_off[:m] = np.cumsum(np.append(0, ((sizes + 15) // 16 * 16)[:-1]))
        total = int(self.pt_off[m - 1]) + int(sizes[-1]) + 32
        self.plain = np.full(total, PAD, np.uint8)
        src = np.zeros(int(self.ad_off[m - 1]) + int(sizes[-1]) + AD + TAG + 32, np.uint8)
        for p, (i, b, good) in enumerate(flat):
            src[int(self.ad_off[p]):int(self.ad_off[p]) + AD] = rng.integers(0, 256, AD)
            src[int(self.ad_off[p]) + AD:int(self.ad_off[p]) + AD + b.size] = b
            if good:
                self.plain[int(self.pt_off[p]):int(self.pt_off[p]) + b.size] = b
        self.wire = OC.null_encrypt_batch(src, self.ad_off[:m], self.ad_len[:m],
                                          (self.ad_off[:m] + np.uint64(AD)), self.ln[:m],
                                          self.ct_off[:m], src.size, out=src.copy())
        for p in np.flatnonzero(self.good[:m] == 0):
            self.wire[int(self.ct_off[p]) + TAG + int(rng.integers(0, self.ln[p]))] ^= 0x40
        _, ok = OC.null_decrypt_batch(self.wire, self.ad_off[:m], self.ad_len[:m], self.ct_off[:m],
                                      self.ct_len[:m], self.pt_off[:m], total)
        assert np.array_equal(ok, self.good[:m])  # (the corruption is what fails)


@gpu
def test_three_turns_one_sync(ctx):
    rng = np.random.default_rng(3000)
    n, n_slots, n_quiet = 300, 330, 80
    groups = make_groups(rng, n)
    cands, kind, lost, verified, dup = scenario(rng, groups, quiet_last=set(range(n_quiet)))
    slot = rng.permutation(n_slots)[:n].astype(np.uint32)
    acc = np.full(n_slots * STRIDE + 32, POISON, np.uint8)
    acc[:n_slots * STRIDE] = rng.integers(0, 256, n_slots * STRIDE, dtype=np.uint8)
    acc_len = np.zeros(n_slots, np.uint16)
    maps = np.full((n_slots + 1, MS), 0xFF, np.uint8)  # stale: all ones
    slot_k = np.full(n_slots, POISON, np.uint8)
    slot_k[slot] = [len(g) - 1 for g in groups]
    d_acc, d_len, d_maps = dview(acc), dview(acc_len), dview(maps)
    out_off = np.arange(n, dtype=np.uint64) * np.uint64(STRIDE)
    d_out_off = dview(out_off)
    turn_groups, turn_slot = list(groups), slot
    keep, results = [], []
    for t in range(3):
        per_group = cands[t]
        if t == 2:
            # new groups in slots the first two turns released; their old owners
            # (quiet since turn 1) leave the batch.  The host learns of the
            # releases from the rule here; a receiver would from an earlier sync.
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
        # the rules on the host
        r_ptr, r_off, r_ln = (np.full(n + 1, POISON, np.uint32), np.zeros(m + 1, np.uint64),
                              np.zeros(m + 1, np.uint16))
        r_v = np.full(m + 1, POISON, np.uint8)
        errs, r_cnt = R.admit(w.pt_off, w.ln, w.idx, w.good, w.ptr, slot_k, maps[:n_slots],
                              acc_len, STRIDE, r_ptr, r_off, r_ln, r_v, turn_slot)
        assert not errs.any()
        assert not AR.accumulate(w.plain, r_off, r_ln, r_ptr, acc, STRIDE, acc_len,
                                 turn_slot).any()
        r_out = np.full(n * STRIDE + 32, PAD, np.uint8)
        r_olen, r_st, r_idx = (np.zeros(n, np.uint16), np.zeros(n, np.uint8),
                               np.zeros(n, np.uint8))
        errs, r_list, r_counts = R.revive_tracked(acc, STRIDE, acc_len, maps[:n_slots], slot_k, n,
                                                  r_out, out_off, r_olen, r_st, r_idx, turn_slot,
                                                  0b011)
        assert not errs.any()
        # the same turn queued on the device
        d = dict(wire=dview(w.wire), ad_off=dview(w.ad_off), ad_len=dview(w.ad_len),
                 ct_off=dview(w.ct_off), ct_len=dview(w.ct_len), pt_off=dview(w.pt_off),
                 ln=dview(w.ln), idx=dview(w.idx), ptr=dview(w.ptr), slot=dview(turn_slot),
                 slot_k=dview(slot_k),
                 plain=torch.full((w.plain.size,), PAD, dtype=torch.uint8, device=DEV),
                 ok=dview(np.full(m + 1, POISON, np.uint8)),
                 o_ptr=dview(np.zeros(n + 1, np.uint32)), o_off=dview(np.zeros(m + 1, np.uint64)),
                 o_ln=dview(np.zeros(m + 1, np.uint16)),
                 v=dview(np.full(m + 1, POISON, np.uint8)), cnt=dview(np.zeros(4, np.uint64)),
                 out=torch.full((n * STRIDE + 32,), PAD, dtype=torch.uint8, device=DEV),
                 olen=dview(np.full(n, 0xA5A5, np.uint16)), st=dview(np.full(n, POISON, np.uint8)),
                 ridx=dview(np.full(n, POISON, np.uint8)), counts=dview(np.zeros(3, np.uint64)))
        ctx.null_decrypt(d["wire"], d["ad_off"], d["ad_len"], d["ct_off"], d["ct_len"], m,
                         d["plain"], d["pt_off"], d["ok"])
        ctx.admit_ragged(d["pt_off"], d["ln"], d["idx"], d["ok"], d["ptr"], n, d["slot_k"], d_maps,
                         MS, d_len, STRIDE, d["o_ptr"], d["o_off"], d["o_ln"], d["v"],
                         slot=d["slot"], n_slots=n_slots, counts=d["cnt"])
        ctx.accumulate_ragged(d["plain"], d["o_off"], d["o_ln"], d["o_ptr"], n, d_acc, STRIDE,
                              d_len, slot=d["slot"], n_slots=n_slots)
        ctx.revive_tracked(d_acc, STRIDE, d_len, d_maps, MS, d["slot_k"], n, d["out"], d_out_off,
                           d["olen"], status=d["st"], slot=d["slot"], n_slots=n_slots,
                           revived_idx=d["ridx"], counts=d["counts"], release_mask=0b011)
        keep.append(d)
        results.append(dict(w=w, v=r_v, cnt=r_cnt, st=r_st.copy(), idx=r_idx.copy(),
                            olen=r_olen.copy(), out=r_out, counts=r_counts, groups=turn_groups,
                            slot=turn_slot.copy(), len_after=acc_len.copy()))
    ctx.sync()  # the only one
    revived_total = 0
    for t, (d, r) in enumerate(zip(keep, results)):
        w = r["w"]
        assert np.array_equal(host(d["ok"], np.uint8)[:w.m], w.good[:w.m]), t
        assert np.array_equal(host(d["v"], np.uint8), r["v"]), t
        assert host(d["cnt"], np.uint64).tolist() == r["cnt"].tolist()
        assert np.array_equal(host(d["st"], np.uint8), r["st"]), t
        assert np.array_equal(host(d["ridx"], np.uint8), r["idx"]), t
        assert np.array_equal(host(d["olen"], np.uint16), r["olen"]), t
        assert host(d["counts"], np.uint64).tolist() == r["counts"].tolist()
        assert np.array_equal(host(d["out"], np.uint8), r["out"]), t
        # the revived packets are qfec_recover_ragged's from the clean payloads
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
        rec = torch.full((rev.size * STRIDE,), PAD, dtype=torch.uint8, device=DEV)
        ctx.recover_ragged(dview(data), dview(off), dview(ln), dview(ptr), rev.size, dview(par),
                           dview(poff), dview(plen), dview(r["idx"][rev]), rec, dview(poff))
        ctx.sync()
        rec, got = host(rec, np.uint8), host(d["out"], np.uint8)
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
