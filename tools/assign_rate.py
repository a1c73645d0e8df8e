#!/usr/bin/env python3
"""qfec_assign_slots beside the bin and the fold it feeds and the host lookup it replaces.

One MI355X, the workload and protocol of tools/bin_rate.py: BASELINE configs[3]
in the payload arena's layout resident on the device, 2^20 groups, 2^20 slots,
k 5-15, 64-1350 B, about 10.5 M packets, every data packet a candidate of the
turn.  A record of this call is (pkt_key 8, pkt_k 1) in and (pkt_slot 4) out
per packet; group g's key is (g % 4096) << 40 | g // 4096 + 1.

  (a) assign alone, every group already open (group g in slot g), the arrival
      order a uniform random permutation;
  (b) the same, the arrivals already grouped (the identity order);
  (c) assign alone, every group new, all slots free (their keys stale), random
      order: 2^20 groups opened per call;
  (d) assign alone, a sparse turn: the packets of 1% of the groups, all open,
      random order;
  (e) the yardsticks in the same process on the same inputs: qfec_bin_arrivals
      on (a)'s slots, and qfec_accumulate_ragged alone over host-built tables;
  (f) the turn from keys, every group new: assign + bin + admit + accumulate,
      beside bin + admit + accumulate over the same arrivals with the slots the
      host assigned (group g in slot g);
  (g) what it replaces, on the host's wall clock over (a)'s records: the key ->
      slot lookup as a Python dict (one lookup per packet, as GetFecGroup does
      one per packet -- but Python: a native hash map is SUPPOSED 20-50 times
      faster) and as NumPy (unique over the open keys once, searchsorted per
      turn).
  A round of a folding leg first zeroes the 2 MB of lengths (timed with the
  round and on its own as `restore`).

EXPECTATION, stated before the first run, to confirm or refute.  The table has
2^25 entries at this shape (twice 11.5 M keys, rounded up): a 512-MiB memset,
130-170 us at 3-4 TB/s, paid by every call.  The slots pass makes 2^20
compare-and-swaps and 2^20 atomic minima on scattered entries (SUPPOSED 50-100
us).  (a): the probe finds every key with a plain scattered 16-B load, no
atomic, and the emit loads 8 scattered bytes per packet again: two passes of
the kind of the bin's random-order count pass, so (a) lands near the bin's
random order as a whole (it was 966 us), 600-900 us, a quarter of it the
memset.  (b): one probe per run of about ten packets and coalesced loads in
the emit: the memset and the slots pass dominate, 250-400 us.  (c): as (a)
plus a compare-and-swap per group and an atomic minimum per packet run, and
the open pass: 100-300 us over (a).  (d): the table shrinks to 2^22 entries
(64 MiB), but 2^20 open keys are still inserted for 105 k packets: the per-call
rebuild dominates the sparse leg, 60-150 us against the bin's 44.  (f): the
assign adds its (c) figure to a turn of about 2.6 ms.

The legs alternate in this process: warm-up, then `--reps` alternations, each
timed with HIP events around back-to-back rounds -- as many as fill
`--window-ms`; medians with the 10th / 90th percentiles.  After timing every
assign leg's pkt_slot_out, slot_key, slot_k and counts equal tests/assign_rule.py
run over the whole input, and the rows of leg (f)'s two turns equal
qfec_encode_ragged's parity, per key.

Writes one JSON document (default profiles/assign_rate.json); DESIGN.md §4
quotes it.  Needs the GPU: there is no fallback.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def pct(v, q):
    return float(np.percentile(np.asarray(v), q))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--groups", type=int, default=1 << 20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=2)
    ap.add_argument("--window-ms", type=float, default=20.0,
                    help="least timed window; rounds repeat until they fill it")
    ap.add_argument("--host-reps", type=int, default=2, help="repetitions of leg (g)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "assign_rate.json"))
    args = ap.parse_args()

    import torch
    import assign_rule as AS
    from libquic_amd import qfec, synth
    from oracle import qfec_np as Q

    if not torch.cuda.is_available():
        sys.exit("assign_rate: no HIP device (this tool only measures on the GPU)")
    dev = "cuda:0"
    n, align, stride, ms = args.groups, 16, 1536, 2
    ctx = qfec.Context(0)
    ctx.set_stream(torch.cuda.current_stream())

    def timed(fn, inner):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / inner  # us per round

    def rounds_per_window(fn):
        for _ in range(args.warmup):
            est = timed(fn, args.inner)
        return int(min(4096, max(args.inner, np.ceil(args.window_ms * 1e3 / est))))

    def up(a, view):
        return torch.from_numpy(np.ascontiguousarray(a).view(view)).to(dev)

    def host(tn, dt):
        return tn.cpu().numpy().view(dt)

    ks, ptr, ln, off = synth.ragged_layout(0, n, 5, 15, 64, 1350, Q.SEED_RAGGED, align=align)
    ptr = ptr.astype(np.uint32)
    p0 = ptr[:-1].astype(np.int64)
    npk = int(ln.size)
    grp = np.repeat(np.arange(n, dtype=np.uint32), ks.astype(np.int64))
    idx_in_group = (np.arange(npk) - np.repeat(p0, ks.astype(np.int64))).astype(np.uint8)
    g64 = np.arange(n, dtype=np.uint64)
    group_key = ((g64 % np.uint64(4096)) << np.uint64(40)) | (g64 // np.uint64(4096) + np.uint64(1))
    assert np.unique(group_key).size == n
    data = torch.empty(int(off[-1]) + int(ln[-1]) + 16, dtype=torch.uint8, device=dev)
    ctx.synth_ragged(data, up(off, np.int64), up(ln, np.int16), up(ptr, np.int32), 0, n,
                     Q.SEED_RAGGED)
    t_k = up(ks.astype(np.uint8), np.uint8)
    acc = torch.zeros(n * stride, dtype=torch.uint8, device=dev)
    acc_len = torch.zeros(n, dtype=torch.int16, device=dev)  # the folding legs': zeroed per round
    maps = torch.full((n * ms,), 0xFF, dtype=torch.uint8, device=dev)  # stale: all ones
    rng = np.random.default_rng(20261020)
    # per-slot state of the assign-alone legs: all open (group g in slot g), and
    # all free with stale keys (a rotation of the arriving ones)
    len_open = torch.full((n,), 9, dtype=torch.int16, device=dev)
    len_free = torch.zeros(n, dtype=torch.int16, device=dev)
    stale_key = np.roll(group_key, 12345)

    def arrival_set(order, is_open):
        m = int(order.size)
        rec = {"key": group_key[grp[order]], "k": ks[grp[order]].astype(np.uint8),
               "slot": grp[order], "off": off[order], "ln": ln[order], "idx": idx_in_group[order]}
        d = {"key": up(rec["key"], np.int64), "k": up(rec["k"], np.uint8),
             "slot_key": up(group_key if is_open else stale_key, np.int64),
             "slot_k": up(ks.astype(np.uint8) if is_open else np.ones(n, np.uint8), np.uint8),
             "acc_len": len_open if is_open else len_free,
             "out": torch.zeros(m, dtype=torch.int32, device=dev),
             "cnt": torch.zeros(5, dtype=torch.int64, device=dev)}
        return {"m": m, "rec": rec, "d": d, "open": is_open}

    def assign_fn(s, acc_len_override=None, slot_k=None):
        d = s["d"]

        def fn():
            ctx.assign_slots(d["key"], d["k"], s["m"], d["slot_key"],
                             d["slot_k"] if slot_k is None else slot_k,
                             d["acc_len"] if acc_len_override is None else acc_len_override, n,
                             d["out"], counts=d["cnt"])
        return fn

    perm = rng.permutation(npk)
    open_random = arrival_set(perm, True)
    open_grouped = arrival_set(np.arange(npk), True)
    new_random = arrival_set(perm, False)
    some = np.sort(rng.permutation(n)[:max(1, n // 100)])
    sparse_pk = np.flatnonzero(np.isin(grp, some))
    sparse = arrival_set(rng.permutation(sparse_pk), True)

    # the bin and the rest of the turn over `perm`'s arrivals
    m = npk
    rec = open_random["rec"]
    b = {"slot": up(rec["slot"], np.int32), "off": up(rec["off"], np.int64),
         "ln": up(rec["ln"], np.int16), "idx": up(rec["idx"], np.uint8),
         "ok": up(np.ones(m, np.uint8), np.uint8),
         "t_ptr": torch.zeros(n + 1, dtype=torch.int32, device=dev),
         "t_off": torch.zeros(m, dtype=torch.int64, device=dev),
         "t_ln": torch.zeros(m, dtype=torch.int16, device=dev),
         "t_idx": torch.zeros(m, dtype=torch.uint8, device=dev),
         "t_ok": torch.zeros(m, dtype=torch.uint8, device=dev),
         "o_ptr": torch.zeros(n + 1, dtype=torch.int32, device=dev),
         "o_off": torch.zeros(m, dtype=torch.int64, device=dev),
         "o_ln": torch.zeros(m, dtype=torch.int16, device=dev),
         "v": torch.zeros(m, dtype=torch.uint8, device=dev)}
    key_k = torch.ones(n, dtype=torch.uint8, device=dev)  # the key-driven turn's slot_k

    def bin_fn(slots):
        def fn():
            ctx.bin_arrivals(slots, b["off"], b["ln"], b["idx"], b["ok"], m, n, b["t_ptr"],
                             b["t_off"], b["t_ln"], b["t_idx"], pkt_ok_out=b["t_ok"])
        return fn

    def admit_fold(slot_k):
        def fn():
            ctx.admit_ragged(b["t_off"], b["t_ln"], b["t_idx"], b["t_ok"], b["t_ptr"], n, slot_k,
                             maps, ms, acc_len, stride, b["o_ptr"], b["o_off"], b["o_ln"], b["v"])
            ctx.accumulate_ragged(data, b["o_off"], b["o_ln"], b["o_ptr"], n, acc, stride, acc_len)
        return fn

    def restore():
        acc_len.zero_()

    t_off_d, t_ln_d, t_ptr_d = up(off, np.int64), up(ln, np.int16), up(ptr, np.int32)

    def fold_alone():
        restore()
        ctx.accumulate_ragged(data, t_off_d, t_ln_d, t_ptr_d, n, acc, stride, acc_len)

    turn_assign = assign_fn(new_random, acc_len_override=acc_len, slot_k=key_k)
    bin_keys, bin_host = bin_fn(new_random["d"]["out"]), bin_fn(b["slot"])
    fold_keys, fold_host = admit_fold(key_k), admit_fold(t_k)

    def turn_from_keys():
        restore()
        turn_assign()
        bin_keys()
        fold_keys()

    def turn_host_slots():
        restore()
        bin_host()
        fold_host()

    fns = {"assign_open_random": assign_fn(open_random), "assign_open_grouped": assign_fn(open_grouped),
           "assign_new_random": assign_fn(new_random), "assign_sparse": assign_fn(sparse),
           "bin_random": bin_host, "restore": restore, "fold_alone": fold_alone,
           "turn_from_keys": turn_from_keys, "turn_host_slots": turn_host_slots}
    order = list(fns)
    for name in order:  # every leg once on its own, so that a latched error names its leg
        fns[name]()
        try:
            ctx.sync()
        except qfec.QfecError as e:
            sys.exit(f"assign_rate: leg {name}: {e}")
    inner ={name: rounds_per_window(fns[name]) for name in order}
    t = {name: [] for name in order}
    for _ in range(args.reps):
        for name in order:
            t[name].append(timed(fns[name], inner[name]))
    ctx.sync()

    # (g) the host's lookup over (a)'s records, wall clock
    hostleg = {"dict_build": [], "dict_lookup": [], "numpy_build": [], "numpy_lookup": []}
    keys_list = rec["key"].tolist()
    for _ in range(args.host_reps):
        t0 = time.perf_counter()
        table = dict(zip(group_key.tolist(), range(n)))
        t1 = time.perf_counter()
        got = [table[x] for x in keys_list]
        t2 = time.perf_counter()
        okeys, oslot = np.unique(group_key, return_index=True)
        t3 = time.perf_counter()
        got_np = oslot[np.searchsorted(okeys, rec["key"])]
        t4 = time.perf_counter()
        for k, v in (("dict_build", t1 - t0), ("dict_lookup", t2 - t1), ("numpy_build", t3 - t2),
                     ("numpy_lookup", t4 - t3)):
            hostleg[k].append(v * 1e6)
    assert np.array_equal(np.asarray(got, np.uint32), rec["slot"])
    assert np.array_equal(got_np.astype(np.uint32), rec["slot"])

    # the outputs of the timed calls against tests/assign_rule.py, whole inputs
    # (lists: the rule indexes one element at a time)
    slot_of_group = None
    for name, s in (("assign_open_random", open_random), ("assign_open_grouped", open_grouped),
                    ("assign_new_random", new_random), ("assign_sparse", sparse)):
        d = s["d"]
        w_key = (group_key if s["open"] else stale_key).tolist()
        w_k = (ks.astype(np.uint8) if s["open"] else np.ones(n, np.uint8)).tolist()
        w_out = [0] * s["m"]
        w_cnt = AS.assign_slots(s["rec"]["key"].tolist(), s["rec"]["k"].tolist(), w_key, w_k,
                                [9 if s["open"] else 0] * n, w_out)
        d["out"].fill_(-1)
        d["cnt"].fill_(-1)
        assign_fn(s)()
        ctx.sync()
        assert np.array_equal(host(d["out"], np.uint32), np.asarray(w_out, np.uint32)), name
        assert np.array_equal(host(d["slot_key"], np.uint64), np.asarray(w_key, np.uint64)), name
        assert np.array_equal(host(d["slot_k"], np.uint8), np.asarray(w_k, np.uint8)), name
        assert host(d["cnt"], np.uint64).tolist() == w_cnt.tolist(), name
        if name == "assign_new_random":
            slot_of_group = np.zeros(n, np.int64)
            slot_of_group[grp[perm]] = np.asarray(w_out, np.int64)
            assert w_cnt.tolist() == [0, s["m"], 0, n, 0]
        else:
            assert w_cnt.tolist() == [s["m"], 0, 0, 0, 0]
    par = torch.zeros(n * stride, dtype=torch.uint8, device=dev)
    plen = torch.zeros(n, dtype=torch.int16, device=dev)
    ctx.encode_ragged(data, t_off_d, t_ln_d, t_ptr_d, n, par,
                      up(np.arange(n, dtype=np.uint64) * np.uint64(stride), np.int64), plen)
    where = {"turn_from_keys": up(slot_of_group, np.int64), "turn_host_slots": None,
             "fold_alone": None}
    for name, at in where.items():
        acc.zero_()
        fns[name]()
        ctx.sync()
        torch.cuda.synchronize()
        rows, lens = acc.view(n, stride), acc_len
        if at is not None:  # group g's row lies in the slot its key was given
            rows, lens = rows[at], lens[at]
        assert torch.equal(lens, plen), name
        assert torch.equal(rows, par.view(n, stride)), name  # (rows zeroed before: zero beyond)
        del rows

    us = {name: {"median": pct(v, 50), "p10": pct(v, 10), "p90": pct(v, 90)}
          for name, v in t.items()}
    host_us = {k: {"median": pct(v, 50), "min": float(min(v))} for k, v in hostleg.items()}
    rst = us["restore"]["median"]
    fold = us["fold_alone"]
    legs = []
    for name, s in (("assign_open_random", open_random), ("assign_open_grouped", open_grouped),
                    ("assign_new_random", new_random), ("assign_sparse", sparse)):
        a = us[name]
        legs.append({"leg": name, "packets": s["m"], "slots": n,
                     "table_entries": int(2 ** np.ceil(np.log2(2 * (s["m"] + n)))), "us": a,
                     "ps_per_packet": a["median"] * 1e6 / s["m"],
                     "over_bin_random": a["median"] / us["bin_random"]["median"],
                     "over_fold": a["median"] / (fold["median"] - rst)})

    doc = {
        "tool": "tools/assign_rate.py",
        "device": torch.cuda.get_device_properties(0).name,
        "shape": {"groups": n, "slots": n, "k": [5, 15], "len": [64, 1350], "payload_align": align,
                  "acc_stride": stride, "map_stride": ms, "packets": npk,
                  "sparse_groups": int(some.size), "sparse_packets": int(sparse_pk.size),
                  "record_bytes_per_packet": "8 + 1 in; 4 out"},
        "expectation": "stated before measuring (the tool's docstring has it in full): a 512-MiB "
                       "memset of the table per call, 130-170 us; (a) 600-900 us, near the bin's "
                       "random order; (b) 250-400 us; (c) 100-300 us over (a); (d) 60-150 us, "
                       "dominated by rebuilding 2^20 open keys; (f) adds (c) to the turn",
        "method": {"timer": "HIP events around back-to-back rounds, as many as fill window_ms; "
                            "leg (g) on the host's wall clock, one at a time",
                   "inner": args.inner, "window_ms": args.window_ms, "reps": args.reps,
                   "warmup": args.warmup, "rounds_per_window": inner, "host_reps": args.host_reps,
                   "order": ", ".join(order) + ", alternating; then leg (g)",
                   "round": "folding legs and turns: acc_len zeroed by one device memset (the "
                            "`restore` row alone), then the calls; the assign legs have no "
                            "restore (an assign changes no length, so every round sees the same "
                            "state; the all-new leg rewrites the same keys)",
                   "host_lookup": "Python dict (build once per turn set, one lookup per packet) "
                                  "and NumPy unique + searchsorted.  It is Python / NumPy: a "
                                  "native hash map is SUPPOSED 20-50 times faster than the dict",
                   "verified": "after timing: every assign leg's pkt_slot_out, slot_key, slot_k "
                               "and counts equal tests/assign_rule.py over the whole input; rows "
                               "and lengths of both turns and of the fold alone equal "
                               "qfec_encode_ragged, the key-driven turn's per key"},
        "restore_us": us["restore"],
        "fold_alone_us": fold,
        "fold_alone_us_without_restore": fold["median"] - rst,
        "bin_random_us": us["bin_random"],
        "assign": legs,
        "turn": {"from_keys_us": us["turn_from_keys"], "host_slots_us": us["turn_host_slots"],
                 "difference_us": us["turn_from_keys"]["median"] - us["turn_host_slots"]["median"],
                 "ratio": us["turn_from_keys"]["median"] / us["turn_host_slots"]["median"]},
        "host_replaced_us": host_us,
        "host_dict_lookup_over_assign_open_random":
            host_us["dict_lookup"]["median"] / us["assign_open_random"]["median"],
        "host_numpy_lookup_over_assign_open_random":
            host_us["numpy_lookup"]["median"] / us["assign_open_random"]["median"],
    }
    for row in legs:
        print(json.dumps(row))
    for key in ("turn", "host_replaced_us", "bin_random_us", "fold_alone_us", "restore_us"):
        print(json.dumps({key: doc[key]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
