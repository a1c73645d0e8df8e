#!/usr/bin/env python3
"""qfec_bin_arrivals beside the fold it feeds and the host grouping it replaces.

One MI355X, BASELINE configs[3] in the payload arena's layout resident on the
device: 2^20 groups in 2^20 slots (group g holds slot g), k 5-15, 64-1350 B,
payloads on 16-B boundaries, running rows of 1,536 B, one 2-byte running map per
slot.  Every data packet of every group is a candidate of the turn; a record is
(pkt_slot 4, pkt_off 8, pkt_len 2, pkt_idx 1, pkt_ok 1) = 16 B per packet.

  (a) bin alone, the arrival order a uniform random permutation of the
      candidates;
  (b) bin alone, the arrivals already grouped (the identity order: best case);
  (c) bin alone, a sparse turn: 1% of the slots receive their packets (in
      random order); and beside it qfec_admit_ragged + qfec_accumulate_ragged
      over the resulting LOCKSTEP tables (2^20 groups, nearly all empty) against
      the same packets in COMPACT host-built tables with a slot list -- the
      price of the 2^20 empty groups;
  (d) the dense turn: bin + admit + accumulate on (a)'s input beside admit +
      accumulate over host-built tables of the same turn;
  (e) what it replaces, on the wall clock: a stable host grouping of the same
      records (NumPy: argsort(kind="stable"), a bincount, a cumulative sum and
      four gathers into pinned memory) and the H2D copy of the grouped tables,
      against the H2D copy of the arrival-order records.  It is NumPy: a native
      counting sort would be faster (SUPPOSED: several times).
  The fold alone (qfec_accumulate_ragged over host-built tables) is measured in
  the same process; (a)-(c) are given absolutely and as a fraction of it.
  The fold raises acc_len, after which every candidate would be a duplicate, so
  a round of every admitting or folding leg first zeroes the 2 MB of lengths
  (timed with the round and on its own as `restore`).

EXPECTATION, to confirm or refute: by its bytes the call moves roughly 80-100 B
per packet (4 + 4 in the count; 20 in, a 4-B pointer gather and 16 out in the
scatter; 16 in, 4 per segment neighbour from cache and 20 out in the order
pass) against about 700 B of payload for the fold, so if it ran at the fold's
rate it would cost 11-14% of the fold, 170-210 us.  What the bytes do not
price: 10.5 M returning atomics on 2^20 addresses and 10.5 M scattered 16-B
stores.  So: (b), where both are coalesced, near the bytes figure; (a) above
it, by an unknown factor.

The legs alternate in this process: warm-up, then `--reps` alternations, each
timed with HIP events around back-to-back rounds -- as many as fill
`--window-ms`; medians with the 10th / 90th percentiles.  After timing every
leg's outputs are compared with the rule stated in NumPy here (a stable
argsort), which is itself compared with tests/bin_rule.py on the packets of the
first `--sample` slots; the rows and lengths of the folding legs of (d) equal
each other and qfec_encode_ragged's parity, those of (c) each other.

Writes one JSON document (default profiles/bin_rate.json); DESIGN.md §4 quotes
it.  Needs the GPU: there is no fallback.
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
    ap.add_argument("--host-reps", type=int, default=5, help="repetitions of leg (e)")
    ap.add_argument("--sample", type=int, default=2000,
                    help="slots on whose packets the argsort rule is compared with tests/bin_rule.py")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bin_rate.json"))
    args = ap.parse_args()

    import torch
    import bin_rule as B
    from libquic_amd import qfec, synth
    from oracle import qfec_np as Q

    if not torch.cuda.is_available():
        sys.exit("bin_rate: no HIP device (this tool only measures on the GPU)")
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
    payload_bytes = int(ln.astype(np.int64).sum())
    data = torch.empty(int(off[-1]) + int(ln[-1]) + 16, dtype=torch.uint8, device=dev)
    ctx.synth_ragged(data, up(off, np.int64), up(ln, np.int16), up(ptr, np.int32), 0, n,
                     Q.SEED_RAGGED)
    t_k = up(ks.astype(np.uint8), np.uint8)
    acc = torch.zeros(n * stride, dtype=torch.uint8, device=dev)
    acc_len = torch.zeros(n, dtype=torch.int16, device=dev)
    maps = torch.full((n * ms,), 0xFF, dtype=torch.uint8, device=dev)  # stale: all ones
    rng = np.random.default_rng(20261020)

    def arrival_set(order):
        """the records of packets `order` (indices into the grouped tables) in
        that arrival order, the rule's outputs and the device buffers"""
        m = int(order.size)
        rec = {"slot": grp[order], "off": off[order], "ln": ln[order], "idx": idx_in_group[order],
               "ok": np.ones(m, np.uint8)}
        by_slot = np.argsort(rec["slot"], kind="stable")  # the rule: a stable sort by slot
        want = {"ptr": np.zeros(n + 1, np.uint32), "src": by_slot.astype(np.uint32)}
        want["ptr"][1:] = np.cumsum(np.bincount(rec["slot"], minlength=n))
        for key in ("off", "ln", "idx", "ok"):
            want[key] = rec[key][by_slot]
        # the argsort rule against tests/bin_rule.py on the packets of the first slots
        h = min(args.sample, n)
        sub = np.flatnonzero(rec["slot"] < h)
        r_ptr = np.zeros(h + 1, np.uint32)
        r = {"off": np.zeros(sub.size, np.uint64), "ln": np.zeros(sub.size, np.uint16),
             "idx": np.zeros(sub.size, np.uint8), "ok": np.zeros(sub.size, np.uint8),
             "src": np.zeros(sub.size, np.uint32)}
        errs, cnt = B.bin_arrivals(rec["slot"][sub], rec["off"][sub], rec["ln"][sub], rec["idx"][sub],
                                   rec["ok"][sub], h, r_ptr, r["off"], r["ln"], r["idx"], r["ok"],
                                   r["src"])
        assert not errs.any() and cnt.tolist() == [sub.size, 0, 0]
        assert np.array_equal(r_ptr, want["ptr"][:h + 1])
        assert np.array_equal(sub[r["src"]], want["src"][:sub.size])
        for key in ("off", "ln", "idx", "ok"):
            assert np.array_equal(r[key], want[key][:sub.size]), key
        d = {"slot": up(rec["slot"], np.int32), "off": up(rec["off"], np.int64),
             "ln": up(rec["ln"], np.int16), "idx": up(rec["idx"], np.uint8),
             "ok": up(rec["ok"], np.uint8),
             "t_ptr": torch.zeros(n + 1, dtype=torch.int32, device=dev),
             "t_off": torch.zeros(m, dtype=torch.int64, device=dev),
             "t_ln": torch.zeros(m, dtype=torch.int16, device=dev),
             "t_idx": torch.zeros(m, dtype=torch.uint8, device=dev),
             "t_ok": torch.zeros(m, dtype=torch.uint8, device=dev),
             "t_src": torch.zeros(m, dtype=torch.int32, device=dev),
             "cnt": torch.zeros(3, dtype=torch.int64, device=dev),
             # the admit's outputs over the binned tables
             "o_ptr": torch.zeros(n + 1, dtype=torch.int32, device=dev),
             "o_off": torch.zeros(m, dtype=torch.int64, device=dev),
             "o_ln": torch.zeros(m, dtype=torch.int16, device=dev),
             "v": torch.zeros(m, dtype=torch.uint8, device=dev)}
        return {"m": m, "rec": rec, "want": want, "d": d}

    dense_random = arrival_set(rng.permutation(npk))
    dense_grouped = arrival_set(np.arange(npk))
    some = np.sort(rng.permutation(n)[:max(1, n // 100)])  # the sparse turn's slots
    sparse_pk = np.flatnonzero(np.isin(grp, some))
    sparse = arrival_set(rng.permutation(sparse_pk))

    def bin_fn(s):
        d = s["d"]

        def fn():
            ctx.bin_arrivals(d["slot"], d["off"], d["ln"], d["idx"], d["ok"], s["m"], n, d["t_ptr"],
                             d["t_off"], d["t_ln"], d["t_idx"], pkt_ok_out=d["t_ok"],
                             src_out=d["t_src"], counts=d["cnt"])
        return fn

    def restore():
        acc_len.zero_()

    def admit_fold_lockstep(s):
        """admit + accumulate over s's binned tables, group s = slot s"""
        d = s["d"]

        def fn():
            ctx.admit_ragged(d["t_off"], d["t_ln"], d["t_idx"], d["t_ok"], d["t_ptr"], n, t_k, maps,
                             ms, acc_len, stride, d["o_ptr"], d["o_off"], d["o_ln"], d["v"])
            ctx.accumulate_ragged(data, d["o_off"], d["o_ln"], d["o_ptr"], n, acc, stride, acc_len)
        return fn

    # host-built tables: the dense turn's are the layout's own; the sparse
    # turn's are compact, one group per named slot, with a slot list
    h_dense = {"off": up(off, np.int64), "ln": up(ln, np.int16), "idx": up(idx_in_group, np.uint8),
               "ok": up(np.ones(npk, np.uint8), np.uint8), "ptr": up(ptr, np.int32),
               "o_ptr": torch.zeros(n + 1, dtype=torch.int32, device=dev),
               "o_off": torch.zeros(npk, dtype=torch.int64, device=dev),
               "o_ln": torch.zeros(npk, dtype=torch.int16, device=dev),
               "v": torch.zeros(npk, dtype=torch.uint8, device=dev)}
    ns = int(some.size)
    c_ptr = np.zeros(ns + 1, np.uint32)
    c_ptr[1:] = np.cumsum(ks[some])
    h_sparse = {"off": up(off[sparse_pk], np.int64), "ln": up(ln[sparse_pk], np.int16),
                "idx": up(idx_in_group[sparse_pk], np.uint8),
                "ok": up(np.ones(sparse_pk.size, np.uint8), np.uint8), "ptr": up(c_ptr, np.int32),
                "slot": up(some.astype(np.uint32), np.int32),
                "o_ptr": torch.zeros(ns + 1, dtype=torch.int32, device=dev),
                "o_off": torch.zeros(sparse_pk.size, dtype=torch.int64, device=dev),
                "o_ln": torch.zeros(sparse_pk.size, dtype=torch.int16, device=dev),
                "v": torch.zeros(sparse_pk.size, dtype=torch.uint8, device=dev)}

    def admit_fold_host(h, groups, slot=None):
        def fn():
            ctx.admit_ragged(h["off"], h["ln"], h["idx"], h["ok"], h["ptr"], groups, t_k, maps, ms,
                             acc_len, stride, h["o_ptr"], h["o_off"], h["o_ln"], h["v"], slot=slot,
                             n_slots=n)
            ctx.accumulate_ragged(data, h["o_off"], h["o_ln"], h["o_ptr"], groups, acc, stride,
                                  acc_len, slot=slot, n_slots=n)
        return fn

    bin_random, bin_grouped, bin_sparse = bin_fn(dense_random), bin_fn(dense_grouped), bin_fn(sparse)
    lock_sparse, lock_dense = admit_fold_lockstep(sparse), admit_fold_lockstep(dense_random)
    host_sparse = admit_fold_host(h_sparse, ns, h_sparse["slot"])
    host_dense = admit_fold_host(h_dense, n)
    t_off_d, t_ln_d, t_ptr_d = h_dense["off"], h_dense["ln"], h_dense["ptr"]

    def with_restore(*fs):
        def fn():
            restore()
            for f in fs:
                f()
        return fn

    def fold_alone():
        restore()
        ctx.accumulate_ragged(data, t_off_d, t_ln_d, t_ptr_d, n, acc, stride, acc_len)

    bin_sparse()  # (the lockstep legs read its tables)
    bin_random()
    fns = {"bin_random": bin_random, "bin_grouped": bin_grouped, "bin_sparse": bin_sparse,
           "restore": restore, "fold_alone": fold_alone,
           "sparse_admit_fold_lockstep": with_restore(lock_sparse),
           "sparse_admit_fold_compact": with_restore(host_sparse),
           "dense_bin_admit_fold": with_restore(bin_random, lock_dense),
           "dense_admit_fold_host_tables": with_restore(host_dense)}
    order = list(fns)
    inner = {name: rounds_per_window(fns[name]) for name in order}
    t = {name: [] for name in order}
    for _ in range(args.reps):
        for name in order:
            t[name].append(timed(fns[name], inner[name]))
    ctx.sync()

    # (e) the host grouping and the two H2D copies, wall clock
    rec = dense_random["rec"]
    views = {"slot": np.int32, "off": np.int64, "ln": np.int16, "idx": np.uint8, "ok": np.uint8}
    pin_in = {k: torch.from_numpy(rec[k].view(views[k]).copy()).pin_memory() for k in views}
    pin_out = {k: torch.empty_like(pin_in[k]).pin_memory() for k in ("off", "ln", "idx", "ok")}
    pin_ptr = torch.empty(n + 1, dtype=torch.int32).pin_memory()
    dst_in = {k: torch.empty_like(v, device=dev) for k, v in pin_in.items()}
    dst_out = {k: torch.empty_like(v, device=dev) for k, v in pin_out.items()}
    dst_ptr = torch.empty(n + 1, dtype=torch.int32, device=dev)
    hostleg = {"group": [], "h2d_grouped": [], "h2d_arrival": []}
    for _ in range(1 + args.host_reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        o = np.argsort(rec["slot"], kind="stable")
        hp = pin_ptr.numpy().view(np.uint32)
        hp[0] = 0
        np.cumsum(np.bincount(rec["slot"], minlength=n), out=hp[1:])
        for k in pin_out:
            np.take(pin_in[k].numpy(), o, out=pin_out[k].numpy())
        t1 = time.perf_counter()
        dst_ptr.copy_(pin_ptr, non_blocking=True)
        for k in pin_out:
            dst_out[k].copy_(pin_out[k], non_blocking=True)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        for k in pin_in:
            dst_in[k].copy_(pin_in[k], non_blocking=True)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        for k, v in (("group", t1 - t0), ("h2d_grouped", t2 - t1), ("h2d_arrival", t3 - t2)):
            hostleg[k].append(v * 1e6)
    hostleg = {k: v[1:] for k, v in hostleg.items()}
    assert np.array_equal(pin_ptr.numpy().view(np.uint32), dense_random["want"]["ptr"])
    assert np.array_equal(pin_out["off"].numpy().view(np.uint64), dense_random["want"]["off"])

    # the outputs of the timed calls
    for name, s in (("random", dense_random), ("grouped", dense_grouped), ("sparse", sparse)):
        d, w, m = s["d"], s["want"], s["m"]
        for key in ("t_ptr", "t_off", "t_ln", "t_idx", "t_ok", "t_src", "cnt"):
            d[key].fill_(-1 if d[key].dtype != torch.uint8 else 0xA5)
        bin_fn(s)()
        ctx.sync()
        assert np.array_equal(host(d["t_ptr"], np.uint32), w["ptr"]), name
        for key, dt in (("off", np.uint64), ("ln", np.uint16), ("idx", np.uint8), ("ok", np.uint8),
                        ("src", np.uint32)):
            assert np.array_equal(host(d["t_" + key], dt), w[key]), (name, key)
        assert host(d["cnt"], np.uint64).tolist() == [m, 0, 0], name
    par = torch.zeros(n * stride, dtype=torch.uint8, device=dev)
    plen = torch.zeros(n, dtype=torch.int16, device=dev)
    ctx.encode_ragged(data, t_off_d, t_ln_d, t_ptr_d, n, par,
                      up(np.arange(n, dtype=np.uint64) * np.uint64(stride), np.int64), plen)
    for name in ("dense_bin_admit_fold", "dense_admit_fold_host_tables", "fold_alone"):
        acc.zero_()
        fns[name]()
        ctx.sync()
        torch.cuda.synchronize()
        assert torch.equal(acc_len, plen), name
        assert torch.equal(acc, par), name  # (rows hold zero beyond their lengths: zeroed before)
    rows = {}
    for name in ("sparse_admit_fold_lockstep", "sparse_admit_fold_compact"):
        acc.zero_()
        fns[name]()
        ctx.sync()
        torch.cuda.synchronize()
        rows[name] = (acc.clone(), acc_len.clone())
        touched = host(acc_len, np.uint16) != 0
        assert np.array_equal(np.flatnonzero(touched), some), name
        assert torch.equal(acc_len[up(some.astype(np.int64), np.int64)],
                           plen[up(some.astype(np.int64), np.int64)]), name
    a, b = rows["sparse_admit_fold_lockstep"], rows["sparse_admit_fold_compact"]
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])

    us = {name: {"median": pct(v, 50), "p10": pct(v, 10), "p90": pct(v, 90)}
          for name, v in t.items()}
    host_us = {k: {"median": pct(v, 50), "p10": pct(v, 10), "p90": pct(v, 90)}
               for k, v in hostleg.items()}
    rst = us["restore"]["median"]
    fold = us["fold_alone"]
    bins = []
    for name, s in (("bin_random", dense_random), ("bin_grouped", dense_grouped),
                    ("bin_sparse", sparse)):
        a = us[name]
        bins.append({"leg": name, "packets": s["m"], "slots": n, "us": a,
                     "ps_per_packet": a["median"] * 1e6 / s["m"],
                     "over_fold": {"median": a["median"] / (fold["median"] - rst),
                                   "p10": a["p10"] / (fold["p90"] - rst),
                                   "p90": a["p90"] / (fold["p10"] - rst)}})

    def ratio(x, y):
        return {"median": us[x]["median"] / us[y]["median"], "p10": us[x]["p10"] / us[y]["p90"],
                "p90": us[x]["p90"] / us[y]["p10"],
                "difference_us": us[x]["median"] - us[y]["median"]}

    doc = {
        "tool": "tools/bin_rate.py",
        "device": torch.cuda.get_device_properties(0).name,
        "shape": {"groups": n, "slots": n, "k": [5, 15], "len": [64, 1350], "payload_align": align,
                  "acc_stride": stride, "map_stride": ms, "packets": npk,
                  "payload_bytes": payload_bytes, "sparse_slots": ns,
                  "sparse_packets": int(sparse_pk.size),
                  "record_bytes_per_packet": "4 + 8 + 2 + 1 + 1 in; 8 + 2 + 1 + 1 + 4 out"},
        "expectation": "stated before measuring: about 80-100 B moved per packet against about "
                       "700 B of payload for the fold, so 11-14% of the fold (170-210 us) at the "
                       "fold's rate; the returning atomics and the scattered 16-B stores are not "
                       "priced by bytes: the grouped order near that figure, the random order "
                       "above it by an unknown factor",
        "method": {"timer": "HIP events around back-to-back rounds, as many as fill window_ms; "
                            "leg (e) on the host's wall clock, one at a time",
                   "inner": args.inner, "window_ms": args.window_ms, "reps": args.reps,
                   "warmup": args.warmup, "rounds_per_window": inner, "host_reps": args.host_reps,
                   "order": ", ".join(order) + ", alternating; then leg (e)",
                   "round": "admitting and folding legs: acc_len zeroed by one device memset (the "
                            "`restore` row alone) so the slots are fresh, then the calls; the bin "
                            "legs have no restore; over_fold is against the fold without its "
                            "restore",
                   "ratio_ranges": "p10 over p90 and p90 over p10 of the two legs: bounds, not "
                                   "percentiles of a paired ratio",
                   "host_grouping": "NumPy: argsort(kind='stable') of pkt_slot, bincount + cumsum "
                                    "for grp_ptr, four gathers into pinned memory; the H2D copies "
                                    "from pinned memory.  SUPPOSED: a native counting sort groups "
                                    "several times faster than NumPy; the copies do not change",
                   "verified": "after timing: every bin leg's grp_ptr_out, four tables, src_out "
                               "and counts equal a stable argsort by slot (equal to "
                               "tests/bin_rule.py on the packets of the first %d slots); rows and "
                               "lengths of the dense turn's legs and of the fold alone equal "
                               "qfec_encode_ragged; rows and lengths of the two sparse legs equal "
                               "each other" % min(args.sample, n)},
        "restore_us": us["restore"],
        "fold_alone_us": fold,
        "fold_alone_us_without_restore": fold["median"] - rst,
        "bin": bins,
        "sparse_turn": {"lockstep_us": us["sparse_admit_fold_lockstep"],
                        "compact_us": us["sparse_admit_fold_compact"],
                        "lockstep_over_compact": ratio("sparse_admit_fold_lockstep",
                                                       "sparse_admit_fold_compact")},
        "dense_turn": {"bin_admit_fold_us": us["dense_bin_admit_fold"],
                       "admit_fold_host_tables_us": us["dense_admit_fold_host_tables"],
                       "ratio": ratio("dense_bin_admit_fold", "dense_admit_fold_host_tables")},
        "host_replaced_us": host_us,
        "host_grouping_over_bin_random": host_us["group"]["median"] / us["bin_random"]["median"],
    }
    for row in bins:
        print(json.dumps(row))
    for key in ("sparse_turn", "dense_turn", "host_replaced_us", "fold_alone_us", "restore_us"):
        print(json.dumps({key: doc[key]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
