#!/usr/bin/env python3
"""qfec_admit_ragged beside the fold it feeds and the round trip it replaces.

One MI355X, BASELINE configs[3] in the payload arena's layout resident on the
device: 2^20 groups, k 5-15, 64-1350 B, payloads on 16-B boundaries, 2^20
running rows of 1,536 B, one 2-byte running map per slot.  A turn's candidates
are every data packet of every group; a candidate set may mark a share of them
as failed (pkt_ok = 0) and list a share twice (the copy right behind the
original).

  (a) admit alone on fresh slots: all admitted; 5% failed; 5% listed twice.
  (b) admit + accumulate on the mixed set (5% failed and 5% listed twice)
      beside qfec_accumulate_ragged over host-built tables of the same admitted
      packets -- the path without the admit.
      The fold raises acc_len, after which every candidate would be a
      duplicate, so a round of every leg first zeroes the 2 MB of lengths
      (timed with the round and on its own as `restore`).
  (c) what the admit replaces for packets opened on the device: qfec_sync, a
      D2H copy of ok, a host rebuild of the tables (NumPy: ok and the host's
      own first-arrival mask, a reduceat and three gathers) and their H2D copy,
      on the wall clock.

EXPECTATION, to confirm or refute: the tables are about 25 B per packet against
about 700 B of payload, so the admit should cost a few percent of the fold.

(a) and (b) alternate in this process: warm-up, then `--reps` alternations,
each timed with HIP events around back-to-back rounds -- as many as fill
`--window-ms`; medians with the 10th / 90th percentiles.  After timing every
leg's outputs are compared with the rule stated in NumPy here (vectorised: a
fresh slot, copies adjacent), which is itself compared with tests/admit_rule.py
on the first groups; the rows of both (b) legs equal qfec_encode_ragged's
parity over the admitted packets.

Writes one JSON document (default profiles/admit_rate.json); DESIGN.md §4
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

ADMITTED, FAILED, DUPLICATE = 0, 1, 2


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
    ap.add_argument("--sample", type=int, default=2000,
                    help="groups on which the vectorised rule is compared with tests/admit_rule.py")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "admit_rate.json"))
    args = ap.parse_args()

    import torch
    import admit_rule as R
    from libquic_amd import qfec, synth
    from oracle import qfec_np as Q

    if not torch.cuda.is_available():
        sys.exit("admit_rate: no HIP device (this tool only measures on the GPU)")
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

    ks, ptr, ln, off = synth.ragged_layout(0, n, 5, 15, 64, 1350, Q.SEED_RAGGED, align=align)
    p0 = ptr[:-1].astype(np.int64)
    npk = int(ln.size)
    idx_in_group = (np.arange(npk) - np.repeat(p0, ks.astype(np.int64))).astype(np.uint8)
    payload_bytes = int(ln.astype(np.int64).sum())
    data = torch.empty(int(off[-1]) + int(ln[-1]) + 16, dtype=torch.uint8, device=dev)
    ctx.synth_ragged(data, up(off, np.int64), up(ln, np.int16), up(ptr, np.int32), 0, n,
                     Q.SEED_RAGGED)
    t_k = up(ks.astype(np.uint8), np.uint8)
    acc = torch.zeros(n * stride, dtype=torch.uint8, device=dev)
    acc_len = torch.zeros(n, dtype=torch.int16, device=dev)
    stale = np.full((n, ms), 0xFF, np.uint8)  # fresh slots: the old maps are all ones
    rng = np.random.default_rng(20261020)

    def cand_set(fail, twice):
        """candidates, the expected verdicts (fresh slots, copies adjacent) and
        the tables a host would build from them"""
        rep = 1 + (rng.random(npk) < twice).astype(np.int64)
        c = np.repeat(np.arange(npk), rep)
        m = int(c.size)
        cnt = np.add.reduceat(rep, p0)
        cptr = np.zeros(n + 1, np.uint32)
        cptr[1:] = np.cumsum(cnt)
        ok = (rng.random(m) >= fail).astype(np.uint8)
        first = np.ones(m, bool)  # the host's own knowledge: not a copy of its predecessor
        first[1:] = c[1:] != c[:-1]
        prev_ok = np.zeros(m, bool)
        prev_ok[1:] = ~first[1:] & (ok[:-1] != 0)
        v = np.where(ok == 0, FAILED, np.where(prev_ok, DUPLICATE, ADMITTED)).astype(np.uint8)
        adm = v == ADMITTED
        c0 = cptr[:-1].astype(np.int64)
        optr = np.zeros(n + 1, np.uint32)
        optr[1:] = np.cumsum(np.add.reduceat(adm.astype(np.int64), c0))
        c_off, c_ln, c_idx = off[c], ln[c], idx_in_group[c]
        bits = np.bitwise_or.reduceat(np.where(adm, 1 << c_idx.astype(np.int64), 0), c0)
        maps = stale.copy()
        some = np.diff(optr.astype(np.int64)) > 0
        two = some & (ks >= 8)  # (K / 8 + 1 bytes of a map are written, no more)
        maps[some, 0], maps[two, 1] = bits[some] & 0xFF, bits[two] >> 8
        s = {"m": m, "off": c_off, "ln": c_ln, "idx": c_idx, "ok": ok, "ptr": cptr, "first": first,
             "v": v, "optr": optr, "ooff": c_off[adm], "oln": c_ln[adm], "maps": maps,
             "counts": [int((v == x).sum()) for x in range(4)]}
        # the vectorised rule against tests/admit_rule.py on the first groups
        h = min(args.sample, n)
        mh = int(cptr[h])
        r_ptr, r_off, r_ln = (np.zeros(h + 1, np.uint32), np.zeros(mh, np.uint64),
                              np.zeros(mh, np.uint16))
        r_v, r_maps = np.zeros(mh, np.uint8), stale[:h].copy()
        errs, _ = R.admit(c_off, c_ln, c_idx, ok, cptr[:h + 1], ks.astype(np.uint8), r_maps,
                          np.zeros(h, np.uint16), stride, r_ptr, r_off, r_ln, r_v)
        na = int(r_ptr[h])
        assert not errs.any() and np.array_equal(r_v, v[:mh]) and np.array_equal(r_ptr, optr[:h + 1])
        assert np.array_equal(r_off[:na], s["ooff"][:na]) and np.array_equal(r_ln[:na], s["oln"][:na])
        assert np.array_equal(r_maps, maps[:h])
        # device side
        s["d"] = {"off": up(c_off, np.int64), "ln": up(c_ln, np.int16), "idx": up(c_idx, np.uint8),
                  "ok": up(ok, np.uint8), "ptr": up(cptr, np.int32),
                  "maps": up(stale, np.uint8),
                  "optr": torch.zeros(n + 1, dtype=torch.int32, device=dev),
                  "ooff": torch.zeros(m, dtype=torch.int64, device=dev),
                  "oln": torch.zeros(m, dtype=torch.int16, device=dev),
                  "v": torch.zeros(m, dtype=torch.uint8, device=dev),
                  "counts": torch.zeros(4, dtype=torch.int64, device=dev)}
        return s

    sets = {"all_admitted": cand_set(0.0, 0.0), "failed_5pct": cand_set(0.05, 0.0),
            "twice_5pct": cand_set(0.0, 0.05), "mixed": cand_set(0.05, 0.05)}

    def admit(s, fresh=True):
        d = s["d"]

        def fn():
            if fresh:  # (the folding legs leave acc_len raised: every candidate a duplicate)
                acc_len.zero_()
            ctx.admit_ragged(d["off"], d["ln"], d["idx"], d["ok"], d["ptr"], n, t_k, d["maps"], ms,
                             acc_len, stride, d["optr"], d["ooff"], d["oln"], d["v"],
                             counts=d["counts"])
        return fn

    mixed = sets["mixed"]
    h_optr, h_ooff, h_oln = (up(mixed["optr"], np.int32), up(mixed["ooff"], np.int64),
                             up(mixed["oln"], np.int16))
    admit_mixed = admit(mixed, fresh=False)

    def restore():
        acc_len.zero_()

    def admit_accumulate():
        restore()
        admit_mixed()
        d = mixed["d"]
        ctx.accumulate_ragged(data, d["ooff"], d["oln"], d["optr"], n, acc, stride, acc_len)

    def accumulate_host_tables():
        restore()
        ctx.accumulate_ragged(data, h_ooff, h_oln, h_optr, n, acc, stride, acc_len)

    fns = {"restore": restore, "admit_accumulate": admit_accumulate,
           "accumulate_host_tables": accumulate_host_tables}
    order = []
    for name in ("all_admitted", "failed_5pct", "twice_5pct"):
        fns["admit_" + name] = admit(sets[name])
        order.append("admit_" + name)
    order += ["restore", "admit_accumulate", "accumulate_host_tables"]
    inner = {name: rounds_per_window(fns[name]) for name in order}
    t = {name: [] for name in order}
    for _ in range(args.reps):
        for name in order:
            t[name].append(timed(fns[name], inner[name]))
    ctx.sync()

    # (c) the round trip: sync, ok to the host, the tables rebuilt, the tables back
    d = mixed["d"]
    ok_host = torch.empty(mixed["m"], dtype=torch.uint8).pin_memory()
    pin = {k: torch.empty_like(v.cpu()).pin_memory() for k, v in
           (("optr", h_optr), ("ooff", h_ooff), ("oln", h_oln))}
    c0 = mixed["ptr"][:-1].astype(np.int64)
    trip = {"sync_and_d2h": [], "rebuild": [], "h2d": [], "total": []}
    for _ in range(args.warmup + args.reps):
        restore()
        accumulate_host_tables()  # (something in flight for the sync to wait for)
        t0 = time.perf_counter()
        ctx.sync()
        ok_host.copy_(d["ok"])
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        keep = (ok_host.numpy() != 0) & mixed["first"]
        # (a copy whose original failed is admitted: the host would know from ok)
        keep[1:] |= (~mixed["first"][1:]) & (ok_host.numpy()[1:] != 0) & (ok_host.numpy()[:-1] == 0)
        optr = np.zeros(n + 1, np.uint32)
        optr[1:] = np.cumsum(np.add.reduceat(keep.astype(np.int64), c0))
        pin["optr"].numpy().view(np.uint32)[:] = optr
        na = int(optr[n])
        pin["ooff"].numpy().view(np.uint64)[:na] = mixed["off"][keep]
        pin["oln"].numpy().view(np.uint16)[:na] = mixed["ln"][keep]
        t2 = time.perf_counter()
        h_optr.copy_(pin["optr"], non_blocking=True)
        h_ooff[:na].copy_(pin["ooff"][:na], non_blocking=True)
        h_oln[:na].copy_(pin["oln"][:na], non_blocking=True)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        for k, v in (("sync_and_d2h", t1 - t0), ("rebuild", t2 - t1), ("h2d", t3 - t2),
                     ("total", t3 - t0)):
            trip[k].append(v * 1e6)
    trip = {k: v[args.warmup:] for k, v in trip.items()}
    assert np.array_equal(optr, mixed["optr"]) and np.array_equal(mixed["off"][keep], mixed["ooff"])

    # the outputs of the timed calls
    def host(tn, dt):
        return tn.cpu().numpy().view(dt)

    for name in ("all_admitted", "failed_5pct", "twice_5pct", "mixed"):
        s, d = sets[name], sets[name]["d"]
        restore()
        d["maps"].copy_(up(stale, np.uint8))
        admit(s)()
        ctx.sync()
        na = int(s["optr"][n])
        assert np.array_equal(host(d["v"], np.uint8), s["v"]), name
        assert np.array_equal(host(d["optr"], np.uint32), s["optr"]), name
        assert np.array_equal(host(d["ooff"], np.uint64)[:na], s["ooff"]), name
        assert np.array_equal(host(d["oln"], np.uint16)[:na], s["oln"]), name
        assert np.array_equal(host(d["maps"], np.uint8), s["maps"]), name
        assert host(d["counts"], np.uint64).tolist() == s["counts"], name
    par = torch.zeros(n * stride, dtype=torch.uint8, device=dev)
    plen = torch.zeros(n, dtype=torch.int16, device=dev)
    ctx.encode_ragged(data, h_ooff, h_oln, h_optr, n, par,
                      up(np.arange(n, dtype=np.uint64) * np.uint64(stride), np.int64), plen)
    rows = {}
    for name in ("admit_accumulate", "accumulate_host_tables"):
        acc.zero_()
        fns[name]()
        ctx.sync()
        torch.cuda.synchronize()
        assert torch.equal(acc_len, plen), name
        rows[name] = acc.clone()
        # (rows hold zero beyond their lengths here: both start from a zeroed buffer)
        assert torch.equal(acc, par), name
    assert torch.equal(rows["admit_accumulate"], rows["accumulate_host_tables"])

    us = {name: {"median": pct(v, 50), "p10": pct(v, 10), "p90": pct(v, 90)}
          for name, v in t.items()}
    trip_us = {k: {"median": pct(v, 50), "p10": pct(v, 10), "p90": pct(v, 90)}
               for k, v in trip.items()}
    rst = us["restore"]["median"]
    fold = us["accumulate_host_tables"]
    both = us["admit_accumulate"]
    admit_rows = []
    for name in ("all_admitted", "failed_5pct", "twice_5pct"):
        a = us["admit_" + name]
        admit_rows.append({"set": name, "candidates": sets[name]["m"], "verdicts": sets[name]["counts"],
                           "us": a, "us_without_restore": a["median"] - rst,
                           "ps_per_candidate": (a["median"] - rst) * 1e6 / sets[name]["m"],
                           "over_fold": {"median": (a["median"] - rst) / (fold["median"] - rst),
                                         "p10": (a["p10"] - rst) / (fold["p90"] - rst),
                                         "p90": (a["p90"] - rst) / (fold["p10"] - rst)}})
    pair = {"set": "mixed", "candidates": mixed["m"], "verdicts": mixed["counts"],
            "admit_accumulate_us": both, "accumulate_host_tables_us": fold,
            "ratio": {"median": both["median"] / fold["median"], "p10": both["p10"] / fold["p90"],
                      "p90": both["p90"] / fold["p10"]},
            "ratio_without_restore": (both["median"] - rst) / (fold["median"] - rst),
            "admit_us_by_difference": both["median"] - fold["median"],
            "round_trip_us": trip_us,
            "round_trip_over_admit_by_difference":
                trip_us["total"]["median"] / max(both["median"] - fold["median"], 1e-9)}
    doc = {
        "tool": "tools/admit_rate.py",
        "device": torch.cuda.get_device_properties(0).name,
        "shape": {"groups": n, "k": [5, 15], "len": [64, 1350], "payload_align": align,
                  "acc_stride": stride, "map_stride": ms, "packets": npk,
                  "payload_bytes": payload_bytes,
                  "table_bytes_per_candidate": "8 + 2 + 1 + 1 in, 1 + 8 + 2 out when admitted"},
        "expectation": "stated before measuring: tables of about 25 B per packet against about "
                       "700 B of payload, so the admit should cost a few percent of the fold",
        "method": {"timer": "HIP events around back-to-back rounds, as many as fill window_ms; the "
                            "round trip on the host's wall clock, one at a time",
                   "inner": args.inner, "window_ms": args.window_ms, "reps": args.reps,
                   "warmup": args.warmup, "rounds_per_window": inner,
                   "order": ", ".join(order) + ", alternating; then the round trips",
                   "round": "every leg: acc_len zeroed by one device memset (the `restore` row "
                            "alone), so the slots are fresh, then the calls; ratios are given "
                            "without the restore",
                   "ratio_ranges": "p10 over p90 and p90 over p10 of the two legs: bounds, not "
                                   "percentiles of a paired ratio",
                   "round_trip": "qfec_sync behind a fold in flight + D2H of ok into pinned memory; "
                                 "NumPy rebuild (mask, reduceat, cumsum, two gathers) into pinned "
                                 "memory; H2D of the three tables.  SUPPOSED: a native loop "
                                 "rebuilds several times faster than NumPy; the copies and the "
                                 "sync do not change with it",
                   "verified": "after timing: every admit leg's verdict, grp_ptr_out, tables, "
                               "maps and counts equal the NumPy rule (vectorised here, equal to "
                               "tests/admit_rule.py on the first %d groups); the rows and lengths "
                               "of both folding legs equal each other and qfec_encode_ragged over "
                               "the admitted packets; the round trip's tables equal the rule's"
                               % min(args.sample, n)},
        "restore_us": us["restore"],
        "admit": admit_rows,
        "turn": pair,
    }
    for row in admit_rows:
        print(json.dumps(row))
    print(json.dumps(pair), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
