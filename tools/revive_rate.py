#!/usr/bin/env python3
"""qfec_revive_batch against the dense one-pass recover, by revived fraction.

One MI355X, 2^20 groups x 10 x 1350 B resident on the device.  For each
revived fraction (1.0, 0.25, 0.05, 0.0; every other group complete) the
revive call (out of place and in place) alternates in this process with
qfec_recover_batch under QFEC_ONE_PASS on the same rows and parity buffers:
warm-up, then `--reps` rounds of revive / revive in place / dense, each timed
with HIP events around back-to-back calls -- `--inner` of them, or as many as
fill a window of `--window-ms` (the calls of a batch with little to revive
take tens of microseconds: four of them would measure the clock); the table
holds medians and the 10th / 90th percentiles.  Algorithmic bytes of a revived group:
(k - 1) L row bytes + L parity bytes read, L bytes written = (k + 1) L.

--ragged: qfec_revive_ragged against qfec_recover_ragged over all groups, on
BASELINE configs[3] in the payload arena's layout (2^20 groups, k 5-15,
64-1350 B, payloads on 16-B boundaries, 1,536-B parity / out slots: bench.py's
default ragged line), same fractions, same method; bytes of a revived group:
its received packets and its parity read, its parity length written.

Writes one JSON document (default profiles/revive_rate.json, with --ragged
profiles/revive_ragged_rate.json); DESIGN.md §4 quotes both.  Needs the GPU:
there is no fallback.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def pct(v, q):
    return float(np.percentile(np.asarray(v), q))


def make_timers(torch, args):
    def timed(fn, inner):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / inner  # us per call

    def calls_per_window(fn):
        """Warm fn up; the calls that fill the window (at least --inner, at most 4096)."""
        for _ in range(args.warmup):
            est = timed(fn, args.inner)
        return int(min(4096, max(args.inner, np.ceil(args.window_ms * 1e3 / est))))

    return timed, calls_per_window


METHOD = {"timer": "HIP events around back-to-back calls: `inner` of them or, for "
                   "short calls, as many as fill `window_ms` (calls_per_window)"}


def main_ragged(args):
    import torch
    from libquic_amd import qfec, synth
    from oracle import qfec_np as Q

    if not torch.cuda.is_available():
        sys.exit("revive_rate: no HIP device (this tool only measures on the GPU)")
    dev = "cuda:0"
    n, align, slot = args.groups, 16, 1536
    timed, calls_per_window = make_timers(torch, args)
    ctx = qfec.Context(0)
    ctx.set_stream(torch.cuda.current_stream())
    gs = np.arange(n, dtype=np.uint64)
    ks, ptr, ln, off = synth.ragged_layout(0, n, 5, 15, 64, 1350, Q.SEED_RAGGED, align=align)
    miss_np = synth.drop_indices(Q.SEED_DROP, gs, ks).astype(np.uint8)
    plen_np = np.maximum.reduceat(ln, ptr[:-1].astype(np.int64)).astype(np.int64)
    lost = ptr[:-1].astype(np.int64) + miss_np
    # bytes a revived group moves: received packets + parity in, parity length out
    gbytes = (np.add.reduceat(ln.astype(np.int64), ptr[:-1].astype(np.int64))
              - ln[lost].astype(np.int64) + 2 * plen_np)
    t_off = torch.from_numpy(off.view(np.int64)).to(dev)
    t_len = torch.from_numpy(ln.view(np.int16)).to(dev)
    t_ptr = torch.from_numpy(ptr.view(np.int32)).to(dev)
    t_poff = torch.from_numpy((gs * np.uint64(slot)).view(np.int64)).to(dev)
    miss = torch.from_numpy(miss_np).to(dev)
    data = torch.empty(int(off[-1]) + int(ln[-1]), dtype=torch.uint8, device=dev)
    ctx.synth_ragged(data, t_off, t_len, t_ptr, 0, n, Q.SEED_RAGGED)
    par = torch.empty(n * slot, dtype=torch.uint8, device=dev)
    plen = torch.empty(n, dtype=torch.int16, device=dev)
    ctx.encode_ragged(data, t_off, t_len, t_ptr, n, par, t_poff, plen)
    out = torch.empty(n * slot, dtype=torch.uint8, device=dev)
    dense_out = torch.empty(n * slot, dtype=torch.uint8, device=dev)
    status = torch.empty(n, dtype=torch.uint8, device=dev)
    ridx = torch.empty(n, dtype=torch.uint8, device=dev)
    rlist = torch.empty(n, dtype=torch.int64, device=dev)
    counts = torch.zeros(3, dtype=torch.int64, device=dev)
    ctx.sync()

    def dense():
        ctx.recover_ragged(data, t_off, t_len, t_ptr, n, par, t_poff, plen, miss, dense_out,
                           t_poff)

    rng = np.random.default_rng(20)
    table = []
    for f in args.fractions:
        revived = rng.random(n) < f if 0.0 < f < 1.0 else np.full(n, f >= 1.0)
        rcv = np.ones(ln.size, dtype=bool)
        rcv[lost[revived]] = False
        maps_np = qfec.pack_received_ragged(rcv, np.ones(n, dtype=bool), ptr, 2)
        maps = torch.from_numpy(maps_np.ravel()).to(dev)
        n_rev = int(revived.sum())

        def revive():
            ctx.revive_ragged(data, t_off, t_len, t_ptr, n, par, t_poff, plen, maps, 2, out,
                              t_poff, status=status, revived_idx=ridx, revived_list=rlist,
                              counts=counts)

        # the results at the timed size, against the dense call on the same buffers
        out.fill_(0)
        dense_out.fill_(0)
        revive()
        dense()
        ctx.sync()
        torch.cuda.synchronize()
        sel = torch.from_numpy(np.flatnonzero(revived)).to(dev)
        assert counts.tolist() == [n - n_rev, n_rev, 0], counts.tolist()
        assert torch.equal(rlist[:n_rev], sel)
        assert torch.equal(ridx[sel], miss[sel])
        assert torch.equal(out.view(n, slot)[sel], dense_out.view(n, slot)[sel])

        fns = {"revive": revive, "dense": dense}
        inner = {name: calls_per_window(fn) for name, fn in fns.items()}
        t = {name: [] for name in fns}
        for _ in range(args.reps):
            for name, fn in fns.items():
                t[name].append(timed(fn, inner[name]))
        ctx.sync()
        row = {"fraction": f, "revived_groups": n_rev, "calls_per_window": inner}
        for name, v in t.items():
            row[name + "_us"] = {"median": pct(v, 50), "p10": pct(v, 10), "p90": pct(v, 90)}
        med = row["revive_us"]["median"]
        row["revive_over_dense"] = med / row["dense_us"]["median"]
        row["revive_revived_TBps"] = int(gbytes[revived].sum()) / (med * 1e-6) / 1e12
        row["dense_TBps"] = int(gbytes.sum()) / (row["dense_us"]["median"] * 1e-6) / 1e12
        table.append(row)
        print(json.dumps(row), flush=True)

    full = next((r for r in table if r["fraction"] >= 1.0), None)
    floor = next((r for r in table if r["fraction"] <= 0.0), None)
    for r in table:
        # time above the nothing-to-do floor per revived fraction, against the same
        # at fraction 1: 1.0 = the time falls in proportion to the fraction
        if full and floor and 0.0 < r["fraction"]:
            r["proportionality"] = ((r["revive_us"]["median"] - floor["revive_us"]["median"])
                                    / r["fraction"]
                                    / (full["revive_us"]["median"] - floor["revive_us"]["median"]))
    doc = {
        "tool": "tools/revive_rate.py --ragged",
        "device": torch.cuda.get_device_properties(0).name,
        "shape": {"groups": n, "k": [5, 15], "len": [64, 1350], "payload_align": align,
                  "slot": slot, "map_stride": 2, "packets": int(ln.size),
                  "bytes_all_groups": int(gbytes.sum())},
        "method": dict(METHOD, inner=args.inner, window_ms=args.window_ms, reps=args.reps,
                       warmup=args.warmup,
                       order="revive, dense ragged recover, alternating",
                       dense="qfec_recover_ragged over all groups on the same buffers"),
        "fixed_call_floor_us": 22.0,
        "table": table,
    }
    if floor:
        doc["floor_over_fixed_call_floor"] = floor["revive_us"]["median"] / 22.0
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    ctx.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--groups", type=int, default=1 << 20)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--L", type=int, default=1350)
    ap.add_argument("--fractions", type=float, nargs="+", default=[1.0, 0.25, 0.05, 0.0])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=4)
    ap.add_argument("--window-ms", type=float, default=20.0,
                    help="least timed window; short calls repeat until they fill it")
    ap.add_argument("--ragged", action="store_true",
                    help="qfec_revive_ragged on configs[3] against qfec_recover_ragged")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "revive_ragged_rate.json" if args.ragged
                                else "revive_rate.json")
    if args.ragged:
        return main_ragged(args)

    import torch
    from libquic_amd import qfec
    from oracle import qfec_np as Q

    if not torch.cuda.is_available():
        sys.exit("revive_rate: no HIP device (this tool only measures on the GPU)")
    dev = "cuda:0"
    n, k, L = args.groups, args.k, args.L
    group_bytes = (k + 1) * L
    ctx = qfec.Context(0)
    ctx.set_stream(torch.cuda.current_stream())
    rows = torch.empty(n * k * L, dtype=torch.uint8, device=dev)
    ctx.synth_fixed(rows, k, L, 0, n, Q.SEED_FIXED)
    par = torch.empty(n * L, dtype=torch.uint8, device=dev)
    ctx.encode(rows, k, L, n, par)
    out = torch.empty(n * L, dtype=torch.uint8, device=dev)
    dense_out = torch.empty(n * L, dtype=torch.uint8, device=dev)
    status = torch.empty(n, dtype=torch.uint8, device=dev)
    ridx = torch.empty(n, dtype=torch.uint8, device=dev)
    rlist = torch.empty(n, dtype=torch.int64, device=dev)
    counts = torch.zeros(3, dtype=torch.int64, device=dev)
    miss_np = Q.drop_index(Q.SEED_DROP, np.arange(n), k).astype(np.uint8)
    miss = torch.from_numpy(miss_np).to(dev)
    ctx.sync()

    timed, calls_per_window = make_timers(torch, args)

    def dense():
        ctx.recover(rows, par, miss, k, L, n, dense_out, one_pass=True)

    rng = np.random.default_rng(20)
    table = []
    for f in args.fractions:
        revived = rng.random(n) < f if 0.0 < f < 1.0 else np.full(n, f >= 1.0)
        data = np.ones((n, k), dtype=bool)
        data[np.flatnonzero(revived), miss_np[revived].astype(np.int64)] = False
        maps = torch.from_numpy(qfec.pack_received(data, np.ones(n, dtype=bool)).ravel()).to(dev)
        n_rev = int(revived.sum())

        def revive():
            ctx.revive(rows, par, maps, k, L, n, out, status=status, revived_idx=ridx,
                       revived_list=rlist, counts=counts)

        def revive_in_place():
            # (rows already hold the lost packets: the call rewrites the same bytes)
            ctx.revive(rows, par, maps, k, L, n, None, status=status, revived_idx=ridx,
                       revived_list=rlist, counts=counts)

        # the results at the timed size, against the dense call on the same buffers
        out.fill_(0)
        revive()
        dense()
        ctx.sync()
        torch.cuda.synchronize()
        sel = torch.from_numpy(np.flatnonzero(revived)).to(dev)
        assert counts.tolist() == [n - n_rev, n_rev, 0], counts.tolist()
        assert torch.equal(rlist[:n_rev], sel)
        assert torch.equal(out.view(n, L)[sel], dense_out.view(n, L)[sel])
        keep = rows.clone()
        revive_in_place()
        ctx.sync()
        assert torch.equal(rows, keep)
        del keep

        fns = {"revive": revive, "revive_in_place": revive_in_place, "dense": dense}
        inner = {name: calls_per_window(fn) for name, fn in fns.items()}
        t = {name: [] for name in fns}
        for _ in range(args.reps):
            for name, fn in fns.items():
                t[name].append(timed(fn, inner[name]))
        ctx.sync()
        row = {"fraction": f, "revived_groups": n_rev, "calls_per_window": inner}
        for name, v in t.items():
            row[name + "_us"] = {"median": pct(v, 50), "p10": pct(v, 10), "p90": pct(v, 90)}
        for name in ("revive", "revive_in_place"):
            med = row[name + "_us"]["median"]
            row[name + "_over_dense"] = med / row["dense_us"]["median"]
            row[name + "_revived_TBps"] = n_rev * group_bytes / (med * 1e-6) / 1e12
        row["dense_TBps"] = n * group_bytes / (row["dense_us"]["median"] * 1e-6) / 1e12
        table.append(row)
        print(json.dumps(row), flush=True)

    doc = {
        "tool": "tools/revive_rate.py",
        "device": torch.cuda.get_device_properties(0).name,
        "shape": {"groups": n, "k": k, "L": L, "bytes_per_revived_group": group_bytes},
        "method": {"timer": METHOD["timer"],
                   "inner": args.inner, "window_ms": args.window_ms,
                   "reps": args.reps, "warmup": args.warmup,
                   "order": "revive, revive in place, dense one-pass recover, alternating",
                   "dense": "qfec_recover_batch with QFEC_ONE_PASS on the same rows / parity"},
        "table": table,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
