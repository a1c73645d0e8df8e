#!/usr/bin/env python3
"""qfec_accumulate_ragged against qfec_encode_ragged over the same packets.

One MI355X, BASELINE configs[3] in the payload arena's layout resident on the
device: 2^20 groups, k 5-15, 64-1350 B, payloads on 16-B boundaries, 1,536-B
accumulator rows (and parity slots for the encode).  Three shapes of the same
work, each leaving every group's parity in its accumulator row:

  (a) whole:   every group whole in one call into fresh slots (acc_len 0).
               The algorithmic bytes are the encode's (packets read, parity
               written), so the time ratio to qfec_encode_ragged is what the
               accumulate mode costs.
  (b) halves:  each group in two calls (the first ceil(k / 2) packets, then the
               rest); bytes: packets read + old row read + new row written.
  (c) singles: one packet per group per call, 15 calls; call i lists the groups
               that have a packet i, by slot.  Same byte count as (b).

A round of a shape resets acc_len to zero (one memset, timed with the round
and reported on its own as well) and makes the shape's calls.  The rounds
alternate in this process with qfec_encode_ragged: warm-up, then `--reps`
alternations, each timed with HIP events around back-to-back rounds -- as many
as fill `--window-ms`; the table holds medians and the 10th / 90th
percentiles.  After timing, the accumulator rows and lengths each shape left
are compared with the encode's parity and lengths, whole buffers.

Writes one JSON document (default profiles/accumulate_rate.json); DESIGN.md §4
quotes it.  Needs the GPU: there is no fallback.
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


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--groups", type=int, default=1 << 20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=2)
    ap.add_argument("--window-ms", type=float, default=20.0,
                    help="least timed window; rounds repeat until they fill it")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "accumulate_rate.json"))
    args = ap.parse_args()

    import torch
    from libquic_amd import qfec, synth
    from oracle import qfec_np as Q

    if not torch.cuda.is_available():
        sys.exit("accumulate_rate: no HIP device (this tool only measures on the GPU)")
    dev = "cuda:0"
    n, align, slot = args.groups, 16, 1536
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

    gs = np.arange(n, dtype=np.uint64)
    ks, ptr, ln, off = synth.ragged_layout(0, n, 5, 15, 64, 1350, Q.SEED_RAGGED, align=align)
    p0 = ptr[:-1].astype(np.int64)
    plen_np = np.maximum.reduceat(ln, p0).astype(np.int64)
    pkt_bytes = int(ln.astype(np.int64).sum())
    idx_in_group = np.arange(ln.size, dtype=np.int64) - np.repeat(p0, ks)

    def up(a, view):
        return torch.from_numpy(np.ascontiguousarray(a).view(view)).to(dev)

    t_off, t_len, t_ptr = up(off, np.int64), up(ln, np.int16), up(ptr, np.int32)
    t_poff = up(gs * np.uint64(slot), np.int64)
    data = torch.empty(int(off[-1]) + int(ln[-1]) + 16, dtype=torch.uint8, device=dev)
    ctx.synth_ragged(data, t_off, t_len, t_ptr, 0, n, Q.SEED_RAGGED)
    par = torch.zeros(n * slot, dtype=torch.uint8, device=dev)
    plen = torch.zeros(n, dtype=torch.int16, device=dev)
    acc = torch.zeros(n * slot, dtype=torch.uint8, device=dev)
    acc_len = torch.zeros(n, dtype=torch.int16, device=dev)
    ctx.sync()

    def sub_batch(sel_pkts, groups):
        """CSR tables of the packets sel_pkts (ascending), which belong to `groups`
        (ascending group numbers, each with at least one of them)."""
        cnt = np.bincount(np.repeat(np.arange(n), ks)[sel_pkts], minlength=n)[groups]
        sptr = np.zeros(groups.size + 1, np.uint32)
        sptr[1:] = np.cumsum(cnt)
        return {"off": up(off[sel_pkts], np.int64), "len": up(ln[sel_pkts], np.int16),
                "ptr": up(sptr, np.int32), "n": int(groups.size),
                "slot": None if groups.size == n else up(groups.astype(np.uint32), np.int32),
                "max": np.maximum.reduceat(ln[sel_pkts], sptr[:-1].astype(np.int64))}

    def call(b):
        ctx.accumulate_ragged(data, b["off"], b["len"], b["ptr"], b["n"], acc, slot, acc_len,
                              slot=b["slot"], n_slots=n)

    half = (ks + 1) // 2
    first = idx_in_group < np.repeat(half, ks)
    all_groups = np.arange(n)
    b_whole = sub_batch(np.arange(ln.size), all_groups)
    b_halves = [sub_batch(np.flatnonzero(first), all_groups),
                sub_batch(np.flatnonzero(~first), all_groups)]
    b_singles = [sub_batch(np.flatnonzero(idx_in_group == i), np.flatnonzero(ks > i))
                 for i in range(int(ks.max()))]

    def moved(batches):
        """packets read + old rows read + new rows written, over a round's calls"""
        cur = np.zeros(n, np.int64)
        total = pkt_bytes
        for b in batches:
            g = all_groups if b["slot"] is None else b["slot"].cpu().numpy().view(np.uint32)
            new = np.maximum(cur[g], b["max"].astype(np.int64))
            total += int(cur[g].sum()) + int(new.sum())
            cur[g] = new
        assert np.array_equal(cur, plen_np)
        return total

    def reset():
        acc_len.zero_()

    def encode():
        ctx.encode_ragged(data, t_off, t_len, t_ptr, n, par, t_poff, plen)

    def make_round(batches):
        def fn():
            reset()
            for b in batches:
                call(b)
        return fn

    shapes = {"whole": [b_whole], "halves": b_halves, "singles": b_singles}
    fns = {"encode": encode, "reset": reset}
    fns.update({name: make_round(bs) for name, bs in shapes.items()})
    order = ["whole", "encode", "halves", "singles", "reset"]
    inner = {name: rounds_per_window(fns[name]) for name in order}
    t = {name: [] for name in order}
    for _ in range(args.reps):
        for name in order:
            t[name].append(timed(fns[name], inner[name]))
    ctx.sync()

    # the outputs of the timed calls: every shape left the encode's parity
    for name in shapes:
        acc.zero_()
        fns[name]()
        ctx.sync()
        torch.cuda.synchronize()
        assert torch.equal(acc_len, plen), name
        assert torch.equal(acc, par), name

    us = {name: {"median": pct(v, 50), "p10": pct(v, 10), "p90": pct(v, 90)}
          for name, v in t.items()}
    enc_bytes = pkt_bytes + int(plen_np.sum())
    table = []
    for name, bs in shapes.items():
        by = moved(bs)
        med = us[name]["median"]
        table.append({"shape": name, "calls_per_round": len(bs), "bytes": by, "us": us[name],
                      "us_without_reset": med - us["reset"]["median"],
                      "TBps": by / (med * 1e-6) / 1e12,
                      "time_over_encode": med / us["encode"]["median"],
                      "bytes_over_encode": by / enc_bytes})
    doc = {
        "tool": "tools/accumulate_rate.py",
        "device": torch.cuda.get_device_properties(0).name,
        "shape": {"groups": n, "k": [5, 15], "len": [64, 1350], "payload_align": align,
                  "acc_stride": slot, "packets": int(ln.size), "packet_bytes": pkt_bytes,
                  "parity_bytes": int(plen_np.sum())},
        "method": {"timer": "HIP events around back-to-back rounds, as many as fill window_ms",
                   "inner": args.inner, "window_ms": args.window_ms, "reps": args.reps,
                   "warmup": args.warmup, "rounds_per_window": inner,
                   "order": ", ".join(order) + ", alternating",
                   "round": "acc_len memset to 0 (the `reset` row alone), then the shape's calls",
                   "verified": "after timing, every shape's rows and lengths equal "
                               "qfec_encode_ragged's parity and lengths (whole buffers)"},
        "encode": {"bytes": enc_bytes, "us": us["encode"],
                   "TBps": enc_bytes / (us["encode"]["median"] * 1e-6) / 1e12},
        "reset_us": us["reset"],
        "table": table,
    }
    print(json.dumps(doc["encode"]))
    for row in table:
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
