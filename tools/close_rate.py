#!/usr/bin/env python3
"""qfec_emit_accumulated / qfec_revive_accumulated against their baselines.

One MI355X, BASELINE configs[3] in the payload arena's layout resident on the
device: 2^20 groups, k 5-15, 64-1350 B, payloads on 16-B boundaries, 2^20
running rows of 1,536 B, outputs in 1,536-B slots.

  (a) emit:   every row out with release, beside the box's own copy rate:
              qfec_stream_probe in copy mode over the same number of bytes
              (the rows' lengths summed), one contiguous buffer.
  (b) revive: qfec_revive_accumulated (release_mask 0b011) with 0%, 5% and 25%
              of the groups revivable and the rest complete, beside
              qfec_revive_ragged over the same groups held whole -- the way to
              the same bytes without the accumulator.  The rows hold what a
              receiver's folds leave (the dense recover's output per group).

A release zeroes acc_len, so a round of the accumulated legs first restores the
lengths (one 2-MB device copy, timed with the round and reported on its own as
`restore`).  The legs alternate in this process: warm-up, then `--reps`
alternations, each timed with HIP events around back-to-back rounds -- as many
as fill `--window-ms`; the table holds medians and the 10th / 90th percentiles.
After timing, the emit's output equals the encode's parity and lengths and each
revive's outputs equal qfec_revive_ragged's, whole buffers.

Writes one JSON document (default profiles/close_rate.json); DESIGN.md §4
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "close_rate.json"))
    args = ap.parse_args()

    import torch
    from libquic_amd import qfec, synth
    from oracle import qfec_np as Q

    if not torch.cuda.is_available():
        sys.exit("close_rate: no HIP device (this tool only measures on the GPU)")
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
    row_bytes = int(plen_np.sum())

    def up(a, view):
        return torch.from_numpy(np.ascontiguousarray(a).view(view)).to(dev)

    t_off, t_len, t_ptr = up(off, np.int64), up(ln, np.int16), up(ptr, np.int32)
    t_poff = up(gs * np.uint64(slot), np.int64)
    t_k = up(ks.astype(np.uint8), np.uint8)
    data = torch.empty(int(off[-1]) + int(ln[-1]) + 16, dtype=torch.uint8, device=dev)
    ctx.synth_ragged(data, t_off, t_len, t_ptr, 0, n, Q.SEED_RAGGED)
    par = torch.zeros(n * slot, dtype=torch.uint8, device=dev)
    plen = torch.zeros(n, dtype=torch.int16, device=dev)
    ctx.encode_ragged(data, t_off, t_len, t_ptr, n, par, t_poff, plen)

    # sender rows: every group folded whole
    acc = torch.zeros(n * slot, dtype=torch.uint8, device=dev)
    acc_len = torch.zeros(n, dtype=torch.int16, device=dev)
    ctx.accumulate_ragged(data, t_off, t_len, t_ptr, n, acc, slot, acc_len, n_slots=n)
    # receiver rows: what folding every packet but `lost` and the redundancy leaves
    rng = np.random.default_rng(20261020)
    lost = (rng.integers(0, 1 << 30, n) % ks).astype(np.uint8)
    t_lost = up(lost, np.uint8)
    rx = torch.zeros(n * slot, dtype=torch.uint8, device=dev)
    ctx.recover_ragged(data, t_off, t_len, t_ptr, n, par, t_poff, plen, t_lost, rx, t_poff)
    rx_len = plen.clone()
    ctx.sync()
    torch.cuda.synchronize()
    assert torch.equal(acc, par) and torch.equal(acc_len, plen)

    out = torch.zeros(n * slot, dtype=torch.uint8, device=dev)
    out_len = torch.zeros(n, dtype=torch.int16, device=dev)
    out_rag = torch.zeros(n * slot, dtype=torch.uint8, device=dev)
    flat_src = torch.empty(row_bytes, dtype=torch.uint8, device=dev).random_(0, 256)
    flat_dst = torch.empty(row_bytes, dtype=torch.uint8, device=dev)

    def outputs():
        return {"status": torch.zeros(n, dtype=torch.uint8, device=dev),
                "idx": torch.zeros(n, dtype=torch.uint8, device=dev),
                "list": torch.zeros(n, dtype=torch.int64, device=dev),
                "counts": torch.zeros(3, dtype=torch.int64, device=dev)}

    fracs = [0.0, 0.05, 0.25]
    legs = {}
    for f in fracs:
        rev = rng.random(n) < f
        rcv = np.ones(ln.size, bool)
        rcv[p0[rev] + lost[rev].astype(np.int64)] = False
        maps = qfec.pack_received_ragged(rcv, np.ones(n, bool), ptr)
        legs[f] = {"maps": up(maps, np.uint8), "ms": int(maps.shape[1]), "revived": int(rev.sum()),
                   "bytes": int(plen_np[rev].sum()), "acc": outputs(), "rag": outputs()}

    def restore_tx():
        acc_len.copy_(plen)

    def restore_rx():
        rx_len.copy_(plen)

    def emit():
        restore_tx()
        ctx.emit_accumulated(acc, slot, acc_len, n, out, t_poff, out_len, release=True)

    def copy():
        ctx.stream_probe(flat_src, row_bytes, flat_dst, copy=True)

    def revive_acc(f):
        L, o = legs[f], legs[f]["acc"]

        def fn():
            restore_rx()
            ctx.revive_accumulated(rx, slot, rx_len, t_k, L["maps"], L["ms"], n, out, t_poff,
                                   out_len, status=o["status"], revived_idx=o["idx"],
                                   revived_list=o["list"], counts=o["counts"], release_mask=0b011)
        return fn

    def revive_rag(f):
        L, o = legs[f], legs[f]["rag"]

        def fn():
            ctx.revive_ragged(data, t_off, t_len, t_ptr, n, par, t_poff, plen, L["maps"], L["ms"],
                              out_rag, t_poff, status=o["status"], revived_idx=o["idx"],
                              revived_list=o["list"], counts=o["counts"])
        return fn

    fns = {"emit": emit, "copy": copy, "restore": restore_rx}
    order = ["emit", "copy", "restore"]
    for f in fracs:
        fns[f"revive_accumulated_{f:g}"] = revive_acc(f)
        fns[f"revive_ragged_{f:g}"] = revive_rag(f)
        order += [f"revive_accumulated_{f:g}", f"revive_ragged_{f:g}"]
    inner = {name: rounds_per_window(fns[name]) for name in order}
    t = {name: [] for name in order}
    for _ in range(args.reps):
        for name in order:
            t[name].append(timed(fns[name], inner[name]))
    ctx.sync()

    # the outputs of the timed calls
    out.zero_()
    emit()
    ctx.sync()
    torch.cuda.synchronize()
    assert torch.equal(out, par) and torch.equal(out_len, plen) and not acc_len.any()
    for f in fracs:
        out.zero_()
        out_rag.zero_()
        fns[f"revive_accumulated_{f:g}"]()
        fns[f"revive_ragged_{f:g}"]()
        ctx.sync()
        torch.cuda.synchronize()
        a, r = legs[f]["acc"], legs[f]["rag"]
        cnt = int(a["counts"][1])
        assert cnt == legs[f]["revived"] and torch.equal(a["counts"], r["counts"]), f
        assert torch.equal(a["status"], r["status"]) and torch.equal(a["idx"], r["idx"]), f
        assert torch.equal(a["list"][:cnt], r["list"][:cnt]), f
        assert torch.equal(out, out_rag), f
        assert torch.equal(out_len, torch.where(a["status"] == 1, plen, torch.zeros_like(plen))), f
        assert not rx_len.any(), f  # every group was complete or revived: all released

    us = {name: {"median": pct(v, 50), "p10": pct(v, 10), "p90": pct(v, 90)}
          for name, v in t.items()}
    rst = us["restore"]["median"]
    emit_row = {"bytes_read_plus_written": 2 * row_bytes, "us": us["emit"],
                "us_without_restore": us["emit"]["median"] - rst,
                "TBps": 2 * row_bytes / (us["emit"]["median"] * 1e-6) / 1e12,
                "copy_us": us["copy"],
                "copy_TBps": 2 * row_bytes / (us["copy"]["median"] * 1e-6) / 1e12,
                "time_over_copy": us["emit"]["median"] / us["copy"]["median"],
                "time_without_restore_over_copy": (us["emit"]["median"] - rst)
                / us["copy"]["median"]}
    table = []
    for f in fracs:
        a, r = us[f"revive_accumulated_{f:g}"], us[f"revive_ragged_{f:g}"]
        table.append({"revivable": f, "revived_groups": legs[f]["revived"],
                      "revived_bytes": legs[f]["bytes"], "revive_accumulated_us": a,
                      "revive_accumulated_us_without_restore": a["median"] - rst,
                      "revive_ragged_us": r,
                      "time_over_ragged": a["median"] / r["median"],
                      "time_without_restore_over_ragged": (a["median"] - rst) / r["median"]})
    doc = {
        "tool": "tools/close_rate.py",
        "device": torch.cuda.get_device_properties(0).name,
        "shape": {"groups": n, "k": [5, 15], "len": [64, 1350], "payload_align": align,
                  "acc_stride": slot, "out_slot": slot, "packets": int(ln.size),
                  "row_bytes": row_bytes},
        "method": {"timer": "HIP events around back-to-back rounds, as many as fill window_ms",
                   "inner": args.inner, "window_ms": args.window_ms, "reps": args.reps,
                   "warmup": args.warmup, "rounds_per_window": inner,
                   "order": ", ".join(order) + ", alternating",
                   "round": "accumulated legs: acc_len restored by one device copy (the "
                            "`restore` row alone), then the call; the others: the call",
                   "verified": "after timing, the emit's out / out_len equal "
                               "qfec_encode_ragged's parity and lengths and each "
                               "revive_accumulated's out, status, revived_idx, revived_list "
                               "and counts equal qfec_revive_ragged's (whole buffers)"},
        "restore_us": us["restore"],
        "emit": emit_row,
        "revive": table,
    }
    print(json.dumps(emit_row))
    for row in table:
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
