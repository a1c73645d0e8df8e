#!/usr/bin/env python3
"""qfec_retire_groups beside the assign it runs in front of.

One MI355X, the workload and protocol of tools/assign_rate.py: BASELINE
configs[3], 2^20 groups, 2^20 slots (group g open in slot g unless a leg says
otherwise), k 5-15, about 10.5 M packets, every data packet a candidate of the
turn, the arrival order a uniform random permutation.  Group g's key is
(g % 4096) << 40 | g // 4096 + 1: 4,096 connections of 256 groups, key_shift 40.
A record of this call is (pkt_key 8) in and (pkt_key_out 8) out per packet,
(slot_key 8, acc_len 2) per slot.

  (a) nothing to close: marks 0, max_groups 0;
  (b) max_groups 2 with every connection over the bound: 254 of every 256
      slots close, every packet but those of two groups a connection is refused;
  (c) n_packets == 0, one raise per connection to 14: the pure
      CloseFecGroupsBefore, 13 of every 256 slots (5%) close;
  (d) a sparse turn: the packets of 1% of the groups, marks 0, max_groups 0;
  (e) the contention case: the same packets keyed onto 4 connections
      ((g % 4) << 40 | g // 4 + 1), max_groups 2 -- every atomic of a round on
      one of four words;
  (f) the turn, every group new: retire + assign + bin + admit + accumulate
      beside assign + bin + admit + accumulate over the same arrivals.
  The yardstick is qfec_assign_slots alone on the same inputs in the same
  process ((c) has no packets: (a)'s assign).  A round of a retire leg first
  restores the 2 MB of lengths and the 32 KB of marks (timed with the round and
  on its own as `restore`); a round of a turn zeroes the lengths.

EXPECTATION, stated before the first run, to confirm or refute.  The call
builds no table: a pass streams 84 MB of packet keys and 10.5 MB of slot keys
and lengths, 30-40 us at 3 TB/s, and with max_groups 0 the packets are read
once (filter: 84 MB in, 84 MB out, a gathered 8-byte mark per packet out of a
32-KB table that stays in L2) and the slots twice (classify, close).  (a):
80-140 us, a fifth of the assign on the same inputs or less (that was 600-900
us).  (b): three retain rounds more, each a streaming pass plus atomics that
the load in front of them turns away once a connection's word holds its
maximum; in a random order runs are short, so a round is SUPPOSED 40-90 us and
(b) 250-400 us, still below the assign.  (c): no packet pass at all, four small
kernels and a memset: 25-50 us, launch-bound.  (d): 105 k packets; the two slot
passes and the launches dominate: 25-50 us, below the sparse assign's 60-150.
(e): four words take every atomic of a round; the load in front SHOULD keep
nearly all of them away, but the first wave of each round cannot know, and the
losers of a same-address 64-bit atomic serialise in L2: SUPPOSED 1-3 times
(b)'s rounds, and the one leg that may pass the assign.  (f): the retire adds
its (a) figure to a turn of about 3 ms: 3-5%.

The legs alternate in this process: warm-up, then `--reps` alternations, each
timed with HIP events around back-to-back rounds -- as many as fill
`--window-ms`; medians with the 10th / 90th percentiles.  After timing every
retire leg's acc_len, conn_mark, pkt_key_out, closed_list and counts equal
tests/retire_rule.py run over the whole input, and leg (f)'s turn with the
retire leaves the rows and lengths of the turn without it.

Writes one JSON document (default profiles/retire_rate.json); DESIGN.md §4
quotes it.  Needs the GPU: there is no fallback.
"""
import argparse
import json
import os
import sys

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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "retire_rate.json"))
    args = ap.parse_args()

    import torch
    import retire_rule as RR
    from libquic_amd import qfec, synth
    from oracle import qfec_np as Q

    if not torch.cuda.is_available():
        sys.exit("retire_rate: no HIP device (this tool only measures on the GPU)")
    dev = "cuda:0"
    n, align, stride, ms, shift, n_conns = args.groups, 16, 1536, 2, 40, 4096
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
    group_key = ((g64 % np.uint64(n_conns)) << np.uint64(shift)) | (g64 // np.uint64(n_conns) + np.uint64(1))
    four_key = ((g64 % np.uint64(4)) << np.uint64(shift)) | (g64 // np.uint64(4) + np.uint64(1))
    per_conn = (n + n_conns - 1) // n_conns  # groups of a connection: the numbers 1 .. per_conn
    rng = np.random.default_rng(20261021)
    perm = rng.permutation(npk)
    some = np.sort(rng.permutation(n)[:max(1, n // 100)])
    sparse_order = rng.permutation(np.flatnonzero(np.isin(grp, some)))
    raise_to = per_conn * 5 // 100 + 2  # numbers 1 .. raise_to - 1 die: 5% of a connection's

    len_open = torch.full((n,), 9, dtype=torch.int16, device=dev)
    mark_zero = torch.zeros(n_conns, dtype=torch.int64, device=dev)
    slot_key_d = up(group_key, np.int64)
    slot_k_d = up(ks.astype(np.uint8), np.uint8)
    acc_len = torch.zeros(n, dtype=torch.int16, device=dev)  # every leg's working lengths
    marks = torch.zeros(n_conns, dtype=torch.int64, device=dev)  # ... and marks

    def leg(name, keys, max_groups, raises=None):
        m = int(keys.size)
        d = {"name": name, "m": m, "keys": keys, "max_groups": max_groups,
             "key": up(keys, np.int64) if m else None,
             "out": torch.zeros(max(m, 1), dtype=torch.int64, device=dev),
             "closed": torch.zeros(n, dtype=torch.int32, device=dev),
             "cnt": torch.zeros(5, dtype=torch.int64, device=dev),
             "a_out": torch.zeros(max(m, 1), dtype=torch.int32, device=dev),
             "k": up(np.ones(max(m, 1), np.uint8), np.uint8),
             "raises": raises, "rc": None, "rm": None}
        if raises is not None:
            d["rc"], d["rm"] = up(raises[0], np.int32), up(raises[1], np.int64)
        return d

    legs = [leg("a_nothing_to_close", group_key[grp[perm]], 0),
            leg("b_every_connection_over_2", group_key[grp[perm]], 2),
            leg("c_raises_only", np.zeros(0, np.uint64), 0,
                (np.arange(n_conns, dtype=np.uint32), np.full(n_conns, raise_to, np.uint64))),
            leg("d_sparse", group_key[grp[sparse_order]], 0),
            leg("e_four_connections", four_key[grp[perm]], 2)]

    def restore():
        acc_len.copy_(len_open)
        marks.copy_(mark_zero)

    def retire_fn(d):
        def fn():
            restore()
            ctx.retire_groups(d["key"], d["m"], slot_key_d, acc_len, n, marks, n_conns, shift,
                              d["max_groups"], d["out"] if d["m"] else None, raise_conn=d["rc"],
                              raise_mark=d["rm"], n_raise=n_conns if d["raises"] else 0,
                              closed_list=d["closed"], counts=d["cnt"])
        return fn

    def assign_fn(d):
        def fn():  # (an assign changes no length and, every key open, no slot table)
            ctx.assign_slots(d["key"], d["k"], d["m"], slot_key_d, slot_k_d, len_open, n, d["a_out"])
        return fn

    # (f) the turn, every group new: the slots free under stale keys
    m = npk
    new_keys = legs[0]["key"]
    stale_key_d = up(np.roll(group_key, 12345), np.int64)
    key_k = torch.ones(n, dtype=torch.uint8, device=dev)
    data = torch.empty(int(off[-1]) + int(ln[-1]) + 16, dtype=torch.uint8, device=dev)
    ctx.synth_ragged(data, up(off, np.int64), up(ln, np.int16), up(ptr, np.int32), 0, n,
                     Q.SEED_RAGGED)
    acc = torch.zeros(n * stride, dtype=torch.uint8, device=dev)
    maps = torch.full((n * ms,), 0xFF, dtype=torch.uint8, device=dev)  # stale: all ones
    b = {"k": up(ks[grp[perm]].astype(np.uint8), np.uint8), "off": up(off[perm], np.int64),
         "ln": up(ln[perm], np.int16), "idx": up(idx_in_group[perm], np.uint8),
         "ok": up(np.ones(m, np.uint8), np.uint8),
         "key_out": torch.zeros(m, dtype=torch.int64, device=dev),
         "slot": torch.zeros(m, dtype=torch.int32, device=dev),
         "t_ptr": torch.zeros(n + 1, dtype=torch.int32, device=dev),
         "t_off": torch.zeros(m, dtype=torch.int64, device=dev),
         "t_ln": torch.zeros(m, dtype=torch.int16, device=dev),
         "t_idx": torch.zeros(m, dtype=torch.uint8, device=dev),
         "t_ok": torch.zeros(m, dtype=torch.uint8, device=dev),
         "o_ptr": torch.zeros(n + 1, dtype=torch.int32, device=dev),
         "o_off": torch.zeros(m, dtype=torch.int64, device=dev),
         "o_ln": torch.zeros(m, dtype=torch.int16, device=dev),
         "v": torch.zeros(m, dtype=torch.uint8, device=dev)}

    def turn(with_retire):
        def fn():
            acc_len.zero_()
            marks.zero_()  # (both turns, so that they differ by the retire alone)
            keys = new_keys
            if with_retire:
                ctx.retire_groups(new_keys, m, stale_key_d, acc_len, n, marks, n_conns, shift, 0,
                                  b["key_out"])
                keys = b["key_out"]
            ctx.assign_slots(keys, b["k"], m, stale_key_d, key_k, acc_len, n, b["slot"])
            ctx.bin_arrivals(b["slot"], b["off"], b["ln"], b["idx"], b["ok"], m, n, b["t_ptr"],
                             b["t_off"], b["t_ln"], b["t_idx"], pkt_ok_out=b["t_ok"])
            ctx.admit_ragged(b["t_off"], b["t_ln"], b["t_idx"], b["t_ok"], b["t_ptr"], n, key_k,
                             maps, ms, acc_len, stride, b["o_ptr"], b["o_off"], b["o_ln"], b["v"])
            ctx.accumulate_ragged(data, b["o_off"], b["o_ln"], b["o_ptr"], n, acc, stride, acc_len)
        return fn

    fns = {"restore": restore}
    for d in legs:
        fns["retire_" + d["name"]] = retire_fn(d)
        if d["m"]:
            fns["assign_" + d["name"]] = assign_fn(d)
    marks.zero_()
    fns["turn_with_retire"], fns["turn_without_retire"] = turn(True), turn(False)
    order = list(fns)
    for name in order:  # every leg once on its own, so that a latched error names its leg
        fns[name]()
        try:
            ctx.sync()
        except qfec.QfecError as e:
            sys.exit(f"retire_rate: leg {name}: {e}")
    inner = {name: rounds_per_window(fns[name]) for name in order}
    t = {name: [] for name in order}
    for _ in range(args.reps):
        for name in order:
            t[name].append(timed(fns[name], inner[name]))
    ctx.sync()
    print("timed", flush=True)

    # the outputs of the timed calls against tests/retire_rule.py, whole inputs
    # (lists: the rule indexes one element at a time)
    slot_key_l = group_key.tolist()
    results = {}
    for d in legs:
        w_len, w_mark = [9] * n, [0] * n_conns
        w_out, w_closed = [0] * d["m"], [0] * n
        rc, rm = (d["raises"][0].tolist(), d["raises"][1].tolist()) if d["raises"] else ([], [])
        w_cnt = RR.retire_groups(d["keys"].tolist(), slot_key_l, w_len, w_mark, shift,
                                 d["max_groups"], rc, rm, w_out, w_closed)
        for name in ("out", "closed", "cnt"):
            d[name].fill_(-1)
        retire_fn(d)()
        ctx.sync()
        nc = int(w_cnt[RR.CLOSED])
        assert host(d["cnt"], np.uint64).tolist() == w_cnt.tolist(), d["name"]
        assert np.array_equal(host(acc_len, np.uint16), np.asarray(w_len, np.uint16)), d["name"]
        assert np.array_equal(host(marks, np.uint64), np.asarray(w_mark, np.uint64)), d["name"]
        assert np.array_equal(host(d["out"], np.uint64)[:d["m"]], np.asarray(w_out, np.uint64)), d["name"]
        assert np.array_equal(host(d["closed"], np.uint32)[:nc], np.asarray(w_closed[:nc], np.uint32)), \
            d["name"]
        results[d["name"]] = w_cnt.tolist()
        print(json.dumps({"verified": d["name"], "counts": results[d["name"]]}), flush=True)
    assert results["a_nothing_to_close"] == [0, 0, 0, npk, 0]
    assert results["b_every_connection_over_2"][0] == n - 2 * n_conns
    assert abs(results["c_raises_only"][0] / n - 0.05) < 0.01
    marks.zero_()
    rows = {}
    for name in ("turn_with_retire", "turn_without_retire"):
        acc.zero_()
        fns[name]()
        ctx.sync()
        rows[name] = (acc.clone(), acc_len.clone())
    assert torch.equal(rows["turn_with_retire"][0], rows["turn_without_retire"][0])
    assert torch.equal(rows["turn_with_retire"][1], rows["turn_without_retire"][1])
    assert int((rows["turn_with_retire"][1] != 0).sum()) == n
    del rows

    us = {name: {"median": pct(v, 50), "p10": pct(v, 10), "p90": pct(v, 90)}
          for name, v in t.items()}
    rst = us["restore"]["median"]
    table = []
    for d in legs:
        r = us["retire_" + d["name"]]
        yard = "assign_" + (d["name"] if d["m"] else legs[0]["name"])
        table.append({"leg": d["name"], "packets": d["m"], "slots": n, "max_groups": d["max_groups"],
                      "counts": results[d["name"]], "us": r,
                      "us_without_restore": r["median"] - rst, "assign_us": us[yard],
                      "assign_leg": yard,
                      "over_assign": (r["median"] - rst) / us[yard]["median"]})
    doc = {
        "tool": "tools/retire_rate.py",
        "device": torch.cuda.get_device_properties(0).name,
        "shape": {"groups": n, "slots": n, "connections": n_conns, "key_shift": shift,
                  "k": [5, 15], "packets": npk, "sparse_packets": int(sparse_order.size),
                  "raise_to": raise_to, "acc_stride": stride, "map_stride": ms,
                  "record_bytes": "8 in, 8 out per packet; 8 + 2 per slot"},
        "expectation": "stated before measuring (the tool's docstring has it in full): no table, "
                       "30-40 us a streaming pass; (a) 80-140 us, a fifth of the assign or less; "
                       "(b) 250-400 us, below the assign; (c) 25-50 us; (d) 25-50 us; (e) 1-3 times "
                       "(b)'s rounds, the one leg that may pass the assign; (f) 3-5% of the turn",
        "method": {"timer": "HIP events around back-to-back rounds, as many as fill window_ms",
                   "inner": args.inner, "window_ms": args.window_ms, "reps": args.reps,
                   "warmup": args.warmup, "rounds_per_window": inner,
                   "order": ", ".join(order) + ", alternating",
                   "round": "retire legs: acc_len and conn_mark restored by two device copies "
                            "(the `restore` row alone; us_without_restore and over_assign have it "
                            "subtracted), then the call; assign legs: the call; turns: acc_len "
                            "zeroed, then the calls",
                   "verified": "after timing: every retire leg's acc_len, conn_mark, pkt_key_out, "
                               "closed_list and counts equal tests/retire_rule.py over the whole "
                               "input; the turn with the retire leaves the rows and lengths of "
                               "the turn without it"},
        "restore_us": us["restore"],
        "retire": table,
        "turn": {"with_retire_us": us["turn_with_retire"],
                 "without_retire_us": us["turn_without_retire"],
                 "difference_us": us["turn_with_retire"]["median"] - us["turn_without_retire"]["median"],
                 "ratio": us["turn_with_retire"]["median"] / us["turn_without_retire"]["median"]},
    }
    for row in table:
        print(json.dumps(row))
    print(json.dumps({"turn": doc["turn"], "restore_us": doc["restore_us"]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
