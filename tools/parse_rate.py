#!/usr/bin/env python3
"""qfec_parse_opened beside the calls it runs in front of.

One MI355X, the workload and protocol of tools/retire_rate.py: BASELINE
configs[3], 2^20 groups of k 5-15 packets of 64-1350 bytes, 10,491,121 packets,
16-byte aligned in one arena of about 7.4 GB, the arrival order a uniform
random permutation.  A packet's first two bytes are its private header
(qfec_write_private_headers puts them there: flags 2, the position as the
offset), group g is number 16 * (g // 4096) + 1 on connection g % 4096, the
packet number is the group number plus the position, key_shift 40.  A record of
the parse is (pkt_off 8, pkt_len 2, packet_number 8, pkt_conn 4, pkt_ok 1) = 23
bytes in and (pkt_key_out 8, pkt_idx_out 1, body_off_out 8, body_len_out 2,
hdr_out 1, entropy_out 1) = 21 bytes out, plus the two header bytes wherever
the packet lies.

  (a) every packet in a group, pkt_ok NULL;
  (b) 5% of the packets FAILED (pkt_ok given);
  (c) a sparse turn: the packets of 1% of the groups;
  (d) the turn, every group new: parse + retire + assign + bin + admit +
      accumulate beside retire + assign + bin + admit + accumulate fed the
      same tables built on the host.
  Yardsticks, on the same inputs in the same process: qfec_retire_groups with
  nothing to close (one streaming pass plus a gather: 84 us in
  profiles/retire_rate.json), qfec_assign_slots, and qfec_null_decrypt_batch
  over the same packets (NULL-protected copies of them, in arrival order).

EXPECTATION, stated before the first run, to confirm or refute.  The streamed
part is 241 MB in and 220 MB out: at the 3-4 TB/s the other one-pass calls
reach, 120-160 us, twice the retire's 84 us for 2.7 times its bytes.  The
header bytes are the other part: in a random arrival order every packet's two
bytes lie in a cache line no other lane of the pass wants, so the pass SUPPOSEDLY
pulls a whole line (64-128 B) per packet from HBM, 0.7-1.3 GB of traffic for 21
MB of use, at the rate of a random gather rather than a stream.  (a): 350-700
us, four to eight times the retire on the same inputs and 0.3-0.6 of the
assign (about 1,200 us); if it lands near 150 us the lines are cheaper than
supposed, if above the assign the gather is latency-bound and the pass wants
more loads in flight per lane.  (b): the failed packets' bytes are not loaded:
within 5% of (a), no slower.  (c): 105 k packets, a memset and one kernel:
8-20 us, launch-bound, below the sparse retire's 25 us.  (d): the parse adds
its (a) figure to a turn of about 3.3 ms: 10-20%.  Against the NULL decrypt of
the same packets (which reads and writes all 7.4 GB: 4-6 ms) the parse is
0.06-0.15.

The legs alternate in this process: warm-up, then `--reps` alternations, each
timed with HIP events around back-to-back rounds -- as many as fill
`--window-ms`; medians with the 10th / 90th percentiles.  After timing every
parse leg's outputs equal tests/parse_rule.py (the whole-array form) over the
whole input, and leg (d)'s turn from the parse leaves the rows and lengths of
the turn from host-built tables.

Writes one JSON document (default profiles/parse_rate.json); DESIGN.md §4
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "parse_rate.json"))
    args = ap.parse_args()

    import torch
    import parse_rule as PR
    from libquic_amd import qfec, synth
    from oracle import qfec_np as Q

    if not torch.cuda.is_available():
        sys.exit("parse_rate: no HIP device (this tool only measures on the GPU)")
    dev = "cuda:0"
    n, align, stride, ms, shift, n_conns, version, tag = args.groups, 16, 1536, 2, 40, 4096, 31, 12
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
    pos = (np.arange(npk) - np.repeat(p0, ks.astype(np.int64))).astype(np.uint8)
    g64 = grp.astype(np.uint64)
    conn = (g64 % np.uint64(n_conns)).astype(np.uint32)
    number = g64 // np.uint64(n_conns) * np.uint64(16) + np.uint64(1)
    pn = number + pos
    key = (conn.astype(np.uint64) << np.uint64(shift)) | number
    off, ln = off.astype(np.uint64), ln.astype(np.uint16)
    rng = np.random.default_rng(20261021)
    perm = rng.permutation(npk)
    some = np.sort(rng.permutation(n)[:max(1, n // 100)])
    sparse_order = rng.permutation(np.flatnonzero(np.isin(grp, some)))
    ok_b = (rng.random(npk) >= 0.05).astype(np.uint8)

    # the arena: synthetic packets, then their first two bytes made a header
    data = torch.empty(int(off[-1]) + int(ln[-1]) + 16, dtype=torch.uint8, device=dev)
    ctx.synth_ragged(data, up(off, np.int64), up(ln, np.int16), up(ptr, np.int32), 0, n,
                     Q.SEED_RAGGED)
    w_cnt = torch.zeros(2, dtype=torch.int64, device=dev)
    ctx.write_private_headers(data, up(off, np.int64), up(np.full(npk, 2, np.uint8), np.uint8),
                              up(pos, np.uint8), npk, version, counts=w_cnt)
    ctx.sync()
    assert host(w_cnt, np.uint64).tolist() == [npk, 0]

    def leg(name, order, ok=None):
        m = int(order.size)
        d = {"name": name, "m": m, "order": order, "ok_h": ok,
             "off": up(off[order], np.int64), "len": up(ln[order], np.int16),
             "pn": up(pn[order], np.int64), "conn": up(conn[order], np.int32),
             "ok": None if ok is None else up(ok, np.uint8),
             "key": torch.zeros(m, dtype=torch.int64, device=dev),
             "idx": torch.zeros(m, dtype=torch.uint8, device=dev),
             "body_off": torch.zeros(m, dtype=torch.int64, device=dev),
             "body_len": torch.zeros(m, dtype=torch.int16, device=dev),
             "hdr": torch.zeros(m, dtype=torch.uint8, device=dev),
             "entropy": torch.zeros(m, dtype=torch.uint8, device=dev),
             "cnt": torch.zeros(6, dtype=torch.int64, device=dev),
             "k": up(ks[grp[order]].astype(np.uint8), np.uint8),
             "r_out": torch.zeros(m, dtype=torch.int64, device=dev),
             "a_out": torch.zeros(m, dtype=torch.int32, device=dev)}
        return d

    legs = [leg("a_every_packet_in_a_group", perm),
            leg("b_5_percent_failed", perm, ok_b),
            leg("c_sparse", sparse_order)]

    def parse_fn(d):
        def fn():
            ctx.parse_opened(data, d["off"], d["len"], d["pn"], d["conn"], d["m"], version, shift,
                             d["key"], d["idx"], d["body_off"], d["body_len"], d["hdr"],
                             pkt_ok=d["ok"], entropy_out=d["entropy"], counts=d["cnt"])
        return fn

    # the yardsticks: every group open in slot g, marks 0, nothing to close
    slot_key_d = up((np.arange(n, dtype=np.uint64) % np.uint64(n_conns)) << np.uint64(shift) |
                    (np.arange(n, dtype=np.uint64) // np.uint64(n_conns) * np.uint64(16) +
                     np.uint64(1)), np.int64)
    slot_k_d = up(ks.astype(np.uint8), np.uint8)
    len_open = torch.full((n,), 9, dtype=torch.int16, device=dev)
    acc_len = torch.zeros(n, dtype=torch.int16, device=dev)
    marks = torch.zeros(n_conns, dtype=torch.int64, device=dev)
    host_key = {d["name"]: up(key[d["order"]], np.int64) for d in legs}

    def retire_fn(d):
        def fn():  # (nothing closes: the lengths and marks stay as they are)
            ctx.retire_groups(host_key[d["name"]], d["m"], slot_key_d, len_open, n, marks, n_conns,
                              shift, 0, d["r_out"])
        return fn

    def assign_fn(d):
        def fn():
            ctx.assign_slots(host_key[d["name"]], d["k"], d["m"], slot_key_d, slot_k_d, len_open, n,
                             d["a_out"])
        return fn

    # the NULL decrypt of the same packets, in arrival order
    ct_len = ln[perm].astype(np.int64) + tag
    w_off = np.cumsum((ct_len + 15) // 16 * 16) - (ct_len + 15) // 16 * 16
    wire = torch.empty(int(w_off[-1] + ct_len[-1]) + 16, dtype=torch.uint8, device=dev)
    opened = torch.empty(data.numel(), dtype=torch.uint8, device=dev)
    zero_len = torch.zeros(npk, dtype=torch.int16, device=dev)
    w_off_d, ct_len_d = up(w_off.astype(np.uint64), np.int64), up(ct_len.astype(np.uint16), np.int16)
    null_ok = torch.zeros(npk, dtype=torch.uint8, device=dev)
    a = legs[0]
    ctx.null_encrypt(data, a["off"], zero_len, a["off"], a["len"], npk, wire, w_off_d)

    def null_fn():
        ctx.null_decrypt(wire, w_off_d, zero_len, w_off_d, ct_len_d, npk, opened, a["off"], null_ok)

    # (d) the turn, every group new: the slots free under stale keys
    m = npk
    stale_key_d = up(np.roll(host(slot_key_d, np.uint64), 12345), np.int64)
    key_k = torch.ones(n, dtype=torch.uint8, device=dev)
    acc = torch.zeros(n * stride, dtype=torch.uint8, device=dev)
    maps = torch.full((n * ms,), 0xFF, dtype=torch.uint8, device=dev)  # stale: all ones
    all_ok = up(np.ones(m, np.uint8), np.uint8)
    h = {"key": host_key[a["name"]], "idx": up(pos[perm], np.uint8),
         "body_off": up(off[perm] + np.uint64(2), np.int64),
         "body_len": up(ln[perm] - np.uint16(2), np.int16)}
    b = {"key_out": torch.zeros(m, dtype=torch.int64, device=dev),
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

    def turn(with_parse):
        def fn():
            acc_len.zero_()
            marks.zero_()
            t = h
            if with_parse:
                ctx.parse_opened(data, a["off"], a["len"], a["pn"], a["conn"], m, version, shift,
                                 a["key"], a["idx"], a["body_off"], a["body_len"], a["hdr"],
                                 pkt_ok=all_ok, entropy_out=a["entropy"])
                t = a
            ctx.retire_groups(t["key"], m, stale_key_d, acc_len, n, marks, n_conns, shift, 0,
                              b["key_out"])
            ctx.assign_slots(b["key_out"], a["k"], m, stale_key_d, key_k, acc_len, n, b["slot"])
            ctx.bin_arrivals(b["slot"], t["body_off"], t["body_len"], t["idx"], all_ok, m, n,
                             b["t_ptr"], b["t_off"], b["t_ln"], b["t_idx"], pkt_ok_out=b["t_ok"])
            ctx.admit_ragged(b["t_off"], b["t_ln"], b["t_idx"], b["t_ok"], b["t_ptr"], n, key_k,
                             maps, ms, acc_len, stride, b["o_ptr"], b["o_off"], b["o_ln"], b["v"])
            ctx.accumulate_ragged(data, b["o_off"], b["o_ln"], b["o_ptr"], n, acc, stride, acc_len)
        return fn

    fns = {}
    for d in legs:
        fns["parse_" + d["name"]] = parse_fn(d)
        fns["retire_" + d["name"]] = retire_fn(d)
        fns["assign_" + d["name"]] = assign_fn(d)
    fns["null_decrypt"] = null_fn
    fns["turn_from_parse"], fns["turn_from_host_tables"] = turn(True), turn(False)
    order = list(fns)
    for name in order:  # every leg once on its own, so that a latched error names its leg
        fns[name]()
        try:
            ctx.sync()
        except qfec.QfecError as e:
            sys.exit(f"parse_rate: leg {name}: {e}")
    assert bool(null_ok.all())
    inner = {name: rounds_per_window(fns[name]) for name in order}
    t = {name: [] for name in order}
    for _ in range(args.reps):
        for name in order:
            t[name].append(timed(fns[name], inner[name]))
    ctx.sync()
    print("timed", flush=True)

    # the outputs of the timed calls against tests/parse_rule.py, whole inputs:
    # the rule is independent of position, so it runs over the header bytes
    # alone, packet p's at 2 * p, and its body offsets are moved back
    results = {}
    for d in legs:
        o, mm = d["order"], d["m"]
        heads = np.empty(2 * mm, np.uint8)
        heads[0::2], heads[1::2] = 2, pos[o]
        at = np.arange(mm, dtype=np.uint64) * np.uint64(2)
        w = PR.parse_opened_np(heads, at, ln[o], pn[o], conn[o], d["ok_h"], version, shift)
        w["body_off"] = w["body_off"] - at + off[o]
        for name in ("key", "idx", "body_off", "body_len", "hdr", "entropy", "cnt"):
            d[name].fill_(-1 if d[name].dtype != torch.uint8 else 0xA5)
        parse_fn(d)()
        ctx.sync()
        for name, dt in (("key", np.uint64), ("idx", np.uint8), ("body_off", np.uint64),
                         ("body_len", np.uint16), ("hdr", np.uint8), ("entropy", np.uint8)):
            assert np.array_equal(host(d[name], dt), w[name]), (d["name"], name)
        assert host(d["cnt"], np.uint64).tolist() == w["counts"].tolist(), d["name"]
        results[d["name"]] = w["counts"].tolist()
        print(json.dumps({"verified": d["name"], "counts": results[d["name"]]}), flush=True)
    assert results["a_every_packet_in_a_group"] == [npk, 0, 0, 0, 0, 0]
    assert results["b_5_percent_failed"][3] == npk - int(ok_b.sum())
    rows = {}
    for name in ("turn_from_parse", "turn_from_host_tables"):
        acc.zero_()
        fns[name]()
        ctx.sync()
        rows[name] = (acc.clone(), acc_len.clone())
    assert torch.equal(rows["turn_from_parse"][0], rows["turn_from_host_tables"][0])
    assert torch.equal(rows["turn_from_parse"][1], rows["turn_from_host_tables"][1])
    assert int((rows["turn_from_parse"][1] != 0).sum()) == n
    del rows

    us = {name: {"median": pct(v, 50), "p10": pct(v, 10), "p90": pct(v, 90)}
          for name, v in t.items()}
    table = []
    for d in legs:
        r, y, s = us["parse_" + d["name"]], us["retire_" + d["name"]], us["assign_" + d["name"]]
        table.append({"leg": d["name"], "packets": d["m"], "counts": results[d["name"]], "us": r,
                      "retire_us": y, "assign_us": s, "over_retire": r["median"] / y["median"],
                      "over_assign": r["median"] / s["median"],
                      "streamed_GBps": 44e-3 * d["m"] / r["median"]})
    doc = {
        "tool": "tools/parse_rate.py",
        "device": torch.cuda.get_device_properties(0).name,
        "shape": {"groups": n, "slots": n, "connections": n_conns, "key_shift": shift,
                  "k": [5, 15], "packets": npk, "sparse_packets": int(sparse_order.size),
                  "arena_bytes": int(data.numel()), "acc_stride": stride, "map_stride": ms,
                  "record_bytes": "23 in, 21 out per packet, and the two header bytes"},
        "expectation": "stated before measuring (the tool's docstring has it in full): 120-160 us "
                       "for the streamed 461 MB, but a cache line per packet for the two header "
                       "bytes, 0.7-1.3 GB at a gather's rate; (a) 350-700 us, 4-8 times the retire, "
                       "0.3-0.6 of the assign; (b) within 5% of (a), no slower; (c) 8-20 us; "
                       "(d) 10-20% of the turn; 0.06-0.15 of the NULL decrypt",
        "method": {"timer": "HIP events around back-to-back rounds, as many as fill window_ms",
                   "inner": args.inner, "window_ms": args.window_ms, "reps": args.reps,
                   "warmup": args.warmup, "rounds_per_window": inner,
                   "order": ", ".join(order) + ", alternating",
                   "round": "parse, retire and assign legs and the NULL decrypt: the call; turns: "
                            "acc_len and the marks zeroed, then the calls",
                   "verified": "after timing: every parse leg's pkt_key_out, pkt_idx_out, "
                               "body_off_out, body_len_out, hdr_out, entropy_out and counts equal "
                               "tests/parse_rule.py over the whole input; the turn from the parse "
                               "leaves the rows and lengths of the turn from host-built tables"},
        "parse": table,
        "null_decrypt_us": us["null_decrypt"],
        "parse_over_null_decrypt": us["parse_" + legs[0]["name"]]["median"] /
        us["null_decrypt"]["median"],
        "turn": {"from_parse_us": us["turn_from_parse"],
                 "from_host_tables_us": us["turn_from_host_tables"],
                 "difference_us": us["turn_from_parse"]["median"] -
                 us["turn_from_host_tables"]["median"],
                 "ratio": us["turn_from_parse"]["median"] / us["turn_from_host_tables"]["median"]},
    }
    for row in table:
        print(json.dumps(row))
    print(json.dumps({"turn": doc["turn"], "null_decrypt_us": doc["null_decrypt_us"]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
