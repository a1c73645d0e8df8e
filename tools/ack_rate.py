#!/usr/bin/env python3
"""qfec_record_received and qfec_build_acks beside the calls they run behind.

One MI355X, the workload and protocol of tools/parse_rate.py: BASELINE
configs[3], 2^20 groups of k 5-15 packets, 10,491,121 packets in one arena of
about 7.4 GB, the arrival order a uniform random permutation; group g is number
16 * (g // 4096) + 1 on connection g % 4096, the packet number is the group
number plus the position, key_shift 40.  A connection so receives about 2,560
packets with numbers up to 4,111 in the turn: 4,096 connections at window 8,192,
a ring of 32 MiB.  A record of the call is (packet_number 8, pkt_conn 4, hdr 1,
entropy 1) = 14 bytes in, read by two passes, and 1 byte out, plus the cell.

  (a) record, every packet new (the state reset to "new connection" in front of
      every round: three small memsets, so the round clears its cells itself);
  (b) record with 5% of the packets received in an earlier call (DUPLICATE) and
      the lost packet of 1% of the groups revived; the state of before is
      copied back in front of every round, and that copy is timed on its own;
  (c) a sparse turn: the packets of 1% of the connections;
  (d) build for every connection: 65,536 connections of about 160 packet
      numbers at window 256, and 16,384 of about 640 at window 1,024 (a tenth
      of the numbers missing, a tenth of those revived; max_ranges 255,
      max_revived 16);
  (e) the turn parse + retire + assign + bin + admit + accumulate with and
      without record + build (every connection, window 8,192) behind it.
  Yardsticks, on the same inputs in the same process: qfec_parse_opened and
  qfec_retire_groups (nothing to close) over legs (a) and (c).

EXPECTATION, stated before the first run, to confirm or refute.  Nobody has
measured any of this.  The record streams 14 B in twice and 1 B out and back:
about 320 MB, 80-110 us at the 3-4 TB/s of the one-pass calls.  What it does per
packet besides is one byte load of the cell (classify) and one 32-bit atomic OR
on the cell's word (set), both scattered -- but over a ring of 32 MiB, which
SUPPOSEDLY stays in the 256 MiB Infinity Cache and mostly in the L2s, where the
parse's two header bytes came from a 7.4 GB arena (a line from HBM per packet,
376 us).  So the gather should be cheaper than the parse's and the atomics the
larger part: 10.5 M device-scope atomics at SUPPOSEDLY 20-40 G/s are 260-520
us if they serialise per channel, far less if the L2s absorb them.  (a):
250-600 us, 0.7-1.6 of the parse on the same inputs, 3-7 times the retire.  If
it lands under 200 us the ring is cache-resident and the atomics are cheap; if
above 800 us the atomics bound it and the set pass wants one OR per word, not
per packet.  (b): the duplicates skip the atomic, the revived add 1 M lanes of
one pass: within 10% of (a) after the copy is taken off.  (c): 105 k packets,
two memsets and three kernels, the advance over all 4,096 connections: 15-30
us, launch-bound.  (d): 10.5 M cells read twice as bytes, 64 a trip by a wave
per connection: window 256 is 65,536 waves of 3 trips, SUPPOSEDLY latency-bound
per wave: 60-150 us; window 1,024 a quarter of the waves and four times the
trips: the same or a little less.  (e): record + build add (a) plus a build of
4,096 long walks (65 trips each, 16 waves per CU busy: 50-100 us) to a turn of
about 4.8 ms: 7-15%, around the parse's 9.4%.

The legs alternate in this process: warm-up, then `--reps` alternations, each
timed with HIP events around back-to-back rounds -- as many as fill
`--window-ms`; medians with the 10th / 90th percentiles.  After timing every
leg's outputs equal tests/ack_rule.py (the whole-array forms) over the whole
input.

Writes one JSON document (default profiles/ack_rate.json); DESIGN.md §4 quotes
it.  Needs the GPU: there is no fallback.
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ack_rate.json"))
    args = ap.parse_args()

    import torch
    import ack_rule as A
    from libquic_amd import qfec, synth
    from oracle import qfec_np as Q

    if not torch.cuda.is_available():
        sys.exit("ack_rate: no HIP device (this tool only measures on the GPU)")
    dev = "cuda:0"
    n, align, stride, ms, shift, n_conns, version = args.groups, 16, 1536, 2, 40, 4096, 31
    window = 8192
    U64 = np.uint64
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

    def zeros(m, dt):
        return torch.zeros(m, dtype=dt, device=dev)

    ks, ptr, ln, off = synth.ragged_layout(0, n, 5, 15, 64, 1350, Q.SEED_RAGGED, align=align)
    ptr = ptr.astype(np.uint32)
    p0 = ptr[:-1].astype(np.int64)
    npk = int(ln.size)
    grp = np.repeat(np.arange(n, dtype=np.uint32), ks.astype(np.int64))
    pos = (np.arange(npk) - np.repeat(p0, ks.astype(np.int64))).astype(np.uint8)
    g64 = grp.astype(U64)
    conn = (g64 % U64(n_conns)).astype(np.uint32)
    number = g64 // U64(n_conns) * U64(16) + U64(1)
    pn = number + pos
    key = (conn.astype(U64) << U64(shift)) | number
    group_key = (np.arange(n, dtype=U64) % U64(n_conns)) << U64(shift) | \
        (np.arange(n, dtype=U64) // U64(n_conns) * U64(16) + U64(1))
    off, ln = off.astype(U64), ln.astype(np.uint16)
    rng = np.random.default_rng(20261021)
    perm = rng.permutation(npk)
    flags = (2 | rng.integers(0, 2, npk)).astype(np.uint8)  # in a group, a random entropy bit
    ent = ((flags & 1) << (pn % U64(8)).astype(np.uint8)).astype(np.uint8)
    some = np.sort(rng.permutation(n_conns)[:max(1, n_conns // 100)])
    sparse_order = rng.permutation(np.flatnonzero(np.isin(conn, some)))
    # (b): the packets of an earlier call, and the revived packet of 1% of the groups
    early = rng.random(npk) < 0.05
    rev_group = np.sort(rng.permutation(n)[:n // 100])
    rev_pos = (rng.integers(0, 1 << 30, rev_group.size) % (ks[rev_group] - 1)).astype(np.uint8)
    lost = p0[rev_group] + rev_pos  # (never a group's last packet: below the largest)
    status_b, ridx_b = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    status_b[rev_group], ridx_b[rev_group] = A.GROUP_REVIVED, rev_pos
    arrives_b = np.ones(npk, bool)
    arrives_b[lost] = False
    early &= arrives_b
    order_b = perm[arrives_b[perm]]

    # the arena of the yardsticks and of the turn: synthetic packets with their headers
    data = torch.empty(int(off[-1]) + int(ln[-1]) + 16, dtype=torch.uint8, device=dev)
    ctx.synth_ragged(data, up(off, np.int64), up(ln, np.int16), up(ptr, np.int32), 0, n,
                     Q.SEED_RAGGED)
    ctx.write_private_headers(data, up(off, np.int64), up(flags, np.uint8), up(pos, np.uint8), npk,
                              version)
    ctx.sync()

    # the ack state of legs (a), (b), (c) and (e)
    cells = zeros(n_conns * window, torch.uint8)
    least, largest, hsh = zeros(n_conns, torch.int64), zeros(n_conns, torch.int64), \
        zeros(n_conns, torch.uint8)
    st_args = (cells, least, largest, hsh, n_conns, window)

    def reset_new():
        least.zero_()
        largest.zero_()
        hsh.zero_()

    def leg(name, order, **more):
        m = int(order.size)
        d = {"name": name, "m": m, "order": order, "pn": up(pn[order], np.int64),
             "conn": up(conn[order], np.int32), "hdr": up(flags[order], np.uint8),
             "ent": up(ent[order], np.uint8), "out": zeros(m, torch.uint8),
             "cnt": zeros(12, torch.int64), "off": up(off[order], np.int64),
             "len": up(ln[order], np.int16), "key_h": up(key[order], np.int64),
             "key": zeros(m, torch.int64), "idx": zeros(m, torch.uint8),
             "body_off": zeros(m, torch.int64), "body_len": zeros(m, torch.int16),
             "p_hdr": zeros(m, torch.uint8), "p_ent": zeros(m, torch.uint8),
             "r_out": zeros(m, torch.int64), "reset": reset_new, "rev": {}}
        d.update(more)
        return d

    legs = [leg("a_every_packet_new", perm), leg("b_duplicates_and_revived", order_b),
            leg("c_sparse", sparse_order)]
    a, b = legs[0], legs[1]
    # (b)'s state of before: the early packets recorded, then kept aside
    e_order = np.flatnonzero(early)
    ctx.record_received(*st_args, packet_number=up(pn[e_order], np.int64),
                        pkt_conn=up(conn[e_order], np.int32), n_packets=int(e_order.size),
                        rcv_out=zeros(e_order.size, torch.uint8), entropy=up(ent[e_order], np.uint8))
    ctx.sync()
    before_b = [t.clone() for t in (cells, least, largest, hsh)]

    def restore_b():
        for t, s in zip((cells, least, largest, hsh), before_b):
            t.copy_(s)

    slot_key_d = up(group_key, np.int64)
    b["reset"] = restore_b
    b["rev"] = dict(status=up(status_b, np.uint8), revived_idx=up(ridx_b, np.uint8),
                    slot_key=slot_key_d, n_groups=n, n_slots=n, key_shift=shift)

    def record_fn(d):
        def fn():
            d["reset"]()
            ctx.record_received(*st_args, packet_number=d["pn"], pkt_conn=d["conn"],
                                n_packets=d["m"], rcv_out=d["out"], hdr=d["hdr"], entropy=d["ent"],
                                counts=d["cnt"], **d["rev"])
        return fn

    def parse_fn(d):
        def fn():
            ctx.parse_opened(data, d["off"], d["len"], d["pn"], d["conn"], d["m"], version, shift,
                             d["key"], d["idx"], d["body_off"], d["body_len"], d["p_hdr"],
                             entropy_out=d["p_ent"])
        return fn

    len_open = torch.full((n,), 9, dtype=torch.int16, device=dev)
    marks = zeros(n_conns, torch.int64)

    def retire_fn(d):
        def fn():  # (nothing closes: the lengths and marks stay as they are)
            ctx.retire_groups(d["key_h"], d["m"], slot_key_d, len_open, n, marks, n_conns, shift, 0,
                              d["r_out"])
        return fn

    # (d) the build: states of their own, built by one record each
    def build_leg(name, nc, w, span):
        c = np.repeat(np.arange(nc, dtype=np.uint32), span)
        q = np.tile(np.arange(1, span + 1, dtype=U64), nc)
        gone = rng.random(c.size) < 0.1
        gone[q == U64(span)] = False  # (the largest arrives)
        rv = np.flatnonzero(gone & (rng.random(c.size) < 0.1))
        got = rng.permutation(np.flatnonzero(~gone))
        turn = dict(packet_number=q[got], pkt_conn=c[got],
                    entropy=rng.integers(0, 2, got.size).astype(np.uint8),
                    status=np.ones(rv.size, np.uint8), revived_idx=np.zeros(rv.size, np.uint8),
                    slot_key=(c[rv].astype(U64) << U64(shift)) | q[rv], key_shift=shift)
        s = dict(cells=zeros(nc * w, torch.uint8), least=zeros(nc, torch.int64),
                 largest=zeros(nc, torch.int64), hash=zeros(nc, torch.uint8))
        ctx.record_received(s["cells"], s["least"], s["largest"], s["hash"], nc, w,
                            packet_number=up(turn["packet_number"], np.int64),
                            pkt_conn=up(turn["pkt_conn"], np.int32), n_packets=int(got.size),
                            rcv_out=zeros(got.size, torch.uint8), entropy=up(turn["entropy"], np.uint8),
                            status=up(turn["status"], np.uint8),
                            revived_idx=up(turn["revived_idx"], np.uint8),
                            slot_key=up(turn["slot_key"], np.int64), n_groups=int(rv.size),
                            n_slots=int(rv.size), key_shift=shift)
        ctx.sync()
        return dict(name=name, nc=nc, w=w, turn=turn, s=s, mr=255, mv=16,
                    o=acks_out(nc, 255, 16), conn=up(np.arange(nc, dtype=np.uint32), np.int32))

    def acks_out(nc, mr, mv):
        return dict(largest=zeros(nc, torch.int64), hash=zeros(nc, torch.uint8),
                    truncated=zeros(nc, torch.uint8), range_ptr=zeros(nc + 1, torch.int32),
                    range_lo=zeros(nc * mr, torch.int64), range_hi=zeros(nc * mr, torch.int64),
                    rev_ptr=zeros(nc + 1, torch.int32), rev_pn=zeros(nc * mv, torch.int64))

    def build_fn(d):
        o, s = d["o"], d["s"]

        def fn():
            ctx.build_acks(d["conn"], d["nc"], s["cells"], s["least"], s["largest"], s["hash"],
                           d["nc"], d["w"], d["mr"], d["mv"], o["largest"], o["hash"],
                           o["truncated"], o["range_ptr"], o["range_lo"], o["range_hi"],
                           o["rev_ptr"], o["rev_pn"])
        return fn

    builds = [build_leg("d_build_window_256", 65536, 256, 160),
              build_leg("d_build_window_1024", 16384, 1024, 640)]

    # (e) the turn, every group new, and record + build behind it
    m = npk
    stale_key_d = up(np.roll(group_key, 12345), np.int64)
    key_k = torch.ones(n, dtype=torch.uint8, device=dev)
    k_of = up(ks[grp[perm]].astype(np.uint8), np.uint8)
    acc = zeros(n * stride, torch.uint8)
    acc_len = zeros(n, torch.int16)
    maps = torch.full((n * ms,), 0xFF, dtype=torch.uint8, device=dev)  # stale: all ones
    all_ok = up(np.ones(m, np.uint8), np.uint8)
    no_status, no_idx = zeros(n, torch.uint8), zeros(n, torch.uint8)
    w = {"key_out": zeros(m, torch.int64), "slot": zeros(m, torch.int32),
         "t_ptr": zeros(n + 1, torch.int32), "t_off": zeros(m, torch.int64),
         "t_ln": zeros(m, torch.int16), "t_idx": zeros(m, torch.uint8),
         "t_ok": zeros(m, torch.uint8), "o_ptr": zeros(n + 1, torch.int32),
         "o_off": zeros(m, torch.int64), "o_ln": zeros(m, torch.int16), "v": zeros(m, torch.uint8)}
    turn_acks = dict(name="e_turn_acks", nc=n_conns, w=window, mr=255, mv=16,
                     s=dict(cells=cells, least=least, largest=largest, hash=hsh),
                     o=acks_out(n_conns, 255, 16),
                     conn=up(np.arange(n_conns, dtype=np.uint32), np.int32))
    build_turn = build_fn(turn_acks)

    def turn(with_acks):
        def fn():
            acc_len.zero_()
            marks.zero_()
            ctx.parse_opened(data, a["off"], a["len"], a["pn"], a["conn"], m, version, shift,
                             a["key"], a["idx"], a["body_off"], a["body_len"], a["p_hdr"],
                             pkt_ok=all_ok, entropy_out=a["p_ent"])
            ctx.retire_groups(a["key"], m, stale_key_d, acc_len, n, marks, n_conns, shift, 0,
                              w["key_out"])
            ctx.assign_slots(w["key_out"], k_of, m, stale_key_d, key_k, acc_len, n, w["slot"])
            ctx.bin_arrivals(w["slot"], a["body_off"], a["body_len"], a["idx"], all_ok, m, n,
                             w["t_ptr"], w["t_off"], w["t_ln"], w["t_idx"], pkt_ok_out=w["t_ok"])
            ctx.admit_ragged(w["t_off"], w["t_ln"], w["t_idx"], w["t_ok"], w["t_ptr"], n, key_k,
                             maps, ms, acc_len, stride, w["o_ptr"], w["o_off"], w["o_ln"], w["v"])
            ctx.accumulate_ragged(data, w["o_off"], w["o_ln"], w["o_ptr"], n, acc, stride, acc_len)
            if with_acks:  # (no group is revived: the revived pass runs over n COMPLETE groups)
                reset_new()
                ctx.record_received(*st_args, packet_number=a["pn"], pkt_conn=a["conn"],
                                    n_packets=m, rcv_out=a["out"], hdr=a["p_hdr"],
                                    entropy=a["p_ent"], status=no_status, revived_idx=no_idx,
                                    slot_key=stale_key_d, n_groups=n, n_slots=n, key_shift=shift,
                                    counts=a["cnt"])
                build_turn()
        return fn

    fns = {}
    for d in legs:
        fns["record_" + d["name"]] = record_fn(d)
    for d in (legs[0], legs[2]):
        fns["parse_" + d["name"]] = parse_fn(d)
        fns["retire_" + d["name"]] = retire_fn(d)
    fns["restore_b"] = restore_b
    fns["reset_new"] = reset_new
    for d in builds:
        fns[d["name"]] = build_fn(d)
    fns["turn_with_acks"], fns["turn_without"] = turn(True), turn(False)
    order = list(fns)
    for name in order:  # every leg once on its own, so that a latched error names its leg
        fns[name]()
        try:
            ctx.sync()
        except qfec.QfecError as e:
            sys.exit(f"ack_rate: leg {name}: {e}")
    inner = {name: rounds_per_window(fns[name]) for name in order}
    t = {name: [] for name in order}
    for _ in range(args.reps):
        for name in order:
            t[name].append(timed(fns[name], inner[name]))
    ctx.sync()
    print("timed", flush=True)

    # the outputs of the timed calls against tests/ack_rule.py, whole inputs
    def state_of(s, nc, wd):
        return dict(cells=host(s["cells"], np.uint8).reshape(nc, wd), least=host(s["least"], U64),
                    largest=host(s["largest"], U64), hash=host(s["hash"], np.uint8), window=wd)

    def check_acks(d, state):
        want = A.build_acks_np(state, np.arange(d["nc"]), d["mr"], d["mv"])
        o = d["o"]
        for k, dt in (("largest", U64), ("hash", np.uint8), ("truncated", np.uint8),
                      ("range_ptr", np.uint32), ("rev_ptr", np.uint32)):
            assert np.array_equal(host(o[k], dt), want[k]), (d["name"], k)
        for k, p in (("range_lo", "range_ptr"), ("range_hi", "range_ptr"), ("rev_pn", "rev_ptr")):
            assert np.array_equal(host(o[k], U64)[:want[p][-1]], want[k]), (d["name"], k)
        return dict(intervals=int(want["range_ptr"][-1]), revived=int(want["rev_ptr"][-1]),
                    truncated=int(want["truncated"].sum()))

    mine = dict(cells=cells, least=least, largest=largest, hash=hsh)
    results = {}
    for d in legs:
        d["reset"]()
        ctx.sync()
        start = state_of(mine, n_conns, window)
        for name in ("out", "cnt"):
            d[name].fill_(-1 if d[name].dtype != torch.uint8 else 0xA5)
        fns["record_" + d["name"]]()
        ctx.sync()
        o = d["order"]
        rev = {k: (host(v, U64 if k == "slot_key" else np.uint8) if torch.is_tensor(v) else v)
               for k, v in d["rev"].items() if k in ("status", "revived_idx", "slot_key", "key_shift")}
        want = A.record_received_np(start, packet_number=pn[o], pkt_conn=conn[o], hdr=flags[o],
                                    entropy=ent[o], **rev)
        assert np.array_equal(host(d["out"], np.uint8), want["rcv_out"]), d["name"]
        assert host(d["cnt"], U64).tolist() == want["counts"].tolist(), d["name"]
        assert A.same_state(state_of(mine, n_conns, window), want["state"]), d["name"]
        results[d["name"]] = want["counts"].tolist()
        print(json.dumps({"verified": d["name"], "counts": results[d["name"]]}), flush=True)
    assert results["a_every_packet_new"][A.RECORDED] == npk == results["a_every_packet_new"][A.N_NEW]
    assert results["b_duplicates_and_revived"][A.DUPLICATE] == int(early.sum())
    assert results["b_duplicates_and_revived"][A.N_REVIVED] == rev_group.size
    built = {}
    for d in builds:
        state = A.record_received_np(A.new_state(d["nc"], d["w"]), **d["turn"])["state"]
        assert A.same_state(state_of(d["s"], d["nc"], d["w"]), state), d["name"]
        fns[d["name"]]()
        ctx.sync()
        built[d["name"]] = check_acks(d, state)
        print(json.dumps({"verified": d["name"], **built[d["name"]]}), flush=True)
    fns["turn_with_acks"]()
    ctx.sync()
    assert host(a["cnt"], U64).tolist() == results["a_every_packet_new"][:7] + [0, 0, 0, 0, 0]
    built["e_turn_acks"] = check_acks(turn_acks, state_of(mine, n_conns, window))
    print(json.dumps({"verified": "e_turn_acks", **built["e_turn_acks"]}), flush=True)

    us = {name: {"median": pct(v, 50), "p10": pct(v, 10), "p90": pct(v, 90)}
          for name, v in t.items()}
    med = lambda name: us[name]["median"]
    net = {"a_every_packet_new": med("record_a_every_packet_new") - med("reset_new"),
           "b_duplicates_and_revived": med("record_b_duplicates_and_revived") - med("restore_b"),
           "c_sparse": med("record_c_sparse") - med("reset_new")}
    table = []
    for d in legs:
        row = {"leg": d["name"], "packets": d["m"], "counts": results[d["name"]],
               "round_us": us["record_" + d["name"]], "record_us_net_of_reset": net[d["name"]]}
        if "parse_" + d["name"] in us:
            row.update(parse_us=us["parse_" + d["name"]], retire_us=us["retire_" + d["name"]],
                       over_parse=net[d["name"]] / med("parse_" + d["name"]),
                       over_retire=net[d["name"]] / med("retire_" + d["name"]))
        table.append(row)
    table[1]["over_leg_a"] = net["b_duplicates_and_revived"] / net["a_every_packet_new"]
    diff = med("turn_with_acks") - med("turn_without")
    doc = {
        "tool": "tools/ack_rate.py",
        "device": torch.cuda.get_device_properties(0).name,
        "shape": {"groups": n, "connections": n_conns, "window": window, "key_shift": shift,
                  "packets": npk, "sparse_packets": int(sparse_order.size),
                  "ring_bytes": n_conns * window,
                  "record_bytes": "14 in (read by two passes), 1 out, and the cell"},
        "expectation": "stated before measuring (the tool's docstring has it in full): (a) 250-600 "
                       "us, 0.7-1.6 of the parse, 3-7 times the retire; (b) within 10% of (a) net "
                       "of the copy; (c) 15-30 us; (d) 60-150 us at both windows; (e) 7-15% of "
                       "the turn",
        "method": {"timer": "HIP events around back-to-back rounds, as many as fill window_ms",
                   "inner": args.inner, "window_ms": args.window_ms, "reps": args.reps,
                   "warmup": args.warmup, "rounds_per_window": inner,
                   "order": ", ".join(order) + ", alternating",
                   "round": "record legs: the state reset (a, c: three memsets; b: the state of "
                            "before copied back), then the call; reset_new and restore_b time the "
                            "resets alone, and record_us_net_of_reset is the difference of the "
                            "medians; builds, parse, retire: the call; turns: acc_len and the "
                            "marks zeroed, then the calls",
                   "verified": "after timing: every record leg's rcv_out, counts and state "
                               "(through live_cells), every build's scalars and tables, and the "
                               "turn's counts and acks equal tests/ack_rule.py over the whole input"},
        "record": table,
        "resets_us": {"reset_new": us["reset_new"], "restore_b": us["restore_b"]},
        "build": [{"leg": d["name"], "connections": d["nc"], "window": d["w"], **built[d["name"]],
                   "us": us[d["name"]], "over_parse": med(d["name"]) / med("parse_a_every_packet_new"),
                   "over_retire": med(d["name"]) / med("retire_a_every_packet_new")}
                  for d in builds],
        "turn": {"with_record_and_build_us": us["turn_with_acks"], "without_us": us["turn_without"],
                 "difference_us": diff, "share_of_turn": diff / med("turn_without"),
                 "parse_share_for_comparison": 0.094, "acks": built["e_turn_acks"]},
    }
    for row in table:
        print(json.dumps(row))
    print(json.dumps({"build": doc["build"], "turn": doc["turn"], "resets": doc["resets_us"]}),
          flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
