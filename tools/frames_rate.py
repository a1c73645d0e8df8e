#!/usr/bin/env python3
"""qfec_scan_frames beside qfec_parse_opened, and the cost of its dense raises.

One MI355X, the workload and protocol of tools/parse_rate.py: BASELINE
configs[3], 2^20 groups of k 5-15 packets of 64-1350 bytes, 10,491,121 packets,
16-byte aligned in one arena of about 7.4 GB, the arrival order a uniform random
permutation, group g number 16 * (g // 4096) + 1 on connection g % 4096.  A
packet's first two bytes are its private header; behind them the tool writes
frames over the synthetic bytes, one mix after the other in the same arena:

  mix 1: one stream frame to the packet's end (one byte written: 0x80);
  mix 2: an ack without nacks (7 bytes), a STOP_WAITING (8 bytes, delta 1, the
         packet number 6 bytes long) and the stream frame: 3 frames a packet.

A record of the scan is (body_off 8, body_len 2, packet_number 8, pkt_conn 4,
pkt_pn_len 1, hdr 1) = 24 bytes in, read by both walks, frm_status 1 and
frm_ptr 4 out, and 34 bytes of table per frame listed.

  (a) scan and parse on the same inputs, mix 1;      (b) the same, mix 2;
  (c) a sparse turn, mix 2: the packets of 1% of the groups;
  (d) qfec_retire_groups (nothing to close) and qfec_record_received (raises
      only) with the scan's dense n_raise = n_conns = 4096 entries beside a
      compact host-built list of the 1% of connections that moved;
  (e) the turn of parse_rate's leg (d) -- parse + retire + assign + bin + admit
      + accumulate, every group new -- with the scan behind the parse and its
      dense raises, beside the same turn without;
  (f) what the scan replaces, in part: the copy of opened packets back to
      pinned host memory, timed over a 256 MiB slice and scaled to the arena.

EXPECTATION, stated before the first run, to confirm or refute.  The parse
takes 376 us here (profiles/parse_rate.json), most of it the gather of one
cache line per packet in a random order.  The scan walks twice, so it gathers
every packet's line twice, and streams 48 bytes of records per packet in, 9 out
and 34 per frame: (a) 600-1,100 us, 1.6-3.0 times the parse.  (b) reads 17
bytes of the same line in about ten dependent steps per walk and writes 1.07 GB
of table: 900-1,800 us, 2.4-4.8 times the parse, 1.3-2.0 times (a); if (b) is
above 2.5 times (a) the dependent loads are not hidden by the other waves and
the walk is latency-bound.  (c) 105 k packets, three memsets and four kernels:
25-60 us, launch-bound.  (d) the dense lists cost one more pass over 4,096
entries each: retire +1-6 us, record +2-12 us (a wave per raise, each finding
nothing to drop); not small would be above 30 us, and then the follow-up is a
compaction pass in the scan.  (e) the scan adds its (a)-(b) figure to a turn of
about 3.6 ms: mix 2, 25-50%.  (f) 7.4 GB at 40-55 GB/s: 130-190 ms, two orders
of magnitude above the scan.

The legs of a mix alternate in this process: warm-up, then `--reps`
alternations, each timed with HIP events around back-to-back rounds -- as many
as fill `--window-ms`; medians with the 10th / 90th percentiles.  After timing:
the sparse leg's every output equals tests/frames_rule.py (scan_arrays) over
its whole input; the full legs' verdicts, frm_ptr, counts and STOP_WAITING
state equal what the mixes give by construction; the turn with the scan leaves
the rows and lengths of the turn without.

NOT MEASURED: the host's walk over the copied packets (a per-call figure from
Python would measure ctypes); frames of mixed validity (every packet here
walks to its end); max_frames below the frames present; bodies in an order
other than uniformly random.

Writes one JSON document (default profiles/frames_rate.json); DESIGN.md §4
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

BANDS = {  # us, or a ratio where named so: written before the first run
    "a_scan_us": (600, 1100), "a_scan_over_parse": (1.6, 3.0),
    "b_scan_us": (900, 1800), "b_scan_over_parse": (2.4, 4.8), "b_over_a": (1.3, 2.0),
    "c_sparse_scan_us": (25, 60),
    "d_retire_dense_minus_compact_us": (1, 6), "d_record_dense_minus_compact_us": (2, 12),
    "e_turn_added_fraction": (0.25, 0.50), "f_copy_back_ms": (130, 190),
}


def pct(v, q):
    return float(np.percentile(np.asarray(v), q))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--groups", type=int, default=1 << 20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--inner", type=int, default=2)
    ap.add_argument("--window-ms", type=float, default=20.0,
                    help="least timed window; rounds repeat until they fill it")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frames_rate.json"))
    args = ap.parse_args()

    import torch
    import frames_rule as FR
    from libquic_amd import qfec, synth
    from oracle import qfec_np as Q

    if not torch.cuda.is_available():
        sys.exit("frames_rate: no HIP device (this tool only measures on the GPU)")
    dev = "cuda:0"
    n, align, stride, ms, shift, n_conns, version = args.groups, 16, 1536, 2, 40, 4096, 31
    window, max_frames = 256, 8
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

    def measure(fns):
        """the legs alternating: {name: {median, p10, p90}}, rounds per window"""
        for name, fn in fns.items():  # once on its own, so that a latched error names its leg
            fn()
            try:
                ctx.sync()
            except qfec.QfecError as e:
                sys.exit(f"frames_rate: leg {name}: {e}")
        inner = {name: rounds_per_window(fn) for name, fn in fns.items()}
        t = {name: [] for name in fns}
        for _ in range(args.reps):
            for name, fn in fns.items():
                t[name].append(timed(fn, inner[name]))
        ctx.sync()
        return {name: {"median": pct(v, 50), "p10": pct(v, 10), "p90": pct(v, 90)}
                for name, v in t.items()}, inner

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

    data = torch.empty(int(off[-1]) + int(ln[-1]) + 16, dtype=torch.uint8, device=dev)
    ctx.synth_ragged(data, up(off, np.int64), up(ln, np.int16), up(ptr, np.int32), 0, n,
                     Q.SEED_RAGGED)
    # flags 2 (in a group, a data packet) and the position as the offset: the frames
    # of every packet are walked, whatever its place in the group
    ctx.write_private_headers(data, up(off, np.int64), up(np.full(npk, 2, np.uint8), np.uint8),
                              up(pos, np.uint8), npk, version)
    ctx.sync()
    body_at = up(off + np.uint64(2), np.int64)

    def write_mix(head):
        for j, byte in enumerate(head):
            data[body_at + j] = byte
        torch.cuda.synchronize()

    MIX1 = [0x80]
    #       ack: type (ll 2, mm 1), hash, largest, delay, no times; stop waiting; stream
    MIX2 = [0x44, 0x5A, 0x10, 0x27, 0x34, 0x12, 0x00, 0x06, 0xC3, 1, 0, 0, 0, 0, 0, 0x80]

    def leg(name, order):
        m = int(order.size)
        z = lambda dt, k=m: torch.zeros(k, dtype=dt, device=dev)  # noqa: E731
        return {"name": name, "m": m, "order": order,
                "off": up(off[order], np.int64), "len": up(ln[order], np.int16),
                "pn": up(pn[order], np.int64), "conn": up(conn[order], np.int32),
                "pn_len": up(np.full(m, 6, np.uint8), np.uint8),
                "key": z(torch.int64), "idx": z(torch.uint8), "body_off": z(torch.int64),
                "body_len": z(torch.int16), "hdr": z(torch.uint8), "entropy": z(torch.uint8),
                "status": z(torch.uint8), "ptr": z(torch.int32, m + 1),
                "cnt": z(torch.int64, FR.N_COUNTS),
                "k": up(ks[grp[order]].astype(np.uint8), np.uint8)}

    full, sparse = leg("full", perm), leg("sparse", sparse_order)
    cap = 3 * npk
    table = {"pkt": torch.zeros(cap, dtype=torch.int32, device=dev),
             "type": torch.zeros(cap, dtype=torch.uint8, device=dev),
             "flags": torch.zeros(cap, dtype=torch.uint8, device=dev),
             "off": torch.zeros(cap, dtype=torch.int64, device=dev),
             "len": torch.zeros(cap, dtype=torch.int16, device=dev),
             "id": torch.zeros(cap, dtype=torch.int32, device=dev),
             "val": torch.zeros(cap, dtype=torch.int64, device=dev),
             "code": torch.zeros(cap, dtype=torch.int32, device=dev)}
    sw = {"seen": torch.zeros(n_conns, dtype=torch.int64, device=dev),
          "least": torch.zeros(n_conns, dtype=torch.int64, device=dev),
          "hash": torch.zeros(n_conns, dtype=torch.uint8, device=dev),
          "conn": torch.zeros(n_conns, dtype=torch.int32, device=dev)}

    def parse_fn(d):
        def fn():
            ctx.parse_opened(data, d["off"], d["len"], d["pn"], d["conn"], d["m"], version, shift,
                             d["key"], d["idx"], d["body_off"], d["body_len"], d["hdr"],
                             entropy_out=d["entropy"])
        return fn

    def scan_fn(d, fresh=True):
        def fn():
            if fresh:  # a new connection every round: every round replaces the state
                sw["seen"].zero_()
            ctx.scan_frames(data, d["body_off"], d["body_len"], d["pn"], d["conn"], d["pn_len"],
                            d["m"], version, max_frames, d["status"], d["ptr"], sw["seen"],
                            sw["least"], sw["hash"], sw["conn"], n_conns, hdr=d["hdr"],
                            frm_pkt=table["pkt"], frm_type=table["type"], frm_flags=table["flags"],
                            frm_off=table["off"], frm_len=table["len"], frm_id=table["id"],
                            frm_val=table["val"], frm_code=table["code"], frm_cap=cap,
                            counts=d["cnt"])
        return fn

    for d in (full, sparse):
        parse_fn(d)()
    ctx.sync()
    us, inner = {}, {}

    def phase(tag, fns):
        u, i = measure(fns)
        us.update({f"{tag}_{k}": v for k, v in u.items()})
        inner.update({f"{tag}_{k}": v for k, v in i.items()})
        print(json.dumps({tag: {k: round(v["median"], 1) for k, v in u.items()}}), flush=True)

    # ---- (a) mix 1
    write_mix(MIX1)
    phase("a", {"scan": scan_fn(full), "parse": parse_fn(full)})
    scan_fn(full)()
    ctx.sync()
    cnt_a = host(full["cnt"], np.uint64).tolist()
    assert cnt_a[:10] == [npk, 0, 0, 0, 0, npk, 0, 0, 0, npk], cnt_a
    assert np.array_equal(host(full["ptr"], np.uint32), np.arange(npk + 1, dtype=np.uint32))

    # ---- (b), (c) mix 2
    write_mix(MIX2)
    phase("b", {"scan": scan_fn(full), "parse": parse_fn(full)})
    phase("c", {"sparse_scan": scan_fn(sparse), "sparse_parse": parse_fn(sparse)})
    for tn in sw.values():
        tn.zero_()
    scan_fn(sparse)()
    ctx.sync()
    # the rule over the sparse leg's bodies, gathered into an arena of their own
    o = sparse["order"]
    b_len = (ln[o] - np.uint16(2)).astype(np.int64)
    b_at = np.cumsum(b_len) - b_len
    starts, lens_d = up((off[o] + np.uint64(2)).astype(np.int64), np.int64), up(b_len, np.int64)
    inside = torch.arange(int(b_len.sum()), device=dev) - torch.repeat_interleave(up(b_at, np.int64), lens_d)
    small = host(data[torch.repeat_interleave(starts, lens_d) + inside], np.uint8)
    del inside
    want = FR.scan_arrays(small, b_at.astype(np.uint64), b_len.astype(np.uint16), pn[o], conn[o],
                          np.full(o.size, 6, np.uint8), np.full(o.size, 2, np.uint8), version,
                          max_frames, cap, FR.new_state(n_conns), n_conns)
    placed = np.isin(want["table"]["type"], (FR.F_STREAM, FR.F_ACK, 0, 2, 3))
    moved_by = (off[o] + np.uint64(2) - b_at.astype(np.uint64))[want["table"]["pkt"]]
    want["table"]["off"] = np.where(placed, want["table"]["off"] + moved_by, np.uint64(0))
    total = int(want["ptr"][-1])
    assert np.array_equal(host(sparse["status"], np.uint8), want["status"])
    assert np.array_equal(host(sparse["ptr"], np.uint32), want["ptr"])
    for name, dt in FR.COLUMNS:
        assert np.array_equal(host(table[name][:total], dt), want["table"][name]), name
    for k2, dt in (("seen", np.uint64), ("least", np.uint64), ("hash", np.uint8)):
        assert np.array_equal(host(sw[k2], dt), want[k2]), k2
    assert host(sparse["cnt"], np.uint64).tolist() == want["counts"].tolist()
    print(json.dumps({"verified": "sparse", "counts": want["counts"].tolist()}), flush=True)
    for tn in sw.values():
        tn.zero_()
    scan_fn(full)()
    ctx.sync()
    cnt_b = host(full["cnt"], np.uint64).tolist()
    assert cnt_b == [npk, 0, 0, 0, 0, npk, npk, npk, 0, 3 * npk, 0, n_conns, 0], cnt_b
    # the newest STOP_WAITING of a connection: its largest packet number, delta 1
    top = np.zeros(n_conns, np.uint64)
    np.maximum.at(top, conn, pn)
    assert np.array_equal(host(sw["seen"], np.uint64), top)
    assert np.array_equal(host(sw["least"], np.uint64), top - np.uint64(1))

    # ---- (d) the dense raises beside a compact list
    moved = np.sort(rng.permutation(n_conns)[:n_conns // 100]).astype(np.uint32)
    dense_mark = np.zeros(n_conns, np.uint64)
    dense_mark[moved] = 5
    slot_key_d = up((np.arange(n, dtype=np.uint64) % np.uint64(n_conns)) << np.uint64(shift) |
                    (np.arange(n, dtype=np.uint64) // np.uint64(n_conns) * np.uint64(16) +
                     np.uint64(17)), np.int64)  # (every open group above the thresholds)
    len_open = torch.full((n,), 9, dtype=torch.int16, device=dev)
    marks = torch.zeros(n_conns, dtype=torch.int64, device=dev)
    host_key = up(key[perm] + np.uint64(16), np.int64)
    r_out = torch.zeros(npk, dtype=torch.int64, device=dev)
    lists = {"dense": (up(np.arange(n_conns, dtype=np.uint32), np.int32), up(dense_mark, np.int64),
                       up(np.zeros(n_conns, np.uint8), np.uint8), n_conns),
             "compact": (up(moved, np.int32), up(dense_mark[moved], np.int64),
                         up(np.zeros(moved.size, np.uint8), np.uint8), int(moved.size))}
    cells = torch.zeros(n_conns * window, dtype=torch.uint8, device=dev)
    r_least = torch.ones(n_conns, dtype=torch.int64, device=dev)
    r_largest = torch.zeros(n_conns, dtype=torch.int64, device=dev)
    r_hash = torch.zeros(n_conns, dtype=torch.uint8, device=dev)

    def retire_fn(which):
        rc, rm, _, nr = lists[which]

        def fn():
            ctx.retire_groups(host_key, npk, slot_key_d, len_open, n, marks, n_conns, shift, 0,
                              r_out, raise_conn=rc, raise_mark=rm, n_raise=nr)
        return fn

    def record_fn(which):
        rc, rm, rh, nr = lists[which]

        def fn():
            ctx.record_received(cells, r_least, r_largest, r_hash, n_conns, window, raise_conn=rc,
                                raise_least=rm, raise_hash=rh, n_raise=nr)
        return fn

    phase("d", {"retire_dense": retire_fn("dense"), "retire_compact": retire_fn("compact"),
                "record_dense": record_fn("dense"), "record_compact": record_fn("compact")})
    assert int((len_open != 9).sum()) == 0  # (nothing closed)

    # ---- (e) the turn, every group new, with and without the scan
    m = npk
    a = full
    stale_key_d = up(np.roll(host(slot_key_d, np.uint64), 12345), np.int64)
    key_k = torch.ones(n, dtype=torch.uint8, device=dev)
    acc = torch.zeros(n * stride, dtype=torch.uint8, device=dev)
    acc_len = torch.zeros(n, dtype=torch.int16, device=dev)
    maps = torch.full((n * ms,), 0xFF, dtype=torch.uint8, device=dev)
    all_ok = up(np.ones(m, np.uint8), np.uint8)
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
    # (thresholds of 0: the scan's least_unacked here would refuse every group)
    zero_mark = torch.zeros(n_conns, dtype=torch.int64, device=dev)

    def turn(with_scan):
        def fn():
            acc_len.zero_()
            marks.zero_()
            ctx.parse_opened(data, a["off"], a["len"], a["pn"], a["conn"], m, version, shift,
                             a["key"], a["idx"], a["body_off"], a["body_len"], a["hdr"],
                             pkt_ok=all_ok, entropy_out=a["entropy"])
            kw = {}
            if with_scan:
                scan_fn(a)()
                kw = dict(raise_conn=sw["conn"], raise_mark=zero_mark, n_raise=n_conns)
            ctx.retire_groups(a["key"], m, stale_key_d, acc_len, n, marks, n_conns, shift, 0,
                              b["key_out"], **kw)
            ctx.assign_slots(b["key_out"], a["k"], m, stale_key_d, key_k, acc_len, n, b["slot"])
            ctx.bin_arrivals(b["slot"], a["body_off"], a["body_len"], a["idx"], all_ok, m, n,
                             b["t_ptr"], b["t_off"], b["t_ln"], b["t_idx"], pkt_ok_out=b["t_ok"])
            ctx.admit_ragged(b["t_off"], b["t_ln"], b["t_idx"], b["t_ok"], b["t_ptr"], n, key_k,
                             maps, ms, acc_len, stride, b["o_ptr"], b["o_off"], b["o_ln"], b["v"])
            ctx.accumulate_ragged(data, b["o_off"], b["o_ln"], b["o_ptr"], n, acc, stride, acc_len)
        return fn

    phase("e", {"turn_with_scan": turn(True), "turn_without": turn(False)})
    rows = {}
    for name, fn in (("with", turn(True)), ("without", turn(False))):
        acc.zero_()
        fn()
        ctx.sync()
        rows[name] = (acc.clone(), acc_len.clone())
    assert torch.equal(rows["with"][0], rows["without"][0])
    assert torch.equal(rows["with"][1], rows["without"][1])
    assert int((rows["with"][1] != 0).sum()) == n
    del rows, acc

    # ---- (f) the copy back, over a slice
    piece = 256 << 20
    pinned = torch.empty(piece, dtype=torch.uint8, pin_memory=True)

    def copy_fn():
        pinned.copy_(data[:piece], non_blocking=True)

    phase("f", {"copy_back_256MiB": copy_fn})
    scale = data.numel() / piece

    med = lambda k: us[k]["median"]  # noqa: E731
    got = {
        "a_scan_us": med("a_scan"), "a_scan_over_parse": med("a_scan") / med("a_parse"),
        "b_scan_us": med("b_scan"), "b_scan_over_parse": med("b_scan") / med("b_parse"),
        "b_over_a": med("b_scan") / med("a_scan"), "c_sparse_scan_us": med("c_sparse_scan"),
        "d_retire_dense_minus_compact_us": med("d_retire_dense") - med("d_retire_compact"),
        "d_record_dense_minus_compact_us": med("d_record_dense") - med("d_record_compact"),
        "e_turn_added_fraction": med("e_turn_with_scan") / med("e_turn_without") - 1.0,
        "f_copy_back_ms": med("f_copy_back_256MiB") * scale / 1e3,
    }
    verdicts = {k: {"expected": list(BANDS[k]), "measured": v,
                    "verdict": "confirmed" if BANDS[k][0] <= v <= BANDS[k][1] else "refuted"}
                for k, v in got.items()}
    doc = {
        "tool": "tools/frames_rate.py",
        "device": torch.cuda.get_device_properties(0).name,
        "shape": {"groups": n, "connections": n_conns, "packets": npk,
                  "sparse_packets": int(sparse_order.size), "arena_bytes": int(data.numel()),
                  "max_frames": max_frames, "frm_cap": cap, "quic_version": version,
                  "mix_1": "one stream frame", "mix_2": "ack, stop waiting, stream",
                  "record_bytes": "24 in (read twice), 5 out per packet, 34 per frame listed"},
        "method": {"timer": "HIP events around back-to-back rounds, as many as fill window_ms",
                   "inner": args.inner, "window_ms": args.window_ms, "reps": args.reps,
                   "warmup": args.warmup, "rounds_per_window": inner,
                   "order": "the legs of a phase alternate; the phases follow one another "
                            "(one arena, rewritten between the mixes)",
                   "round": "scan legs: sw_seen zeroed, then the call; turns: acc_len and the "
                            "marks zeroed, then the calls",
                   "verified": "after timing: the sparse leg's every output equals "
                               "tests/frames_rule.py over its whole input; the full legs' "
                               "verdicts, frm_ptr (mix 1), counts and STOP_WAITING state equal "
                               "what the mixes give by construction; the turn with the scan "
                               "leaves the rows and lengths of the turn without"},
        "us": us,
        "expectations": verdicts,
        "counts_mix_1": cnt_a, "counts_mix_2": cnt_b,
        "not_measured": ["the host's walk over the copied packets",
                         "frames of mixed validity: every packet here walks to its end",
                         "max_frames below the frames present",
                         "an arrival order other than uniformly random",
                         "the copy back of the whole arena (a 256 MiB slice, scaled)"],
    }
    print(json.dumps(verdicts), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
