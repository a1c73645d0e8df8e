#!/usr/bin/env python3
"""qfec_write_ack_frames beside the build it follows, and the copy-back it removes.

One MI355X.  The states are those of tools/ack_rate.py leg (d), each built by
one qfec_record_received: 65,536 connections of 160 packet numbers at window
256, and 16,384 of 640 at window 1,024, a tenth of the numbers missing, a tenth
of those revived; max_ranges 255, max_revived 16; an ack per connection.

  (a), (b) the writer with room for every frame of the shape (out_cap 170 and
      490, a slot of 192 and 512 bytes an ack), at the two shapes, alternating in one process with qfec_build_acks on the same state:
      the writer is reported as a ratio of the build it follows;
  (c) the same with out_cap 20, so that every ack is cut and every wave walks
      the ring from the largest it writes to the largest it was given;
  (d) build -> write -> qfec_write_private_headers -> ChaCha20-Poly1305 seal of
      the ack packets against the build alone, for the turn's shape of
      ack_rate.py leg (e): 4,096 connections at window 8,192 with 4,111 numbers;
  (e) the copy-back the call is for, at shape (a): the D2H of the build's tables
      (the used part, after a first copy of the two pointer arrays that sizes
      it; pinned memory) + the host writer over them + the H2D of the frames,
      against the D2H of the sealed packets alone.

EXPECTATION, stated before the first run, to confirm or refute.  Nobody has
measured any of this.  (a): 16 of 160 numbers are missing, nearly all alone:
about 14.5 intervals an ack, a frame of 6 + 1 + 29 + 1 + 1.6 = about 39 bytes;
65,536 waves of one trip.  A wave is a chain of dependent round trips -- the
ack's scalars and pointers, the intervals, the interval above, the same again in
the second walk, the revived numbers, the stores -- say 8 of 1-2 us under load;
at 73 VGPRs 6 waves a SIMD, 6,144 resident, 11 rounds: 90-180 us if latency
binds all of it, less where the trips of different waves overlap fully (they
do: that is what the residency is for), so SUPPOSEDLY 40-120 us, 0.5-1.6 of the
build's 72 us (three launches, two walks of three trips).  (b): a quarter of
the waves, 58 intervals in one trip, frames of about 140 bytes: 20-60 us,
0.1-0.35 of the build's 183 us.  (c): the walk adds 3 trips of cells at window
256 and 10 at window 1,024 but drops most stores: within -20% .. +40% of (a) and
(b).  (d): 4,096 acks of about 370 intervals are cut by the BUILD at 255; the
writer's two walks are 4 trips each, the frames about 780 bytes: write 10-30
us, headers 3-6 us, seal of 3.2 MB 15-40 us: 30-80 us behind a build of
50-100 us, 1-2% of the 4.8 ms turn.  (e): 65,536 x 14.5 intervals x 16 B = 15 MB
of tables + 1.2 MB of scalars at 20-25 GB/s: 0.7-0.9 ms, + 2.6 MB of frames
back up 0.1-0.15 ms, against 3.9 MB of sealed packets down, 0.15-0.25 ms: 3-6
times the bytes and the time, before the host writer -- 65,536 frames at a
SUPPOSED 0.3-1 us each in C++ are 20-65 ms on one core, two orders above
everything else (through this tool's per-ack ctypes call it is more; the tool
reports that figure as what it is).

RESULT, recorded after the run (profiles/ackwire_rate.json has every figure).
(a) 78 us, confirmed; 0.43 of the build, REFUTED: the build takes 183 us at this
shape -- the band above put its 72 us here, which is the other shape's.  (b) 57
us, confirmed; 0.79 of the build (72 us), REFUTED by the same mix-up.  A quarter
of the waves cost 0.73 of the time: the chain inside a wave, not the number of
waves, is most of it.  (c) 1.09 and 1.04, confirmed.  (d) +77 us behind the
build (write 22 us), 1.3% of the recorded turn: both confirmed.  (e) 447 us
against 80 us, 5.6 times, confirmed; the host writer through ctypes 5.5 us an
ack, 360 ms in all.

The legs alternate in this process: warm-up, then `--reps` alternations, each
timed with HIP events around back-to-back rounds -- as many as fill
`--window-ms`; medians with the 10th / 90th percentiles.  After timing every
leg's frames equal tests/ackwire_rule.py (the whole-array form) byte for byte.

NOT measured: the whole turn of ack_rate.py leg (e) with and without write +
seal in one process (leg (d) times the tail of that turn alone and quotes the
turn's recorded median from profiles/ack_rate.json); AES-128-GCM; the host
writer as a C++ loop.

Writes one JSON document (default profiles/ackwire_rate.json); DESIGN.md §4
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

EXPECTED = {"a_write_over_build": [0.5, 1.6], "a_write_us": [40, 120],
            "b_write_over_build": [0.1, 0.35], "b_write_us": [20, 60],
            "c_over_uncut": [0.8, 1.4], "d_tail_us": [30, 80], "d_share_of_turn": [0.01, 0.02],
            "e_copies_ratio": [3, 6]}


def pct(v, q):
    return float(np.percentile(np.asarray(v), q))


def verdict(value, band):
    return "confirmed" if band[0] <= value <= band[1] else "refuted"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=2)
    ap.add_argument("--window-ms", type=float, default=20.0,
                    help="least timed window; rounds repeat until they fill it")
    ap.add_argument("--host-sample", type=int, default=4096, help="acks the host writer is timed over")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ackwire_rate.json"))
    args = ap.parse_args()

    import torch
    import ackwire_rule as R
    from libquic_amd import qfec

    if not torch.cuda.is_available():
        sys.exit("ackwire_rate: no HIP device (this tool only measures on the GPU)")
    dev, shift, U64 = "cuda:0", 40, np.uint64
    ctx = qfec.Context(0)
    ctx.set_stream(torch.cuda.current_stream())
    rng = np.random.default_rng(20161107)

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

    def shape(name, nc, w, span, slot):
        """a state built by one record (ack_rate.py's build_leg), its acks and a frame slot each"""
        c = np.repeat(np.arange(nc, dtype=np.uint32), span)
        q = np.tile(np.arange(1, span + 1, dtype=U64), nc)
        gone = rng.random(c.size) < 0.1
        gone[q == U64(span)] = False  # (the largest arrives)
        rv = np.flatnonzero(gone & (rng.random(c.size) < 0.1))
        got = rng.permutation(np.flatnonzero(~gone))
        s = dict(cells=zeros(nc * w, torch.uint8), least=zeros(nc, torch.int64),
                 largest=zeros(nc, torch.int64), hash=zeros(nc, torch.uint8))
        ctx.record_received(s["cells"], s["least"], s["largest"], s["hash"], nc, w,
                            packet_number=up(q[got], np.int64), pkt_conn=up(c[got], np.int32),
                            n_packets=int(got.size), rcv_out=zeros(got.size, torch.uint8),
                            entropy=up(rng.integers(0, 2, got.size).astype(np.uint8), np.uint8),
                            status=up(np.ones(rv.size, np.uint8), np.uint8),
                            revived_idx=zeros(rv.size, torch.uint8),
                            slot_key=up((c[rv].astype(U64) << U64(shift)) | q[rv], np.int64),
                            n_groups=int(rv.size), n_slots=int(rv.size), key_shift=shift)
        ctx.sync()
        mr, mv = 255, 16
        o = dict(largest=zeros(nc, torch.int64), hash=zeros(nc, torch.uint8),
                 truncated=zeros(nc, torch.uint8), range_ptr=zeros(nc + 1, torch.int32),
                 range_lo=zeros(nc * mr, torch.int64), range_hi=zeros(nc * mr, torch.int64),
                 rev_ptr=zeros(nc + 1, torch.int32), rev_pn=zeros(nc * mv, torch.int64))
        ad = 9  # an 8-byte connection id and flags in front of the private byte: the prefix
        off = np.arange(nc, dtype=U64) * U64(slot) + U64(ad + 1)
        d = dict(name=name, nc=nc, w=w, s=s, o=o, mr=mr, mv=mv, slot=slot, ad=ad, off_h=off,
                 conn=up(np.arange(nc, dtype=np.uint32), np.int32), off=up(off, np.int64),
                 arena=zeros(nc * slot, torch.uint8), wire=zeros(nc * slot, torch.uint8),
                 delay=up(rng.integers(0, 1 << 24, nc).astype(U64), np.int64),
                 out_len=zeros(nc, torch.int16), wl=zeros(nc, torch.int64),
                 wh=zeros(nc, torch.uint8), st=zeros(nc, torch.uint8), cnt=zeros(4, torch.int64))
        for cap in (min(slot - ad - 1 - 12, 1452), 20):
            d[f"cap{cap}"] = up(np.full(nc, cap, np.uint16), np.int16)
        d["caps"] = (min(slot - ad - 1 - 12, 1452), 20)
        return d

    def build_fn(d):
        o, s = d["o"], d["s"]

        def fn():
            ctx.build_acks(d["conn"], d["nc"], s["cells"], s["least"], s["largest"], s["hash"],
                           d["nc"], d["w"], d["mr"], d["mv"], o["largest"], o["hash"],
                           o["truncated"], o["range_ptr"], o["range_lo"], o["range_hi"],
                           o["rev_ptr"], o["rev_pn"])
        return fn

    def write_fn(d, cap):
        o, s = d["o"], d["s"]

        def fn():
            ctx.write_ack_frames(d["conn"], d["nc"], o["largest"], o["hash"], o["truncated"],
                                 o["range_ptr"], o["range_lo"], o["range_hi"], o["rev_ptr"],
                                 o["rev_pn"], s["cells"], d["nc"], d["w"], d["arena"], d["off"],
                                 d[f"cap{cap}"], d["out_len"], d["wl"], d["wh"], d["st"],
                                 ack_delay_us=d["delay"], prefix_len=1, counts=d["cnt"])
        return fn

    def seal_fns(d):
        keys = up(rng.integers(0, 256, 32, dtype=np.uint8), np.uint8)
        prefixes = up(rng.integers(0, 256, 4, dtype=np.uint8), np.uint8)
        nc = d["nc"]
        key_idx, path = zeros(nc, torch.int32), zeros(nc, torch.uint8)
        pn = up(np.arange(1, nc + 1, dtype=U64), np.int64)
        ad_off = up(d["off_h"] - U64(d["ad"] + 1), np.int64)
        ad_len = up(np.full(nc, d["ad"], np.uint16), np.int16)
        priv = up(d["off_h"] - U64(1), np.int64)
        hdr, fo = zeros(nc, torch.uint8), zeros(nc, torch.uint8)

        def headers():
            ctx.write_private_headers(d["arena"], priv, hdr, fo, nc, 31)

        def seal():
            ctx.chacha20poly1305_seal(keys, prefixes, key_idx, pn, path, d["arena"], ad_off, ad_len,
                                      priv, d["out_len"], nc, d["wire"], priv)
        return headers, seal

    A, B = shape("a_window_256", 65536, 256, 160, 192), shape("b_window_1024", 16384, 1024, 640, 512)
    T = shape("d_turn_window_8192", 4096, 8192, 4111, 2048)
    fns = {}
    for d in (A, B, T):
        fns["build_" + d["name"]] = build_fn(d)
        fns["write_" + d["name"]] = write_fn(d, d["caps"][0])
    for d in (A, B):
        fns["write_cut_" + d["name"]] = write_fn(d, 20)
    t_headers, t_seal = seal_fns(T)
    a_headers, a_seal = seal_fns(A)
    t_build, t_write = fns["build_" + T["name"]], fns["write_" + T["name"]]

    def tail_fn():
        t_build(), t_write(), t_headers(), t_seal()
    fns["d_build_write_headers_seal"] = tail_fn
    order = list(fns)
    for name in order:  # every leg once on its own, so that a latched error names its leg
        fns[name]()
        try:
            ctx.sync()
        except qfec.QfecError as e:
            sys.exit(f"ackwire_rate: leg {name}: {e}")
    inner = {name: rounds_per_window(fns[name]) for name in order}
    t = {name: [] for name in order}
    for _ in range(args.reps):
        for name in order:
            t[name].append(timed(fns[name], inner[name]))
    ctx.sync()
    print("timed", flush=True)

    # the frames of the timed calls against tests/ackwire_rule.py, whole inputs
    def batch_of(d):
        o = d["o"]
        return dict(ack_conn=np.arange(d["nc"], dtype=np.uint32), largest=host(o["largest"], U64),
                    hash=host(o["hash"], np.uint8), truncated=host(o["truncated"], np.uint8),
                    range_ptr=host(o["range_ptr"], np.uint32), range_lo=host(o["range_lo"], U64),
                    range_hi=host(o["range_hi"], U64), rev_ptr=host(o["rev_ptr"], np.uint32),
                    rev_pn=host(o["rev_pn"], U64), delay=host(d["delay"], U64))

    checked = {}
    for d in (A, B, T):
        fns["build_" + d["name"]]()
        ctx.sync()
        batch = batch_of(d)
        cells = host(d["s"]["cells"], np.uint8).reshape(d["nc"], d["w"])
        for cap in d["caps"] if d is not T else d["caps"][:1]:
            d["arena"].zero_()
            write_fn(d, cap)()
            ctx.sync()
            want = R.write_ack_frames_np(batch, cells, d["w"], np.zeros(d["nc"] * d["slot"], np.uint8),
                                         d["off_h"], np.full(d["nc"], cap), 1)
            assert np.array_equal(host(d["arena"], np.uint8), want["out"]), (d["name"], cap)
            for k, v, dt in (("out_len", d["out_len"], np.uint16), ("wire_largest", d["wl"], U64),
                             ("wire_hash", d["wh"], np.uint8), ("status", d["st"], np.uint8),
                             ("counts", d["cnt"], U64)):
                assert np.array_equal(host(v, dt), want[k]), (d["name"], cap, k)
            checked[f"{d['name']}_cap{cap}"] = dict(
                counts=want["counts"].tolist(), intervals=int(batch["range_ptr"][-1]),
                revived=int(batch["rev_ptr"][-1]), truncated_by_build=int(batch["truncated"].sum()),
                frame_bytes=int(want["out_len"].astype(np.int64).sum() - (want["out_len"] != 0).sum()))
            print(json.dumps({"verified": f"{d['name']}_cap{cap}", **checked[f"{d['name']}_cap{cap}"]}),
                  flush=True)

    # (e) the copy-back at shape (a): wall clock around synchronous copies, pinned memory
    d, o = A, A["o"]
    fns["build_" + d["name"]](), write_fn(d, d["caps"][0])(), a_headers(), a_seal()
    ctx.sync()
    n_rng, n_rev = int(host(o["range_ptr"], np.uint32)[-1]), int(host(o["rev_ptr"], np.uint32)[-1])
    small = [o["largest"], o["hash"], o["truncated"]]
    pin = lambda tn: torch.empty(tn.shape, dtype=tn.dtype).pin_memory()
    p_ptr = [pin(o["range_ptr"]), pin(o["rev_ptr"])]
    p_small = [pin(x) for x in small]
    p_tab = [pin(o["range_lo"][:n_rng]), pin(o["range_hi"][:n_rng]), pin(o["rev_pn"][:n_rev])]
    out_len = host(d["out_len"], np.uint16).astype(np.int64)
    frames_h = torch.empty(int(out_len.sum()), dtype=torch.uint8).pin_memory()
    frames_d = zeros(frames_h.numel(), torch.uint8)
    sealed_h = torch.empty(int((out_len + 12 + d["ad"]).sum()), dtype=torch.uint8).pin_memory()
    sealed_d = zeros(sealed_h.numel(), torch.uint8)

    def wall(fn):
        v = []
        for _ in range(args.reps + args.warmup):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            v.append((time.perf_counter() - t0) * 1e6)
        v = v[args.warmup:]
        return {"median": pct(v, 50), "p10": pct(v, 10), "p90": pct(v, 90)}

    def tables_down():
        for dst, src in zip(p_ptr, (o["range_ptr"], o["rev_ptr"])):
            dst.copy_(src)  # (sizes the rest: a synchronous copy of its own)
        for dst, src in zip(p_small + p_tab, small + [o["range_lo"][:n_rng], o["range_hi"][:n_rng],
                                                      o["rev_pn"][:n_rev]]):
            dst.copy_(src, non_blocking=True)

    copies = {"tables_d2h_us": wall(tables_down),
              "frames_h2d_us": wall(lambda: frames_d.copy_(frames_h, non_blocking=True)),
              "sealed_d2h_us": wall(lambda: sealed_h.copy_(sealed_d, non_blocking=True))}
    batch = batch_of(d)
    ns = min(args.host_sample, d["nc"])
    acks = [R.ack_of(batch, a) for a in range(ns)]
    t0 = time.perf_counter()
    for k in acks:
        qfec.wire_write_ack_frame(k["largest"], k["entropy_hash"], k["ranges"], k["revived"],
                                  k["delay_us"], 1452)
    per_ack = (time.perf_counter() - t0) * 1e6 / ns
    table_bytes = sum(x.numel() * x.element_size() for x in p_ptr + p_small + p_tab)
    copies.update(table_bytes=table_bytes, frame_bytes=int(frames_h.numel()),
                  sealed_bytes=int(sealed_h.numel()),
                  table_capacity_bytes=sum(o[k].numel() * 8 for k in ("range_lo", "range_hi", "rev_pn")),
                  host_writer_us_per_ack_through_ctypes=per_ack,
                  host_writer_us_all_acks_through_ctypes=per_ack * d["nc"])
    host_path = copies["tables_d2h_us"]["median"] + copies["frames_h2d_us"]["median"]
    copies["copies_ratio"] = host_path / copies["sealed_d2h_us"]["median"]
    copies["with_host_writer_ratio"] = (host_path + per_ack * d["nc"]) / copies["sealed_d2h_us"]["median"]

    us = {name: {"median": pct(v, 50), "p10": pct(v, 10), "p90": pct(v, 90)} for name, v in t.items()}
    med = lambda name: us[name]["median"]
    turn_us = None
    try:
        with open(os.path.join(ROOT, "profiles", "ack_rate.json")) as fh:
            turn_us = json.load(fh)["turn"]["with_record_and_build_us"]["median"]
    except (OSError, KeyError, ValueError):
        pass
    tail = med("d_build_write_headers_seal") - med("build_" + T["name"])
    result = {
        "a_write_us": med("write_" + A["name"]), "b_write_us": med("write_" + B["name"]),
        "a_write_over_build": med("write_" + A["name"]) / med("build_" + A["name"]),
        "b_write_over_build": med("write_" + B["name"]) / med("build_" + B["name"]),
        "c_over_uncut": [med("write_cut_" + x["name"]) / med("write_" + x["name"]) for x in (A, B)],
        "d_tail_us": tail, "d_share_of_turn": tail / turn_us if turn_us else None,
        "e_copies_ratio": copies["copies_ratio"]}
    verdicts = {k: ([verdict(x, EXPECTED[k]) for x in v] if isinstance(v, list)
                    else verdict(v, EXPECTED[k]) if v is not None else "not measured")
                for k, v in result.items()}
    doc = {"tool": "tools/ackwire_rate.py", "device": torch.cuda.get_device_properties(0).name,
           "expectation": {"stated": "before measuring (the tool's docstring has the arithmetic)",
                           "bands": EXPECTED},
           "method": {"timer": "HIP events around back-to-back rounds, as many as fill window_ms; "
                               "leg (e): wall clock around synchronous pinned copies",
                      "inner": args.inner, "window_ms": args.window_ms, "reps": args.reps,
                      "warmup": args.warmup, "rounds_per_window": inner,
                      "order": ", ".join(order) + ", alternating",
                      "verified": "after timing: every leg's whole frame buffer, out_len, "
                                  "wire_largest, wire_hash, status and counts equal "
                                  "tests/ackwire_rule.py (write_ack_frames_np)"},
           "legs_us": us, "frames": checked, "copy_back": copies,
           "turn_us_from_ack_rate_json": turn_us, "result": result, "verdict": verdicts,
           "not_measured": "the whole turn of ack_rate.py leg (e) with write + seal in one process "
                           "(leg d times the turn's tail and divides by the recorded turn); "
                           "AES-128-GCM; the host writer as a C++ loop (the figure is through a "
                           "ctypes call per ack)"}
    print(json.dumps({"result": result, "verdict": verdicts, "copy_back": copies}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
