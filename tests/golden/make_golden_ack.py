"""Generates tests/golden/ack_ref.npz: the REFERENCE QuicReceivedPacketManager's
acks over multi-turn traces, so that tests/ack_rule.py and the device are
pinned to it where the reference tree is absent.
Run:  python tests/golden/make_golden_ack.py [path of the reference tree]

The manager is the reference's own, unpatched quic_received_packet_manager.cc
compiled from its tree as a release build (-DNDEBUG, linked with -z defs: no
stand-in) behind tests/golden/ack_ref_shim.cc, into oracle/_ref/ack/ (outside
git).  Only the recorded traces and acks are committed.

The traces stay inside the domain in which the reference is defined and the
rule of include/qfec.h is the reference's: every STOP_WAITING has least_unacked
<= largest_observed + 1 at its turn, and copies of a packet agree on the
entropy flag.  Every live range fits a window of 64 packet numbers, so the
fixture runs at any window.  A turn is fed to the manager as its accepted
arrivals in arrival order, then its STOP_WAITING; then the ack is taken.
"""
import ctypes as C
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "oracle", "_ref", "ack")
SOURCES = """net/quic/core/quic_received_packet_manager.cc net/quic/core/quic_protocol.cc
net/quic/core/quic_connection_stats.cc net/quic/core/quic_bandwidth.cc net/quic/core/quic_flags.cc
net/quic/core/quic_time.cc net/quic/core/quic_utils.cc net/base/int128.cc base/logging.cc
base/debug/alias.cc base/debug/debugger.cc base/debug/stack_trace.cc base/debug/activity_tracker.cc
base/synchronization/lock.cc base/synchronization/lock_impl_posix.cc
base/threading/platform_thread_posix.cc base/threading/platform_thread_linux.cc
base/threading/thread_checker_impl.cc base/threading/thread_local_storage.cc
base/threading/thread_local_storage_posix.cc base/threading/thread_local_posix.cc
base/strings/string_piece.cc base/time/time.cc base/time/time_posix.cc base/sequence_token.cc
base/lazy_instance.cc base/at_exit.cc base/callback_internal.cc base/vlog.cc
base/strings/stringprintf.cc base/strings/string_number_conversions.cc""".split()
CXXFLAGS = ["-std=gnu++11", "-O2", "-DNDEBUG", "-w", "-fPIC", "-ffunction-sections",
            "-fdata-sections", "-fvisibility=hidden", "-fvisibility-inlines-hidden"]

N_CONNS, N_ROUNDS, SPAN = 320, 12, 64


def build(ref):
    src = os.path.join(ref, "src")
    os.makedirs(OUT, exist_ok=True)
    jobs = [(os.path.join(src, s), os.path.join(OUT, s.replace("/", "_")[:-3] + ".o"))
            for s in SOURCES]
    jobs.append((os.path.join(ROOT, "tests", "golden", "ack_ref_shim.cc"),
                 os.path.join(OUT, "ack_ref_shim.o")))

    def compile_one(job):
        if not os.path.exists(job[1]) or os.path.getmtime(job[1]) < os.path.getmtime(job[0]):
            subprocess.run(["g++", *CXXFLAGS, "-I", src, "-c", job[0], "-o", job[1]], check=True)

    with ThreadPoolExecutor(8) as pool:
        list(pool.map(compile_one, jobs))
    so = os.path.join(OUT, "libref_ack.so")
    subprocess.run(["g++", "-shared", "-pthread", "-Wl,--gc-sections", "-Wl,-z,defs", "-o", so,
                    *[o for _, o in jobs]], check=True)
    lib = C.CDLL(so)
    lib.ackref_new.restype = C.c_void_p
    lib.ackref_free.argtypes = [C.c_void_p]
    lib.ackref_receive.argtypes = [C.c_void_p, C.c_uint64, C.c_int]
    lib.ackref_stop_waiting.argtypes = [C.c_void_p, C.c_uint64, C.c_uint8]
    lib.ackref_ack.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    return lib


def flag_of(conn, pn):
    """the sender's entropy flag of a packet: one per (connection, number)"""
    return (conn * 2654435761 + pn * 40503 + (pn >> 3)) >> 4 & 1


def main():
    sys.path.insert(0, ROOT)
    from oracle import ref_quic  # (where oracle/ref/Makefile finds the reference tree)
    lib = build(sys.argv[1] if len(sys.argv) > 1 else ref_quic.REF)
    rng = np.random.default_rng(20161031)
    ref = [lib.ackref_new() for _ in range(N_CONNS)]
    least, big, got = [0] * N_CONNS, [0] * N_CONNS, [set() for _ in range(N_CONNS)]
    loss = rng.choice([0.0, 0.02, 0.1, 0.3, 0.5], N_CONNS)
    pkt_ptr, pkt_pn, pkt_conn, pkt_flag, pkt_taken = [0], [], [], [], []
    raise_ptr, raise_conn, raise_least, raise_hash = [0], [], [], []
    ack_big, ack_hash, range_ptr, range_lo, range_hi = [], [], [0], [], []
    lo_buf, hi_buf = (C.c_uint64 * 1024)(), (C.c_uint64 * 1024)()
    big_out, hash_out = C.c_uint64(), C.c_uint8()
    for rnd in range(N_ROUNDS):
        arrivals = []
        for c in range(N_CONNS):
            lo = max(least[c], 1)
            top = min(big[c] + int(rng.integers(0, 40)), lo + SPAN - 1)
            mine = [pn for pn in range(big[c] + 1, top + 1) if rng.random() >= loss[c]]
            # late arrivals of missing packets, copies of received ones, old ones, number 0
            for pn in range(lo, big[c]):
                if pn not in got[c] and rng.random() < 0.25:
                    mine.append(pn)
            known = sorted(got[c])
            for pn in rng.choice(known, min(len(known), int(rng.integers(0, 3))), replace=False) \
                    if known else []:
                mine.append(int(pn))
            if mine and rng.random() < 0.2:
                mine.append(mine[int(rng.integers(len(mine)))])  # a copy inside the turn
            if rng.random() < 0.1:
                mine.append(int(rng.integers(0, lo)))
            arrivals += [(c, pn) for pn in mine]
        order = rng.permutation(len(arrivals))
        for i in order:
            c, pn = arrivals[i]
            taken = lib.ackref_receive(ref[c], pn, flag_of(c, pn))
            if taken:
                got[c].add(pn)
                big[c] = max(big[c], pn)
            pkt_pn.append(pn), pkt_conn.append(c), pkt_flag.append(flag_of(c, pn))
            pkt_taken.append(taken)
        pkt_ptr.append(len(pkt_pn))
        for c in rng.permutation(N_CONNS):
            c = int(c)
            if big[c] + 1 > least[c] and rng.random() < 0.45:
                kind = rng.random()
                up = big[c] + 1 if kind < 0.2 else int(rng.integers(least[c] + 1, big[c] + 2))
                h = int(rng.integers(0, 256))
                lib.ackref_stop_waiting(ref[c], up, h)
                least[c] = up
                got[c] = {pn for pn in got[c] if pn >= up}
                raise_conn.append(c), raise_least.append(up), raise_hash.append(h)
        raise_ptr.append(len(raise_conn))
        for c in range(N_CONNS):
            n = lib.ackref_ack(ref[c], C.byref(big_out), C.byref(hash_out), lo_buf, hi_buf, 1024)
            assert n <= 1024 and big_out.value == big[c]
            ack_big.append(big_out.value), ack_hash.append(hash_out.value)
            range_lo += list(lo_buf[:n])
            range_hi += list(hi_buf[:n])
            range_ptr.append(len(range_lo))
    for r in ref:
        lib.ackref_free(r)
    path = os.path.join(ROOT, "tests", "golden", "ack_ref.npz")
    np.savez_compressed(
        path, n_conns=np.int64(N_CONNS), n_rounds=np.int64(N_ROUNDS), span=np.int64(SPAN),
        pkt_ptr=np.array(pkt_ptr, np.int64), pkt_pn=np.array(pkt_pn, np.uint64),
        pkt_conn=np.array(pkt_conn, np.uint32), pkt_flag=np.array(pkt_flag, np.uint8),
        pkt_taken=np.array(pkt_taken, np.uint8), raise_ptr=np.array(raise_ptr, np.int64),
        raise_conn=np.array(raise_conn, np.uint32), raise_least=np.array(raise_least, np.uint64),
        raise_hash=np.array(raise_hash, np.uint8),
        ack_largest=np.array(ack_big, np.uint64).reshape(N_ROUNDS, N_CONNS),
        ack_hash=np.array(ack_hash, np.uint8).reshape(N_ROUNDS, N_CONNS),
        range_ptr=np.array(range_ptr, np.int64), range_lo=np.array(range_lo, np.uint64),
        range_hi=np.array(range_hi, np.uint64))
    print(f"{N_ROUNDS * N_CONNS} turns, {len(pkt_pn)} packets ({sum(pkt_taken)} taken), "
          f"{len(raise_conn)} raises, {len(range_lo)} intervals, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
