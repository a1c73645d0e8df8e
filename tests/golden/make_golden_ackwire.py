"""Generates tests/golden/ackwire_ref.npz: the REFERENCE QuicFramer's own v<=31
ack frames, byte for byte, so that tests/ackwire_rule.py, the host C++ and the
device are pinned to it where the reference tree is absent.
Run:  python tests/golden/make_golden_ackwire.py [path of the reference tree]

The framer is the reference's own, unpatched quic_framer.cc compiled from its
tree as a release build (-DNDEBUG, linked with -z defs: no stand-in; the source
list is the one oracle/ref/Makefile links) behind
tests/golden/ackwire_ref_shim.cc, into oracle/_ref/ackwire/ (outside git).  Only
the cases and the frames' bytes behind the packet header are committed.

A case is an ack (largest observed, missing intervals, entropy hash), a delay
and the room the frame gets.  Its received entropy is listed: the received
packets with the entropy flag set (flag_pn), every other one having flag 0, on
top of base_hash; the ack's hash is base_hash ^ the hashes of the listed ones,
and the framer's calculator answers from the same list when it truncates.
Inputs on which the reference writer itself fails (QUIC_BUG, no room for a
mandatory byte) are left out and counted.  The unpatched framer always writes a
revived count of 0: the revived tail is pinned to qfec_wire_write_revived.
"""
import ctypes as C
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "oracle", "_ref", "ackwire")
SOURCES = """net/quic/core/quic_framer.cc net/quic/core/crypto/quic_decrypter.cc
net/quic/core/crypto/quic_encrypter.cc net/quic/core/quic_flags.cc net/quic/core/quic_protocol.cc
net/quic/core/quic_data_reader.cc net/quic/core/quic_data_writer.cc net/quic/core/quic_utils.cc
net/quic/core/crypto/crypto_framer.cc net/quic/core/crypto/crypto_handshake_message.cc
net/quic/core/quic_socket_address_coder.cc net/base/ip_endpoint.cc net/base/ip_address.cc
net/quic/core/crypto/null_encrypter.cc net/quic/core/crypto/null_decrypter.cc
net/quic/core/crypto/aes_128_gcm_12_encrypter.cc net/quic/core/crypto/aes_128_gcm_12_decrypter.cc
net/quic/core/crypto/chacha20_poly1305_encrypter.cc
net/quic/core/crypto/chacha20_poly1305_decrypter.cc net/quic/core/crypto/aead_base_encrypter.cc
net/quic/core/crypto/aead_base_decrypter.cc net/quic/core/crypto/scoped_evp_aead_ctx.cc
net/base/int128.cc crypto/hkdf.cc crypto/hmac.cc base/logging.cc base/debug/alias.cc
base/debug/debugger.cc base/debug/stack_trace.cc base/debug/activity_tracker.cc
base/synchronization/lock.cc base/synchronization/lock_impl_posix.cc
base/threading/platform_thread_posix.cc base/threading/platform_thread_linux.cc
base/threading/thread_checker_impl.cc base/threading/thread_local_storage.cc
base/threading/thread_local_storage_posix.cc base/threading/thread_local_posix.cc
base/strings/string_piece.cc base/time/time.cc base/time/time_posix.cc base/sequence_token.cc
base/lazy_instance.cc base/at_exit.cc base/callback_internal.cc base/vlog.cc
base/strings/stringprintf.cc base/strings/string_number_conversions.cc""".split()
BSSL = """crypto/cipher/aead.c crypto/cipher/e_aes.c crypto/cipher/e_chacha20poly1305.c
crypto/err/err.c crypto/mem.c crypto/crypto.c crypto/cpu-intel.c crypto/thread_pthread.c
crypto/aes/aes.c crypto/modes/gcm.c crypto/modes/ctr.c crypto/chacha/chacha.c
crypto/poly1305/poly1305.c crypto/poly1305/poly1305_vec.c crypto/hkdf/hkdf.c crypto/hmac/hmac.c
crypto/digest/digest.c crypto/digest/digests.c crypto/sha/sha1.c crypto/sha/sha256.c
crypto/sha/sha512.c crypto/md4/md4.c crypto/md5/md5.c""".split()
CXXFLAGS = ["-std=gnu++11", "-O2", "-DNDEBUG", "-w", "-fPIC", "-ffunction-sections",
            "-fdata-sections", "-fvisibility=hidden", "-fvisibility-inlines-hidden"]
CFLAGS = ["-std=gnu11", "-O2", "-DNDEBUG", "-w", "-fPIC", "-D_GNU_SOURCE", "-DOPENSSL_NO_ASM",
          "-ffunction-sections", "-fdata-sections", "-fvisibility=hidden"]

INFINITE = (1 << 64) - 1
UFLOAT16_MAX = 0x3FFC0000000
DELAYS = [0, 1, 4095, 4096, 4097, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, (1 << 31) + 12345,
          UFLOAT16_MAX - 1, UFLOAT16_MAX, UFLOAT16_MAX + 1, INFINITE]
EDGES = [255, 256, 65535, 65536, (1 << 32) - 1, 1 << 32]
LENGTHS = [1, 255, 256, 257, 512, 513]
COUNTS = [1, 63, 64, 65, 255]
DROPPED = 913  # cases on which the reference writer fails (asserted below)


def build(ref):
    src, bssl = os.path.join(ref, "src"), os.path.join(ref, "boringssl")
    os.makedirs(OUT, exist_ok=True)
    jobs = [("g++", CXXFLAGS, os.path.join(src, s), s.replace("/", "_")[:-3] + ".o") for s in SOURCES]
    jobs += [("gcc", CFLAGS, os.path.join(bssl, s), "bssl_" + s.replace("/", "_")[:-2] + ".o")
             for s in BSSL]
    jobs.append(("g++", CXXFLAGS, os.path.join(ROOT, "tests", "golden", "ackwire_ref_shim.cc"),
                 "ackwire_ref_shim.o"))

    def compile_one(job):
        cc, flags, s, o = job
        o = os.path.join(OUT, o)
        if not os.path.exists(o) or os.path.getmtime(o) < os.path.getmtime(s):
            subprocess.run([cc, *flags, "-I", src, "-I", os.path.join(bssl, "include"), "-c", s,
                            "-o", o], check=True)
        return o

    with ThreadPoolExecutor(8) as pool:
        objs = list(pool.map(compile_one, jobs))
    so = os.path.join(OUT, "libref_ackwire.so")
    subprocess.run(["g++", "-shared", "-pthread", "-Wl,--gc-sections", "-Wl,-z,defs", "-o", so,
                    *objs], check=True)
    lib = C.CDLL(so)
    lib.ackwire_ref_frame.restype = C.c_size_t
    lib.ackwire_ref_frame.argtypes = [C.c_uint64, C.c_uint8, C.c_void_p, C.c_void_p, C.c_size_t,
                                      C.c_uint64, C.c_size_t, C.c_uint8, C.c_void_p, C.c_size_t,
                                      C.c_void_p, C.c_size_t]
    return lib


def structure(largest, top_gap, lengths, gaps):
    """intervals, ascending, from the top down: the last missing number is
    largest - top_gap, gaps[i] >= 2 lies between the last number of an interval
    and the first of the one above; None where it would reach below 1"""
    out, last = [], largest - top_gap
    for i, n in enumerate(lengths):
        lo = last - n + 1
        if lo < 1:
            return None
        out.append((lo, last + 1))
        if i < len(gaps):
            last = lo - gaps[i]
    return out[::-1]


def structures(rng):
    """(tag, largest, intervals)"""
    out = []
    for big in [1, 2, 200] + EDGES + [(1 << 48) - 2]:
        out.append(("none", big, []))
    for big in EDGES + [(1 << 48) - 2, 70000, 5000]:
        for top in [1, 2] + EDGES:  # largest and max_delta at the edges
            if top < big:
                out.append(("edge", big, structure(big, top, [1], [])))
                if top >= 2:  # (a gap of 1 would be one interval)
                    out.append(("edge", big, structure(big, 1, [2, 3], [top])))
    for n in LENGTHS:  # interval lengths, alone and in company
        out.append((f"len{n}", 5000, structure(5000, 3, [n], [])))
        out.append((f"len{n}", 70000, structure(70000, 1, [2, n, 1], [2, 9])))
        out.append((f"len{n}", (1 << 32) + 4000, structure((1 << 32) + 4000, 300, [n, n], [2])))
    for c in COUNTS:
        for n, gap in ((1, 2), (1, 3), (3, 2), (513, 2)):
            base = (n + gap) * c + 1000
            out.append((f"count{c}", base, structure(base, 1, [n] * c, [gap] * (c - 1))))
        out.append((f"count{c}", (1 << 32) + 90000,
                    structure((1 << 32) + 90000, 2, [1] * c, [300] * (c - 1))))
    for _ in range(150):  # anything
        c = int(rng.integers(1, 40))
        big = int(rng.choice([300, 3000, 70000, 1 << 33, (1 << 48) - 2]))
        lengths = [int(rng.choice([1, 1, 2, 5, 40, 256, 300])) for _ in range(c)]
        gaps = [int(rng.choice([2, 2, 3, 7, 100, 257])) for _ in range(c - 1)]
        out.append(("random", big, structure(big, int(rng.integers(1, 20)), lengths, gaps)))
    return [s for s in out if s[2] is not None]


def main():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from oracle import ref_quic  # (where oracle/ref/Makefile finds the reference tree)
    import ackwire_rule as R  # (to choose capacities around a frame's own size, nothing more)
    lib = build(sys.argv[1] if len(sys.argv) > 1 else ref_quic.REF)
    rng = np.random.default_rng(20161107)
    cases, tags, dropped = [], {}, 0
    out = (C.c_uint8 * 4096)()
    for s_i, (tag, big, ivs) in enumerate(structures(rng)):
        near = {big, max(big - 1, 1)}
        for lo, hi in ivs:
            near |= {lo - 1, hi, lo - 2, hi + 1}
        near = sorted(p for p in near if 1 <= p <= big and not any(l <= p < h for l, h in ivs))
        flagged = [p for p in near if rng.random() < 0.6]
        base_hash = int(rng.integers(0, 256))
        h = base_hash
        for p in flagged:
            h ^= 1 << p % 8
        full = len(R.write_ack_frame(big, h, ivs, [], 0, 4000, entropy_up_to=lambda pn: 0)["frame"])
        ll = R.number_length(big)
        caps = [full + int(rng.integers(1, 900)), full, full - 1, full - 2, 6 + ll, 7 + ll,
                5 + ll, 4 + ll, 3, (full + 6 + ll) // 2, int(rng.integers(6 + ll, full + 2))]
        delays = DELAYS if s_i % 9 == 0 else [DELAYS[(s_i + j * 5) % len(DELAYS)] for j in range(2)]
        for cap in sorted(set(c for c in caps if c >= 0)):
            for delay in delays if cap in (caps[0], full) else delays[:1]:
                lo_a = (C.c_uint64 * max(1, len(ivs)))(*[iv[0] for iv in ivs])
                hi_a = (C.c_uint64 * max(1, len(ivs)))(*[iv[1] for iv in ivs])
                fl_a = (C.c_uint64 * max(1, len(flagged)))(*flagged)
                n = lib.ackwire_ref_frame(big, h, lo_a, hi_a, len(ivs), delay, cap, base_hash, fl_a,
                                          len(flagged), out, 4096)
                if n == 0:
                    dropped += 1
                    continue
                assert n <= cap
                kind = "generous" if cap == caps[0] else "exact" if cap == full else "short"
                for t in (tag, "cap_" + kind, "delay_%d" % DELAYS.index(delay)):
                    tags[t] = tags.get(t, 0) + 1
                frame = bytes(out[:n])
                if frame[0] & 0x10:
                    tags["truncated"] = tags.get("truncated", 0) + 1
                cases.append(dict(largest=big, hash=h, base_hash=base_hash, ivs=ivs, flagged=flagged,
                                  delay=delay, cap=cap, frame=frame))
    print(f"{len(cases)} cases, {dropped} dropped (the reference writer fails)")
    print(" ".join(f"{k}:{v}" for k, v in sorted(tags.items())))
    assert dropped == DROPPED, dropped
    need = ["none", "edge", "random", "truncated", "cap_generous", "cap_exact", "cap_short"]
    need += [f"len{n}" for n in LENGTHS] + [f"count{c}" for c in COUNTS]
    need += ["delay_%d" % i for i in range(len(DELAYS))]
    assert all(tags.get(t, 0) >= 3 for t in need), [t for t in need if tags.get(t, 0) < 3]

    def csr(key, dtype):
        ptr = np.cumsum([0] + [len(c[key]) for c in cases]).astype(np.int64)
        flat = [x for c in cases for x in c[key]]
        return ptr, np.array(flat, dtype)

    range_ptr = np.cumsum([0] + [len(c["ivs"]) for c in cases]).astype(np.int64)
    flag_ptr, flag_pn = csr("flagged", np.uint64)
    frame_ptr, frame = csr("frame", np.uint8)
    path = os.path.join(ROOT, "tests", "golden", "ackwire_ref.npz")
    np.savez_compressed(
        path, largest=np.array([c["largest"] for c in cases], np.uint64),
        hash=np.array([c["hash"] for c in cases], np.uint8),
        base_hash=np.array([c["base_hash"] for c in cases], np.uint8),
        delay=np.array([c["delay"] for c in cases], np.uint64),
        cap=np.array([c["cap"] for c in cases], np.uint16), range_ptr=range_ptr,
        range_lo=np.array([iv[0] for c in cases for iv in c["ivs"]], np.uint64),
        range_hi=np.array([iv[1] for c in cases for iv in c["ivs"]], np.uint64),
        flag_ptr=flag_ptr, flag_pn=flag_pn, frame_ptr=frame_ptr, frame=frame,
        dropped=np.int64(dropped))
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
