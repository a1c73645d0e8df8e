"""Generates tests/golden/frames_ref.npz: what the REFERENCE QuicFramer makes of
a packet's frame area, so that tests/frames_rule.py, the host C++ and the device
are pinned to it where the reference tree is absent.
Run:  python tests/golden/make_golden_frames.py [path of the reference tree]

The framer is the reference's own, unpatched quic_framer.cc compiled from its
tree as a release build (the source list, the flags and the link of
make_golden_ackwire.py) behind tests/golden/frames_ref_shim.cc, into
oracle/_ref/frames/ (outside git).  Only cases and verdicts are committed: per
case the bytes behind the private flags, the version, the packet number and its
length; the framer's error code; every frame its visitor was shown.

Cases: packets BuildDataPacket wrote (every frame kind alone and together;
stream frames at every id and offset width, with and without a length and fin;
acks with 0 / 1 / 255 missing packets, 0 / 1 / 3 receipt times, truncated for
want of room; versions 31 and 33; all four packet number lengths; padding first
and last), every prefix of a set of them, every type byte 0..255 as a one-byte
body, and bodies put together from frames and noise.  Inputs on which the
reference is undefined -- a STOP_WAITING delta above the packet number: it trips
a DCHECK, and the release build reports a least_unacked that wrapped -- are left
out and counted.
"""
import ctypes as C
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "oracle", "_ref", "frames")
DROPPED = 96  # cases with a STOP_WAITING delta above the packet number (asserted below)
MAX_SEEN = 64
PN_FOR = {1: 100, 2: 30000, 4: 1 << 30, 6: (1 << 40) + 5}
U32P, U64P = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)


def build(ref):
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import make_golden_ackwire as W
    src, bssl = os.path.join(ref, "src"), os.path.join(ref, "boringssl")
    os.makedirs(OUT, exist_ok=True)
    jobs = [("g++", W.CXXFLAGS, os.path.join(src, s), s.replace("/", "_")[:-3] + ".o")
            for s in W.SOURCES]
    jobs += [("gcc", W.CFLAGS, os.path.join(bssl, s), "bssl_" + s.replace("/", "_")[:-2] + ".o")
             for s in W.BSSL]
    jobs.append(("g++", W.CXXFLAGS, os.path.join(ROOT, "tests", "golden", "frames_ref_shim.cc"),
                 "frames_ref_shim.o"))

    def compile_one(job):
        cc, flags, s, o = job
        o = os.path.join(OUT, o)
        if not os.path.exists(o) or os.path.getmtime(o) < os.path.getmtime(s):
            subprocess.run([cc, *flags, "-I", src, "-I", os.path.join(bssl, "include"), "-c", s,
                            "-o", o], check=True)
        return o

    with ThreadPoolExecutor(8) as pool:
        objs = list(pool.map(compile_one, jobs))
    so = os.path.join(OUT, "libref_frames.so")
    subprocess.run(["g++", "-shared", "-pthread", "-Wl,--gc-sections", "-Wl,-z,defs", "-o", so,
                    *objs], check=True)
    lib = C.CDLL(so)
    lib.frames_ref_build.restype = C.c_size_t
    lib.frames_ref_build.argtypes = [C.c_int, C.c_uint64, C.c_int, C.c_size_t, U32P, U64P, U64P,
                                     U64P, U64P, C.c_size_t, C.c_void_p, C.c_size_t]
    lib.frames_ref_process.restype = C.c_size_t
    lib.frames_ref_process.argtypes = [C.c_int, C.c_uint64, C.c_int, C.c_char_p, C.c_size_t,
                                       C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                       C.POINTER(C.c_int32), U64P, C.c_char_p, C.c_size_t,
                                       C.c_size_t, U32P, U32P, U32P, U32P, U64P, U32P, U32P]
    lib.frames_ref_limits.argtypes = [U32P, U32P, U32P]
    return lib


def built(lib, version, pn, pn_len, frames, room=1200):
    """the bytes BuildDataPacket writes behind the private flags for `frames`,
    tuples (kind, a, b, c, d); None where it fails"""
    n = len(frames)
    kind = (C.c_uint32 * n)(*[f[0] for f in frames])
    cols = [(C.c_uint64 * n)(*[f[i] for f in frames]) for i in range(1, 5)]
    out = (C.c_uint8 * 2048)()
    got = lib.frames_ref_build(version, pn, pn_len, n, kind, *cols, room, out, 2048)
    return bytes(out[:got]) if got else None


def processed(lib, version, pn, pn_len, body):
    err, acc, comp, seen_pn = C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_uint64(0)
    text = C.create_string_buffer(256)
    cols = [(C.c_uint32 * MAX_SEEN)() for _ in range(4)] + [(C.c_uint64 * MAX_SEEN)()] + \
        [(C.c_uint32 * MAX_SEEN)() for _ in range(2)]
    n = lib.frames_ref_process(version, pn, pn_len, body, len(body), C.byref(err), C.byref(acc),
                               C.byref(comp), C.byref(seen_pn), text, 256, MAX_SEEN, *cols)
    assert n <= MAX_SEEN, n
    assert seen_pn.value == pn, (seen_pn.value, pn)
    frames = [tuple(int(c[k]) for c in cols) for k in range(n)]  # type flags len id val code sum
    return dict(error=err.value, accepted=acc.value, complete=comp.value,
                text=text.value.decode(), frames=frames)


def valid_packets(lib, tags):
    """(tag, version, pn, pn_len, body) from BuildDataPacket"""
    out = []

    def add(tag, version, pn_len, frames, room=1200, pn=None):
        pn = PN_FOR[pn_len] if pn is None else pn
        body = built(lib, version, pn, pn_len, frames, room)
        assert body is not None, (tag, frames)
        out.append((tag, version, pn, pn_len, body))
        tags[tag] = tags.get(tag, 0) + 1

    ids = [5, 0x1FF, 0x1FFFF, 0x1FFFFFF]
    offsets = [0, 9, 0x10000, 0x1000000, 1 << 32, 1 << 40, 1 << 48, 1 << 56]
    for version in (31, 33):
        for i, sid in enumerate(ids):
            for j, so in enumerate(offsets):
                fin, n = (i + j) & 1, 1 + 3 * ((i * 8 + j) % 5)
                add("stream_last", version, 6, [(0x80, sid, so, n, fin)])
                add("stream_length", version, 6, [(0x80, sid, so, n, 1 - fin), (7, 0, 0, 0, 0)])
        add("stream_empty_fin", version, 6, [(0x80, 7, 0, 0, 1), (0x80, 9, 300, 0, 1)])
        for big in (1000, 70000, (1 << 33) + 600):
            for missing in (0, 1, 255):
                for times in (0, 1, 3):
                    add("ack_%d_%d" % (missing, times), version, 6,
                        [(0x40, big, missing, times, 0x5A), (7, 0, 0, 0, 0)])
            add("ack_truncated", version, 6, [(0x40, big, 255, 0, 0x33)], room=200)
        add("ack_small", version, 6, [(0x40, 200, 1, 1, 1), (0x40, 7, 0, 0, 2)])
        for pn_len in (1, 2, 4, 6):
            pn = PN_FOR[pn_len]
            for delta in (0, 1, pn - 1):
                add("stop_waiting_%d" % pn_len, version, pn_len,
                    [(6, pn - delta, 0, 0, 0xC3), (0x80, 3, 0, 4, 0)])
        every = [(1, 0x01020304, (1 << 40) + 7, 6, 0), (2, 0, 0, 25, 11), (3, 77, 0, 16, 5),
                 (4, 0x0A0B0C0D, (1 << 50) + 3, 0, 0), (5, 0x11223344, 0, 0, 0),
                 (6, 1, 0, 0, 0x77), (7, 0, 0, 0, 0), (8, 3, 0, 0, 0), (0x40, 900, 1, 1, 9), (0x80, 3, 77, 10, 1)]
        for f in every:
            add("kind_%d" % f[0], version, 6, [f])
        add("every_kind", version, 6, every)
        add("every_kind", version, 2, every[::-1])
        add("padding_last", version, 6, every[:5] + [(0, 0, 0, 0, 0)], room=140)
        add("padding_first", version, 6, [(0, 0, 0, 0, 0)], room=30)
        add("two_stop_waitings", version, 4,
            [(6, 5, 0, 0, 1), (7, 0, 0, 0, 0), (6, 900, 0, 0, 2), (6, 0, 0, 0, 3)])
        add("codes_above_the_last", version, 6,
            [(1, 1, 2, 0xFFFFFFF0, 0), (2, 0, 0, 0x7FFFFFFF, 2), (3, 9, 0, 0x0FFFFFFF, 0)])
    return out


def noise(rng):
    """a body put together from frames and bytes nobody chose"""
    parts = []
    for _ in range(int(rng.integers(1, 6))):
        k = int(rng.integers(0, 10))
        if k == 0:
            parts.append(bytes([0x80 | int(rng.integers(0, 128))]) + rng.bytes(int(rng.integers(0, 24))))
        elif k == 1:
            parts.append(bytes([0x40 | int(rng.integers(0, 64))]) + rng.bytes(int(rng.integers(0, 40))))
        elif k == 2:
            parts.append(bytes([6, int(rng.integers(0, 256)), int(rng.integers(0, 4))]) +
                         bytes(int(rng.integers(0, 6))))
        elif k == 3:
            parts.append(bytes([7]))
        elif k == 4:
            parts.append(bytes([int(rng.integers(1, 9))]) + rng.bytes(int(rng.integers(0, 20))))
        elif k == 5:
            parts.append(bytes([2, 1, 0, 0, 0, 3, 0, 65, 66, 67]))
        elif k == 6:
            parts.append(bytes([0xA0, 5, 2, 0, 1, 2]))
        elif k == 7:
            parts.append(bytes([0x60, 1, 9, 0, 0, 2, 1, 0, 1, 3, 1, 8]))
        else:
            parts.append(rng.bytes(int(rng.integers(1, 10))))
    return b"".join(parts)


def main():
    sys.path.insert(0, ROOT)
    from oracle import ref_quic  # (where oracle/ref/Makefile finds the reference tree)
    lib = build(sys.argv[1] if len(sys.argv) > 1 else ref_quic.REF)
    rng = np.random.default_rng(20161108)
    tags = {}
    inputs = valid_packets(lib, tags)
    n_valid = len(inputs)
    for tag, version, pn, pn_len, body in inputs[:n_valid]:
        if len(body) <= 150 and not tag.startswith(("stream_last", "stream_length")):
            for cut in range(len(body)):
                inputs.append(("prefix", version, pn, pn_len, body[:cut]))
    # (the stream frames: one prefix set per id width, at the widest offset)
    for tag, version, pn, pn_len, body in inputs[:n_valid]:
        if tag == "stream_length" and version == 31 and body[0] & 0x1C == 0x1C:
            for cut in range(len(body)):
                inputs.append(("prefix", version, pn, pn_len, body[:cut]))
    for version in (31, 33):
        for t in range(256):
            inputs.append(("one_byte", version, PN_FOR[6], 6, bytes([t])))
    for i in range(1500):
        pn_len = int(rng.choice([1, 2, 4, 6]))
        pn = int(rng.choice([1, 2, 90])) if i % 3 else PN_FOR[pn_len]
        inputs.append(("noise", int(rng.choice([31, 33])), pn, pn_len, noise(rng)))

    cases, dropped = [], 0
    unique = set()
    for tag, version, pn, pn_len, body in inputs:
        key = (version, pn, pn_len, body)
        if key in unique and tag in ("prefix", "noise"):
            continue
        unique.add(key)
        r = processed(lib, version, pn, pn_len, body)
        # undefined in the reference: a least_unacked that wrapped
        if any(f[0] == 6 and f[4] > pn for f in r["frames"]):
            dropped += 1
            continue
        assert r["accepted"] == (r["error"] == 0) == r["complete"], r
        if tag not in ("prefix", "noise", "one_byte"):
            assert r["accepted"], (tag, r)
        tags[tag + "_cases"] = tags.get(tag + "_cases", 0) + 1
        tags["error_%d" % r["error"]] = tags.get("error_%d" % r["error"], 0) + 1
        cases.append(dict(version=version, pn=pn, pn_len=pn_len, body=body, **r))
    print(f"{len(cases)} cases, {dropped} dropped (a STOP_WAITING delta above the packet number)")
    print(" ".join(f"{k}:{v}" for k, v in sorted(tags.items())))
    texts = sorted({c["text"] for c in cases})
    print("\n".join(texts))
    assert dropped == DROPPED, dropped

    codes = (C.c_uint32 * 12)()
    last, stream_last = C.c_uint32(0), C.c_uint32(0)
    lib.frames_ref_limits(C.byref(last), C.byref(stream_last), codes)
    assert {c["error"] for c in cases} == set(codes), sorted({c["error"] for c in cases})
    body_ptr = np.cumsum([0] + [len(c["body"]) for c in cases]).astype(np.int64)
    frame_ptr = np.cumsum([0] + [len(c["frames"]) for c in cases]).astype(np.int64)
    flat = [f for c in cases for f in c["frames"]]
    col = lambda i, dt: np.array([f[i] for f in flat], dt)  # noqa: E731
    path = os.path.join(ROOT, "tests", "golden", "frames_ref.npz")
    np.savez_compressed(
        path, version=np.array([c["version"] for c in cases], np.uint8),
        pn=np.array([c["pn"] for c in cases], np.uint64),
        pn_len=np.array([c["pn_len"] for c in cases], np.uint8), body_ptr=body_ptr,
        body=np.frombuffer(b"".join(c["body"] for c in cases), np.uint8),
        error=np.array([c["error"] for c in cases], np.int32), frame_ptr=frame_ptr,
        f_type=col(0, np.uint8), f_flags=col(1, np.uint8), f_len=col(2, np.uint32),
        f_id=col(3, np.uint32), f_val=col(4, np.uint64), f_code=col(5, np.uint32),
        f_sum=col(6, np.uint32), error_codes=np.array(list(codes), np.int32),
        last_error=np.uint32(last.value), stream_last_error=np.uint32(stream_last.value),
        dropped=np.int64(dropped), n_valid=np.int64(n_valid))
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
