"""Inputs for the frame-scan tests: frame writers (the wire format of
include/qfec.h's qfec_wire_scan_frames, written out by hand), bodies put together
from frames and noise, and the arena that holds a turn's bodies with guard bytes
around every one."""
import os

import numpy as np

GUARD = 0xEE
U64 = np.uint64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frames_ref.npz")


def le(v, n):
    return int(v).to_bytes(n, "little")


def stream(sid, offset, data, fin=False, length=True, id_len=None, off_len=None):
    id_len = id_len or max(1, (int(sid).bit_length() + 7) // 8)
    if off_len is None:
        off_len = 0 if offset == 0 else max(2, (int(offset).bit_length() + 7) // 8)
    t = 0x80 | fin << 6 | length << 5 | (off_len - 1 if off_len else 0) << 2 | (id_len - 1)
    return bytes([t]) + le(sid, id_len) + le(offset, off_len) + \
        (le(len(data), 2) if length else b"") + data


def ack(largest, hsh, ll=2, mm=1, ranges=(), revived=(), times=0, truncated=False, version=31):
    """ranges: (delta, length - 1) pairs as they lie on the wire"""
    code = {1: 0, 2: 1, 4: 2, 6: 3}
    t = 0x40 | bool(ranges) << 5 | truncated << 4 | code[ll] << 2 | code[mm]
    out = bytes([t, hsh]) + le(largest, ll) + b"\x34\x12"
    if not truncated:
        out += bytes([times]) + (bytes(5 + 3 * (times - 1)) if times else b"")
    if ranges:
        out += bytes([len(ranges)]) + b"".join(le(d, mm) + bytes([n]) for d, n in ranges)
        if version <= 31:
            out += bytes([len(revived)]) + b"".join(le(r, ll) for r in revived)
    return out


def stop_waiting(pn, pn_len, least, hsh=0):
    return bytes([6, hsh]) + le(pn - least, pn_len)


PING = b"\x07"


def rst(sid, offset, code):
    return b"\x01" + le(sid, 4) + le(offset, 8) + le(code, 4)


def close(code, text):
    return b"\x02" + le(code, 4) + le(len(text), 2) + text


def goaway(code, last, text):
    return b"\x03" + le(code, 4) + le(last, 4) + le(len(text), 2) + text


def window_update(sid, offset):
    return b"\x04" + le(sid, 4) + le(offset, 8)


def blocked(sid):
    return b"\x05" + le(sid, 4)


def path_close(path):
    return bytes([8, path])


def rand_body(rng, pn=None, pn_len=None):
    """frames and noise; with pn and pn_len also STOP_WAITINGs that fit them"""
    parts = []
    for _ in range(int(rng.integers(0, 6))):
        k = int(rng.integers(0, 14))
        if k == 0:
            parts.append(bytes([0x80 | int(rng.integers(0, 128))]) + rng.bytes(int(rng.integers(0, 24))))
        elif k == 1:
            parts.append(bytes([0x40 | int(rng.integers(0, 64))]) + rng.bytes(int(rng.integers(0, 40))))
        elif k == 2:
            parts.append(bytes([6]) + rng.bytes(int(rng.integers(0, 8))))
        elif k == 3 and pn is not None:
            parts.append(stop_waiting(pn, pn_len, int(rng.integers(0, min(pn, 200) + 1)),
                                      int(rng.integers(0, 256))))
        elif k == 4:
            parts.append(PING)
        elif k == 5:
            parts.append(bytes([int(rng.integers(0, 10))]) + rng.bytes(int(rng.integers(0, 20))))
        elif k == 6:
            parts.append(close(int(rng.integers(0, 1 << 32)), rng.bytes(int(rng.integers(0, 9)))))
        elif k == 7:
            parts.append(stream(int(rng.integers(1, 1 << 32)), int(rng.integers(0, 1 << 62)),
                                rng.bytes(int(rng.integers(0, 30))), fin=bool(rng.integers(0, 2))))
        elif k == 8:
            parts.append(ack(int(rng.integers(1, 1 << 16)), 7, ranges=[(1, 3), (0, 255)],
                             revived=[5], times=int(rng.integers(0, 4)),
                             version=31 if rng.integers(0, 2) else 33))
        elif k == 9:
            parts.append(rst(9, 1 << 40, 3) + window_update(8, 1 << 50) + blocked(7))
        elif k == 10:
            parts.append(goaway(4, 5, b"bye") + path_close(3))
        else:
            parts.append(rng.bytes(int(rng.integers(0, 12))))
    return b"".join(parts)


def arena(bodies, rng=None, offsets=None, lead=3):
    """(data, body_off, body_len): the bodies in one buffer of GUARD bytes, a gap
    of 0..4 bytes (rng) between two, or at the offsets given"""
    lens = np.array([len(b) for b in bodies], np.uint16)
    if not bodies:
        return np.full(lead + 9, GUARD, np.uint8), np.zeros(0, U64), lens
    if offsets is None:
        gaps = rng.integers(0, 5, len(bodies)) if rng is not None else np.ones(len(bodies), int)
        ends = np.cumsum(lens.astype(np.int64) + gaps)
        offsets = lead + np.concatenate(([0], ends[:-1]))
    offsets = np.asarray(offsets, U64)
    size = int(max((int(o) + int(n) for o, n in zip(offsets, lens)), default=0)) + 9
    data = np.full(size, GUARD, np.uint8)
    for b, o in zip(bodies, offsets):
        data[int(o):int(o) + len(b)] = np.frombuffer(b, np.uint8)
    return data, offsets, lens


def fixture_rows(version):
    """the golden fixture's cases of one version: (bodies, pn, pn_len)"""
    g = np.load(GOLDEN)
    rows = np.flatnonzero(g["version"] == version)
    ptr, body = g["body_ptr"], g["body"]
    return ([body[ptr[r]:ptr[r + 1]].tobytes() for r in rows], g["pn"][rows], g["pn_len"][rows])
