"""qfec_scan_frames on the device against tests/frames_rule.py, whole buffers
(frames_device.scan): the reference framer's fixture, the sizes around a wave
and a workgroup, every alignment of a body, the shortest and the longest body,
frame counts around max_frames, table capacities around the total, the optional
pointers, packets that must not be read, connections out of range, the
STOP_WAITING state with ties and stale packets, and turns of more packets than
one trip of the scan over the tiles and than one full grid take."""
import numpy as np
import pytest

import frames_cases as K
import frames_device as D
import frames_rule as R
from ack_device import same
from turn_sizes import GRID_PER_CU, SCAN_BLOCK, TILE, SCAN_WRAP, grid_wrap, ncu

gpu = pytest.mark.gpu
U64 = np.uint64


def random_turn(rng, n, n_conns, stale=True):
    pn_len = rng.choice([1, 2, 4, 6], n).astype(np.uint8)
    pn = rng.integers(1, 40, n).astype(U64)
    bodies = [K.rand_body(rng, int(pn[p]), int(pn_len[p])) for p in range(n)]
    conn = rng.integers(0, n_conns, n).astype(np.uint32)
    state = R.new_state(n_conns)
    if stale:
        state["seen"][:] = rng.integers(0, 30, n_conns)
        state["least"][:] = rng.integers(0, 30, n_conns)
        state["hash"][:] = rng.integers(0, 256, n_conns)
    return bodies, pn, conn, pn_len, state


@gpu
@pytest.mark.parametrize("version", [31, 33])
def test_the_reference_fixture(ctx, version):
    bodies, pn, pn_len = K.fixture_rows(version)
    n = len(bodies)
    data, off, lens = K.arena(bodies, np.random.default_rng(version))
    conn = (np.arange(n) % 4).astype(np.uint32)
    want = D.scan(ctx, data, off, lens, pn, conn, pn_len, None, version, 255, 1 << 14,
                  R.new_state(4), 4)
    assert want["counts"][0] > 500 and want["counts"][2] > 500 and want["counts"][10] == 0
    assert {int(s) for s in want["status"]} == set(range(R.NO_FRAMES, R.PATH_CLOSE + 1)) | {R.OK}


@gpu
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_sizes(ctx, n):
    rng = np.random.default_rng(100 + n)
    bodies, pn, conn, pn_len, state = random_turn(rng, n, 3)
    data, off, lens = K.arena(bodies, rng)
    hdr = rng.choice([0, 1, 2, 3], n).astype(np.uint8)
    # (n == 0: nothing is looked at; counts zeroed, one entry of frm_ptr, the state as it was)
    D.scan(ctx, data, off, lens, pn, conn, pn_len, hdr, 31, 255, 4 * n + 1, state, 3)


@gpu
def test_every_alignment_and_the_shortest_and_longest_bodies(ctx):
    rng = np.random.default_rng(7)
    long_stream = K.stream(9, 1 << 33, rng.bytes(1350 - 12), fin=True, length=False, id_len=4,
                           off_len=7)
    assert len(long_stream) == 1350
    padded = K.PING + bytes(1349)  # a ping and 1348 bytes of padding behind its type byte
    kinds = [K.PING, b"\x00", b"\x09", b"\x80", long_stream, padded,
             K.stop_waiting(300, 6, 299, 0x42) + K.rst(1, 2, 3),
             K.ack(70000, 3, ll=4, mm=2, ranges=[(5, 1)] * 40, revived=[9, 8]) + K.blocked(1)]
    bodies, offsets, at = [], [], 0
    for r in range(16):  # every residue of body_off mod 16, for every kind of body
        for b in kinds:
            at += (r - at) % 16 or 16
            bodies.append(b), offsets.append(at)
            at += len(b)
    n = len(bodies)
    data, off, lens = K.arena(bodies, offsets=offsets)
    assert sorted(set(int(o) % 16 for o in off)) == list(range(16))
    pn = np.full(n, 300, U64)
    want = D.scan(ctx, data, off, lens, pn, np.zeros(n, np.uint32), np.full(n, 6, np.uint8), None,
                  31, 255, 4 * n, R.new_state(1), 1)
    assert want["status"][:8].tolist() == [R.OK, R.OK, R.ILLEGAL_TYPE, R.STREAM] + [R.OK] * 4
    assert (want["table"]["len"] == 1338).any() and want["table"]["len"].max() == 1348


@gpu
@pytest.mark.parametrize("max_frames", [1, 255])
def test_frame_counts_around_max_frames(ctx, max_frames):
    counts = [0, 1, max_frames, max_frames + 1, max_frames - 1 or 1, max_frames + 7]
    bodies = [K.PING * c for c in counts]
    # ... and mixed frames instead of pings, the last one a stream without a length
    bodies += [(K.blocked(5) + K.PING) * (c // 2) + K.stream(3, 0, b"xy", length=False)
               for c in counts]
    n = len(bodies)
    data, off, lens = K.arena(bodies, np.random.default_rng(1))
    want = D.scan(ctx, data, off, lens, np.full(n, 5, U64), np.zeros(n, np.uint32),
                  np.full(n, 1, np.uint8), None, 33, max_frames, n * max_frames + 3,
                  R.new_state(1), 1)
    assert want["status"][:4].tolist() == [R.NO_FRAMES, R.OK, R.OK, R.TOO_MANY]
    assert np.diff(want["ptr"].astype(np.int64))[:4].tolist() == [0, 1, max_frames, 0]


@gpu
def test_table_capacity_and_optional_pointers(ctx):
    rng = np.random.default_rng(11)
    bodies, pn, conn, pn_len, state = random_turn(rng, 400, 5)
    data, off, lens = K.arena(bodies, rng)
    args = (data, off, lens, pn, conn, pn_len)
    total = int(R.scan_arrays(*args, None, 31, 255, 0, state, 5)["counts"][9])
    assert total > 100
    for cap in (0, total, total - 1, total + 5, 1):
        want = D.scan(ctx, *args, None, 31, 255, cap, state, 5)
        assert want["counts"][10] == max(0, total - cap) and want["ptr"][-1] == total
    D.scan(ctx, *args, None, 31, 255, 0, state, 5, tables=False)  # NULL tables with frm_cap == 0
    D.scan(ctx, *args, None, 33, 255, total, state, 5, counts=False)  # NULL hdr and counts


@gpu
def test_packets_that_are_not_read_and_callers_errors(ctx):
    rng = np.random.default_rng(13)
    n = 130
    bodies, pn, conn, pn_len, state = random_turn(rng, n, 4)
    # well-formed frames in every skipped packet: reading one would list them
    hdr = rng.choice([0, 1, 2, 3, 4, 5, 6, 7, 0x80, 0x81, 0x85, 0x86, 0xFF], n,
                     p=[.15] * 4 + [.4 / 9] * 9).astype(np.uint8)
    skipped = (hdr >= 0x80) | ((hdr & 4) != 0)
    for p in np.flatnonzero(skipped):
        bodies[p] = K.stop_waiting(int(pn[p]), int(pn_len[p]), int(pn[p]), 0xA5) + K.PING * 3
    pn[skipped] = 1 << 40  # (the newest of all, had they counted)
    pn_len[::9] = np.resize(np.array([3, 0, 5, 7, 8, 255], np.uint8), len(pn_len[::9]))
    conn[::7] = np.resize(np.array([4, 5, 1 << 31, 0xFFFFFFFF], np.uint32), len(conn[::7]))
    data, off, lens = K.arena(bodies, rng)
    want = D.scan(ctx, data, off, lens, pn, conn, pn_len, hdr, 31, 255, 600, state, 4)
    assert (want["status"][skipped] == R.SKIPPED).all() and want["latched"]
    assert want["counts"][1] == skipped.sum() and want["counts"][4] > 8
    assert {R.PN_LEN, R.RANGE} <= set(want["status"].tolist())
    assert want["seen"].max() < 1 << 40
    # no connection at all: the state pointers may be NULL, every packet is out of range
    ok = ~skipped
    want = D.scan(ctx, data, off, lens, pn, conn, np.full(n, 2, np.uint8), hdr, 31, 255, 8,
                  R.new_state(0), 0)
    assert (want["status"][ok] == R.RANGE).all() and want["counts"][9] == 0


@gpu
@pytest.mark.parametrize("n_conns", [1, 300])
def test_stop_waiting_state(ctx, n_conns):
    rng = np.random.default_rng(17 + n_conns)
    n = 2000
    pn = rng.integers(1, 25, n).astype(U64)  # few numbers: ties and stale packets abound
    conn = rng.integers(0, n_conns, n).astype(np.uint32)
    pn_len = rng.choice([1, 2, 4, 6], n).astype(np.uint8)
    bodies = []
    for p in range(n):
        frames = [K.PING, K.blocked(p)][:int(rng.integers(0, 3))]
        for _ in range(int(rng.integers(0, 3))):  # none, one or two in a packet
            frames.append(K.stop_waiting(int(pn[p]), int(pn_len[p]), int(rng.integers(0, pn[p] + 1)),
                                         int(rng.integers(0, 256))))
        if rng.integers(0, 12) == 0:
            frames.append(b"\x1f")  # the walk fails behind the frame
        bodies.append(b"".join(frames) or K.PING)
    data, off, lens = K.arena(bodies, rng)
    state = R.new_state(n_conns)
    state["seen"][:] = rng.integers(0, 20, n_conns)
    state["least"][:] = rng.integers(0, 20, n_conns)
    state["hash"][:] = rng.integers(0, 256, n_conns)
    want = D.scan(ctx, data, off, lens, pn, conn, pn_len, None, 33, 4, 3 * n, state, n_conns)
    assert 0 < want["counts"][11] <= n_conns and want["counts"][12] > 0
    if n_conns > 1:
        assert (want["seen"] == state["seen"]).any() and (want["seen"] != state["seen"]).any()
    # the state the call left is the next call's: the same packets again are all stale
    again = D.scan(ctx, data, off, lens, pn, conn, pn_len, None, 33, 4, 3 * n,
                   dict(seen=want["seen"], least=want["least"], hash=want["hash"]), n_conns)
    assert again["counts"][11] == 0 and np.array_equal(again["least"], want["least"])


# ---- turns beyond one scan trip and one full grid ----------------------------------------------
def vocabulary(version):
    """(body, pn_len): one to three frames, or a body that fails.  A STOP_WAITING
    holds pn - least, so the bytes fit every packet number above 7."""
    return [(K.PING, 1),
            (K.stop_waiting(3, 2, 0, 0x42) + K.PING, 2),
            (K.blocked(5) + K.stream(3, 0, b"xy", length=False), 4),
            (K.ack(70000, 3, ll=4, mm=2, ranges=[(5, 1)] * 3, revived=[9, 8], version=version), 6),
            (b"\x1f", 1),                                       # an illegal type
            (K.rst(1, 2, 3)[:9], 2),                            # a cut frame
            (K.PING + K.blocked(7) + K.window_update(8, 1 << 50), 1),
            (K.stop_waiting(1, 1, 0, 0x11) + K.stop_waiting(7, 1, 0, 0xA5), 1),  # the last one counts
            (K.PING + b"\x1f", 4),                              # fails behind a frame: none listed
            (b"", 2)]


def listed_per_body(vocab, version, max_frames):
    """the frames a packet of every body lists, by the packet-by-packet walk"""
    out = []
    for body, pn_len in vocab:
        verdict, frames = R.walk(body, version, 1000, pn_len, max_frames)
        out.append(len(frames) if verdict == R.OK else 0)
    return np.array(out, np.int64)


def vocabulary_arena(rng, vocab, pick):
    """frames_cases.arena for bodies vocab[pick], by array operations: 1..4
    guard bytes between two bodies, so body_off takes every residue mod 16"""
    size = np.array([len(b) for b, _ in vocab], np.int64)
    start = np.cumsum(size) - size
    flat = np.frombuffer(b"".join(b for b, _ in vocab), np.uint8)
    lens = size[pick]
    step = lens + rng.integers(1, 5, len(pick))
    off = 3 + np.cumsum(step) - step
    data = np.full(int(off[-1] + lens[-1]) + 9, K.GUARD, np.uint8)
    within = np.arange(int(lens.sum())) - np.repeat(np.cumsum(lens) - lens, lens)
    data[np.repeat(off, lens) + within] = flat[np.repeat(start[pick], lens) + within]
    assert sorted(set((off % 16).tolist())) == list(range(16))
    return data, off.astype(U64), lens.astype(np.uint16)


def runs(hdr, pn_len, conn, n_conns):
    """the packets frames_rule.gate lets through to the walk"""
    code = hdr.astype(np.int64) << 9 | pn_len.astype(np.int64) << 1 | (conn >= n_conns)
    kinds, of = np.unique(code, return_inverse=True)
    through = [R.gate(int(c) >> 9, int(c) >> 1 & 0xFF, n_conns if c & 1 else 0, n_conns) is None
               for c in kinds]
    return np.array(through)[of]


PLACED = (R.F_STREAM, R.F_ACK, 0, 2, 3)  # the types whose off is a place in the arena
_tied = []


def tie_to_the_packet_rule(args, hdr, version, max_frames, state, n_conns, want):
    """scan_arrays against scan_packets on the 2,000 packets around index
    SCAN_BLOCK * TILE, cut out of the turn with their piece of the arena: the
    same verdicts, and the rows the full table holds between the range's two
    frm_ptr values, pkt and off counted from the slice's start.  Once a module."""
    if _tied:
        return
    data, off, lens, pn, conn, pn_len = args
    a, b = SCAN_BLOCK * TILE - 1900, min(len(off), SCAN_BLOCK * TILE + 100)
    assert a < SCAN_BLOCK * TILE < b
    base = int(off[a]) - 3
    part = R.scan_packets(data[base:int(off[b - 1]) + int(lens[b - 1]) + 9], off[a:b] - U64(base),
                          lens[a:b], pn[a:b], conn[a:b], pn_len[a:b],
                          None if hdr is None else hdr[a:b], version, max_frames, 1 << 30, state,
                          n_conns)
    r0, r1 = int(want["ptr"][a]), int(want["ptr"][b])
    assert r1 - r0 > 1000 and r1 <= len(want["table"]["pkt"])
    same("status", part["status"], want["status"][a:b])
    same("ptr", part["ptr"].astype(np.int64), want["ptr"][a:b + 1].astype(np.int64) - r0)
    placed = np.isin(want["table"]["type"][r0:r1], PLACED)
    for name, dt in R.COLUMNS:
        rows = want["table"][name][r0:r1]
        if name == "pkt":
            rows = rows - np.uint32(a)
        if name == "off":
            rows = np.where(placed, rows - U64(base), rows)
        same(name, part["table"][name], rows)
    _tied.append(True)


@gpu
def test_packets_beyond_one_scan_trip(ctx):
    """262,145 packets are 1,025 tiles: frames_scan_kernel takes a second trip
    and carries its base into it, and frm_ptr of the last tile hangs on it"""
    n, version = SCAN_WRAP, 31
    assert (n + TILE - 1) // TILE > SCAN_BLOCK, "the packets no longer make the scan take a second trip"
    rng = np.random.default_rng(23)
    vocab = vocabulary(version)
    pick = rng.integers(0, len(vocab), n)
    pick[[0, n - 1]] = 1, 6
    data, off, lens = vocabulary_arena(rng, vocab, pick)
    pn_len = np.array([ln for _, ln in vocab], np.uint8)[pick]
    pn = rng.integers(8, 40, n).astype(U64)
    conn = rng.integers(0, 5, n).astype(np.uint32)
    state = R.new_state(5)
    state["seen"][:] = rng.integers(0, 60, 5)
    total = int(listed_per_body(vocab, version, 255)[pick].sum())
    args = (data, off, lens, pn, conn, pn_len)
    want = D.scan(ctx, *args, None, version, 255, total, state, 5)
    assert want["counts"][9] == total and want["counts"][10] == 0
    assert (want["counts"][[0, 2, 5, 6, 7, 8, 11]] > 0).all()
    listed = np.diff(want["ptr"].astype(np.int64))
    for tile in (0, SCAN_BLOCK - 1, SCAN_BLOCK, (n - 1) // TILE):
        assert listed[tile * TILE:(tile + 1) * TILE].any(), tile
    assert want["ptr"][-1] > want["ptr"][SCAN_BLOCK * TILE] > 0
    tie_to_the_packet_rule(args, None, version, 255, state, 5, want)


@gpu
def test_packets_beyond_one_grid(ctx):
    """one packet more than ncu * 16 workgroups of 256 take in a trip: the
    first workgroup's second trip brings the call's last packet, whose tile
    is tile_off's last entry in both passes, whose verdict and frames enter
    the tallies the workgroup kept from its first trip, and whose STOP_WAITING
    is its connection's newest"""
    n, n_conns, version, max_frames = grid_wrap(), 300, 31, 2
    grid = ncu() * GRID_PER_CU * TILE
    assert n > grid, "the packets no longer make the grid loop"
    rng = np.random.default_rng(29)
    vocab = vocabulary(version)
    per_body = listed_per_body(vocab, version, max_frames)
    assert per_body.max() == 2 and per_body[6] == 0  # (three frames: too many)
    pick = rng.integers(0, len(vocab), n)
    pick[n - 1] = 1
    data, off, lens = vocabulary_arena(rng, vocab, pick)
    pn_len = np.array([ln for _, ln in vocab], np.uint8)[pick]
    pn = rng.integers(8, 40, n).astype(U64)
    conn = rng.integers(0, n_conns, n).astype(np.uint32)
    hdr = rng.choice([0, 1, 2, 3, 4, 5, 0x80, 0x85, 0xFF], n,  # (from 4 on: skipped)
                     p=[.2375] * 4 + [.01] * 5).astype(np.uint8)
    wrong = rng.random(n) < 0.01
    pn_len[wrong] = np.resize(np.array([3, 0, 5, 7, 8, 255], np.uint8), wrong.sum())
    wrong = rng.random(n) < 0.01
    conn[wrong] = np.resize(np.array([n_conns, n_conns + 1, 1 << 31, 0xFFFFFFFF], np.uint32),
                            wrong.sum())
    # the last packet: a STOP_WAITING newer than any of its connection
    last = n - 1
    hdr[last], pn_len[last], conn[last], pn[last] = 0, vocab[1][1], 7, 1000
    state = R.new_state(n_conns)
    state["seen"][:] = rng.integers(0, 60, n_conns)
    state["least"][:] = rng.integers(0, 60, n_conns)
    state["hash"][:] = rng.integers(0, 256, n_conns)
    total = int(per_body[pick][runs(hdr, pn_len, conn, n_conns)].sum())
    args = (data, off, lens, pn, conn, pn_len)
    want = D.scan(ctx, *args, hdr, version, max_frames, total, state, n_conns)
    assert want["counts"][9] == total and want["counts"][10] == 0 and want["latched"]
    assert (want["counts"][:9] > 0).all(), want["counts"]
    assert want["counts"][11] > 1 and want["counts"][12] > 0
    # connection 7's winner is the packet of the second trip; the other
    # connections that took a new STOP_WAITING took it from the first trip
    assert last >= grid and want["seen"][7] == pn[last] == 1000
    assert (pn[:last][conn[:last] == 7] < 1000).all()
    moved = np.flatnonzero(want["seen"] != state["seen"])
    assert moved.size > 1 and (want["seen"][moved[moved != 7]] < 1000).all()
    tie_to_the_packet_rule(args, hdr, version, max_frames, state, n_conns, want)
