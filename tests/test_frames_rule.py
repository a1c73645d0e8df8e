"""The frame walk's rule on the CPU: tests/frames_rule.py's two forms and the host
C++ (qfec_wire_scan_frames) against the reference QuicFramer's own verdicts and
frames (tests/golden/frames_ref.npz, from the unpatched reference), and the two
forms against each other over random bodies and over the STOP_WAITING state
rule.  No device is opened."""
import numpy as np
import pytest

import frames_cases as K
import frames_rule as R
from libquic_amd import qfec

U64 = np.uint64


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(K.GOLDEN))


def fnv(b):
    h = 2166136261
    for x in b:
        h = ((h ^ x) * 16777619) & 0xFFFFFFFF
    return h


def verdict_of(g):
    """the fixture's error codes as verdict classes: error_codes is in the order
    OK, NO_FRAMES, ILLEGAL_TYPE, STREAM .. PATH_CLOSE"""
    classes = [R.OK] + list(range(R.NO_FRAMES, R.PATH_CLOSE + 1))
    return {int(code): cls for code, cls in zip(g["error_codes"], classes)}


def as_seen(f, body, g):
    """a frame of the rule as the reference's visitor would have been shown it:
    (type, flags, len, id, val, code, sum), the columns of the fixture"""
    typ, flags, off, ln, fid, val, code = f
    text = body[off:off + ln]
    if typ == R.F_STREAM:
        return (typ, flags & 1, ln, fid, val, 0, fnv(text))
    if typ == R.F_ACK:
        return (typ, (flags >> 4) & 1, None, 0, val, code, 0)  # (missing packets: not walked)
    if typ == 0:
        return (0, 0, ln, 0, 0, 0, 0)
    if typ == 1:
        return (1, 0, 0, fid, val, min(code, int(g["stream_last_error"])), 0)
    if typ in (2, 3):
        return (typ, 0, ln, fid, 0, min(code, int(g["last_error"])), fnv(text))
    return (typ, 0, 0, fid, val, code, 0)


def test_fixture_covers_its_classes(golden):
    g = golden
    assert len(g["version"]) > 3000 and int(g["dropped"]) == 96
    assert set(g["version"].tolist()) == {31, 33} and set(g["pn_len"].tolist()) == {1, 2, 4, 6}
    assert set(g["error"].tolist()) == set(g["error_codes"].tolist())  # every error class
    kinds = set(g["f_type"].tolist())
    assert kinds == {0, 1, 2, 3, 4, 5, 6, 7, 8, 0x40, 0x80}
    ptr, body = g["body_ptr"], g["body"]
    lens = np.diff(ptr)
    one = np.flatnonzero(lens == 1)
    for v in (31, 33):  # every type byte alone
        assert set(body[ptr[one[g["version"][one] == v]]].tolist()) == set(range(256))
    first = body[ptr[:-1][lens > 0]]
    stream = first[(first & 0x80) != 0]
    assert {int(t) & 3 for t in stream} == {0, 1, 2, 3}          # every id width
    assert {(int(t) >> 2) & 7 for t in stream} == set(range(8))  # every offset width
    assert {(int(t) >> 5) & 3 for t in stream} == {0, 1, 2, 3}   # length and fin
    ok = g["error"] == g["error_codes"][0]
    n_frames = np.diff(g["frame_ptr"])
    assert (ok & (first_type(g, 0) == 0) & (n_frames == 1)).any()  # padding first
    missing = g["f_len"][g["f_type"] == 0x40]
    assert {0, 1, 255} <= set(missing.tolist())
    assert (g["f_flags"][g["f_type"] == 0x40] == 1).any()  # truncated by the writer


def first_type(g, k):
    """the type of every case's frame k (0xFF where it has none)"""
    ptr = g["frame_ptr"]
    has = np.diff(ptr) > k
    out = np.full(len(ptr) - 1, 0xFF, np.int64)
    out[has] = g["f_type"][ptr[:-1][has] + k]
    return out


def test_both_forms_and_host_equal_the_reference(golden):
    g = golden
    verdict = verdict_of(g)
    ptr, fp = g["body_ptr"], g["frame_ptr"]
    bodies = [g["body"][ptr[i]:ptr[i + 1]].tobytes() for i in range(len(ptr) - 1)]
    cols = [g[k] for k in ("f_type", "f_flags", "f_len", "f_id", "f_val", "f_code", "f_sum")]
    status = np.zeros(len(bodies), np.int64)
    for i, body in enumerate(bodies):
        version, pn, pn_len = int(g["version"][i]), int(g["pn"][i]), int(g["pn_len"][i])
        s, walked = R.walk(body, version, pn, pn_len)
        want = [tuple(int(c[k]) for c in cols) for k in range(fp[i], fp[i + 1])]
        # the verdict class, the frame count and every field; on a failing packet
        # the reference's delivered prefix is the walk up to the error
        assert s == verdict[int(g["error"][i])], (i, body.hex())
        got = [as_seen(f, body, g) for f in walked]
        assert len(got) == len(want), (i, body.hex())
        for a, b in zip(got, want):
            assert a == b or (a[0] == R.F_ACK and a[:2] + a[3:] == b[:2] + b[3:]), (i, a, b)
        host = qfec.wire_scan_frames(body, version, pn, pn_len)
        assert host == (s, walked if s == R.OK else [], walked), i
        status[i] = s
        # a listed ack is parsed as it lies; its missing packets are the reference's
        if s == R.OK and version == 31:
            for f, w in zip(walked, want):
                if f[0] == R.F_ACK:
                    used, p = qfec.wire_parse_ack_frame(body[f[2]:f[2] + f[3]])
                    if used:
                        assert used == f[3] and p["largest"] == f[5] and p["hash"] == f[6]
                        assert sum(hi - lo for lo, hi in p["ranges"]) == w[2], i
    # the array form, the cases of a version as one call
    for version in (31, 33):
        rows = np.flatnonzero(g["version"] == version)
        data, off, lens = K.arena([bodies[r] for r in rows], np.random.default_rng(5))
        zeros = np.zeros(len(rows), np.uint32)
        got = R.scan_arrays(data, off, lens, g["pn"][rows], zeros, g["pn_len"][rows], None,
                            version, 255, 1 << 20, R.new_state(1), 1)
        assert np.array_equal(got["status"], status[rows])
        seq = R.scan_packets(data, off, lens, g["pn"][rows], zeros, g["pn_len"][rows], None,
                             version, 255, 1 << 20, R.new_state(1), 1)
        same_result(got, seq)


def same_result(a, b):
    for k in a:
        if k == "table":
            for c in a[k]:
                assert np.array_equal(a[k][c], b[k][c]), (k, c)
        else:
            assert np.array_equal(a[k], b[k]), k


def test_bad_least_is_where_the_reference_is_undefined():
    # (the 96 cases the fixture leaves out: a delta above the packet number)
    body = K.PING + bytes([6, 0x11, 8])
    assert R.walk(body, 31, 7, 1) == (R.BAD_LEAST, [(7, 0, 0, 0, 0, 0, 0)])
    assert R.walk(body, 31, 8, 1)[0] == R.OK and R.walk(body, 31, 8, 1)[1][1][5] == 0
    assert qfec.wire_scan_frames(body, 31, 7, 1)[0] == R.BAD_LEAST


def test_too_many_is_a_result():
    for max_frames in (1, 2, 255):
        for n in (max_frames - 1, max_frames, max_frames + 1):
            s, walked = R.walk(K.PING * n, 33, 9, 2, max_frames)
            want = R.NO_FRAMES if n == 0 else R.TOO_MANY if n > max_frames else R.OK
            assert (s, len(walked)) == (want, min(n, max_frames))
            assert qfec.wire_scan_frames(K.PING * n, 33, 9, 2, max_frames)[0] == want
    # the walk stops at the type byte of frame max_frames + 1 without judging it
    assert R.walk(K.PING + b"\x1f", 33, 9, 2, 1)[0] == R.TOO_MANY
    assert R.walk(K.PING + b"\x1f", 33, 9, 2, 2)[0] == R.ILLEGAL_TYPE


def test_host_refusals():
    for kw in (dict(quic_version=0), dict(quic_version=34), dict(pn_len=3), dict(max_frames=0),
               dict(max_frames=256)):
        a = dict(quic_version=31, pn_len=2, max_frames=4)
        a.update(kw)
        with pytest.raises(qfec.QfecError):
            qfec.wire_scan_frames(b"\x07", a["quic_version"], 5, a["pn_len"], a["max_frames"])


@pytest.mark.parametrize("seed", range(6))
def test_forms_agree_over_random_turns(seed):
    rng = np.random.default_rng(seed)
    for _ in range(12):
        n, nc = int(rng.integers(1, 90)), int(rng.integers(0, 5))
        pn_len = rng.choice([1, 2, 4, 6, 3], n, p=[.3, .3, .2, .15, .05]).astype(np.uint8)
        pn = rng.integers(1, 14, n).astype(U64)
        bodies = [K.rand_body(rng, int(pn[p]), int(pn_len[p]) if pn_len[p] != 3 else 1)
                  for p in range(n)]
        for b, p in zip(bodies, range(n)):  # the host C++ on the same bodies
            if pn_len[p] != 3:
                s, walked = R.walk(b, 31, int(pn[p]), int(pn_len[p]), 3)
                assert qfec.wire_scan_frames(b, 31, int(pn[p]), int(pn_len[p]), 3)[::2] == (s, walked)
        data, off, lens = K.arena(bodies, rng)
        conn = rng.integers(0, nc + 1, n).astype(np.uint32)
        hdr = rng.choice([0, 1, 4, 0x80, 2, 0x86], n, p=[.5, .2, .1, .1, .05, .05]).astype(np.uint8)
        state = R.new_state(nc)
        state["seen"][:] = rng.integers(0, 8, nc)
        state["least"][:] = rng.integers(0, 8, nc)
        state["hash"][:] = rng.integers(0, 256, nc)
        version, max_frames = int(rng.choice([31, 33])), int(rng.choice([1, 3, 255]))
        args = (data, off, lens, pn, conn, pn_len, hdr if rng.integers(0, 4) else None, version,
                max_frames, int(rng.integers(0, 60)), state, nc)
        same_result(R.scan_packets(*args), R.scan_arrays(*args))


def turn(packets, state, n_conns=2):
    """(pn, conn, body) triples with 2-byte packet numbers -> both forms' result"""
    bodies = [b for _, _, b in packets]
    data, off, lens = K.arena(bodies)
    pn = np.array([p for p, _, _ in packets], U64)
    conn = np.array([c for _, c, _ in packets], np.uint32)
    args = (data, off, lens, pn, conn, np.full(len(packets), 2, np.uint8), None, 31, 255, 64,
            state, n_conns)
    a, b = R.scan_packets(*args), R.scan_arrays(*args)
    same_result(a, b)
    return a


def test_stop_waiting_state_rule():
    sw = lambda pn, least, h: K.stop_waiting(pn, 2, least, h)  # noqa: E731
    state = R.new_state(2)
    state["seen"][:], state["least"][:], state["hash"][:] = [10, 0], [4, 0], [9, 0]
    r = turn([(12, 0, sw(12, 6, 1)),              # newer
              (15, 0, K.PING + sw(15, 7, 2)),     # the newest: wins
              (15, 0, sw(15, 8, 3)),              # a copy of that number, later: loses the tie
              (14, 0, sw(14, 9, 4)),
              (10, 0, sw(10, 10, 5)),             # at sw_seen: stale
              (9, 0, sw(9, 9, 6)),                # below it
              (20, 0, K.PING),                    # no frame
              (30, 0, sw(30, 30, 7) + b"\x1f")],  # the walk fails: takes no part
             state)
    assert (r["seen"][0], r["least"][0], r["hash"][0]) == (15, 7, 2)
    assert (r["seen"][1], r["least"][1], r["hash"][1]) == (0, 0, 0)  # the other keeps its own
    assert r["counts"][11] == 1 and r["counts"][12] == 0 and r["conn"].tolist() == [0, 1]
    assert r["status"].tolist() == [0] * 7 + [R.ILLEGAL_TYPE]
    # two frames in one packet: the last one wins, as the reference lets it overwrite
    r = turn([(5, 1, sw(5, 2, 1) + K.PING + sw(5, 3, 2))], R.new_state(2))
    assert (r["seen"][1], r["least"][1], r["hash"][1]) == (5, 3, 2) and r["counts"][7] == 2
    # ... and a last frame with least_unacked 0 is none (the reference acts on > 0 only)
    r = turn([(5, 1, sw(5, 2, 1) + sw(5, 0, 2))], R.new_state(2))
    assert (r["seen"][1], r["least"][1]) == (0, 0) and r["counts"][11] == 0
    # a winner below the old least_unacked is counted, and applied: policy is the host's
    state = R.new_state(2)
    state["seen"][:], state["least"][:] = [3, 3], [8, 8]
    r = turn([(4, 0, sw(4, 2, 1)), (4, 1, sw(4, 4, 1)), (16, 1, sw(16, 9, 2))], state)
    assert r["least"].tolist() == [2, 9] and r["counts"][11:].tolist() == [2, 1]
    # the order of arrival does not matter except among copies of one number
    rng = np.random.default_rng(3)
    packets = [(int(rng.integers(1, 9)), int(rng.integers(0, 2)), b"") for _ in range(40)]
    packets = [(p, c, sw(p, int(rng.integers(1, p + 1)), p * 16 + c)) for p, c, _ in packets]
    base = turn(packets, R.new_state(2))
    for _ in range(5):
        order = rng.permutation(len(packets))
        again = turn([packets[i] for i in order], R.new_state(2))
        assert np.array_equal(again["seen"], base["seen"])
