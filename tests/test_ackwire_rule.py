"""The v<=31 ack frame's rule on the CPU: tests/ackwire_rule.py's two forms
against each other, against the reference QuicFramer's own frames
(tests/golden/ackwire_ref.npz, from the unpatched reference) and against the host
C++ (qfec_wire_write_ack_frame / qfec_wire_parse_ack_frame), and every written
frame parsed back into the content that went in.  No device is opened."""
import ctypes
import os
import re

import numpy as np
import pytest

import ackwire_cases as K
import ackwire_rule as R
from libquic_amd import qfec
from oracle import ref_framer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return K.fixture()


def both_forms(batch, cells, window, cap, prefix_len=0, slot=None):
    """the two forms over one batch, compared whole; frames laid out in slots
    of `slot` bytes behind guard bytes"""
    n = len(batch["ack_conn"])
    slot = slot or int(max(cap.max(), 1)) + 8
    off = np.arange(n, dtype=np.uint64) * np.uint64(slot) + np.uint64(3)
    out = np.full(n * slot + 16, 0xA5, np.uint8)
    a = R.write_ack_frames(batch, cells, window, out, off, cap, prefix_len)
    b = R.write_ack_frames_np(batch, cells, window, out, off, cap, prefix_len)
    for k in ("out", "out_len", "wire_largest", "wire_hash", "status", "counts"):
        assert np.array_equal(a[k], b[k]), k
    assert a["latched"] == b["latched"]
    return a, off


def test_fixture_covers_its_classes(golden):
    f = golden
    n_int = np.diff(f["range_ptr"])
    assert len(f["largest"]) > 2000 and int(f["dropped"]) > 0
    for c in (0, 1, 63, 64, 65, 255):
        assert (n_int == c).any(), c
    length = (f["range_hi"] - f["range_lo"]).astype(np.int64)
    for n in (1, 255, 256, 257, 512, 513):
        assert (length == n).any(), n
    for big in (255, 256, 65535, 65536, (1 << 32) - 1, 1 << 32, (1 << 48) - 2):
        assert (f["largest"] == big).any(), big
    for d in (0, 4095, 4096, 4097, R.UFLOAT16_MAX - 1, R.UFLOAT16_MAX + 1, R.INFINITE):
        assert (f["delay"] == d).any(), d
    first = f["frame"][f["frame_ptr"][:-1]]
    assert (first & 0x10).any() and (~first & 0x10).any()  # truncated by the framer, and not
    mm = first & 3  # max_delta at 1, 2, 4 and 6 bytes
    assert all((mm == v).any() for v in range(4))


def test_plain_rule_and_host_equal_the_reference(golden):
    f = golden
    for i in range(len(f["largest"])):
        case, want = K.fixture_case(f, i)
        got = R.write_ack_frame(**case)
        assert got["frame"] == want, i
        host = qfec.wire_write_ack_frame(case["largest"], case["entropy_hash"], case["ranges"], [],
                                         case["delay_us"], case["cap"],
                                         entropy_up_to=case["entropy_up_to"])
        assert host == (want, got["largest"], got["hash"], got["truncated"]), i


@pytest.mark.parametrize("window,limit", [(1024, None), (65536, 24)])
def test_both_forms_equal_the_reference_over_rings(golden, window, limit):
    f = golden
    span = K.fixture_span(f)
    pick = np.flatnonzero((span <= window) & (span > (0 if window == 1024 else 1024)))[:limit]
    assert len(pick) > 8
    batch, cells, cap, frames = K.fixture_batch(f, pick, window)
    res, off = both_forms(batch, cells, window, cap)
    for a, frame in enumerate(frames):
        o = int(off[a])
        assert bytes(res["out"][o:o + len(frame)]) == frame, pick[a]
        assert res["out_len"][a] == len(frame)
        assert (res["out"][o + len(frame):o + int(cap[a]) + 5] == 0xA5).all()


STATES = [(64, 255, 255, 0.3), (256, 255, 255, 0.2), (256, 3, 2, 0.4), (1024, 40, 255, 0.5),
          (4096, 255, 255, 0.45)]


def random_case(seed, window, max_ranges, max_revived, loss):
    rng = np.random.default_rng(seed)
    state = K.random_state(rng, 24, window, loss=loss)
    batch = K.random_batch(rng, state, 60, max_ranges, max_revived, bad_conn=seed % 2 == 1)
    full = K.frame_sizes(batch, state["cells"], window)
    # room: generous, exact, one short, around half, the minimum, below it
    kind = rng.integers(0, 7, len(full))
    cap = np.choose(kind, [full + 50, full, full - 1, full // 2, full // 3 + 7,
                           np.full(len(full), 7), np.full(len(full), 4)])
    return state, batch, np.maximum(cap, 0).astype(np.uint16)


@pytest.mark.parametrize("window,max_ranges,max_revived,loss", STATES)
def test_forms_agree_and_frames_parse_back(window, max_ranges, max_revived, loss):
    seen = set()
    for seed in range(6):
        state, batch, cap = random_case(seed, window, max_ranges, max_revived, loss)
        res, off = both_forms(batch, state["cells"], window, cap, prefix_len=seed % 3)
        for a in range(len(cap)):
            ack = R.ack_of(batch, a)
            o, n = int(off[a]), int(res["out_len"][a])
            status = int(res["status"][a])
            if status in (R.NO_ROOM, R.RANGE):
                assert n == 0 and (res["out"][o:o + int(cap[a]) + 1] == 0xA5).all()
                continue
            n -= seed % 3
            frame = bytes(res["out"][o:o + n])
            assert n <= cap[a] and (res["out"][o + n:o + int(cap[a]) + 5] == 0xA5).all()
            conn = int(batch["ack_conn"][a])
            up_to = lambda pn: ack["entropy_hash"] ^ R.entropy_between(
                state["cells"], window, conn, pn, ack["largest"])
            host = qfec.wire_write_ack_frame(ack["largest"], ack["entropy_hash"], ack["ranges"],
                                             ack["revived"], ack["delay_us"], int(cap[a]),
                                             truncated=ack["truncated"], entropy_up_to=up_to)
            assert host[0] == frame and host[1] == res["wire_largest"][a]
            assert host[2] == res["wire_hash"][a]
            # the content that went in comes back out, by both parsers
            used, p = qfec.wire_parse_ack_frame(frame + b"\x5a")
            q = R.parse_ack_frame(frame + b"\x5a")
            assert used == n == q.pop("consumed") and p == q
            wire = dict(largest=int(res["wire_largest"][a]))
            ranges, revived = K.expected_content(ack, wire)
            assert p["largest"] == wire["largest"] and p["hash"] == res["wire_hash"][a]
            assert p["delay"] == R.ufloat16(ack["delay_us"])
            assert p["truncated"] == (ack["truncated"] or status == R.CUT)
            assert p["ranges"] == ranges
            assert p["revived"] == revived[len(revived) - len(p["revived"]):]
            # the hash is the receiver's up to the largest written
            c = conn
            want = int(state["hash"][c]) ^ R.entropy_between(
                state["cells"], window, c, max(int(state["least"][c]), 1) - 1, wire["largest"])
            assert p["hash"] == want
            seen.add((status, bool(ack["truncated"]), min(len(p["revived"]), 2)))
    assert {s for s, _, _ in seen} == {R.WRITTEN, R.CUT}
    if max_ranges < 255:
        assert any(s == R.CUT and t for s, t, _ in seen)  # cut by the build, then by the writer


def test_revived_tail_at_its_edges():
    """0, 1 and 255 revived numbers, and as many as the room holds, newest first,
    in the bytes qfec_wire_write_revived writes"""
    big = 70000
    ranges = [(big - 600, big - 10)]
    for n_rev, spare in ((0, 10), (1, 10), (255, 2000), (300, 2000), (40, 4 * 7 + 3), (5, 0)):
        revived = list(range(big - 600, big - 600 + 2 * n_rev, 2))
        base = len(R.write_ack_frame(big, 9, ranges, [], 0, 4000)["frame"])
        w = R.write_ack_frame(big, 9, ranges, revived, 0, base + spare)
        listed = min(n_rev, 255, spare // 4)
        assert len(w["frame"]) == base + 4 * listed
        tail = qfec.wire_write_revived(revived[::-1][:listed], 4)
        assert w["frame"][base - 1:] == tail
        host = qfec.wire_write_ack_frame(big, 9, ranges, revived, 0, base + spare)
        assert host[0] == w["frame"]
        used, p = qfec.wire_parse_ack_frame(w["frame"])
        assert used == len(w["frame"]) and p["revived"] == revived[len(revived) - listed:]


def test_ufloat16_forms():
    v = [0, 1, 4095, 4096, 4097, 8191, 8192, (1 << 41) - 1, 1 << 41, R.UFLOAT16_MAX - 1,
         R.UFLOAT16_MAX, R.UFLOAT16_MAX + 1, 1 << 63, R.INFINITE]
    v += [(1 << b) + d for b in range(12, 42) for d in (-1, 0, 1)]
    got = R._ufloat16_np(np.array(v, np.uint64))
    assert [R.ufloat16(x) for x in v] == [int(x) for x in got]


def test_parse_refuses_what_is_cut_short():
    frame = R.write_ack_frame(70000, 3, [(100, 700), (900, 901)], [100, 101], 5000, 4000)["frame"]
    assert qfec.wire_parse_ack_frame(frame)[0] == len(frame)
    for n in range(len(frame)):
        assert qfec.wire_parse_ack_frame(frame[:n])[0] == 0, n
        assert R.parse_ack_frame(frame[:n]) is None, n
    assert qfec.wire_parse_ack_frame(b"\x80" + frame[1:])[0] == 0  # a stream frame's type


@pytest.mark.skipif(not ref_framer.available(), reason="oracle/_ref/libref_framer.so not built")
def test_reference_framer_accepts_the_frames():
    rng = np.random.default_rng(5)
    state = K.random_state(rng, 24, 256, loss=0.3, revived=0.0)
    batch = K.random_batch(rng, state, 48, 20, 0)
    full = K.frame_sizes(batch, state["cells"], 256)
    cap = np.where(np.arange(48) % 3 == 0, full // 2 + 6, full).astype(np.uint16)
    res, off = both_forms(batch, state["cells"], 256, cap)
    n_checked = 0
    for a in range(48):
        n = int(res["out_len"][a])
        if n == 0:
            continue
        frame = bytes(res["out"][int(off[a]):int(off[a]) + n])
        head = ref_framer.public_header(31, 77, 6)
        packet = ref_framer.encrypt(31, 77, head + b"\0" + frame, len(head))
        got = ref_framer.parse(31, packet)
        ranges, _ = K.expected_content(R.ack_of(batch, a), dict(largest=int(res["wire_largest"][a])))
        assert got["accepted"] and got["n_ack"] == 1, got["detailed_error"]
        assert got["ack_largest_observed"] == res["wire_largest"][a]
        assert got["ack_missing_count"] == sum(b - a_ for a_, b in ranges)
        n_checked += 1
    assert n_checked > 30


def test_abi_additive():
    """the new calls are declared and exported; QFEC_ABI_VERSION stays (additive)"""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qfec.h")).read(), flags=re.S)
    decl = re.search(r"\bint\s+qfec_write_ack_frames\s*\(([^)]*)\)\s*;", src)
    assert decl and len(decl.group(1).split(",")) == 25
    assert "#define QFEC_ABI_VERSION 1" in src
    lib = ctypes.CDLL(qfec.LIB_PATH)  # (symbol lookup only: no device is opened)
    for name in ("qfec_write_ack_frames", "qfec_wire_write_ack_frame", "qfec_wire_parse_ack_frame"):
        assert hasattr(lib, name), name
    assert (qfec.QFEC_ACKW_WRITTEN, qfec.QFEC_ACKW_CUT, qfec.QFEC_ACKW_NO_ROOM,
            qfec.QFEC_ACKW_RANGE) == (R.WRITTEN, R.CUT, R.NO_ROOM, R.RANGE)
