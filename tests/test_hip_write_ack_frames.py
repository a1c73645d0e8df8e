"""qfec_write_ack_frames on the device against tests/ackwire_rule.py, whole
buffers byte for byte (tests/ackwire_device.py): the guard bytes around every
frame's slot, every output array's trailing entry and every input are part of
the comparison.  The rule itself is pinned to the reference framer on the CPU
(test_ackwire_rule.py); the fixture runs here as well."""
import numpy as np
import pytest

import ack_cases as C
import ack_rule as A
import ackwire_cases as K
import ackwire_device as W
import ackwire_rule as R
from turn_sizes import GRID_PER_CU, TILE, ncu, wave_wrap

gpu = pytest.mark.gpu


@gpu
@pytest.mark.parametrize("window,limit", [(1024, None), (65536, 24)])
def test_reference_fixture_on_the_device(ctx, window, limit):
    """the reference framer's own frames, the state rebuilt into cells"""
    f = K.fixture()
    span = K.fixture_span(f)
    pick = np.flatnonzero((span <= window) & (span > (0 if window == 1024 else 1024)))[:limit]
    batch, cells, cap, frames = K.fixture_batch(f, pick, window)
    off, size = W.slots(cap)
    want = R.write_ack_frames_np(batch, cells, window, np.full(size, W.POISON8), off, cap)
    for a, frame in enumerate(frames):
        assert bytes(want["out"][int(off[a]):int(off[a]) + len(frame)]) == frame
    assert set(want["status"].tolist()) <= {R.WRITTEN, R.CUT}  # (the fixture has no failed frame)
    assert window != 1024 or (want["status"] == R.CUT).sum() > 100
    W.write(ctx, batch, cells, window, off, cap, size, want=want)


def case(seed, n_conns, window, n_acks, max_ranges=255, max_revived=255, loss=0.3, **kw):
    rng = np.random.default_rng(seed)
    state = K.random_state(rng, n_conns, window, loss=loss)
    batch = K.random_batch(rng, state, n_acks, max_ranges, max_revived, **kw)
    return rng, state, batch, K.frame_sizes(batch, state["cells"], window)


@gpu
@pytest.mark.parametrize("n_acks", [1, 4, 5, 257])
def test_ack_counts(ctx, n_acks):
    """one wave, one workgroup, one more, many; repeats in ack_conn"""
    rng, state, batch, full = case(n_acks, 3, 256, n_acks)
    assert n_acks < 4 or len(set(batch["ack_conn"].tolist())) < n_acks
    cap = (full + rng.integers(0, 3, n_acks)).astype(np.uint16)
    off, size = W.slots(cap)
    want = W.write(ctx, batch, state["cells"], 256, off, cap, size, prefix_len=2)
    assert (want["out_len"] == full + 2).all()


@gpu
def test_acks_beyond_one_grid(ctx):
    """one ack more than ack_write_kernel's grid has waves, built from a state
    of more connections than that at max_ranges 3, max_revived 2: the first
    wave's second trip writes the last ack, a cut one, whose hash is walked
    again there; the four tallies hold what both trips counted"""
    n_acks, window = wave_wrap(), 64
    assert n_acks > ncu() * GRID_PER_CU * TILE // 64, "the acks no longer make the grid loop"
    rng = np.random.default_rng(6300)
    state = C.grown_state(rng, n_acks + 39, window)
    n_conns = len(state["least"])
    conn = C.acks_ending_full(rng, state, n_acks, 3, 2, truncated=True)
    conn[rng.integers(0, n_acks - 1, n_acks // 50)] = n_conns + 2
    batch = A.build_acks_np(state, conn, 3, 2)
    batch["ack_conn"] = conn
    batch["delay"] = rng.choice(np.array(K.DELAYS, np.uint64), n_acks)
    full = K.frame_sizes(batch, state["cells"], window)
    cap = np.choose(rng.integers(0, 3, n_acks), [full, full - 1, 3])
    # the last ack lists revived packets, which the writer drops first: the
    # largest room at which it cuts a range as well
    ack = R.ack_of(batch, n_acks - 1)
    for room in range(int(full[-1]) - 1, 0, -1):
        w = R.write_ack_frame(cap=room, entropy_up_to=lambda pn: 0, **ack)
        if w["cut"] and w["frame"]:
            break
    cap[-1] = room
    cap = np.maximum(cap, 0).astype(np.uint16)
    off, size = W.slots(cap)
    want = R.write_ack_frames_np(batch, state["cells"], window, np.full(size, W.POISON8), off, cap)
    assert want["latched"] and (want["counts"] > 0).all(), want["counts"]
    assert set(want["status"].tolist()) == {R.WRITTEN, R.CUT, R.NO_ROOM, R.RANGE}
    assert want["status"][-1] == R.CUT and want["wire_largest"][-1] < batch["largest"][-1]
    W.write(ctx, batch, state["cells"], window, off, cap, size, want=want)


@gpu
def test_no_acks(ctx):
    """n_acks == 0: nothing is looked at, counts receives four zeroes"""
    cnt = W.dview(np.full(5, W.POISON64))
    ctx.write_ack_frames(None, 0, None, None, None, None, None, None, None, None, None, 0, 0, None,
                         None, None, None, None, None, None, counts=cnt)
    ctx.write_ack_frames(None, 0, None, None, None, None, None, None, None, None, None, 0, 0, None,
                         None, None, None, None, None, None)
    W.sync(ctx, False)
    assert W.host(cnt, np.uint64).tolist() == [0, 0, 0, 0, int(W.POISON64)]


@gpu
def test_every_alignment_of_the_frame(ctx):
    """out_off at every residue mod 16, frames of every number length"""
    rng, state, batch, full = case(11, 16, 256, 64)
    cap = full.astype(np.uint16)
    off = (np.arange(64) * 1024 + 64 + np.arange(64) % 16).astype(np.uint64)
    W.write(ctx, batch, state["cells"], 256, off, cap, 64 * 1024 + 64)


@gpu
@pytest.mark.parametrize("window", [64, 256, 4096])
def test_room_at_every_edge(ctx, window):
    """exact fit, one short (cut, or no room for the timestamp byte), half,
    the minimum frame, below it; the cut's entropy walk crosses the ring's wrap"""
    rng, state, batch, full = case(window, 24, window, 240, loss=0.45)
    kind = np.arange(240) % 8
    ll = np.array([R.number_length(int(x)) for x in batch["largest"]])
    cap = np.choose(kind, [full, full - 1, full // 2, 6 + ll, 5 + ll, 4 + ll, full - 2,
                           (6 + ll + full) // 2]).astype(np.uint16)
    off, size = W.slots(cap)
    want = W.write(ctx, batch, state["cells"], window, off, cap, size)
    assert set(want["status"].tolist()) == {R.WRITTEN, R.CUT, R.NO_ROOM}
    # some cut ack's walk (largest written, largest given] wraps around the ring
    cut = np.flatnonzero(want["status"] == R.CUT)
    lo, hi = want["wire_largest"][cut] % window, batch["largest"][cut] % window
    assert (hi < lo).any()
    assert (want["wire_hash"][cut] != batch["hash"][cut]).any()


@gpu
@pytest.mark.parametrize("max_ranges,max_revived", [(1, 0), (3, 2), (40, 255)])
def test_acks_the_build_cut_already(ctx, max_ranges, max_revived):
    """truncated input: written as it is, and cut again where the room is small"""
    rng, state, batch, full = case(max_ranges, 24, 1024, 96, max_ranges, max_revived, loss=0.4)
    assert batch["truncated"].any()
    cap = np.where(np.arange(96) % 2 == 0, full, full // 2 + 4).astype(np.uint16)
    off, size = W.slots(cap)
    want = W.write(ctx, batch, state["cells"], 1024, off, cap, size, rev_pn=max_revived != 0)
    twice = (want["status"] == R.CUT) & (batch["truncated"] != 0)
    assert twice.any() or max_ranges == 1


@gpu
def test_no_delays_no_counts(ctx):
    """ack_delay_us == NULL is an infinite delay for every ack; counts may be NULL"""
    rng, state, batch, full = case(21, 9, 256, 40, delays=False)
    cap = (full + 3).astype(np.uint16)
    off, size = W.slots(cap)
    want = W.write(ctx, batch, state["cells"], 256, off, cap, size, counts=False)
    first = int(off[0])
    ll = R.number_length(int(batch["largest"][0]))
    assert want["out"][first + 2 + ll:first + 4 + ll].tolist() == [0xFF, 0xFF]


@gpu
@pytest.mark.parametrize("prefix_len", [0, 2])
def test_connections_out_of_range(ctx, prefix_len):
    """length 0, QFEC_ACKW_RANGE and the latch; the others are written"""
    rng, state, batch, full = case(31, 9, 256, 60, bad_conn=True)
    cap = full.astype(np.uint16)
    off, size = W.slots(cap)
    want = W.write(ctx, batch, state["cells"], 256, off, cap, size, prefix_len=prefix_len)
    assert want["latched"] and want["counts"][R.RANGE] >= 1
    assert want["counts"][R.WRITTEN] == 60 - want["counts"][R.RANGE]


@gpu
def test_no_connections(ctx):
    """n_conns == 0: every ack is out of range and no ring is needed"""
    batch = A.build_acks(A.new_state(0, 64), np.arange(6, dtype=np.uint32), 255, 255)
    batch["ack_conn"] = np.arange(6, dtype=np.uint32)
    batch["delay"] = None
    cap = np.full(6, 40, np.uint16)
    off, size = W.slots(cap)
    want = W.write(ctx, batch, np.zeros((0, 64), np.uint8), 64, off, cap, size)
    assert want["counts"].tolist() == [0, 0, 0, 6]
