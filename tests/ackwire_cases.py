"""Inputs for the ack-frame tests: the reference fixture
tests/golden/ackwire_ref.npz as batches with their rings rebuilt, and random
ack states put through ack_rule.build_acks."""
import os

import numpy as np

import ack_rule as A
import ackwire_rule as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ackwire_ref.npz")
DELAYS = [0, 4095, 4096, 4097, 1 << 20, (1 << 20) + 1, R.UFLOAT16_MAX - 1, R.UFLOAT16_MAX,
          R.INFINITE]


def fixture():
    return np.load(GOLDEN)


def fixture_case(f, i):
    """case i: (kwargs of write_ack_frame, the reference's frame)"""
    r0, r1 = int(f["range_ptr"][i]), int(f["range_ptr"][i + 1])
    g0, g1 = int(f["flag_ptr"][i]), int(f["flag_ptr"][i + 1])
    b0, b1 = int(f["frame_ptr"][i]), int(f["frame_ptr"][i + 1])
    flagged, base = [int(p) for p in f["flag_pn"][g0:g1]], int(f["base_hash"][i])

    def up_to(pn):
        h = base
        for p in flagged:
            if p <= pn:
                h ^= 1 << p % 8
        return h

    ranges = [(int(a), int(b)) for a, b in zip(f["range_lo"][r0:r1], f["range_hi"][r0:r1])]
    return dict(largest=int(f["largest"][i]), entropy_hash=int(f["hash"][i]), ranges=ranges,
                revived=[], delay_us=int(f["delay"][i]), cap=int(f["cap"][i]),
                entropy_up_to=up_to), bytes(f["frame"][b0:b1])


def fixture_span(f):
    """the live cells a case needs: from its lowest missing number to its largest"""
    first = np.where(np.diff(f["range_ptr"]) > 0,
                     np.append(f["range_lo"], 0)[f["range_ptr"][:-1]], f["largest"])
    return (f["largest"] - first + 1).astype(np.int64)


def fixture_batch(f, pick, window):
    """the cases `pick` (indices; their spans fit `window`) as one batch, one
    connection per case: (batch, cells, out_cap, frames)"""
    pick = np.asarray(pick)
    cells = np.zeros((len(pick), window), np.uint8)
    lo, hi, ptr, frames = [], [], [0], []
    for c, i in enumerate(pick):
        case, frame = fixture_case(f, int(i))
        big = case["largest"]
        first = case["ranges"][0][0] if case["ranges"] else big
        pn = np.arange(first, big + 1)
        cells[c, pn % window] = R.RECEIVED
        for a, b in case["ranges"]:
            cells[c, np.arange(a, b) % window] = 0
        g0, g1 = int(f["flag_ptr"][i]), int(f["flag_ptr"][i + 1])
        for p in f["flag_pn"][g0:g1]:
            if first <= p <= big:
                cells[c, int(p) % window] |= R.ENTROPY
        lo += [a for a, _ in case["ranges"]]
        hi += [b for _, b in case["ranges"]]
        ptr.append(len(lo))
        frames.append(frame)
    n = len(pick)
    batch = dict(ack_conn=np.arange(n, dtype=np.uint32), largest=f["largest"][pick],
                 hash=f["hash"][pick], truncated=np.zeros(n, np.uint8),
                 range_ptr=np.array(ptr, np.uint32), range_lo=np.array(lo, np.uint64),
                 range_hi=np.array(hi, np.uint64), rev_ptr=np.zeros(n + 1, np.uint32),
                 rev_pn=np.zeros(0, np.uint64), delay=f["delay"][pick])
    return batch, cells, f["cap"][pick].astype(np.uint16), frames


def random_state(rng, n_conns, window, loss=0.2, revived=0.3, wrap=True):
    """an ack state with every connection's live range somewhere in the ring
    (across its wrap, where wrap), missing packets of which some are revived"""
    st = A.new_state(n_conns, window)
    for c in range(n_conns):
        span = int(rng.integers(1, window + 1))
        least = int(rng.integers(1, 1 << 20)) if wrap else 1
        if wrap and c % 3 == 0:  # the top of the live range just past a multiple of the window
            least = window * int(rng.integers(1, 1000)) - span // 2
        least = max(least, 1)
        big = least + span - 1
        pn = np.arange(least, big + 1)
        got = rng.random(span) >= (loss if c % 5 else 0.5)
        got[-1] = True  # the largest observed was received
        cell = np.where(got, R.RECEIVED | rng.integers(0, 2, span) << 1,
                        np.where(rng.random(span) < revived, A.REVIVED, 0))
        st["cells"][c, pn % window] = cell
        st["least"][c], st["largest"][c] = least, big
        st["hash"][c] = rng.integers(0, 256)
    return st


def random_batch(rng, state, n_acks, max_ranges=255, max_revived=255, delays=True, bad_conn=False):
    """acks of random connections of `state` (repeats included) as the build leaves them"""
    n_conns = len(state["least"])
    conn = rng.integers(0, n_conns, n_acks).astype(np.uint32)
    if bad_conn:
        conn[rng.integers(0, n_acks, max(1, n_acks // 20))] = n_conns + 2
    batch = A.build_acks(state, conn, max_ranges, max_revived)
    batch["ack_conn"] = conn
    batch["delay"] = rng.choice(np.array(DELAYS, np.uint64), n_acks) if delays else None
    return batch


def frame_sizes(batch, cells, window):
    """every ack's frame length with all the room it could want"""
    n = len(batch["ack_conn"])
    res = R.write_ack_frames_np(batch, cells, window, np.zeros(n * 4096, np.uint8),
                                np.arange(n) * 4096, np.full(n, 4096), 0)
    return res["out_len"].astype(np.int64)


def expected_content(ack, wire):
    """what a frame written from `ack` (write_ack_frame's kwargs) must parse
    to, given the largest observed it carries: the missing numbers below it,
    and the newest revived ones at or below it (as many as were written)"""
    top = wire["largest"]
    ranges = [(a, min(b, top + 1)) for a, b in ack["ranges"] if a <= top]
    return ranges, [p for p in ack["revived"] if p <= top]
