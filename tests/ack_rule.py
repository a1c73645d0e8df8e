"""The rule of qfec_record_received and qfec_build_acks (include/qfec.h),
restated for the tests in two independent forms: sequentially in plain Python,
walking packets, revived groups, raises and packet numbers one at a time the
way QuicReceivedPacketManager does (record_received, build_acks), and once more
over whole NumPy arrays (record_received_np, build_acks_np).  test_ack_rule.py
pins the two to each other and to the reference's own recorded acks
(tests/golden/ack_ref.npz); the GPU tests compare the device with them bit for
bit.  Nothing shared with the HIP path.

A state is a dict: cells uint8[n_conns, window], least and largest
uint64[n_conns], hash uint8[n_conns], window.  Only the cells of packet
numbers in [max(least, 1), largest] are state; live_cells masks the rest, and
every comparison of two states goes through it (same_state).
"""
import numpy as np

NO_KEY = 0xFFFFFFFFFFFFFFFF
NOT_ACCEPTED, RANGE, STALE, OVERFLOW, DUPLICATE, RECORDED = range(6)
# counts behind the six classes
N_NEW, N_REVIVED, N_NOT_MISSING, N_RAISED, N_DROPPED, N_JUMPS = range(6, 12)
RECEIVED, ENTROPY, REVIVED = 1, 2, 4
GROUP_REVIVED = 1
U64 = np.uint64


def new_state(n_conns, window):
    return dict(cells=np.zeros((n_conns, window), np.uint8), least=np.zeros(n_conns, U64),
                largest=np.zeros(n_conns, U64), hash=np.zeros(n_conns, np.uint8), window=window)


def copy_state(s):
    return dict(cells=s["cells"].copy(), least=s["least"].copy(), largest=s["largest"].copy(),
                hash=s["hash"].copy(), window=s["window"])


def live_cells(state):
    """cells with every cell outside [max(least, 1), largest] zeroed"""
    w = U64(state["window"])
    lo = np.maximum(state["least"], U64(1))
    big = state["largest"]
    cnt = np.where(big >= lo, np.minimum(big - lo + U64(1), w), U64(0))
    pos = np.arange(int(w), dtype=U64)[None, :]
    rel = (pos - (lo[:, None] & (w - U64(1)))) & (w - U64(1))
    return np.where(rel < cnt[:, None], state["cells"], 0).astype(np.uint8)


def same_state(a, b):
    return (a["window"] == b["window"] and np.array_equal(a["least"], b["least"])
            and np.array_equal(a["largest"], b["largest"]) and np.array_equal(a["hash"], b["hash"])
            and np.array_equal(live_cells(a), live_cells(b)))


def _flag(entropy, p):
    return 0 if entropy is None else int(entropy[p] != 0)


def record_received(state, packet_number=(), pkt_conn=(), hdr=None, entropy=None, status=(),
                    revived_idx=(), slot=None, slot_key=(), key_shift=40, raise_conn=(),
                    raise_least=(), raise_hash=()):
    """One call, sequentially.  Returns dict(state, rcv_out, counts, latched);
    the state passed in is not modified."""
    st = copy_state(state)
    w, n_conns = state["window"], len(state["least"])
    cells = st["cells"]
    counts = [0] * 12
    latched = False
    out = np.empty(len(packet_number), np.uint8)
    for p in range(len(packet_number)):
        pn, c = int(packet_number[p]), int(pkt_conn[p])
        if hdr is not None and hdr[p] >= 0x80:
            cls = NOT_ACCEPTED
        elif c >= n_conns:
            cls, latched = RANGE, True
        else:  # against the state as the call found it
            least, big = int(state["least"][c]), int(state["largest"][c])
            lo = max(least, 1)
            if pn == 0 or pn < least:
                cls = STALE
            elif pn - lo >= w:
                cls = OVERFLOW
            elif pn <= big and state["cells"][c, pn % w] & RECEIVED:
                cls = DUPLICATE
            else:
                cls = RECORDED
        out[p] = cls
        counts[cls] += 1
        if cls != RECORDED:
            continue
        big = int(st["largest"][c])
        if pn > big:  # the ring takes in (big, pn]: nothing of an earlier lap survives
            for q in range(max(big, lo - 1) + 1, pn + 1):
                cells[c, q % w] = 0
            st["largest"][c] = pn
        if not cells[c, pn % w] & RECEIVED:
            counts[N_NEW] += 1
        cells[c, pn % w] |= RECEIVED | _flag(entropy, p) << 1
    n_slots = len(slot_key)
    for g in range(len(status)):
        s = g if slot is None else int(slot[g])
        if status[g] != GROUP_REVIVED or s >= n_slots:
            continue
        key, missing = int(slot_key[s]), False
        c, pn = key >> key_shift, (key & ((1 << key_shift) - 1)) + int(revived_idx[g])
        if key != NO_KEY and c < n_conns:
            lo = max(int(st["least"][c]), 1)
            if lo <= pn < int(st["largest"][c]) and not cells[c, pn % w] & RECEIVED:
                cells[c, pn % w] |= REVIVED
                missing = True
        counts[N_REVIVED if missing else N_NOT_MISSING] += 1
    for i in range(len(raise_conn)):
        c, up, frame_hash = int(raise_conn[i]), int(raise_least[i]), int(raise_hash[i])
        if c >= n_conns:
            latched = True
            continue
        least, big = int(st["least"][c]), int(st["largest"][c])
        if up <= least:
            continue
        counts[N_RAISED] += 1
        if up > big + 1:
            counts[N_JUMPS] += 1
            st["hash"][c] = frame_hash
        else:
            lost, x = False, 0
            for pn in range(max(least, 1), up):
                cell = int(cells[c, pn % w])
                if cell & RECEIVED:
                    x ^= ((cell >> 1) & 1) << (pn % 8)
                else:
                    lost = True
            if lost:
                counts[N_DROPPED] += 1
                st["hash"][c] = frame_hash
            else:
                st["hash"][c] ^= x
        st["least"][c] = up
    return dict(state=st, rcv_out=out, counts=np.array(counts, U64), latched=latched)


def _ranges(start, count):
    """(owner, value) of the ranges start[i] .. start[i] + count[i] - 1, flat"""
    count = np.asarray(count).astype(np.int64)
    owner = np.repeat(np.arange(len(count)), count)
    first = np.repeat(np.cumsum(count) - count, count)
    off = (np.arange(int(count.sum())) - first).astype(U64)
    return owner, np.repeat(np.asarray(start, U64), count) + off, off == 0


def record_received_np(state, packet_number=(), pkt_conn=(), hdr=None, entropy=None, status=(),
                       revived_idx=(), slot=None, slot_key=(), key_shift=40, raise_conn=(),
                       raise_least=(), raise_hash=()):
    """The same over whole arrays."""
    st = copy_state(state)
    w, n_conns = U64(state["window"]), len(state["least"])
    m = w - U64(1)
    flat = st["cells"].reshape(-1)
    counts = np.zeros(12, U64)
    pn = np.asarray(packet_number, U64)
    conn = np.asarray(pkt_conn, np.int64)
    n = len(pn)
    accepted = np.ones(n, bool) if hdr is None else np.asarray(hdr) < 0x80
    known = conn < n_conns
    cc = np.where(known, conn, 0)
    if n_conns:
        least, big = state["least"][cc], state["largest"][cc]
        cell = state["cells"][cc, (pn & m).astype(np.int64)]
    else:
        least = big = np.zeros(n, U64)
        cell = np.zeros(n, np.uint8)
    lo = np.maximum(least, U64(1))
    cls = np.full(n, RECORDED, np.uint8)
    for mask, c in reversed([(~accepted, NOT_ACCEPTED), (~known, RANGE),
                             ((pn == 0) | (pn < least), STALE), (pn - lo >= w, OVERFLOW),
                             ((pn <= big) & ((cell & RECEIVED) != 0), DUPLICATE)]):
        cls[mask] = c
    counts[:6] = np.bincount(cls, minlength=6)
    latched = bool(counts[RANGE])
    rec = cls == RECORDED
    if rec.any():
        seen = np.zeros(n_conns, U64)
        np.maximum.at(seen, conn[rec], pn[rec])
        moved = seen > st["largest"]
        lo_c = np.maximum(st["least"], U64(1))
        frm = np.maximum(st["largest"], lo_c - U64(1)) + U64(1)
        owner, q, _ = _ranges(frm[moved], (seen - frm + U64(1))[moved])
        flat[np.flatnonzero(moved)[owner] * int(w) + (q & m).astype(np.int64)] = 0
        st["largest"][moved] = seen[moved]
        idx = conn[rec] * int(w) + (pn[rec] & m).astype(np.int64)
        counts[N_NEW] = np.unique(idx[(flat[idx] & RECEIVED) == 0]).size
        flag = np.zeros(n, np.uint8) if entropy is None else (np.asarray(entropy) != 0)
        np.bitwise_or.at(flat, idx, (RECEIVED | flag[rec].astype(np.uint8) << 1).astype(np.uint8))
    if len(status):
        ng, n_slots = len(status), len(slot_key)
        s = np.arange(ng) if slot is None else np.asarray(slot, np.int64)
        cand = (np.asarray(status) == GROUP_REVIVED) & (s < n_slots)
        key = np.asarray(slot_key, U64)[np.where(s < n_slots, s, 0)] if n_slots else \
            np.full(ng, NO_KEY, U64)
        c = (key >> U64(key_shift)).astype(np.int64)  # (below 2^63: key_shift >= 1)
        rpn = (key & U64((1 << key_shift) - 1)) + np.asarray(revived_idx, U64)
        ok = cand & (key != U64(NO_KEY)) & (c < n_conns) & (c >= 0)
        cc = np.where(ok, c, 0)
        if n_conns:
            lo = np.maximum(st["least"][cc], U64(1))
            at = cc * int(w) + (rpn & m).astype(np.int64)
            missing = ok & (rpn >= lo) & (rpn < st["largest"][cc]) & ((flat[at] & RECEIVED) == 0)
            np.bitwise_or.at(flat, at[missing], np.uint8(REVIVED))
        else:
            missing = np.zeros(ng, bool)
        counts[N_REVIVED], counts[N_NOT_MISSING] = missing.sum(), (cand & ~missing).sum()
    if len(raise_conn):
        rc = np.asarray(raise_conn, np.int64)
        up, fh = np.asarray(raise_least, U64), np.asarray(raise_hash, np.uint8)
        inr = rc < n_conns
        latched = latched or bool((~inr).any())
        rc, up, fh = rc[inr], up[inr], fh[inr]
        ap = up > st["least"][rc]
        rc, up, fh = rc[ap], up[ap], fh[ap]
        jump = up > st["largest"][rc] + U64(1)
        lo = np.maximum(st["least"][rc], U64(1))
        owner, q, _ = _ranges(lo, np.where(jump, U64(0), up - lo))
        cell = flat[rc[owner] * int(w) + (q & m).astype(np.int64)]
        got = (cell & RECEIVED) != 0
        lost = np.zeros(len(rc), bool)
        np.logical_or.at(lost, owner[~got], True)
        x = np.zeros(len(rc), np.uint8)
        np.bitwise_xor.at(x, owner[got],
                          (((cell[got] >> 1) & 1) << (q[got] & U64(7)).astype(np.uint8)))
        st["hash"][rc] = np.where(jump | lost, fh, st["hash"][rc] ^ x)
        st["least"][rc] = up
        counts[N_RAISED], counts[N_DROPPED], counts[N_JUMPS] = len(rc), lost.sum(), jump.sum()
    return dict(state=st, rcv_out=cls, counts=counts, latched=latched)


def build_acks(state, ack_conn, max_ranges, max_revived):
    """GetUpdatedAckFrame for every ack_conn, one packet number at a time.
    Returns dict(largest, hash, truncated, range_ptr, range_lo, range_hi,
    rev_ptr, rev_pn, latched)."""
    w, n_conns = state["window"], len(state["least"])
    big_o, hash_o, trunc_o = [], [], []
    rptr, rlo, rhi, vptr, vpn = [0], [], [], [0], []
    latched = False
    for c in (int(c) for c in ack_conn):
        big = h = trunc = 0
        ivs, rev = [], []
        if c >= n_conns:
            latched = True
        else:
            lo, big, h = max(int(state["least"][c]), 1), int(state["largest"][c]), \
                int(state["hash"][c])
            cell = lambda pn: int(state["cells"][c, pn % w])
            if big >= lo:
                for pn in range(lo, big):  # the missing packets, as the queue holds them
                    if not cell(pn) & RECEIVED:
                        if ivs and ivs[-1][1] == pn:
                            ivs[-1][1] = pn + 1
                        else:
                            ivs.append([pn, pn + 1])
                if len(ivs) > max_ranges:  # the framer's truncation
                    big, trunc = ivs[max_ranges][0] - 1, 1
                    ivs = ivs[:max_ranges]
                for pn in range(lo, big + 1):
                    if cell(pn) & RECEIVED:
                        h ^= ((cell(pn) >> 1) & 1) << (pn % 8)
                    elif cell(pn) & REVIVED:
                        rev.append(pn)
                rev = rev[len(rev) - min(len(rev), max_revived):]
        big_o.append(big), hash_o.append(h), trunc_o.append(trunc)
        rlo += [a for a, _ in ivs]
        rhi += [b for _, b in ivs]
        vpn += rev
        rptr.append(len(rlo)), vptr.append(len(vpn))
    return dict(largest=np.array(big_o, U64), hash=np.array(hash_o, np.uint8),
                truncated=np.array(trunc_o, np.uint8), range_ptr=np.array(rptr, np.uint32),
                range_lo=np.array(rlo, U64), range_hi=np.array(rhi, U64),
                rev_ptr=np.array(vptr, np.uint32), rev_pn=np.array(vpn, U64), latched=latched)


def build_acks_np(state, ack_conn, max_ranges, max_revived):
    """The same over whole arrays: every live cell of every ack in one table."""
    w, n_conns = U64(state["window"]), len(state["least"])
    conn = np.asarray(ack_conn, np.int64)
    na = len(conn)
    known = conn < n_conns
    cc = np.where(known, conn, 0)
    if n_conns:
        lo = np.maximum(state["least"][cc], U64(1))
        big = np.where(known, state["largest"][cc], U64(0))
        h = np.where(known, state["hash"][cc], 0).astype(np.uint8)
    else:
        lo, big, h = np.ones(na, U64), np.zeros(na, U64), np.zeros(na, np.uint8)
    cnt = np.where(known & (big >= lo), big - lo + U64(1), U64(0))
    owner, pn, first = _ranges(lo, cnt)
    cell = state["cells"].reshape(-1)[cc[owner] * int(w) + (pn & (w - U64(1))).astype(np.int64)] \
        if len(owner) else np.zeros(0, np.uint8)
    miss = (cell & RECEIVED) == 0
    prev = np.r_[False, miss[:-1]] & ~first
    start, end = miss & ~prev, ~miss & prev

    def within(mask):  # how many of mask lie at or below each element, inside its ack
        cs = np.cumsum(mask)
        base = np.zeros(na, np.int64)
        base[owner[first]] = (cs - mask)[first]
        return cs - base[owner]

    iv = within(start) - 1  # the interval a start opens, an end closes
    n_iv = np.bincount(owner[start], minlength=na)
    trunc = n_iv > max_ranges
    cut = start & (iv == max_ranges)
    big = big.copy()
    big[owner[cut]] = pn[cut] - U64(1)
    live = pn <= big[owner]
    got = live & ~miss
    np.bitwise_xor.at(h, owner[got], (((cell[got] >> 1) & 1) << (pn[got] & U64(7)).astype(np.uint8)))
    revd = live & miss & ((cell & REVIVED) != 0)
    n_rev = np.bincount(owner[revd], minlength=na)
    kept = np.minimum(n_rev, max_revived)
    keep = revd & (within(revd) - 1 >= (n_rev - kept)[owner])
    return dict(largest=big, hash=h, truncated=trunc.astype(np.uint8),
                range_ptr=np.r_[0, np.cumsum(np.minimum(n_iv, max_ranges))].astype(np.uint32),
                range_lo=pn[start & (iv < max_ranges)], range_hi=pn[end & (iv < max_ranges)],
                rev_ptr=np.r_[0, np.cumsum(kept)].astype(np.uint32), rev_pn=pn[keep],
                latched=bool((~known).any()))
