"""The rule of qfec_wire_write_ack_frame and qfec_write_ack_frames
(include/qfec.h), restated for the tests in two independent forms: one ack at a
time in plain Python, the way QuicFramer::AppendAckFrameAndTypeByte walks its
nack ranges (write_ack_frame, and write_ack_frames over a batch), and once more
over whole NumPy arrays with every nack range of every ack expanded at once
(write_ack_frames_np).  parse_ack_frame is ProcessAckFrame.
test_ackwire_rule.py pins the forms to each other, to the reference framer's own
bytes (tests/golden/ackwire_ref.npz) and to the host C++; the GPU tests compare
the device with them byte for byte.  Nothing shared with the HIP path.

A batch is a dict of the arrays qfec_build_acks leaves: ack_conn, largest, hash,
truncated, range_ptr, range_lo, range_hi, rev_ptr, rev_pn, and delay (uint64,
INFINITE for an infinite delay, or None).  Packet numbers stay below 2^63."""
import numpy as np

INFINITE = (1 << 64) - 1
UFLOAT16_MAX = 0x3FFC0000000
WRITTEN, CUT, NO_ROOM, RANGE = range(4)
RECEIVED, ENTROPY = 1, 2
I64 = np.int64


def number_length(n):
    return 1 if n < 1 << 8 else 2 if n < 1 << 16 else 4 if n < 1 << 32 else 6


def ufloat16(v):
    if v < 1 << 12:
        return v
    if v >= UFLOAT16_MAX:
        return 0xFFFF
    exponent = v.bit_length() - 12  # the hidden bit goes to position 11
    return (v >> exponent) + (exponent << 11)


def _le(n, length):
    return (n & ((1 << (8 * length)) - 1)).to_bytes(length, "little")


def write_ack_frame(largest, entropy_hash, ranges, revived, delay_us, cap, truncated=False,
                    entropy_up_to=None):
    """One frame.  ranges: ascending half-open (lo, hi); revived ascending;
    delay_us None or INFINITE: infinite; entropy_up_to(pn) is asked when the
    writer cuts.  Returns dict(frame, largest, hash, truncated, cut); the
    frame is b"" where the reference writer fails."""
    runs, max_delta, last_missing = [], 0, 0
    for lo, hi in ranges:  # GetAckFrameInfo
        for start in range(lo, hi, 256):
            runs.append((start, min(256, hi - start)))
        if last_missing:
            max_delta = max(max_delta, lo - last_missing)
        last_missing = hi - 1
    if ranges:
        max_delta = max(max_delta, largest - last_missing)
    ll, mm = number_length(largest), number_length(max_delta)
    room = cap - 1 - (4 + ll) - 1
    max_num = 255 if room < 0 else min(255, room // (mm + 1))  # (unsigned in the framer: it wraps)
    cut = len(runs) > max_num
    wire_largest, wire_hash = largest, entropy_hash
    if cut:
        wire_largest = runs[max_num][0] - 1
        wire_hash = entropy_up_to(wire_largest)
        runs = runs[:max_num]
    trunc = cut or truncated
    out = bytes([0x40 | bool(ranges) << 5 | trunc << 4 | (ll >> 1) << 2 | mm >> 1, wire_hash])
    out += _le(wire_largest, ll)
    out += _le(ufloat16(INFINITE if delay_us is None else delay_us), 2)
    if not trunc:
        out += b"\0"  # no receipt times
    if ranges:
        out += bytes([len(runs)])
        last = wire_largest
        for start, length in reversed(runs):
            out += _le(last - (start + length - 1), mm) + bytes([length - 1])
            last = start - 1
        if len(out) + 1 <= cap:
            listed = [p for p in reversed(revived) if p <= wire_largest]
            listed = listed[:min(255, (cap - len(out) - 1) // ll)]
            out += bytes([len(listed)]) + b"".join(_le(p, ll) for p in listed)
        else:
            out += b"\0"  # (fails below)
    fits = len(out) <= cap
    return dict(frame=out if fits else b"", largest=wire_largest if fits else largest,
                hash=wire_hash if fits else entropy_hash, truncated=trunc, cut=cut)


def parse_ack_frame(data):
    """ProcessAckFrame: dict(consumed, largest, hash, delay (the ufloat16),
    truncated, ranges (maximal, ascending), revived (ascending)), or None."""
    lengths = (1, 2, 4, 6)
    try:
        t = data[0]
        if t & 0xC0 != 0x40:
            return None
        mm, ll = lengths[t & 3], lengths[t >> 2 & 3]
        trunc, nacks = bool(t & 0x10), bool(t & 0x20)
        o = 1
        h = data[o]
        largest = int.from_bytes(data[o + 1:o + 1 + ll], "little")
        o += 1 + ll
        delay = int.from_bytes(data[o:o + 2], "little")
        o += 2
        if o > len(data):
            return None
        if not trunc:
            n_times = data[o]
            o += 1 + (5 + (n_times - 1) * 3 if n_times else 0)
        ranges, revived = [], []
        if nacks:
            n = data[o]
            o += 1
            last = largest
            for _ in range(n):
                delta = int.from_bytes(data[o:o + mm], "little")
                length = data[o + mm]
                o += mm + 1
                last -= delta
                lo, hi = last - length, last + 1
                if lo < 1:
                    return None
                if ranges and ranges[-1][0] == hi:
                    ranges[-1] = (lo, ranges[-1][1])
                else:
                    ranges.append((lo, hi))
                last -= length + 1
            n = data[o]
            o += 1
            for _ in range(n):
                revived.append(int.from_bytes(data[o:o + ll], "little"))
                o += ll
        if o > len(data):
            return None
    except IndexError:
        return None
    return dict(consumed=o, largest=largest, hash=h, delay=delay, truncated=trunc,
                ranges=ranges[::-1], revived=revived[::-1])


def entropy_between(cells, window, conn, lo, hi):
    """XOR of the hashes of the received numbers in (lo, hi] of conn's ring"""
    x = 0
    for pn in range(lo + 1, hi + 1):
        cell = int(cells[conn, pn % window])
        if cell & RECEIVED:
            x ^= (cell >> 1 & 1) << (pn % 8)
    return x


def ack_of(batch, a):
    """ack a of a batch as write_ack_frame's arguments (all but cap)"""
    r0, r1 = int(batch["range_ptr"][a]), int(batch["range_ptr"][a + 1])
    v0, v1 = int(batch["rev_ptr"][a]), int(batch["rev_ptr"][a + 1])
    delay = None if batch.get("delay") is None else int(batch["delay"][a])
    return dict(largest=int(batch["largest"][a]), entropy_hash=int(batch["hash"][a]),
                ranges=[(int(batch["range_lo"][i]), int(batch["range_hi"][i]))
                        for i in range(r0, r1)],
                revived=[int(batch["rev_pn"][i]) for i in range(v0, v1)], delay_us=delay,
                truncated=bool(batch["truncated"][a]))


def write_ack_frames(batch, cells, window, out, out_off, out_cap, prefix_len=0):
    """qfec_write_ack_frames, an ack at a time.  cells: uint8[n_conns, window];
    out: the buffer as it was (not modified).  Returns dict(out, out_len,
    wire_largest, wire_hash, status, counts, latched)."""
    n, n_conns = len(batch["ack_conn"]), cells.shape[0]
    buf = np.array(out, np.uint8)
    res = dict(out=buf, out_len=np.zeros(n, np.uint16), wire_largest=np.zeros(n, np.uint64),
               wire_hash=np.zeros(n, np.uint8), status=np.zeros(n, np.uint8),
               counts=np.zeros(4, np.uint64), latched=False)
    for a in range(n):
        conn, ack = int(batch["ack_conn"][a]), ack_of(batch, a)
        w = dict(frame=b"", largest=ack["largest"], hash=ack["entropy_hash"], cut=False)
        if conn >= n_conns:
            status, res["latched"] = RANGE, True
        else:
            w = write_ack_frame(cap=int(out_cap[a]), entropy_up_to=lambda pn: ack["entropy_hash"] ^
                                entropy_between(cells, window, conn, pn, ack["largest"]), **ack)
            status = NO_ROOM if not w["frame"] else CUT if w["cut"] else WRITTEN
        off = int(out_off[a])
        buf[off:off + len(w["frame"])] = np.frombuffer(w["frame"], np.uint8)
        res["out_len"][a] = prefix_len + len(w["frame"]) if w["frame"] else 0
        res["wire_largest"][a], res["wire_hash"][a] = w["largest"], w["hash"]
        res["status"][a] = status
        res["counts"][status] += 1
    return res


def _length_np(v):
    return np.where(v < 1 << 8, 1, np.where(v < 1 << 16, 2, np.where(v < 1 << 32, 4, 6))).astype(I64)


def _ufloat16_np(delay):
    d = np.asarray(delay, np.uint64)
    big = d >= np.uint64(UFLOAT16_MAX)
    v = np.where(big, np.uint64(0), d).astype(I64)
    small = v < 1 << 12
    exponent = np.zeros(len(v), I64)
    for offset in (16, 8, 4, 2, 1):  # WriteUFloat16's binary search
        shift = v >= I64(1) << (11 + offset)
        exponent += np.where(shift, offset, 0)
        v = np.where(shift, v >> offset, v)
    return np.where(big, 0xFFFF, np.where(small, v, v + (exponent << 11))).astype(I64)


def _put(buf, pos, value, length, upto=6):
    """the low length[i] bytes of value[i] at buf[pos[i]:], little-endian"""
    for b in range(upto):
        m = length > b
        buf[pos[m] + b] = (value[m] >> (8 * b) & 0xFF).astype(np.uint8)


def write_ack_frames_np(batch, cells, window, out, out_off, out_cap, prefix_len=0):
    """The same over whole arrays: every nack range of every ack at once."""
    conn = np.asarray(batch["ack_conn"], I64)
    n, n_conns = len(conn), cells.shape[0]
    given, given_hash = np.asarray(batch["largest"]).astype(I64), np.asarray(batch["hash"], I64)
    rptr, vptr = np.asarray(batch["range_ptr"], I64), np.asarray(batch["rev_ptr"], I64)
    lo = np.asarray(batch["range_lo"]).astype(I64)[:rptr[-1]]
    hi = np.asarray(batch["range_hi"]).astype(I64)[:rptr[-1]]
    off, cap = np.asarray(out_off).astype(I64), np.asarray(out_cap, I64)
    n_int = np.diff(rptr)
    ack_i = np.repeat(np.arange(n), n_int)  # the ack of an interval
    first_i = np.arange(len(lo)) == rptr[ack_i]
    last_i = np.arange(len(lo)) == rptr[ack_i + 1] - 1
    # GetAckFrameInfo: the ranges of an interval, and the largest gap
    runs_i = (hi - lo + 255) >> 8
    above = np.where(last_i, given[ack_i] + 1, np.append(lo[1:], 0))  # what follows the interval
    gap = np.where(first_i, 0, lo - np.append(0, hi[:-1]) + 1)
    max_delta = np.zeros(n, I64)
    np.maximum.at(max_delta, ack_i, np.maximum(gap, np.where(last_i, above - hi, 0)))
    n_runs = np.zeros(n, I64)
    np.add.at(n_runs, ack_i, runs_i)
    ll, mm = _length_np(given), _length_np(max_delta)
    room = cap - 6 - ll
    max_num = np.where(room < 0, 255, np.minimum(255, room // (mm + 1)))
    cut = n_runs > max_num
    trunc = cut | (np.asarray(batch["truncated"]) != 0)
    kept = np.minimum(n_runs, max_num)
    first_range = 4 + ll + np.where(trunc, 0, 1) + 1
    rev_at = first_range + kept * (mm + 1)
    mandatory = np.where(n_runs != 0, rev_at + 1, first_range - 1)
    known = conn < n_conns
    fits = known & (mandatory <= cap)
    # every range: its ack, its number from below, its start and length
    ack_r = np.repeat(ack_i, runs_i)
    run_ptr = np.append(0, np.cumsum(n_runs))
    k = np.arange(len(ack_r)) - run_ptr[ack_r]
    j = np.arange(len(ack_r)) - np.repeat(np.cumsum(runs_i) - runs_i, runs_i)
    start = np.repeat(lo, runs_i) + 256 * j
    length = np.minimum(256, np.repeat(hi, runs_i) - start)
    delta = np.where(j + 1 == np.repeat(runs_i, runs_i), np.repeat(above - hi, runs_i), 0)
    largest = given.copy()
    dropped = cut[ack_r] & (k == kept[ack_r]) & fits[ack_r]
    largest[ack_r[dropped]] = start[dropped] - 1
    buf = np.array(out, np.uint8)
    w = fits[ack_r] & (k < kept[ack_r])
    pos = (off + first_range)[ack_r] + (kept[ack_r] - 1 - k) * (mm[ack_r] + 1)
    _put(buf, pos[w], delta[w], mm[ack_r][w])
    buf[(pos + mm[ack_r])[w]] = (length[w] - 1).astype(np.uint8)
    # a cut ack's hash: the received numbers above the largest written leave it
    redo = np.flatnonzero(cut & fits)
    span = (given - largest)[redo]
    ack_c = np.repeat(redo, span)
    pn = largest[ack_c] + 1 + np.arange(len(ack_c)) - np.repeat(np.cumsum(span) - span, span)
    cell = cells[conn[ack_c], pn % window].astype(I64) if len(ack_c) else np.zeros(0, I64)
    wire_hash = given_hash.copy()
    np.bitwise_xor.at(wire_hash, ack_c, np.where(cell & RECEIVED, (cell >> 1 & 1) << (pn & 7), 0))
    # the revived tail
    n_rev = np.diff(vptr)
    ack_v = np.repeat(np.arange(n), n_rev)
    rev = np.asarray(batch["rev_pn"]).astype(I64)[:vptr[-1]]
    idx_v = np.arange(len(rev)) - vptr[ack_v]
    below = np.zeros(n, I64)
    np.add.at(below, ack_v, rev <= largest[ack_v])
    n_out = np.minimum(below, np.minimum(255, np.maximum(cap - mandatory, 0) // ll))
    n_out = np.where(fits & (n_runs != 0), n_out, 0)
    t = below[ack_v] - 1 - idx_v  # newest first
    wv = (t >= 0) & (t < n_out[ack_v])
    _put(buf, ((off + rev_at + 1)[ack_v] + t * ll[ack_v])[wv], rev[wv], ll[ack_v][wv])
    # the head
    f, fr = fits, fits & (n_runs != 0)
    buf[off[f]] = (0x40 | (n_runs != 0) << 5 | trunc << 4 | (ll >> 1) << 2 | mm >> 1)[f]
    buf[off[f] + 1] = wire_hash[f]
    _put(buf, off[f] + 2, largest[f], ll[f])
    delay = batch.get("delay")
    uf = _ufloat16_np(np.full(n, INFINITE, np.uint64) if delay is None else delay)
    _put(buf, (off + 2 + ll)[f], uf[f], np.full(int(f.sum()), 2), 2)
    buf[(off + 4 + ll)[f & ~trunc]] = 0
    buf[(off + first_range - 1)[fr]] = kept[fr]
    buf[(off + rev_at)[fr]] = n_out[fr]
    total = np.where(n_runs != 0, mandatory + n_out * ll, mandatory)
    status = np.where(~known, RANGE, np.where(~fits, NO_ROOM, np.where(cut, CUT, WRITTEN)))
    return dict(out=buf, out_len=np.where(fits, prefix_len + total, 0).astype(np.uint16),
                wire_largest=np.where(fits, largest, given).astype(np.uint64),
                wire_hash=np.where(fits, wire_hash, given_hash).astype(np.uint8),
                status=status.astype(np.uint8),
                counts=np.bincount(status, minlength=4).astype(np.uint64),
                latched=bool((~known).any()))
