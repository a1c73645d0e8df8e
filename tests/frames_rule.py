"""The rule of qfec_scan_frames (include/qfec.h), stated twice: packet by
packet (walk, scan_packets: QuicFramer::ProcessFrameData as a loop over one
reader, and the STOP_WAITING bookkeeping as a loop over the arrivals) and over
whole arrays (walk_arrays, scan_arrays: every packet steps to its next frame at
once, the state by sorting).  tests/test_frames_rule.py pins both to the
reference framer's recorded verdicts and to each other; the GPU tests compare
the device's buffers with scan_arrays."""
import numpy as np

(OK, SKIPPED, NO_FRAMES, ILLEGAL_TYPE, STREAM, ACK, RST, CLOSE, GOAWAY, WINDOW_UPDATE, BLOCKED,
 STOP_WAITING, PATH_CLOSE, BAD_LEAST, TOO_MANY, PN_LEN, RANGE) = range(17)
F_STREAM, F_ACK, F_STOP_WAITING = 0x80, 0x40, 6
LENGTHS = (1, 2, 4, 6)
N_COUNTS = 13
U64 = np.uint64
# the table's columns, in the order of the call
COLUMNS = [("pkt", np.uint32), ("type", np.uint8), ("flags", np.uint8), ("off", np.uint64),
           ("len", np.uint16), ("id", np.uint32), ("val", np.uint64), ("code", np.uint32)]


# ---- packet by packet ------------------------------------------------------
class _Reader:
    """QuicDataReader: little-endian, CanRead before every read"""

    def __init__(self, b):
        self.b, self.o = b, 0

    def can(self, n):
        return len(self.b) - self.o >= n

    def get(self, n):
        v = int.from_bytes(self.b[self.o:self.o + n], "little")
        self.o += n
        return v


def walk(body, version, pn, pn_len, max_frames=255):
    """(verdict, the frames read before it was reached); a frame is (type,
    flags, off, len, id, val, code), off counted from the body's first byte"""
    r = _Reader(bytes(body))
    if not r.b:
        return NO_FRAMES, []
    out = []
    while r.o < len(r.b):
        if len(out) == max_frames:
            return TOO_MANY, out
        at, t = r.o, r.get(1)
        typ, flags, off, ln, fid, val, code = t, 0, 0, 0, 0, 0, 0
        if t & 0x80:  # 1 fin len ooo ss
            id_len, off_len = (t & 3) + 1, (t >> 2) & 7
            off_len += 1 if off_len else 0
            has_len = (t >> 5) & 1
            if not r.can(id_len + off_len + 2 * has_len):
                return STREAM, out
            fid, val = r.get(id_len), r.get(off_len)
            ln = r.get(2) if has_len else len(r.b) - r.o
            if not r.can(ln):
                return STREAM, out
            typ, flags, off = F_STREAM, (t >> 6) & 1 | has_len << 1, r.o
            r.o += ln
        elif t & 0x40:  # 0 1 nacks truncated ll mm, stepped over
            mm, ll = LENGTHS[t & 3], LENGTHS[(t >> 2) & 3]
            if not r.can(3 + ll):
                return ACK, out
            code, val = r.get(1), r.get(ll)
            r.o += 2
            if not t & 0x10:  # the timestamp block
                if not r.can(1):
                    return ACK, out
                k = r.get(1)
                need = 5 + 3 * (k - 1) if k else 0
                if not r.can(need):
                    return ACK, out
                r.o += need
            if t & 0x20:
                for unit in [mm + 1] + ([ll] if version <= 31 else []):
                    if not r.can(1):
                        return ACK, out
                    need = r.get(1) * unit
                    if not r.can(need):
                        return ACK, out
                    r.o += need
            typ, flags, off, ln = F_ACK, t & 0x3F, at, r.o - at
        elif t & 0x20:
            return ILLEGAL_TYPE, out
        elif t == 0:  # padding: the rest
            off, ln = r.o, len(r.b) - r.o
            r.o = len(r.b)
        elif t == 1:
            if not r.can(16):
                return RST, out
            fid, val, code = r.get(4), r.get(8), r.get(4)
        elif t in (2, 3):
            bad = CLOSE if t == 2 else GOAWAY
            if not r.can(6 if t == 2 else 10):
                return bad, out
            code = r.get(4)
            if t == 3:
                fid = r.get(4)
            ln = r.get(2)
            if not r.can(ln):
                return bad, out
            off = r.o
            r.o += ln
        elif t == 4:
            if not r.can(12):
                return WINDOW_UPDATE, out
            fid, val = r.get(4), r.get(8)
        elif t == 5:
            if not r.can(4):
                return BLOCKED, out
            fid = r.get(4)
        elif t == 6:
            if not r.can(1 + pn_len):
                return STOP_WAITING, out
            code, delta = r.get(1), r.get(pn_len)
            if delta > pn:
                return BAD_LEAST, out
            val = pn - delta
        elif t == 7:
            pass
        elif t == 8:
            if not r.can(1):
                return PATH_CLOSE, out
            fid = r.get(1)
        else:
            return ILLEGAL_TYPE, out
        out.append((typ, flags, off, ln, fid, val, code))
    return OK, out


def gate(hdr, pn_len, conn, n_conns):
    """the verdict in front of the walk, or None"""
    if hdr >= 0x80 or hdr & 4:
        return SKIPPED
    if pn_len not in LENGTHS:
        return PN_LEN
    if conn >= n_conns:
        return RANGE
    return None


def scan_packets(data, body_off, body_len, pn, conn, pn_len, hdr, version, max_frames, frm_cap,
                 state, n_conns):
    """The call, one packet after the other.  state: dict(seen, least, hash), not
    modified.  Returns what scan_arrays returns."""
    n = len(body_off)
    status, ptr, rows = np.zeros(n, np.uint8), np.zeros(n + 1, np.uint32), []
    seen, least, hsh = (np.array(state[k]).copy() for k in ("seen", "least", "hash"))
    old_least = least.copy()
    counts = np.zeros(N_COUNTS, U64)
    best = {}  # connection -> (packet number, least, hash) of the winner so far
    for p in range(n):
        h = 0 if hdr is None else int(hdr[p])
        s = gate(h, int(pn_len[p]), int(conn[p]), n_conns)
        frames = []
        if s is None:
            a = int(body_off[p])
            s, frames = walk(data[a:a + int(body_len[p])], version, int(pn[p]), int(pn_len[p]),
                             max_frames)
        status[p] = s
        counts[0 if s == OK else 1 if s == SKIPPED else 3 if s == TOO_MANY
               else 4 if s in (PN_LEN, RANGE) else 2] += U64(1)
        if s != OK:
            frames = []
        ptr[p + 1] = ptr[p] + len(frames)
        last = None
        for f in frames:
            kind = 5 if f[0] == F_STREAM else 6 if f[0] == F_ACK else 7 if f[0] == 6 else 8
            counts[kind] += U64(1)
            placed = f[0] in (F_STREAM, F_ACK, 0, 2, 3)
            rows.append((p, f[0], f[1], int(body_off[p]) + f[2] if placed else 0) + f[3:])
            if f[0] == F_STOP_WAITING:
                last = f
        if last is not None and last[5] > 0:
            c, number = int(conn[p]), int(pn[p])
            # newer than the connection's, and than every earlier packet of the call
            if number > int(seen[c]) and (c not in best or number > best[c][0]):
                best[c] = (number, last[5], last[6])
    for c, (number, l, h) in best.items():
        seen[c], least[c], hsh[c] = number, l, h
        counts[11] += U64(1)
        counts[12] += U64(l < int(old_least[c]))
    counts[9] = U64(len(rows))
    counts[10] = U64(max(0, len(rows) - frm_cap))
    table = {name: np.array([r[i] for r in rows[:frm_cap]], dt)
             for i, (name, dt) in enumerate(COLUMNS)}
    return dict(status=status, ptr=ptr, table=table, seen=seen, least=least, hash=hsh,
                conn=np.arange(n_conns, dtype=np.uint32), counts=counts,
                latched=bool(counts[4]))


# ---- whole arrays ------------------------------------------------------------
def walk_arrays(data, body_off, body_len, pn, pn_len, run, version, max_frames):
    """Every packet of `run` steps to its next frame at once.  Returns (verdict
    per packet: OK for the ones not run, frames: a list over the rank k of
    dict(mask, type, flags, off, len, id, val, code) arrays over the packets)."""
    data = np.asarray(data, np.uint8)
    n = len(body_off)
    off0, ln = np.asarray(body_off).astype(np.int64), np.asarray(body_len).astype(np.int64)
    pn, pn_len = np.asarray(pn, U64), np.asarray(pn_len).astype(np.int64)
    padded = np.append(data, np.uint8(0)).astype(U64)

    def byte(i):  # body[i] where it lies inside, else 0
        inside = (i >= 0) & (i < ln)
        return np.where(inside, padded[np.where(inside, off0 + i, len(data))], U64(0))

    def get(i, k):  # k[p] <= 8 bytes at body[i], little-endian
        v = np.zeros(n, U64)
        for b in range(8):
            v |= np.where(b < k, byte(i + b), U64(0)) << U64(8 * b)
        return v

    lengths = np.array(LENGTHS, np.int64)
    status = np.where(run & (ln == 0), NO_FRAMES, OK).astype(np.int64)
    o = np.zeros(n, np.int64)
    live = run & (ln > 0)
    frames = []
    for k in range(max_frames + 1):
        live = live & (o < ln)
        if not live.any():
            break
        if k == max_frames:
            status[live] = TOO_MANY
            break
        t = byte(o).astype(np.int64)
        at, o1 = o, o + 1
        room = ln - o1
        is_stream, is_ack = (t & 0x80) != 0, ((t & 0x80) == 0) & ((t & 0x40) != 0)
        plain = ~is_stream & ~is_ack
        # stream
        id_len, ob = (t & 3) + 1, (t >> 2) & 7
        off_len = np.where(ob != 0, ob + 1, 0)
        has_len = (t & 0x20) != 0
        s_head = id_len + off_len + 2 * has_len
        s_given = get(o1 + id_len + off_len, np.where(has_len, 2, 0)).astype(np.int64)
        s_len = np.where(has_len, s_given, room - s_head)
        s_bad = (room < s_head) | (s_len > room - s_head)
        # ack: the count bytes sit where the blocks in front of them end
        mm, ll = lengths[t & 3], lengths[(t >> 2) & 3]
        q = o1 + 3 + ll
        a_bad = room < 3 + ll
        stamped = (t & 0x10) == 0
        a_bad |= stamped & (q >= ln)
        cnt = byte(q).astype(np.int64)
        q = q + np.where(stamped, 1 + np.where(cnt != 0, 5 + 3 * (cnt - 1), 0), 0)
        a_bad |= q > ln
        nacks = (t & 0x20) != 0
        a_bad |= nacks & (q >= ln)
        q = q + np.where(nacks, 1 + byte(q).astype(np.int64) * (mm + 1), 0)
        a_bad |= q > ln
        tail = nacks & (version <= 31)
        a_bad |= tail & (q >= ln)
        q = q + np.where(tail, 1 + byte(q).astype(np.int64) * ll, 0)
        a_bad |= q > ln
        # the plain types: the fixed bytes behind the type byte
        fixed = np.select([t == 1, t == 2, t == 3, t == 4, t == 5, t == 6, t == 8],
                          [16, 6, 10, 12, 4, 1 + pn_len, 1], 0)
        text = np.where((t == 2) | (t == 3), get(o1 + fixed - 2, np.full(n, 2)).astype(np.int64), 0)
        illegal = plain & (t > 8)
        short = plain & ~illegal & (t != 0) & ((room < fixed) | (text > room - fixed))
        delta = get(o1 + 1, pn_len)
        wrapped = plain & (t == 6) & ~short & (delta > pn)
        cls = np.select([t == 1, t == 2, t == 3, t == 4, t == 5, t == 6, t == 8],
                        [RST, CLOSE, GOAWAY, WINDOW_UPDATE, BLOCKED, STOP_WAITING, PATH_CLOSE], 0)
        bad = np.select([is_stream & s_bad, is_ack & a_bad, illegal, short, wrapped],
                        [STREAM, ACK, ILLEGAL_TYPE, cls, BAD_LEAST], 0)
        failing = live & (bad != 0)
        status[failing] = bad[failing]
        live = live & ~failing
        four = np.full(n, 4)
        f = dict(mask=live.copy())
        f["type"] = np.where(is_stream, F_STREAM, np.where(is_ack, F_ACK, t))
        f["flags"] = np.select([is_stream, is_ack], [(t >> 6) & 1 | 2 * has_len, t & 0x3F], 0)
        f["off"] = np.select([is_stream, is_ack, t == 0, (t == 2) | (t == 3)],
                             [o1 + s_head, at, o1, o1 + fixed], -1)
        f["len"] = np.select([is_stream, is_ack, t == 0, (t == 2) | (t == 3)],
                             [s_len, q - at, room, text], 0)
        f["id"] = np.select([is_stream, plain & np.isin(t, (1, 4, 5)), plain & (t == 3),
                             plain & (t == 8)],
                            [get(o1, id_len), get(o1, four), get(o1 + 4, four),
                             byte(o1)], U64(0))
        f["val"] = np.select([is_stream, is_ack, plain & ((t == 1) | (t == 4)), plain & (t == 6)],
                             [get(o1 + id_len, off_len), get(o1 + 1, ll),
                              get(o1 + 4, np.full(n, 8)), pn - delta], U64(0))
        f["code"] = np.select([is_ack | (plain & (t == 6)), plain & (t == 1),
                               plain & ((t == 2) | (t == 3))],
                              [byte(o1), get(o1 + 12, four), get(o1, four)], U64(0))
        frames.append(f)
        o = np.select([is_stream, is_ack, t == 0], [o1 + s_head + s_len, q, ln], o1 + fixed + text)
    return status, frames


def scan_arrays(data, body_off, body_len, pn, conn, pn_len, hdr, version, max_frames, frm_cap,
                state, n_conns):
    """The call over whole arrays: dict(status, ptr, table: the columns cut at
    frm_cap, seen, least, hash, conn, counts, latched)."""
    n = len(body_off)
    body_off, pn, conn = np.asarray(body_off, U64), np.asarray(pn, U64), np.asarray(conn)
    pn_len = np.asarray(pn_len)
    h = np.zeros(n, np.int64) if hdr is None else np.asarray(hdr).astype(np.int64)
    skipped = (h >= 0x80) | ((h & 4) != 0)
    bad_len = ~skipped & ~np.isin(pn_len, LENGTHS)
    unknown = ~skipped & ~bad_len & (conn >= n_conns)
    run = ~skipped & ~bad_len & ~unknown
    walked, frames = walk_arrays(data, body_off, body_len, pn, np.where(run, pn_len, 1), run,
                                 version, max_frames)
    status = np.select([skipped, bad_len, unknown], [SKIPPED, PN_LEN, RANGE], walked)
    ok = status == OK
    counts = np.zeros(N_COUNTS, U64)
    counts[0], counts[1] = ok.sum(), skipped.sum()
    counts[2] = ((status >= NO_FRAMES) & (status <= BAD_LEAST)).sum()
    counts[3], counts[4] = (status == TOO_MANY).sum(), (bad_len | unknown).sum()
    listed = [f["mask"] & ok for f in frames]
    n_frm = np.sum(listed, axis=0, dtype=np.int64) if frames else np.zeros(n, np.int64)
    ptr = np.concatenate(([0], np.cumsum(n_frm))).astype(np.uint32)
    total = int(ptr[-1])
    cols = {name: np.zeros(total, dt) for name, dt in COLUMNS}
    has_sw, sw_least, sw_hash = np.zeros(n, bool), np.zeros(n, U64), np.zeros(n, U64)
    for k, (f, m) in enumerate(zip(frames, listed)):
        e = ptr[:-1][m].astype(np.int64) + k
        cols["pkt"][e] = np.nonzero(m)[0]
        placed = f["off"][m] >= 0
        cols["off"][e] = np.where(placed, body_off[m] + f["off"][m].astype(U64), U64(0))
        for name in ("type", "flags", "len", "id", "val", "code"):
            cols[name][e] = f[name][m]
        sw = m & (f["type"] == F_STOP_WAITING)
        has_sw[sw], sw_least[sw], sw_hash[sw] = True, f["val"][sw], f["code"][sw]
    kinds = cols["type"]
    counts[5], counts[6] = (kinds == F_STREAM).sum(), (kinds == F_ACK).sum()
    counts[7] = (kinds == F_STOP_WAITING).sum()
    counts[8] = total - int(counts[5] + counts[6] + counts[7])
    counts[9], counts[10] = total, max(0, total - frm_cap)
    # the newest STOP_WAITING per connection: the largest packet number, then the earliest
    seen, least, hsh = (np.array(state[k]).copy() for k in ("seen", "least", "hash"))
    cc = np.where(run, conn, 0).astype(np.int64)
    cand = has_sw & (sw_least > 0)
    if n_conns:
        cand &= pn > seen[cc]
    idx = np.nonzero(cand)[0]
    if idx.size:
        order = idx[np.lexsort((idx, ~pn[idx], cc[idx]))]  # (~: descending, exactly)
        first = np.concatenate(([True], cc[order][1:] != cc[order][:-1]))
        win = order[first]
        c = cc[win]
        counts[11] = win.size
        counts[12] = (sw_least[win] < least[c]).sum()
        seen[c], least[c], hsh[c] = pn[win], sw_least[win], sw_hash[win].astype(hsh.dtype)
    return dict(status=status.astype(np.uint8), ptr=ptr,
                table={name: v[:frm_cap] for name, v in cols.items()}, seen=seen, least=least,
                hash=hsh, conn=np.arange(n_conns, dtype=np.uint32), counts=counts,
                latched=bool(counts[4]))


def new_state(n_conns):
    return dict(seen=np.zeros(n_conns, U64), least=np.zeros(n_conns, U64),
                hash=np.zeros(n_conns, np.uint8))
