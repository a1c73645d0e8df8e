"""The rule of qfec_parse_opened and qfec_write_private_headers
(include/qfec.h), restated for the tests: packet by packet in plain Python
(parse_one, parse_opened) and once more over whole NumPy arrays
(parse_opened_np).  test_parse_rule.py pins the two to each other, to the
reference framer's committed verdicts (tests/golden/wire_ref.npz) and to the
host parser; the GPU tests compare the device with them bit for bit.  Nothing
shared with the HIP path.
"""
import numpy as np

NO_KEY = 0xFFFFFFFFFFFFFFFF
FAILED, NO_FLAGS, ILLEGAL_FLAGS, NO_OFFSET, BAD_OFFSET, RANGE, EMPTY = (
    0x80, 0x81, 0x82, 0x83, 0x84, 0x85, 0x86)
ENTROPY_BIT, GROUP_BIT, FEC_BIT = 1, 2, 4
# counts: data packets in a group, FEC packets in a group, accepted outside any
# group, FAILED, headers rejected, RANGE
N_DATA, N_FEC, N_NONE, N_FAILED, N_REJECTED, N_RANGE = range(6)
# the reference framer's detailed error of every rejected class it knows
DETAIL = {
    "Unable to read private flags.": NO_FLAGS,
    "Illegal private flags value.": ILLEGAL_FLAGS,
    "Unable to read first fec protected packet offset.": NO_OFFSET,
    "First fec protected packet offset must be less than the packet number.": BAD_OFFSET,
}


def max_flags(quic_version):
    return 7 if quic_version <= 31 else 1


def parse_one(data, off, length, pn, conn, ok, quic_version, key_shift):
    """One packet: (hdr, key, idx, body_off, body_len, entropy).  data is only
    indexed inside [off, off + length), and not at all when ok is false."""
    off, length, pn, conn = int(off), int(length), int(pn), int(conn)
    refused = lambda cls: (cls, NO_KEY, 0, off, 0, 0)
    if not ok:
        return refused(FAILED)
    if length == 0:
        return refused(NO_FLAGS)
    flags = int(data[off])
    if flags > max_flags(quic_version):
        return refused(ILLEGAL_FLAGS)
    entropy = (flags & ENTROPY_BIT) << (pn % 8)
    if not flags & GROUP_BIT:
        return flags, NO_KEY, 0, off + 1, length - 1, entropy
    if length < 2:
        return refused(NO_OFFSET)
    offset = int(data[off + 1])
    if offset >= pn:
        return refused(BAD_OFFSET)
    if length == 2:
        return refused(EMPTY)
    group = pn - offset
    key = (conn << key_shift | group) & NO_KEY
    if conn >> (64 - key_shift) or group >> key_shift or key == NO_KEY:
        return refused(RANGE)
    return flags, key, offset, off + 2, length - 2, entropy


def count_class(hdr):
    """which of the six counts a packet of class hdr is counted in"""
    if hdr == FAILED:
        return N_FAILED
    if hdr == RANGE:
        return N_RANGE
    if hdr >= 0x80:
        return N_REJECTED
    if not hdr & GROUP_BIT:
        return N_NONE
    return N_FEC if hdr & FEC_BIT else N_DATA


def parse_opened(data, pkt_off, pkt_len, packet_number, pkt_conn, pkt_ok, quic_version,
                 key_shift):
    """The whole call on host arrays, packet by packet.  Returns a dict of the
    output arrays (key, idx, body_off, body_len, hdr, entropy) and counts[6];
    counts[N_RANGE] != 0 is what the device latches."""
    n = len(pkt_off)
    out = dict(key=np.empty(n, np.uint64), idx=np.empty(n, np.uint8),
               body_off=np.empty(n, np.uint64), body_len=np.empty(n, np.uint16),
               hdr=np.empty(n, np.uint8), entropy=np.empty(n, np.uint8))
    counts = [0] * 6
    for p in range(n):
        ok = True if pkt_ok is None else bool(pkt_ok[p])
        h, k, i, bo, bl, e = parse_one(data, pkt_off[p], pkt_len[p], packet_number[p],
                                       pkt_conn[p], ok, quic_version, key_shift)
        out["hdr"][p], out["key"][p], out["idx"][p] = h, k, i
        out["body_off"][p], out["body_len"][p], out["entropy"][p] = bo, bl, e
        counts[count_class(h)] += 1
    out["counts"] = np.array(counts, np.uint64)
    return out


def parse_opened_np(data, pkt_off, pkt_len, packet_number, pkt_conn, pkt_ok, quic_version,
                    key_shift):
    """The same over whole arrays: every class as a mask, first match wins."""
    off = np.asarray(pkt_off, np.uint64)
    ln = np.asarray(pkt_len, np.int64)
    pn = np.asarray(packet_number, np.uint64)
    conn = np.asarray(pkt_conn, np.uint64)
    n = len(off)
    ok = np.ones(n, bool) if pkt_ok is None else np.asarray(pkt_ok) != 0
    data = np.asarray(data, np.uint8)
    has0, has1 = ok & (ln >= 1), ok & (ln >= 2)
    b0, b1 = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    b0[has0] = data[off[has0].astype(np.int64)]
    b1[has1] = data[off[has1].astype(np.int64) + 1]
    grouped = (b0 & np.uint64(GROUP_BIT)) != 0
    group = pn - b1  # (wraps where b1 > pn: BAD_OFFSET comes first)
    shift, rest = np.uint64(key_shift), np.uint64(64 - key_shift)
    key = (conn << shift) | group
    unfit = ((conn >> rest) != 0) | ((group >> shift) != 0) | (key == np.uint64(NO_KEY))
    masks = [(~ok, FAILED), (ln == 0, NO_FLAGS), (b0 > max_flags(quic_version), ILLEGAL_FLAGS),
             (grouped & (ln < 2), NO_OFFSET), (grouped & (b1 >= pn), BAD_OFFSET),
             (grouped & (ln == 2), EMPTY), (grouped & unfit, RANGE)]
    hdr = b0.astype(np.uint8)
    for mask, cls in reversed(masks):
        hdr[mask] = cls
    accepted = hdr < 0x80
    keyed = accepted & grouped
    used = np.where(keyed, 2, np.where(accepted, 1, 0))
    out = dict(hdr=hdr, key=np.where(keyed, key, np.uint64(NO_KEY)).astype(np.uint64),
               idx=np.where(keyed, b1, 0).astype(np.uint8),
               body_off=off + used.astype(np.uint64),
               body_len=np.where(accepted, ln - used, 0).astype(np.uint16),
               entropy=np.where(accepted, (b0 & np.uint64(1)) << (pn % np.uint64(8)),
                                0).astype(np.uint8))
    fec = (b0 & np.uint64(FEC_BIT)) != 0
    rejected = ~accepted & (hdr != FAILED) & (hdr != RANGE)
    out["counts"] = np.array([(keyed & ~fec).sum(), (keyed & fec).sum(), (accepted & ~keyed).sum(),
                              (hdr == FAILED).sum(), rejected.sum(), (hdr == RANGE).sum()],
                             np.uint64)
    return out


def write_refused(hdr, quic_version):
    """WriteFecPrivateHeader's refusals: FEC without a group, illegal flags"""
    hdr = int(hdr)
    return hdr > max_flags(quic_version) or bool(hdr & FEC_BIT and not hdr & GROUP_BIT)


def write_private_headers(data, pkt_off, hdr, fec_offset, quic_version):
    """The sender's call on host arrays; data is modified in place.  Returns
    (body_off, counts[2]); counts[1] != 0 is what the device latches."""
    body_off = np.empty(len(pkt_off), np.uint64)
    counts = [0, 0]
    for p in range(len(pkt_off)):
        off, h = int(pkt_off[p]), int(hdr[p])
        if write_refused(h, quic_version):
            body_off[p] = off
            counts[1] += 1
            continue
        data[off] = h
        if h & GROUP_BIT:
            data[off + 1] = fec_offset[p]
        body_off[p] = off + (2 if h & GROUP_BIT else 1)
        counts[0] += 1
    return body_off, np.array(counts, np.uint64)
