"""The rule of qfec_accumulate_ragged (include/qfec.h), restated in NumPy for
the tests: test_accumulate_rule.py pins it to oracle/qfec_np.py, and
test_hip_accumulate_ragged.py compares the GPU with it bit for bit.  One group
at a time, byte loops in NumPy slices: nothing shared with the HIP path.
"""
import numpy as np

MAX_PACKET = 1452
ERR_NONE, ERR_GROUP, ERR_SLOT, ERR_ROWLEN, ERR_PKTLEN = 0, 1, 2, 3, 4


def fold(row, old, packets):
    """One group, one turn.  row: the slot's bytes (modified in place), old its
    length on entry, packets: the byte arrays to fold now.  Returns the new
    length.  Bytes of the row at or beyond old count as zero whatever they
    hold; bytes at or beyond the new length are not written; no packets: a
    no-op."""
    if not packets:
        return old
    new = max(old, max(len(p) for p in packets))
    acc = np.zeros(new, np.uint8)
    acc[:old] = row[:old]
    for p in packets:
        acc[:len(p)] ^= np.asarray(p, np.uint8)
    row[:new] = acc
    return new


def accumulate(data, off, ln, ptr, acc, stride, acc_len, slot=None):
    """The whole call on host arrays: acc (flat uint8) and acc_len (uint16) are
    modified in place.  Returns the per-group error class (ERR_*): a group that
    the device rejects keeps its row and its length."""
    n = len(ptr) - 1
    n_slots = len(acc_len)
    lim = min(MAX_PACKET, stride)
    errs = np.zeros(n, np.int64)
    for g in range(n):
        k = (int(ptr[g + 1]) - int(ptr[g])) & 0xFFFFFFFF
        if k > 255:
            errs[g] = ERR_GROUP
            continue
        s = g if slot is None else int(slot[g])
        if s >= n_slots:
            errs[g] = ERR_SLOT
            continue
        old = int(acc_len[s])
        if old > lim:
            errs[g] = ERR_ROWLEN
            continue
        ps = range(int(ptr[g]), int(ptr[g]) + k)
        if any(int(ln[p]) == 0 or int(ln[p]) > lim for p in ps):
            errs[g] = ERR_PKTLEN
            continue
        row = acc[s * stride:s * stride + lim]
        acc_len[s] = fold(row, old, [data[int(off[p]):int(off[p]) + int(ln[p])] for p in ps])
    return errs
