"""The rules of qfec_emit_accumulated and qfec_revive_accumulated
(include/qfec.h), restated in NumPy for the tests: test_close_rule.py pins them
to oracle/qfec_np.py, and test_hip_close_accumulated.py compares the GPU with
them bit for bit.  One group at a time: nothing shared with the HIP path.
"""
import numpy as np

MAX_PACKET = 1452
COMPLETE, REVIVED, UNREVIVABLE = 0, 1, 2
ERR_NONE, ERR_SLOT, ERR_GROUP, ERR_ROWLEN = 0, 1, 2, 3


def classify(bits, k):
    """One group's receive map (bytes, bit i of byte i // 8 = packet i, bit k
    the FEC packet, higher bits ignored) -> (status, revived index or 0xFF)."""
    have = [(int(bits[i // 8]) >> (i % 8)) & 1 for i in range(k + 1)]
    miss = [i for i in range(k) if not have[i]]
    if not miss:
        return COMPLETE, 0xFF
    if len(miss) == 1 and have[k]:
        return REVIVED, miss[0]
    return UNREVIVABLE, 0xFF


def emit(acc, stride, acc_len, n, out, out_off, out_len, slot=None, release=False):
    """The whole emit on host arrays: out, out_len and (with release) acc_len
    are modified in place.  Returns the per-group error class: an offending
    group gets out_len 0, nothing copied and no release."""
    n_slots = len(acc_len)
    lim = min(MAX_PACKET, stride)
    errs = np.zeros(n, np.int64)
    for g in range(n):
        out_len[g] = 0
        s = g if slot is None else int(slot[g])
        if s >= n_slots:
            errs[g] = ERR_SLOT
            continue
        ln = int(acc_len[s])
        if ln > lim:
            errs[g] = ERR_ROWLEN
            continue
        out_len[g] = ln
        o = int(out_off[g])
        out[o:o + ln] = acc[s * stride:s * stride + ln]
        if release:
            acc_len[s] = 0
    return errs


def revive(acc, stride, acc_len, group_k, maps, n, out, out_off, out_len, status, revived_idx,
           slot=None, release_mask=0):
    """The whole revive on host arrays (maps: uint8[n, map_stride]; out None:
    no copy).  out, out_len, status, revived_idx and acc_len are modified in
    place.  Returns (per-group error class, revived_list, counts)."""
    assert 0 <= release_mask <= 7
    n_slots = len(acc_len)
    lim = min(MAX_PACKET, stride)
    errs = np.zeros(n, np.int64)
    rlist, counts = [], [0, 0, 0]
    for g in range(n):
        out_len[g] = 0
        s = g if slot is None else int(slot[g])
        k = int(group_k[g])
        bad_slot = s >= n_slots
        bad_k = k == 0 or k // 8 + 1 > maps.shape[1]
        if bad_slot or bad_k:  # (the map is not read)
            errs[g] = ERR_SLOT if bad_slot else ERR_GROUP
            status[g], revived_idx[g] = UNREVIVABLE, 0xFF
            counts[UNREVIVABLE] += 1
            continue
        st, m = classify(maps[g], k)
        status[g], revived_idx[g] = st, m
        counts[st] += 1
        if st == REVIVED:
            rlist.append(g)
            ln = int(acc_len[s])
            if ln == 0 or ln > lim:  # the status states the map; nothing copied, no release
                errs[g] = ERR_ROWLEN
                continue
            out_len[g] = ln
            if out is not None:
                o = int(out_off[g])
                out[o:o + ln] = acc[s * stride:s * stride + ln]
        if (release_mask >> st) & 1:
            acc_len[s] = 0
    return errs, np.array(rlist, np.uint64), np.array(counts, np.uint64)
