"""The rules of qfec_admit_ragged and qfec_revive_tracked (include/qfec.h),
restated in NumPy for the tests: test_admit_rule.py pins them to
accumulate_rule.py, close_rule.py and oracle/qfec_np.py, and the GPU tests
compare the device with them bit for bit.  One group at a time, the slot's map
as a Python set: nothing shared with the HIP path.
"""
import numpy as np

MAX_PACKET = 1452
ADMITTED, FAILED, DUPLICATE, INVALID = 0, 1, 2, 3
COMPLETE, REVIVED, UNREVIVABLE = 0, 1, 2
# what a group latched, as bits (one group can latch several)
E_INDEX, E_PKTLEN, E_GROUP, E_ROWLEN = 1, 2, 4, 8


def map_bits(mp, k):
    """the set of packets 0..k a map's bytes show"""
    return {i for i in range(k + 1) if (int(mp[i // 8]) >> (i % 8)) & 1}


def admit(off, ln, idx, ok, ptr, slot_k, maps, acc_len, stride, ptr_out, off_out, len_out,
          verdict, slot=None):
    """The whole admit on host arrays.  maps (uint8[n_slots, map_stride]),
    ptr_out, off_out, len_out and verdict are modified in place; ok None: all
    verified.  Returns (per-group latched bits, counts[4])."""
    n = len(ptr) - 1
    n_slots, ms = len(acc_len), maps.shape[1]
    lim = min(MAX_PACKET, stride)
    room = (int(ptr[n]) - int(ptr[0])) & 0xFFFFFFFF
    errs = np.zeros(n, np.int64)
    counts = [0, 0, 0, 0]
    pos = 0
    for g in range(n):
        ptr_out[g] = pos
        p0 = int(ptr[g])
        kg = (int(ptr[g + 1]) - p0) & 0xFFFFFFFF
        if kg > 255:  # (its verdicts are not written)
            errs[g] = E_GROUP
            continue
        s = g if slot is None else int(slot[g])
        bad = 0
        if s >= n_slots:  # (slot_k, acc_len and the map are not read)
            bad = E_INDEX
        else:
            k, old = int(slot_k[s]), int(acc_len[s])
            if k == 0 or k // 8 + 1 > ms:
                bad |= E_GROUP
            if old > lim:
                bad |= E_ROWLEN
        if bad:
            verdict[p0:p0 + kg] = INVALID
            counts[INVALID] += kg
            errs[g] = bad
            continue
        have = set() if old == 0 else map_bits(maps[s], k)  # a fresh slot: all clear
        fresh = False
        for p in range(p0, p0 + kg):
            i, length = int(idx[p]), int(ln[p])
            e = (E_INDEX if i > k else 0) | (E_PKTLEN if length == 0 or length > lim else 0)
            if e:
                v = INVALID
                errs[g] |= e
            elif ok is not None and int(ok[p]) == 0:
                v = FAILED
            elif i in have:
                v = DUPLICATE
            else:
                v = ADMITTED
                have.add(i)
                fresh = True
                if pos < room:
                    off_out[pos], len_out[pos] = off[p], ln[p]
                pos += 1
            verdict[p] = v
            counts[v] += 1
        if fresh:  # base | new, zero above bit k; no byte beyond k // 8 + 1
            bits = np.zeros(8 * (k // 8 + 1), bool)
            bits[sorted(have)] = True
            maps[s, :k // 8 + 1] = np.packbits(bits, bitorder="little")
    ptr_out[n] = pos
    return errs, np.array(counts, np.uint64)


def revive_tracked(acc, stride, acc_len, maps, slot_k, n, out, out_off, out_len, status,
                   revived_idx, slot=None, release_mask=0):
    """The whole tracked revive on host arrays (out None: no copy).  out,
    out_len, status, revived_idx and acc_len are modified in place.  Returns
    (per-group latched bits, revived_list, counts[3])."""
    assert 0 <= release_mask <= 7
    n_slots, ms = len(acc_len), maps.shape[1]
    lim = min(MAX_PACKET, stride)
    errs = np.zeros(n, np.int64)
    rlist, counts = [], [0, 0, 0]
    for g in range(n):
        out_len[g] = 0
        s = g if slot is None else int(slot[g])
        if s >= n_slots:  # (slot_k, the map and the length are not read)
            bad = E_INDEX
        else:
            k = int(slot_k[s])
            bad = E_GROUP if k == 0 or k // 8 + 1 > ms else 0
        if bad:
            errs[g] = bad
            status[g], revived_idx[g] = UNREVIVABLE, 0xFF
            counts[UNREVIVABLE] += 1
            continue
        length = int(acc_len[s])
        have = set() if length == 0 else map_bits(maps[s], k)  # a fresh slot: all clear
        miss = [i for i in range(k) if i not in have]
        if not miss:
            st, m = COMPLETE, 0xFF
        elif len(miss) == 1 and k in have:
            st, m = REVIVED, miss[0]
        else:
            st, m = UNREVIVABLE, 0xFF
        status[g], revived_idx[g] = st, m
        counts[st] += 1
        if st == REVIVED:
            rlist.append(g)
            if length > lim:  # the status states the map; nothing copied, no release
                errs[g] = E_ROWLEN
                continue
            out_len[g] = length
            if out is not None:
                o = int(out_off[g])
                out[o:o + length] = acc[s * stride:s * stride + length]
        if (release_mask >> st) & 1:
            acc_len[s] = 0
    return errs, np.array(rlist, np.uint64), np.array(counts, np.uint64)


def gather(maps, slot_k, acc_len, n, slot=None):
    """What qfec_revive_accumulated is handed to give the tracked revive's
    outputs: group_k[g] = slot_k[slot[g]] and the by-slot maps gathered by
    group, zeroed where the slot is fresh.  (A slot out of range: k 1, no bits;
    it latches on its slot in both calls.)"""
    gk = np.ones(n, np.uint8)
    gm = np.zeros((n, maps.shape[1]), np.uint8)
    for g in range(n):
        s = g if slot is None else int(slot[g])
        if s < len(acc_len):
            gk[g] = slot_k[s]
            if int(acc_len[s]) != 0:
                gm[g] = maps[s]
    return gk, gm
