"""The rule of qfec_bin_arrivals (include/qfec.h), restated in NumPy for the
tests: test_bin_rule.py pins it to a stable argsort and to admit_rule.py over
host-grouped tables, and the GPU tests compare the device with it bit for bit.
One packet at a time, a Python list per slot: nothing shared with the HIP path.
"""
import numpy as np

NO_SLOT = 0xFFFFFFFF
E_INDEX = 1  # what a packet with a slot out of range latches (admit_rule.E_INDEX)


def bin_arrivals(slot, off, ln, idx, ok, n_slots, ptr_out, off_out, len_out, idx_out, ok_out=None,
                 src_out=None):
    """The whole call on host arrays.  ptr_out (n_slots + 1), off_out, len_out,
    idx_out and, if given, ok_out (with ok) and src_out are modified in place;
    entries from ptr_out[n_slots] on are left alone.  Returns (per-packet
    latched bits, counts[3]: binned, NO_SLOT, out of range)."""
    n = len(slot)
    errs = np.zeros(n, np.int64)
    counts = [0, 0, 0]
    bins = [[] for _ in range(n_slots)]
    for p in range(n):
        s = int(slot[p])
        if s == NO_SLOT:
            counts[1] += 1
        elif s >= n_slots:
            counts[2] += 1
            errs[p] = E_INDEX
        else:
            bins[s].append(p)  # arrival order
            counts[0] += 1
    pos = 0
    for s in range(n_slots):
        ptr_out[s] = pos
        for p in bins[s]:
            off_out[pos], len_out[pos], idx_out[pos] = off[p], ln[p], idx[p]
            if ok is not None:
                ok_out[pos] = ok[p]
            if src_out is not None:
                src_out[pos] = p
            pos += 1
    ptr_out[n_slots] = pos
    return errs, np.array(counts, np.uint64)
