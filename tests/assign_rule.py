"""The rule of qfec_assign_slots (include/qfec.h), restated in plain Python
for the tests: test_assign_rule.py pins it to an independent restatement and,
chained with the other rules, to the turn with host-assigned slots, and the GPU
tests compare the device with it bit for bit.  One packet at a time, a dict and
a list: nothing shared with the HIP path.
"""
import numpy as np

NO_KEY = 0xFFFFFFFFFFFFFFFF
NO_SLOT = 0xFFFFFFFF
# counts: packets of open groups, packets of groups opened in this call,
# packets without a key, groups opened, packets turned away
OPEN, NEW, NONE, OPENED, AWAY = range(5)


def assign_slots(key, k, slot_key, slot_k, acc_len, slot_out):
    """The whole call on host arrays.  slot_key and slot_k (one entry per slot,
    len(acc_len) of them) and slot_out[:len(key)] are modified in place.
    Returns counts[5]."""
    n_slots = len(acc_len)
    counts = [0] * 5
    index = {}
    for s in range(n_slots):
        if acc_len[s] > 0 and int(slot_key[s]) != NO_KEY:
            index.setdefault(int(slot_key[s]), s)  # the lowest slot wins
    free = [s for s in range(n_slots) if acc_len[s] == 0]
    used = 0
    opened = {}  # key -> the slot opened in this call, or None: turned away
    for p in range(len(key)):
        x = int(key[p])
        if x == NO_KEY:
            slot_out[p] = NO_SLOT
            counts[NONE] += 1
        elif x in index:
            slot_out[p] = index[x]
            counts[OPEN] += 1
        else:
            if x not in opened:
                if used < len(free):
                    s = free[used]
                    used += 1
                    slot_key[s], slot_k[s] = key[p], k[p]
                    opened[x] = s
                    counts[OPENED] += 1
                else:
                    opened[x] = None
            if opened[x] is None:
                slot_out[p] = NO_SLOT
                counts[AWAY] += 1
            else:
                slot_out[p] = opened[x]
                counts[NEW] += 1
    return np.array(counts, np.uint64)
