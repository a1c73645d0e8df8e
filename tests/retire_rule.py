"""The rule of qfec_retire_groups (include/qfec.h), restated in plain Python
for the tests: test_retire_rule.py pins it to an independent whole-array
restatement and to a packet-by-packet restatement of the reference's group map,
and the GPU tests compare the device with it bit for bit.  One slot and one
packet at a time, dicts and sorted lists: nothing shared with the HIP path.
"""
import numpy as np

NO_KEY = 0xFFFFFFFFFFFFFFFF
# counts: slots closed, packets refused (below their mark), packets without a
# key, packets passed, keys and raises with a connection out of range
CLOSED, REFUSED, NONE, PASSED, BAD = range(5)


def split(key, key_shift):
    """(connection, number) of a key"""
    key = int(key)
    return key >> key_shift, key & ((1 << key_shift) - 1)


def retire_groups(pkt_key, slot_key, acc_len, conn_mark, key_shift, max_groups, raise_conn,
                  raise_mark, pkt_key_out, closed_list=None):
    """The whole call on host arrays.  acc_len, conn_mark (one entry per
    connection), pkt_key_out[:len(pkt_key)] and closed_list[:slots closed] are
    modified in place; pkt_key_out may be pkt_key.  Returns counts[5]; counts[BAD]
    != 0 is what the device latches."""
    n_slots, n_conns = len(acc_len), len(conn_mark)
    counts = [0] * 5
    # 1 raise
    for c, m in zip(raise_conn, raise_mark):
        if int(c) >= n_conns:
            counts[BAD] += 1
        elif int(m) > int(conn_mark[c]):
            conn_mark[c] = m
    # the open keyed slots and the keyed packets, by connection
    open_slots = []  # (s, connection, number), ascending s
    for s in range(n_slots):
        if acc_len[s] > 0 and int(slot_key[s]) != NO_KEY:
            c, x = split(slot_key[s], key_shift)
            if c >= n_conns:
                counts[BAD] += 1
            else:
                open_slots.append((s, c, x))
    packets = []  # per packet: None (no key), False (out of range) or (connection, number)
    for p in range(len(pkt_key)):
        if int(pkt_key[p]) == NO_KEY:
            packets.append(None)
        else:
            c, x = split(pkt_key[p], key_shift)
            packets.append((c, x) if c < n_conns else False)
    # 2 retain
    if max_groups > 0:
        live = {}
        for c, x in [(c, x) for _, c, x in open_slots] + [q for q in packets if q]:
            if x >= int(conn_mark[c]):
                live.setdefault(c, set()).add(x)
        for c, numbers in live.items():
            if len(numbers) > max_groups:
                conn_mark[c] = sorted(numbers)[-max_groups]
    # 3 close
    for s, c, x in open_slots:
        if x < int(conn_mark[c]):
            acc_len[s] = 0
            if closed_list is not None:
                closed_list[counts[CLOSED]] = s
            counts[CLOSED] += 1
    # 4 filter
    for p, q in enumerate(packets):
        if q is None:
            pkt_key_out[p] = NO_KEY
            counts[NONE] += 1
        elif q is False:
            pkt_key_out[p] = NO_KEY
            counts[BAD] += 1
        elif q[1] < int(conn_mark[q[0]]):
            pkt_key_out[p] = NO_KEY
            counts[REFUSED] += 1
        else:
            pkt_key_out[p] = pkt_key[p]
            counts[PASSED] += 1
    return np.array(counts, np.uint64)
