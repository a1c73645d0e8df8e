"""The accumulate rule (tests/accumulate_rule.py) against oracle/qfec_np.py, on
the CPU: folding a group's packets turn by turn gives the group's parity on a
sender and the revived packet on a receiver, whatever the order and however the
turns are cut.  These pin the yardstick the GPU tests compare with; the export
test at the end is the one that needs the library to have the call.
"""
import ctypes
import os

import numpy as np
import pytest

import accumulate_rule as R
from oracle import qfec_np as NP


def random_group(rng):
    k = int(rng.integers(1, 41))
    kind = int(rng.integers(0, 4))
    if kind == 0:
        lens = rng.integers(1, 1453, k)
    elif kind == 1:
        lens = rng.integers(1, 40, k)
    elif kind == 2:
        lens = rng.choice([1, 15, 16, 17, 1350, 1451, 1452], k)
    else:
        lens = rng.integers(64, 1351, k)
    return [rng.integers(0, 256, int(x), dtype=np.uint8) for x in lens]


def random_turns(rng, items):
    """items in a random order, cut into a random number of turns, some empty."""
    order = rng.permutation(len(items))
    nt = int(rng.integers(1, len(items) + 3))
    cuts = np.sort(rng.integers(0, len(items) + 1, nt - 1))
    turns = np.split(order, cuts)
    return [[items[i] for i in t] for t in turns]


@pytest.mark.parametrize("seed", range(6))
def test_send_side_gives_the_parity(seed):
    rng = np.random.default_rng(1000 + seed)
    for _ in range(50):
        pays = random_group(rng)
        parity = NP.group_encode(pays)
        row = rng.integers(0, 256, 1536, dtype=np.uint8)  # never cleared
        before = row.copy()
        ln = 0
        for turn in random_turns(rng, pays):
            ln = R.fold(row, ln, turn)
        assert ln == parity.size
        assert np.array_equal(row[:ln], parity)
        assert np.array_equal(row[ln:], before[ln:])


@pytest.mark.parametrize("seed", range(6))
def test_receive_side_gives_the_revived_packet(seed):
    rng = np.random.default_rng(2000 + seed)
    for _ in range(50):
        pays = random_group(rng)
        parity = NP.group_encode(pays)
        m = int(rng.integers(0, len(pays)))
        want = NP.group_recover(pays, parity, m)
        items = [p for i, p in enumerate(pays) if i != m] + [parity]
        row = rng.integers(0, 256, 1536, dtype=np.uint8)
        before = row.copy()
        ln = 0
        for turn in random_turns(rng, items):
            ln = R.fold(row, ln, turn)
        assert ln == parity.size
        assert np.array_equal(row[:ln], want)
        # and that is the lost packet, zero padded
        assert np.array_equal(want[:pays[m].size], pays[m]) and not want[pays[m].size:].any()
        assert np.array_equal(row[ln:], before[ln:])


def test_batch_form_matches_the_group_form():
    """accumulate() -- CSR tables, slots, error classes -- is fold() per group."""
    rng = np.random.default_rng(3000)
    groups = [random_group(rng) for _ in range(12)]
    groups.insert(4, [])  # a group with nothing to fold this turn
    ks = [len(g) for g in groups]
    ptr = np.zeros(len(groups) + 1, np.uint32)
    ptr[1:] = np.cumsum(ks)
    flat = [p for g in groups for p in g]
    ln = np.array([p.size for p in flat], np.uint16)
    off = np.zeros(ln.size, np.uint64)
    off[1:] = np.cumsum(ln[:-1].astype(np.uint64))
    data = np.concatenate(flat)
    n_slots, stride = 20, 1500
    slot = rng.permutation(n_slots)[:len(groups)].astype(np.uint32)
    acc = rng.integers(0, 256, n_slots * stride, dtype=np.uint8)
    acc_len = np.zeros(n_slots, np.uint16)
    before = acc.copy()
    errs = R.accumulate(data, off, ln, ptr, acc, stride, acc_len, slot)
    assert not errs.any()
    named = np.zeros(n_slots, bool)
    for g, pays in enumerate(groups):
        s = int(slot[g])
        named[s] = True
        row = acc[s * stride:(s + 1) * stride]
        if not pays:
            assert acc_len[s] == 0 and np.array_equal(row, before[s * stride:(s + 1) * stride])
            continue
        par = NP.group_encode(pays)
        assert acc_len[s] == par.size and np.array_equal(row[:par.size], par)
        assert np.array_equal(row[par.size:], before[s * stride + par.size:(s + 1) * stride])
    for s in np.flatnonzero(~named):
        assert acc_len[s] == 0
        assert np.array_equal(acc[s * stride:(s + 1) * stride],
                              before[s * stride:(s + 1) * stride])


def test_library_exports_the_call():
    from libquic_amd import qfec
    names = [s[0] for s in qfec.SIGNATURES]
    assert "qfec_accumulate_ragged" in names
    sig = dict((s[0], s) for s in qfec.SIGNATURES)["qfec_accumulate_ragged"]
    assert sig[1] is ctypes.c_int and len(sig[2]) == 12
    assert os.path.exists(qfec.LIB_PATH), "libqfec.so has not been built"
    # (symbol lookup only: nothing is called, no device is opened)
    lib = ctypes.CDLL(qfec.LIB_PATH)
    assert hasattr(lib, "qfec_accumulate_ragged")
    assert hasattr(qfec.Context, "accumulate_ragged")
