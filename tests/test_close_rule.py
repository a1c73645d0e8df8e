"""The close rules (tests/close_rule.py) against oracle/qfec_np.py, on the CPU:
rows folded by accumulate_rule.fold and closed by the emit rule are the ragged
encode's parity and lengths; rows folded from k - 1 data packets and the parity
and closed by the revive rule are the ragged recover's output.  Then the status
table, release_mask and each error class.  These pin the yardstick the GPU
tests compare with; the export test at the end needs the library to have the
calls.
"""
import ctypes
import os

import numpy as np
import pytest

import accumulate_rule as A
import close_rule as R
from oracle import qfec_np as NP
from libquic_amd import qfec

STRIDE = 1536


def arena(seed, n):
    """random arena groups (k 5-15, 64-1350 B) as a packed CSR batch"""
    return NP.ragged_batch(seed, 0, n, 5, 15, 64, 1350, parity_stride=STRIDE)


def packets(data, off, ln, ptr, g):
    return [data[int(off[p]):int(off[p]) + int(ln[p])] for p in range(int(ptr[g]), int(ptr[g + 1]))]


@pytest.mark.parametrize("seed", range(3))
def test_sender_emit_is_the_ragged_encode(seed):
    rng = np.random.default_rng(100 + seed)
    n, n_slots = 40, 50
    data, off, ln, ptr, poff = arena(7 + seed, n)
    want_par, want_len = NP.encode_ragged(data, off, ln, ptr, poff, n * STRIDE)
    slot = rng.permutation(n_slots)[:n].astype(np.uint32)
    acc = rng.integers(0, 256, n_slots * STRIDE, dtype=np.uint8)  # never cleared
    acc_len = np.zeros(n_slots, np.uint16)
    for g in range(n):
        s = int(slot[g])
        acc_len[s] = A.fold(acc[s * STRIDE:(s + 1) * STRIDE], 0, packets(data, off, ln, ptr, g))
    before = acc.copy()
    out = np.zeros(n * STRIDE, np.uint8)
    out_len = np.full(n, 0xA5A5, np.uint16)
    errs = R.emit(acc, STRIDE, acc_len, n, out, poff, out_len, slot, release=True)
    assert not errs.any()
    assert np.array_equal(out_len, want_len)
    assert np.array_equal(out, want_par)
    assert np.array_equal(acc, before) and not acc_len.any()


@pytest.mark.parametrize("seed", range(3))
def test_receiver_revive_is_the_ragged_recover(seed):
    rng = np.random.default_rng(200 + seed)
    n = 40
    data, off, ln, ptr, poff = arena(17 + seed, n)
    par, plen = NP.encode_ragged(data, off, ln, ptr, poff, n * STRIDE)
    ks = np.diff(ptr.astype(np.int64))
    lost = np.array([int(rng.integers(0, k)) for k in ks], np.uint8)
    want = NP.recover_ragged(data, off, ln, ptr, par, poff, plen, lost, poff, n * STRIDE)
    acc = rng.integers(0, 256, n * STRIDE, dtype=np.uint8)
    acc_len = np.zeros(n, np.uint16)
    rcv = np.ones(ln.size, bool)
    for g in range(n):
        pk = packets(data, off, ln, ptr, g)
        items = [p for i, p in enumerate(pk) if i != lost[g]]
        items.append(par[int(poff[g]):int(poff[g]) + int(plen[g])])
        row, cur = acc[g * STRIDE:(g + 1) * STRIDE], 0
        for i in rng.permutation(len(items)):  # one packet per turn, shuffled
            cur = A.fold(row, cur, [items[i]])
        acc_len[g] = cur
        rcv[int(ptr[g]) + int(lost[g])] = False
    maps = qfec.pack_received_ragged(rcv, np.ones(n, bool), ptr)
    out = np.zeros(n * STRIDE, np.uint8)
    out_len = np.full(n, 0xA5A5, np.uint16)
    status, ridx = np.full(n, 9, np.uint8), np.full(n, 9, np.uint8)
    before = acc.copy()
    errs, rlist, counts = R.revive(acc, STRIDE, acc_len, ks.astype(np.uint8), maps, n, out, poff,
                                   out_len, status, ridx, release_mask=0b011)
    assert not errs.any()
    assert np.all(status == R.REVIVED) and np.array_equal(ridx, lost)
    assert np.array_equal(rlist, np.arange(n, dtype=np.uint64))
    assert counts.tolist() == [0, n, 0]
    assert np.array_equal(out_len, plen)
    assert np.array_equal(out, want)
    assert np.array_equal(acc, before) and not acc_len.any()


def test_status_table():
    # (data bits of a k = 10 group that are clear, FEC bit) -> status, index
    table = [((), 1, R.COMPLETE, 0xFF), ((), 0, R.COMPLETE, 0xFF),
             ((3,), 1, R.REVIVED, 3), ((0,), 1, R.REVIVED, 0), ((9,), 1, R.REVIVED, 9),
             ((3,), 0, R.UNREVIVABLE, 0xFF), ((3, 4), 1, R.UNREVIVABLE, 0xFF),
             (tuple(range(10)), 1, R.UNREVIVABLE, 0xFF), (tuple(range(10)), 0, R.UNREVIVABLE, 0xFF)]
    for clear, fec, st, m in table:
        bits = np.ones(16, bool)  # (junk above bit k stays set)
        bits[list(clear)] = False
        bits[10] = bool(fec)
        mp = np.packbits(bits, bitorder="little")
        assert R.classify(mp, 10) == (st, m), (clear, fec)
        # the same rule as the packer and the k = 10 map of the fixed-shape revive
        d = np.ones((1, 10), bool)
        d[0, list(clear)] = False
        assert R.classify(qfec.pack_received(d, [bool(fec)])[0], 10) == (st, m)
    assert R.classify(np.array([0xFE], np.uint8), 1) == (R.REVIVED, 0)
    assert R.classify(np.array([0xFF] * 31 + [0x7F], np.uint8), 255) == (R.COMPLETE, 0xFF)
    assert R.classify(np.array([0xFF] * 31 + [0x3F], np.uint8), 255) == (R.UNREVIVABLE, 0xFF)
    assert R.classify(np.array([0xFF] * 31 + [0xBF], np.uint8), 255) == (R.REVIVED, 254)


def small_batch(rng):
    """groups 0 / 1 / 2 / 3: complete, revived (lost 1), lacking the FEC packet, two lost"""
    n, k = 4, 6
    acc = rng.integers(0, 256, n * STRIDE, dtype=np.uint8)
    acc_len = np.array([100, 200, 300, 400], np.uint16)
    d = np.ones((n, k), bool)
    d[1, 1] = d[2, 4] = d[3, 0] = d[3, 5] = False
    maps = qfec.pack_received(d, [True, True, False, True])
    return n, np.full(n, k, np.uint8), acc, acc_len, maps


@pytest.mark.parametrize("mask", range(8))
def test_release_mask(mask):
    n, gk, acc, acc_len, maps = small_batch(np.random.default_rng(300))
    out = np.full(n * STRIDE, 0x5A, np.uint8)
    off = np.arange(n, dtype=np.uint64) * np.uint64(STRIDE)
    out_len = np.full(n, 0xA5A5, np.uint16)
    status, ridx = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    lens = acc_len.copy()
    errs, rlist, counts = R.revive(acc, STRIDE, acc_len, gk, maps, n, out, off, out_len, status,
                                   ridx, release_mask=mask)
    assert not errs.any()
    assert status.tolist() == [0, 1, 2, 2] and ridx.tolist() == [0xFF, 1, 0xFF, 0xFF]
    assert rlist.tolist() == [1] and counts.tolist() == [1, 1, 2]
    assert out_len.tolist() == [0, 200, 0, 0]
    assert np.array_equal(out[STRIDE:STRIDE + 200], acc[STRIDE:STRIDE + 200])
    out[STRIDE:STRIDE + 200] = 0x5A
    assert np.all(out == 0x5A)
    for g in range(n):
        assert acc_len[g] == (0 if (mask >> int(status[g])) & 1 else lens[g])
    # out None: the same decisions, nothing copied
    acc_len[:] = lens
    out_len[:] = 0xA5A5
    R.revive(acc, STRIDE, acc_len, gk, maps, n, None, None, out_len, status, ridx,
             release_mask=mask)
    assert out_len.tolist() == [0, 200, 0, 0]


def test_emit_release_and_empty_rows():
    rng = np.random.default_rng(400)
    acc = rng.integers(0, 256, 3 * 64, dtype=np.uint8)
    for release in (False, True):
        acc_len = np.array([0, 64, 5], np.uint16)
        out = np.full(300, 0x5A, np.uint8)
        out_len = np.full(3, 0xA5A5, np.uint16)
        errs = R.emit(acc, 64, acc_len, 3, out, np.array([0, 100, 200], np.uint64), out_len,
                      release=release)
        assert not errs.any() and out_len.tolist() == [0, 64, 5]
        assert np.array_equal(out[100:164], acc[64:128]) and np.array_equal(out[200:205],
                                                                            acc[128:133])
        assert np.all(out[:100] == 0x5A) and np.all(out[164:200] == 0x5A)
        assert np.all(out[205:] == 0x5A)
        assert acc_len.tolist() == ([0, 0, 0] if release else [0, 64, 5])


@pytest.mark.parametrize("case,err", [("slot", R.ERR_SLOT), ("k0", R.ERR_GROUP),
                                      ("k_over_map", R.ERR_GROUP), ("len_over_lim", R.ERR_ROWLEN),
                                      ("revived_len0", R.ERR_ROWLEN)])
def test_revive_error_classes(case, err):
    n, gk, acc, acc_len, maps = small_batch(np.random.default_rng(500))
    slot = np.arange(n, dtype=np.uint32)
    bad = 1
    if case == "slot":
        slot[bad] = n
    elif case == "k0":
        gk[bad] = 0
    elif case == "k_over_map":
        gk[bad] = 8  # 8 // 8 + 1 = 2 bytes, the maps have 1
    elif case == "len_over_lim":
        acc_len[bad] = 1453
    else:
        acc_len[bad] = 0
    assert maps.shape[1] == 1
    lens = acc_len.copy()
    out = np.full(n * STRIDE, 0x5A, np.uint8)
    out_len = np.full(n, 0xA5A5, np.uint16)
    status, ridx = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    errs, rlist, counts = R.revive(acc, STRIDE, acc_len, gk, maps, n, out,
                                   np.arange(n, dtype=np.uint64) * np.uint64(STRIDE), out_len,
                                   status, ridx, slot, release_mask=0b111)
    assert errs[bad] == err and np.count_nonzero(errs) == 1
    assert out_len[bad] == 0 and np.all(out == 0x5A)  # nothing copied
    assert acc_len[bad] == lens[bad]  # no release
    if err == R.ERR_ROWLEN:  # the status states the map
        assert status[bad] == R.REVIVED and rlist.tolist() == [1] and counts.tolist() == [1, 1, 2]
    else:
        assert status[bad] == R.UNREVIVABLE and ridx[bad] == 0xFF
        assert rlist.size == 0 and counts.tolist() == [1, 0, 3]
    others = [g for g in range(n) if g != bad]
    assert not acc_len[others].any() and status[others].tolist() == [0, 2, 2]


@pytest.mark.parametrize("case,err", [("slot", R.ERR_SLOT), ("len_over_lim", R.ERR_ROWLEN),
                                      ("len_over_stride", R.ERR_ROWLEN)])
def test_emit_error_classes(case, err):
    rng = np.random.default_rng(600)
    stride = 1350 if case == "len_over_stride" else STRIDE
    acc = rng.integers(0, 256, 3 * stride, dtype=np.uint8)
    acc_len = np.array([10, 20, 30], np.uint16)
    slot = np.array([2, 0, 1], np.uint32)
    if case == "slot":
        slot[1] = 3
    else:
        acc_len[0] = 1453 if case == "len_over_lim" else 1351
    lens = acc_len.copy()
    out = np.full(3 * stride, 0x5A, np.uint8)
    out_len = np.full(3, 0xA5A5, np.uint16)
    errs = R.emit(acc, stride, acc_len, 3, out, np.arange(3, dtype=np.uint64) * np.uint64(stride),
                  out_len, slot, release=True)
    assert errs.tolist() == [0, err, 0]
    assert out_len.tolist() == [30, 0, 20] and np.all(out[stride:2 * stride] == 0x5A)
    if case != "slot":
        assert acc_len[0] == lens[0]
    assert acc_len[2] == 0 and acc_len[1] == 0


def test_library_exports_the_calls():
    sig = dict((s[0], s) for s in qfec.SIGNATURES)
    for name, nargs in (("qfec_emit_accumulated", 12), ("qfec_revive_accumulated", 19)):
        assert name in sig
        assert sig[name][1] is ctypes.c_int and len(sig[name][2]) == nargs
    assert os.path.exists(qfec.LIB_PATH), "libqfec.so has not been built"
    # (symbol lookup only: nothing is called, no device is opened)
    lib = ctypes.CDLL(qfec.LIB_PATH)
    assert hasattr(lib, "qfec_emit_accumulated") and hasattr(lib, "qfec_revive_accumulated")
    assert hasattr(qfec.Context, "emit_accumulated")
    assert hasattr(qfec.Context, "revive_accumulated")
