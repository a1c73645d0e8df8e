"""qfec.pack_received_ragged (the receive maps of qfec_revive_ragged) against a
bit-by-bit loop over the layout include/qfec.h states.  No GPU."""
import numpy as np
import pytest

from libquic_amd import qfec

KS = [1, 7, 8, 9, 15, 16, 63, 64, 255]


def batch(ks, seed):
    rng = np.random.default_rng(seed)
    ptr = np.zeros(len(ks) + 1, np.uint32)
    ptr[1:] = np.cumsum(ks)
    rcv = rng.random(int(ptr[-1])) < 0.7
    fec = rng.random(len(ks)) < 0.5
    return ptr, rcv, fec


def loop_maps(ptr, rcv, fec, stride):
    n = ptr.size - 1
    maps = np.zeros((n, stride), np.uint8)
    for g in range(n):
        k = int(ptr[g + 1]) - int(ptr[g])
        bits = list(rcv[int(ptr[g]):int(ptr[g + 1])]) + [fec[g]]
        assert len(bits) == k + 1
        for i, b in enumerate(bits):
            if b:
                maps[g, i // 8] |= 1 << (i % 8)
    return maps


@pytest.mark.parametrize("stride", [None, 32, 40])
def test_mixed_batch(stride):
    ks = KS + KS[::-1] + [3, 255, 1]
    ptr, rcv, fec = batch(ks, 5)
    got = qfec.pack_received_ragged(rcv, fec, ptr, stride)
    want_stride = 32 if stride is None else stride  # 255 // 8 + 1
    assert got.dtype == np.uint8 and got.shape == (len(ks), want_stride)
    assert np.array_equal(got, loop_maps(ptr, rcv, fec, want_stride))


@pytest.mark.parametrize("ks,stride", [([1, 7], 1), ([8, 15, 3], 2), ([16], 3), ([63], 8),
                                       ([64, 1], 9)])
def test_default_stride_is_the_largest_groups(ks, stride):
    ptr, rcv, fec = batch(ks, 6)
    got = qfec.pack_received_ragged(rcv, fec, ptr)
    assert got.shape == (len(ks), stride)
    assert np.array_equal(got, loop_maps(ptr, rcv, fec, stride))
    # every bit, all received and none
    ones = qfec.pack_received_ragged(np.ones_like(rcv), np.ones_like(fec), ptr)
    none = qfec.pack_received_ragged(np.zeros_like(rcv), np.zeros_like(fec), ptr)
    assert np.array_equal(ones, loop_maps(ptr, np.ones_like(rcv), np.ones_like(fec), stride))
    assert not none.any()


def test_empty_batch():
    got = qfec.pack_received_ragged(np.zeros(0, bool), np.zeros(0, bool), np.zeros(1, np.uint32))
    assert got.shape[0] == 0


def test_value_errors():
    ptr, rcv, fec = batch([3, 16, 2], 7)
    with pytest.raises(ValueError, match="map_stride"):
        qfec.pack_received_ragged(rcv, fec, ptr, 2)  # k = 16 needs 3 bytes
    qfec.pack_received_ragged(rcv, fec, ptr, 3)
    with pytest.raises(ValueError, match="map_stride"):
        qfec.pack_received_ragged(rcv, fec, ptr, 0)
    p0 = np.array([0, 3, 3, 5], np.uint32)  # an empty group
    with pytest.raises(ValueError, match="1..255"):
        qfec.pack_received_ragged(np.ones(5, bool), np.ones(3, bool), p0)
    p256 = np.array([0, 256], np.uint32)
    with pytest.raises(ValueError, match="1..255"):
        qfec.pack_received_ragged(np.ones(256, bool), np.ones(1, bool), p256, 40)
    pdown = np.array([0, 10, 5, 15], np.uint32)  # not monotone
    with pytest.raises(ValueError, match="1..255"):
        qfec.pack_received_ragged(np.ones(15, bool), np.ones(3, bool), pdown)
    with pytest.raises(ValueError):
        qfec.pack_received_ragged(rcv, fec[:2], ptr)
    with pytest.raises(ValueError):
        qfec.pack_received_ragged(rcv[:-1], fec, ptr)
