"""CPU tests of the receive-map packing of qfec_revive_batch (include/qfec.h):
qfec.pack_received against a hand-written bit loop, and the three group
status constants against the header's #defines."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from libquic_amd import qfec

# the widths where k + 1 crosses a byte, the 64-bit word, and reaches 32 bytes
PACK_K = [1, 7, 8, 15, 16, 63, 64, 255]


def pack_by_hand(data, fec):
    n, k = data.shape
    nb = (k + 1 + 7) // 8
    out = np.zeros((n, nb), dtype=np.uint8)
    for g in range(n):
        for i in range(k + 1):
            bit = bool(data[g, i]) if i < k else bool(fec[g])
            if bit:
                out[g, i // 8] |= 1 << (i % 8)
    return out


@pytest.mark.parametrize("k", PACK_K)
def test_pack_received_matches_bit_loop(k):
    rng = np.random.default_rng(100 + k)
    n = 37
    data = rng.random((n, k)) < 0.6
    fec = rng.random(n) < 0.5
    # the corner maps too: nothing, everything, only the FEC packet, only data
    data[0], fec[0] = False, False
    data[1], fec[1] = True, True
    data[2], fec[2] = False, True
    data[3], fec[3] = True, False
    got = qfec.pack_received(data, fec)
    assert got.dtype == np.uint8
    assert got.shape == (n, k // 8 + 1) == (n, -(-(k + 1) // 8))
    assert np.array_equal(got, pack_by_hand(data, fec))
    # bit i of a map is (map[i // 8] >> (i % 8)) & 1
    for i in range(k):
        assert np.array_equal((got[:, i // 8] >> (i % 8)) & 1, data[:, i].astype(np.uint8))
    assert np.array_equal((got[:, k // 8] >> (k % 8)) & 1, fec.astype(np.uint8))


def test_pack_received_rejects_mismatched_shapes():
    with pytest.raises(ValueError):
        qfec.pack_received(np.ones((3, 4), dtype=bool), np.ones(2, dtype=bool))
    with pytest.raises(ValueError):
        qfec.pack_received(np.ones(4, dtype=bool), np.ones(4, dtype=bool))


def test_group_status_constants_match_header():
    hdr = open(os.path.join(ROOT, "include", "qfec.h")).read()
    for name, value in (("COMPLETE", qfec.GROUP_COMPLETE), ("REVIVED", qfec.GROUP_REVIVED),
                        ("UNREVIVABLE", qfec.GROUP_UNREVIVABLE)):
        m = re.search(r"^#define\s+QFEC_GROUP_%s\s+(\d+)u\b" % name, hdr, flags=re.M)
        assert m, name
        assert int(m.group(1)) == value
    assert (qfec.GROUP_COMPLETE, qfec.GROUP_REVIVED, qfec.GROUP_UNREVIVABLE) == (0, 1, 2)
