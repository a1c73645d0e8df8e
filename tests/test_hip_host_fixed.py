"""The QFEC_PTR_HOST path of the fixed-shape encode / recover (fixed_host in
libquic_amd/csrc/qfec_capi.cpp): every way it brings rows, redundancy and
output across, alone and mixed, and the strided ways past one trip of the slot
rotation; against the C oracle with strides, whole buffers from a 0xA5 fill,
the gaps between L and every stride included.

Rows come in five ways: pageable packed or strided (gathered into the slot's
pinned buffer row by row, or a group at a time where only the groups are
apart), pinned packed (one DMA), pinned uniformly strided (one 2-D DMA of
cnt * k rows), pinned with a free group stride (a 2-D DMA per group).  The
redundancy and the output go three ways each: pageable (bounced), pinned at
stride L (one DMA), pinned strided (a 2-D DMA).  Pinned-ness is decided per
buffer, so the ways mix."""
import itertools

import numpy as np
import pytest
import torch

from oracle import oracle_c as OC
from libquic_amd import qfec

import host_chunks as HC

pytestmark = pytest.mark.gpu

WAYS = ["pageable-packed", "pageable-rowpacked", "pageable-free",
        "pinned-packed", "pinned-uniform", "pinned-free"]
# pinned memory from the library's allocator, from torch, and starting 3 bytes
# into its allocation (an unaligned DMA source / destination)
KINDS = ("hostbuffer", "torch", "hostbuffer+3")


class Buffers:
    """uint8 buffers, pageable or pinned; the pinned allocations live until close()"""

    def __init__(self):
        self.keep, self.used = [], set()

    def get(self, nbytes, kind, role=None):
        if kind is None:
            return np.empty(nbytes, np.uint8)
        self.used.add((role, kind))
        if kind == "torch":
            t = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
            self.keep.append(t)
            return t.numpy()
        hb = qfec.HostBuffer(nbytes + 3)
        self.keep.append(hb)
        return hb.array[3:] if kind == "hostbuffer+3" else hb.array[:nbytes]

    def close(self):
        for b in self.keep:
            if isinstance(b, qfec.HostBuffer):
                b.close()
        self.keep = []


@pytest.fixture
def bufs():
    b = Buffers()
    yield b
    b.close()


def filled(bufs, nbytes, kind, role, content=None):
    a = bufs.get(nbytes, kind, role)
    a[:] = HC.FILL if content is None else content
    return a


SHAPES = [(4, 333), (17, 1351)]


@pytest.mark.parametrize("way", WAYS)
@pytest.mark.parametrize("k,L", SHAPES, ids=lambda v: str(v))
def test_branch_matrix(ctx, bufs, k, L, way):
    """One chunk (n = 301), the full product: this way for the rows x
    {pageable, pinned} x {stride L, stride > L} for the encode's output, and
    for the recover's redundancy and output independently (16 mixes), so every
    branch of every buffer meets both pinned-ness values of the other two."""
    n = 301
    wi, si = WAYS.index(way), SHAPES.index((k, L))
    rs, gs = HC.row_strides(way, k, L)   # strided: row_stride = L + 4, odd or unaligned
    rng = np.random.default_rng([k, L, wi])
    src = rng.integers(0, 256, n * gs, dtype=np.uint8)  # the gaps hold noise too
    miss = (rng.integers(0, 1 << 30, n) % k).astype(np.uint8)
    rows = filled(bufs, n * gs, KINDS[(wi + si) % 3] if way.startswith("pinned") else None,
                  "rows", src)
    kw = dict(row_stride=rs, group_stride=gs, host=True)
    wide = L + 7
    mixes = list(itertools.product((False, True), (L, wide)))
    for i, (pinned, ps) in enumerate(mixes):
        _, want = OC.encode_fixed(src, k, L, n, rs, gs, ps, fill=HC.FILL)
        out = filled(bufs, n * ps, KINDS[(i + wi) % 3] if pinned else None, "parity_out")
        ctx.encode(rows, k, L, n, out, parity_stride=ps, **kw)
        assert np.array_equal(out, want), ("encode", way, pinned, ps)
        assert np.array_equal(rows, src)
    par = OC.encode_fixed(src, k, L, n, rs, gs)[1].reshape(n, L)
    for i, ((ppin, ps), (opin, os_)) in enumerate(itertools.product(mixes, mixes)):
        pin = rng.integers(0, 256, (n, ps), dtype=np.uint8)
        pin[:, :L] = par
        pin = pin.ravel()
        _, want = OC.recover_fixed(src, pin, miss, k, L, n, rs, gs, ps, os_, fill=HC.FILL)
        parity = filled(bufs, n * ps, KINDS[i % 3] if ppin else None, "parity", pin)
        out = filled(bufs, n * os_, KINDS[(i // 2 + 1) % 3] if opin else None, "out")
        ctx.recover(rows, parity, miss, k, L, n, out, parity_stride=ps, out_stride=os_, **kw)
        assert np.array_equal(out, want), ("recover", way, ppin, ps, opin, os_)
        assert np.array_equal(parity, pin) and np.array_equal(rows, src)
    # the revived rows are the erased ones (the oracle agrees with the definition)
    rows3 = np.lib.stride_tricks.as_strided(src, (n, k, L), (gs, rs, 1))
    assert np.array_equal(want.reshape(n, os_)[:, :L], rows3[np.arange(n), miss])
    # the recover's pinned buffers met all three kinds of pinned memory (the
    # rows and the encode's output do across the ways)
    for role in ("parity", "out"):
        assert {kind for r, kind in bufs.used if r == role} == set(KINDS), bufs.used


@pytest.mark.parametrize("name", sorted(HC.FIXED_MULTI))
def test_past_the_slot_rotation(ctx, bufs, name):
    """The branches that never crossed a chunk, over SLOTS full chunks and a
    tail of a few groups (tests/host_chunks.py: why each n, and the proof of
    ceil(n / cg) > SLOTS and n % cg != 0): pinned uniformly strided rows with
    pinned strided redundancy and output (all 2-D DMAs), pinned rows with a
    free group stride, and pageable strided buffers throughout."""
    s = HC.fixed_multi(name)
    k, L, n, rs, gs = s["k"], s["L"], s["n"], s["row_stride"], s["group_stride"]
    ps, os_ = s["parity_stride"], s["out_stride"]
    assert -(-n // s["cg"]) > HC.SLOTS
    pinned = s["way"].startswith("pinned")
    rng = np.random.default_rng(sorted(HC.FIXED_MULTI).index(name))
    rows = bufs.get(n * gs, "hostbuffer+3" if pinned else None, "rows")
    rows[:] = rng.integers(0, 256, n * gs, dtype=np.uint8)
    kw = dict(row_stride=rs, group_stride=gs, host=True)
    _, want_p = OC.encode_fixed(rows, k, L, n, rs, gs, ps, fill=HC.FILL)
    if not s["recover"]:
        out = filled(bufs, n * ps, "torch" if pinned else None, "parity_out")
        ctx.encode(rows, k, L, n, out, parity_stride=ps, **kw)
        assert np.array_equal(out, want_p), first_group(out, want_p, ps, s["cg"])
        return
    miss = (rng.integers(0, 1 << 30, n) % k).astype(np.uint8)
    _, want_o = OC.recover_fixed(rows, want_p, miss, k, L, n, rs, gs, ps, os_, fill=HC.FILL)
    parity = filled(bufs, n * ps, "torch" if pinned else None, "parity", want_p)
    out = filled(bufs, n * os_, "hostbuffer" if pinned else None, "out")
    ctx.recover(rows, parity, miss, k, L, n, out, parity_stride=ps, out_stride=os_, **kw)
    assert np.array_equal(out, want_o), first_group(out, want_o, os_, s["cg"])


def first_group(got, want, stride, cg):
    i = int(np.flatnonzero(got != want)[0])
    g = i // stride
    return (f"byte {i}: group {g} (+{i % stride}), chunk {g // cg} in slot {g // cg % HC.SLOTS}, "
            f"group {g % cg} of it: got {got[i]:#x}, want {want[i]:#x}")


def test_staging_too_small(ctx):
    """One group whose stride no slot holds is refused ("staging too small",
    cg == 0) before anything is read or written: the buffers are 16 bytes."""
    rows = np.arange(16, dtype=np.uint8)
    assert HC.fixed_chunk_groups(16, HC.STAGE + 1, False) == 0
    out = np.full(16, HC.FILL, np.uint8)
    with pytest.raises(qfec.QfecError, match="staging too small"):
        ctx.encode(rows, 1, 16, 1, out, row_stride=16, group_stride=HC.STAGE + 1, parity_stride=16,
                   host=True)
    assert (out == HC.FILL).all()
    with pytest.raises(qfec.QfecError, match="staging too small"):
        ctx.recover(rows, rows.copy(), np.zeros(1, np.uint8), 1, 16, 1, out, row_stride=16,
                    group_stride=HC.STAGE + 1, parity_stride=16, out_stride=16, host=True)
    assert (out == HC.FILL).all()
    # one byte less and the group fits: a chunk of one group
    ctx.encode(rows, 1, 16, 1, out, row_stride=16, group_stride=HC.STAGE, parity_stride=16,
               host=True)
    assert np.array_equal(out, rows)
