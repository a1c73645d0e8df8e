"""qfec_write_private_headers on the GPU: WriteFecPrivateHeader over a batch,
byte for byte against the host writer (qfec_wire_write_private_header) and the
rule of tests/parse_rule.py; the bytes around every header untouched; refused
records written nowhere and latched; and written headers parsed back by
qfec_parse_opened.  Every array carries one trailing entry nobody owns.
"""
import numpy as np
import pytest
import torch

import parse_rule as PR
from libquic_amd import qfec
from test_hip_accumulate_ragged import dview
from test_hip_parse_opened import POISON8, POISON64, TILE, host, same, tail
from turn_sizes import GRID_PER_CU, grid_wrap, ncu

gpu = pytest.mark.gpu
FILL = 0xEE


def layout(n, rng, room=2):
    """n records at every alignment: `room` bytes each and 0..5 bytes between"""
    gaps = rng.integers(0, 6, n)
    off = np.cumsum(gaps + room) - room + 3
    return off.astype(np.uint64), int(off[-1]) + room + 4


def run(ctx, off, hdr, fo, size, version, body=True, counts=True):
    n = len(off)
    want = np.full(size, FILL, np.uint8)
    w_body, w_cnt = PR.write_private_headers(want, off, hdr, fo, version)
    d = dict(data=dview(np.full(size, FILL, np.uint8)), off=dview(tail(off, np.uint64, POISON64)),
             hdr=dview(tail(hdr, np.uint8, POISON8)), fo=dview(tail(fo, np.uint8, POISON8)),
             body=dview(np.full(n + 1, POISON64)), cnt=dview(np.full(3, POISON64)))
    ctx.write_private_headers(d["data"], d["off"], d["hdr"], d["fo"], n, version,
                              body_off_out=d["body"] if body else None,
                              counts=d["cnt"] if counts else None)
    if w_cnt[1]:
        with pytest.raises(qfec.InvalidFecData):
            ctx.sync()
    assert ctx.sync() == qfec.QFEC_OK
    same("bytes", host(d["data"], np.uint8), want)
    same("body_off_out", host(d["body"], np.uint64),
         tail(w_body, np.uint64, POISON64) if body else np.full(n + 1, POISON64))
    same("counts", host(d["cnt"], np.uint64),
         np.append(w_cnt, POISON64) if counts else np.full(3, POISON64))
    same("pkt_off", host(d["off"], np.uint64), tail(off, np.uint64, POISON64))
    same("hdr", host(d["hdr"], np.uint8), tail(hdr, np.uint8, POISON8))
    same("fec_offset", host(d["fo"], np.uint8), tail(fo, np.uint8, POISON8))
    return d, want, w_cnt


@gpu
@pytest.mark.parametrize("version", [31, 32])
def test_every_flags_value_equals_the_host_writer(ctx, version):
    """all 8 flag values x offsets {0, 1, 254, 255}: the bytes are the host
    writer's, where the version has them at all (above 31 only the entropy
    bit); a refused record writes nothing and is latched"""
    hdr = np.repeat(np.arange(8), 4).astype(np.uint8)
    fo = np.tile([0, 1, 254, 255], 8).astype(np.uint8)
    off, size = layout(32, np.random.default_rng(version))
    d, want, cnt = run(ctx, off, hdr, fo, size, version)
    legal = 7 if version <= 31 else 1
    for p in range(32):
        h = int(hdr[p])
        w = qfec.wire_write_private_header(h & 1, h >> 2 & 1, h >> 1 & 1, int(fo[p]))
        if h > legal:
            w = b""
        o = int(off[p])
        assert bytes(want[o:o + len(w)]) == w and np.all(want[o + len(w):o + 2] == FILL)
    assert cnt.tolist() == ([24, 8] if version == 31 else [8, 24])


@gpu
@pytest.mark.parametrize("n", [1, 64, TILE - 1, TILE + 1, 5 * TILE + 3])
def test_sizes_and_surroundings(ctx, n):
    """random flags (a few illegal), every alignment; the whole arena is
    compared, so every byte around a header is untouched"""
    rng = np.random.default_rng(9000 + n)
    hdr = np.where(rng.random(n) < 0.9, rng.integers(0, 8, n), rng.integers(8, 256, n))
    off, size = layout(n, rng)
    run(ctx, off, hdr.astype(np.uint8), rng.integers(0, 256, n).astype(np.uint8), size, 31)


@gpu
def test_records_beyond_one_grid(ctx):
    """one record more than the grid takes in a trip: the last record, a
    refused one, is the first workgroup's second trip -- nothing written for
    it, and counted with the refused ones of the first trip"""
    n = grid_wrap()
    assert n > ncu() * GRID_PER_CU * TILE, "the records no longer make the grid loop"
    rng = np.random.default_rng(9050)
    hdr = np.where(rng.random(n) < 0.9, rng.integers(0, 8, n), rng.integers(8, 256, n))
    hdr[n - 2:] = 3, 0x1F
    off, size = layout(n, rng)
    d, want, cnt = run(ctx, off, hdr.astype(np.uint8), rng.integers(0, 256, n).astype(np.uint8),
                       size, 31)
    assert cnt[0] > n // 2 and cnt[1] > n // 20
    assert np.all(want[int(off[n - 1]):] == FILL) and want[int(off[n - 2])] != FILL


@gpu
def test_without_body_offsets_and_counts(ctx):
    rng = np.random.default_rng(9100)
    hdr, fo = rng.integers(0, 9, 300).astype(np.uint8), rng.integers(0, 256, 300).astype(np.uint8)
    off, size = layout(300, rng)
    run(ctx, off, hdr, fo, size, 31, body=False)
    run(ctx, off, hdr, fo, size, 31, counts=False)
    run(ctx, off, hdr, fo, size, 31, body=False, counts=False)


@gpu
def test_no_records(ctx):
    cnt = dview(np.full(3, POISON64))
    ctx.write_private_headers(None, None, None, None, 0, 31, counts=cnt)
    ctx.write_private_headers(None, None, None, None, 0, 31)
    assert ctx.sync() == qfec.QFEC_OK
    assert host(cnt, np.uint64).tolist() == [0, 0, int(POISON64)]


@gpu
def test_write_then_parse_returns_the_inputs(ctx):
    """headers written on the device, parsed on the device: flags, offsets,
    group numbers and body offsets come back"""
    rng = np.random.default_rng(9200)
    n = 3 * TILE + 11
    hdr = rng.choice([0, 1, 2, 3, 6, 7], n).astype(np.uint8)
    fo = rng.integers(0, 200, n).astype(np.uint8)
    pn = (rng.integers(0, 1 << 30, n) + 201).astype(np.uint64)
    conn = rng.integers(0, 1 << 20, n).astype(np.uint32)
    off, size = layout(n, rng, room=6)
    ln = np.full(n, 6, np.uint16)
    data = dview(np.full(size, FILL, np.uint8))
    d_off, body = dview(off), dview(np.full(n, POISON64))
    ctx.write_private_headers(data, d_off, dview(hdr), dview(fo), n, 31, body_off_out=body)
    out = dict(key=dview(np.full(n, POISON64)), idx=dview(np.full(n, POISON8)),
               body_off=dview(np.full(n, POISON64)), body_len=dview(np.zeros(n, np.uint16)),
               hdr=dview(np.full(n, POISON8)))
    ctx.parse_opened(data, d_off, dview(ln), dview(pn), dview(conn), n, 31, 40, out["key"],
                     out["idx"], out["body_off"], out["body_len"], out["hdr"])
    assert ctx.sync() == qfec.QFEC_OK
    grouped = (hdr & 2) != 0
    same("hdr", host(out["hdr"], np.uint8), hdr)
    same("idx", host(out["idx"], np.uint8), np.where(grouped, fo, 0))
    same("key", host(out["key"], np.uint64),
         np.where(grouped, (conn.astype(np.uint64) << np.uint64(40)) | (pn - fo),
                  np.uint64(PR.NO_KEY)))
    assert torch.equal(out["body_off"], body)
    same("body_len", host(out["body_len"], np.uint16), np.where(grouped, 4, 5))


NAMES = ["data", "off", "hdr", "fo", "n", "version", "body", "cnt", "flags"]
REFUSALS = [
    ("QFEC_PTR_HOST", dict(flags=qfec.QFEC_PTR_HOST), "device pointers only"),
    ("QFEC_PTR_MAPPED", dict(flags=qfec.QFEC_PTR_MAPPED), "device pointers only"),
    ("QFEC_ASYNC", dict(flags=qfec.QFEC_ASYNC), "QFEC_ASYNC"),
    ("bytes NULL", dict(data=None), "null buffer"),
    ("pkt_off NULL", dict(off=None), "null buffer"),
    ("hdr NULL", dict(hdr=None), "null buffer"),
    ("fec_offset NULL", dict(fo=None), "null buffer"),
    ("quic_version 0", dict(version=0), "quic_version"),
    ("quic_version 34", dict(version=34), "quic_version"),
    ("2^32 packets", dict(n=1 << 32), "2^32"),
    ("launch failure injected", dict(inject=True), "launch failure injected"),
]


@gpu
@pytest.mark.parametrize("name,fault,fragment", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refused_on_the_host(ctx, name, fault, fragment):
    n = 9
    bufs = dict(data=dview(np.full(64, FILL, np.uint8)),
                off=dview(np.arange(n, dtype=np.uint64) * np.uint64(5)),
                hdr=dview(np.full(n, 3, np.uint8)), fo=dview(np.full(n, 1, np.uint8)),
                body=dview(np.full(n, POISON64)), cnt=dview(np.full(2, POISON64)))
    before = {key: t.cpu() for key, t in bufs.items()}
    a = dict(bufs, n=n, version=31, flags=0)
    a.update(fault)
    inject = a.pop("inject", False)
    if inject:
        assert ctx.lib.qfec_debug_fail_launches(ctx.ctx, 1) == 0
    try:
        rc = ctx.lib.qfec_write_private_headers(ctx.ctx, *[qfec._ptr(a[x]) for x in NAMES])
    finally:
        if inject:
            assert ctx.lib.qfec_debug_fail_launches(ctx.ctx, 0) == 0
    msg = ctx.lib.qfec_last_error(ctx.ctx).decode()
    assert rc == qfec.QFEC_ERR_INTERNAL and fragment in msg and "write private headers" in msg, \
        (rc, msg)
    assert ctx.sync() == qfec.QFEC_OK
    for key, t in bufs.items():
        assert torch.equal(t.cpu(), before[key]), key
