"""qfec_parse_opened on the GPU: the private flags and the FEC group offset byte
of a turn's opened packets, bit for bit against the rule of tests/parse_rule.py
(pinned by test_parse_rule.py): pkt_key_out, pkt_idx_out, body_off_out,
body_len_out, hdr_out, entropy_out and counts, whole buffers.  On all of
tests/golden/wire_ref.npz the device's verdicts are the reference framer's own.

Discipline, as in test_hip_retire_groups.py: every array carries one trailing
entry nobody owns, POISON where the call could write, so a write past the end
shows as a difference, not a fault; the arena ends in bytes that look like a
valid in-group header, so a read past a packet's end shows as a wrong class.
The inputs are compared unchanged.
"""
import numpy as np
import pytest
import torch

import parse_rule as PR
from libquic_amd import qfec
from test_hip_accumulate_ragged import dview
from test_parse_rule import check_against_reference, fixture_turn, random_turn
from turn_sizes import TILE, grid_wrap  # packets per workgroup trip; one more than a full grid

gpu = pytest.mark.gpu
DEV = "cuda:0"
POISON8 = np.uint8(0xA5)
POISON16 = np.uint16(0xA5A5)
POISON32 = np.uint32(0xA5A5A5A5)
POISON64 = np.uint64(0xA5A5A5A5A5A5A5A5)
# what lies behind the arena's last byte: an in-group data header, offset 0
BEYOND = np.array([0x03, 0x00, 0x11, 0x22, 0x33, 0x44, 0x55, 0x66], np.uint8)
OUTPUTS = [("key", np.uint64, POISON64), ("idx", np.uint8, POISON8),
           ("body_off", np.uint64, POISON64), ("body_len", np.uint16, POISON16),
           ("hdr", np.uint8, POISON8), ("entropy", np.uint8, POISON8)]


def host(t, dtype):
    return t.cpu().numpy().view(dtype)


def same(name, got, want):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{name}: {bad.size} differ, first at {bad[0]}: {got[bad[0]]} " \
                          f"want {want[bad[0]]}"


def tail(a, dtype, poison):
    return np.append(np.asarray(a, dtype), poison)


class Case:
    """One call's inputs (a dict as test_parse_rule.random_turn makes them),
    each with its trailing entry, and the rule's outputs over them (computed
    once, shared by every run of the case)."""

    def __init__(self, c, form=PR.parse_opened):
        self.n, self.version, self.shift = len(c["off"]), c["version"], c["shift"]
        self.data = np.concatenate([np.asarray(c["data"], np.uint8), BEYOND])
        self.off = tail(c["off"], np.uint64, POISON64)
        self.len = tail(c["len"], np.uint16, POISON16)
        self.pn = tail(c["pn"], np.uint64, POISON64)
        self.conn = tail(c["conn"], np.uint32, POISON32)
        self.ok = None if c["ok"] is None else tail(c["ok"], np.uint8, POISON8)
        self.want = {}
        for with_ok in ([False, True] if self.ok is not None else [False]):
            self.want[with_ok] = form(self.data, self.off[:self.n], self.len[:self.n],
                                      self.pn[:self.n], self.conn[:self.n],
                                      self.ok[:self.n] if with_ok else None, self.version,
                                      self.shift)

    def latches(self, with_ok):
        return bool(self.want[with_ok]["counts"][PR.N_RANGE])


def launch(ctx, c, with_ok=True, entropy=True, counts=True, flags=0):
    with_ok = with_ok and c.ok is not None
    d = dict(data=dview(c.data), off=dview(c.off), len=dview(c.len), pn=dview(c.pn),
             conn=dview(c.conn), cnt=dview(np.full(7, POISON64)))
    if c.ok is not None:
        d["ok"] = dview(c.ok)
    for name, dtype, poison in OUTPUTS:
        d[name] = dview(np.full(c.n + 1, poison, dtype))
    ctx.parse_opened(d["data"], d["off"], d["len"], d["pn"], d["conn"], c.n, c.version, c.shift,
                     d["key"], d["idx"], d["body_off"], d["body_len"], d["hdr"],
                     pkt_ok=d["ok"] if with_ok else None,
                     entropy_out=d["entropy"] if entropy else None,
                     counts=d["cnt"] if counts else None, flags=flags)
    return d


def compare(c, d, with_ok=True, entropy=True, counts=True):
    w = c.want[with_ok and c.ok is not None]
    for name, dtype, poison in OUTPUTS:
        want = tail(w[name], dtype, poison)
        if name == "entropy" and not entropy:
            want = np.full(c.n + 1, poison, dtype)
        same(name, host(d[name], dtype), want)
    same("counts", host(d["cnt"], np.uint64),
         np.append(w["counts"], POISON64) if counts else np.full(7, POISON64))
    for name, arr in (("data", c.data), ("off", c.off), ("len", c.len), ("pn", c.pn),
                      ("conn", c.conn), ("ok", c.ok)):
        if arr is not None:
            same(name, host(d[name], arr.dtype), arr)


def sync(ctx, latches):
    """the sync after a case: -QUIC_INVALID_FEC_DATA once where a key did not
    fit, then nothing"""
    if latches:
        with pytest.raises(qfec.InvalidFecData):
            ctx.sync()
    assert ctx.sync() == qfec.QFEC_OK


def run(ctx, c, **how):
    d = launch(ctx, c, **how)
    how.pop("flags", None)
    sync(ctx, c.latches(how.get("with_ok", True) and c.ok is not None))
    compare(c, d, **how)
    return d


@pytest.fixture(scope="module")
def fixture():
    return fixture_turn()


@gpu
@pytest.mark.parametrize("version", [30, 31, 32, 33])
def test_reference_fixture(ctx, fixture, version):
    """every row of wire_ref.npz of one version, each a packet at its own
    offset of one arena: the device's accept / reject, entropy and FEC bits and
    reject classes are the reference framer's, and every buffer is the rule's"""
    g, turns = fixture
    turn, rows = turns[version]
    c = Case(turn, PR.parse_opened_np)
    d = run(ctx, c)
    out = {name: host(d[name], dtype)[:c.n] for name, dtype, _ in OUTPUTS}
    check_against_reference(g, rows, out)
    assert len(rows) > 7000


@gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, TILE - 1, TILE, TILE + 1, "grid + 1"])
def test_sizes(ctx, n):
    big = n == "grid + 1"
    n = grid_wrap() if big else n
    rng = np.random.default_rng(8000 + n % 1000)
    c = Case(random_turn(rng, n, 40, 31), PR.parse_opened_np if big else PR.parse_opened)
    assert c.want[True]["counts"].sum() == n
    run(ctx, c)
    run(ctx, c, with_ok=False)


@gpu
@pytest.mark.parametrize("shift,version", [(1, 30), (40, 32), (63, 31), (32, 33), (31, 31)])
def test_parameters(ctx, shift, version):
    c = Case(random_turn(np.random.default_rng(8100 + shift), 3 * TILE + 17, shift, version))
    run(ctx, c)


def packets(specs, gap=0, version=31, shift=40, ok=None, lead=0):
    """a turn from (header bytes, length, pn, conn) records laid out in order,
    `gap` bytes of 0x03 (an in-group header's flags) between them"""
    data, off = [np.full(lead, 0x03, np.uint8)], []
    at = lead
    for body, ln, pn, conn in specs:
        body = (list(body) + [0x5A] * ln)[:ln]
        off.append(at)
        data += [np.array(body, np.uint8), np.full(gap, 0x03, np.uint8)]
        at += ln + gap
    data = np.concatenate(data)
    data = data[:data.size - gap] if gap else data  # the arena ends at the last packet's last byte
    return dict(data=data, off=np.array(off, np.uint64),
                len=np.array([s[1] for s in specs], np.uint16),
                pn=np.array([s[2] for s in specs], np.uint64),
                conn=np.array([s[3] for s in specs], np.uint32), ok=ok, version=version,
                shift=shift)


@gpu
def test_alignment(ctx):
    """the two header bytes at every residue mod 64 (so across 4-, 16- and
    64-byte boundaries), in 3-byte packets packed against their neighbours and
    in longer ones"""
    for ln, gap in ((3, 0), (9, 8)):
        specs, n = [], 0
        for lead in range(64):
            specs.append(((0x02 | (n & 1), n % 7, 0x77), ln, 1000 + n, n % 5))
            n += 1
        for lead in (0, 1, 3, 15, 63):
            c = Case(packets(specs, gap=gap, lead=lead))
            w = c.want[False]
            assert set((c.off[:64] % np.uint64(64)).tolist()) == set(range(64))
            assert w["counts"][PR.N_DATA] == 64
            assert np.array_equal(w["idx"], np.arange(64) % 7)
            run(ctx, c)


@gpu
@pytest.mark.parametrize("ln", [0, 1, 2, 3])
def test_short_packets(ctx, ln):
    """a packet of 0..3 bytes as the arena's last, the arena ending at its last
    byte and a valid in-group header behind it, for every kind of flags byte"""
    classes = set()
    for flags in (0x00, 0x01, 0x02, 0x03, 0x06, 0x07, 0x04, 0x08, 0xFF):
        first = ((0x03, 0x01, 0x10, 0x20), 4, 50, 1)
        c = Case(packets([first, ((flags, 0x00, 0x99), ln, 9, 2)]))
        assert c.data.size == 4 + ln + BEYOND.size
        run(ctx, c)
        w = c.want[False]
        classes.add(int(w["hdr"][1]))
        assert w["body_off"][1] + w["body_len"][1] <= 4 + ln
    want = {0: {PR.NO_FLAGS}, 1: {0, 1, 4, PR.NO_OFFSET, PR.ILLEGAL_FLAGS},
            2: {0, 1, 4, PR.EMPTY, PR.ILLEGAL_FLAGS},
            3: {0, 1, 2, 3, 4, 6, 7, PR.ILLEGAL_FLAGS}}[ln]
    assert classes == want


@gpu
def test_failed_packets_are_not_read(ctx):
    """pkt_ok NULL against given; a FAILED packet's bytes hold a valid in-group
    header, then an illegal one, then nothing at all (length 0): the outputs
    are the same"""
    rng = np.random.default_rng(8200)
    n = 2 * TILE + 5
    ok = (rng.random(n) < 0.6).astype(np.uint8)
    outs = []
    for body, ln in (((0x03, 0x02, 0x01), 7), ((0xF0, 0xFF, 0x01), 7)):
        specs = [(body if not ok[p] else (0x02, p % 3, 0x01), ln, 100 + p, p % 9)
                 for p in range(n)]
        c = Case(packets(specs, gap=1, ok=ok))
        w = c.want[True]
        assert w["counts"][PR.N_FAILED] == n - ok.sum() and w["counts"][PR.N_DATA] == ok.sum()
        assert np.all(w["body_len"][ok == 0] == 0) and np.all(w["key"][ok == 0] == PR.NO_KEY)
        d = run(ctx, c)
        outs.append({name: host(d[name], dtype) for name, dtype, _ in OUTPUTS})
        if body[0] == 0x03:  # without the verdicts every packet is parsed
            assert c.want[False]["counts"][PR.N_FAILED] == 0
            run(ctx, c, with_ok=False)
    for name in outs[0]:
        assert np.array_equal(outs[0][name], outs[1][name]), name


@gpu
def test_packet_numbers(ctx):
    """packet number 1 (only offset 0 is below it), offset == pn - 1 (group 1,
    the lowest), offset == pn and pn + 1, at pn up to 255 and beyond"""
    specs = []
    for pn in (1, 2, 3, 200, 255, 256, 257, 1 << 33):
        for fo in sorted({0, 1, pn - 1, pn, pn + 1, 254, 255} & set(range(256))):
            specs.append(((0x02, fo, 0x44), 5, pn, 3))
            specs.append(((0x07, fo, 0x44), 5, pn, 3))
    c = Case(packets(specs, gap=2))
    w = c.want[False]
    pn, fo = c.pn[:c.n], c.data[c.off[:c.n].astype(np.int64) + 1]
    assert np.array_equal(w["hdr"] == PR.BAD_OFFSET, fo >= pn)
    assert (w["key"] == ((3 << 40) | 1)).sum() >= 10 and w["counts"][PR.N_RANGE] == 0
    run(ctx, c)


def range_edges(shift):
    """group numbers and connections at both sides of what the key holds"""
    g_top = (1 << shift) - 1
    c_top = min((1 << (64 - shift)) - 1, 0xFFFFFFFF)
    specs = []
    for conn in sorted({0, 1, c_top - 1, c_top, min(c_top + 1, 0xFFFFFFFF), 0xFFFFFFFF} -
                       {-1}):
        for group in (1, g_top - 1, g_top, g_top + 1, g_top + 2):
            if group < 1:
                continue
            for fo in (0, 5):
                specs.append(((0x03, fo, 0x10), 4, group + fo, conn))
    rng = np.random.default_rng(shift)
    specs = [specs[i] for i in rng.permutation(len(specs))]
    return packets(specs, gap=3, shift=shift)


@gpu
@pytest.mark.parametrize("shift", [1, 40, 63])
def test_range_edges(ctx, shift):
    """a group number of 2^key_shift - 1 and 2^key_shift, a connection at the
    top of its range and above it, the key that would be QFEC_NO_KEY: RANGE is
    latched, qfec_sync returns -QUIC_INVALID_FEC_DATA once, and every other
    packet's outputs are right"""
    c = Case(range_edges(shift))
    w = c.want[False]
    g_top, c_top = (1 << shift) - 1, min((1 << (64 - shift)) - 1, 0xFFFFFFFF)
    group = c.pn[:c.n] - c.data[c.off[:c.n].astype(np.int64) + 1]
    conn = c.conn[:c.n]
    bad = (group > g_top) | (conn > c_top)
    no_key = ~bad & (group == g_top) & (conn == c_top) & ((1 << (64 - shift)) - 1 == c_top)
    assert np.array_equal(w["hdr"] == PR.RANGE, bad | no_key)
    assert bad.any() and (~bad & (group == g_top)).any() and (~bad & (conn == c_top)).any()
    assert no_key.any() or shift < 32
    assert c.latches(False) and w["counts"][PR.N_DATA] > 0
    run(ctx, c)


@gpu
def test_no_key_at_a_narrow_connection_field(ctx):
    """key_shift 33: the connection field is 31 bits, all ones with the top
    group is QFEC_NO_KEY; one less is a key"""
    top_conn, top_group = (1 << 31) - 1, (1 << 33) - 1
    specs = [((0x02, 1, 0x10), 5, top_group + 1, top_conn),
             ((0x02, 1, 0x10), 5, top_group, top_conn),
             ((0x02, 1, 0x10), 5, top_group + 1, top_conn - 1),
             ((0x02, 0, 0x10), 5, top_group + 1, 0),
             ((0x02, 0, 0x10), 5, 7, top_conn + 1)]
    c = Case(packets(specs, shift=33))
    w = c.want[False]
    assert w["hdr"].tolist() == [PR.RANGE, 2, 2, PR.RANGE, PR.RANGE]
    assert w["key"][1] == PR.NO_KEY - 1 and w["key"][2] == PR.NO_KEY - (1 << 33)
    run(ctx, c)


@gpu
def test_offsets_beyond_4_gib(ctx):
    """pkt_off at and above 2^32: half of the packets lie there, and where
    their offsets truncated to 32 bits would point lies a different header"""
    HI, REGION = 1 << 32, 1 << 16
    big = torch.empty(HI + REGION, dtype=torch.uint8, device=DEV)
    rng = np.random.default_rng(8300)
    c = random_turn(rng, 900, 40, 31, gap=9)
    assert c["data"].size + 64 < REGION
    high = np.arange(900) % 2 == 1
    c["off"] = c["off"] + np.uint64(48) + np.where(high, np.uint64(HI), np.uint64(0))
    low = np.concatenate([np.zeros(48, np.uint8), c["data"], BEYOND])
    low_img, high_img = low.copy(), low.copy()
    for p in range(900):  # each packet in one image, its complement in the other
        s = slice(int(c["off"][p]) % HI, int(c["off"][p]) % HI + int(c["len"][p]))
        (low_img if high[p] else high_img)[s] ^= 0xFF
    big[:low.size] = torch.from_numpy(low_img).to(DEV)
    big[HI:HI + low.size] = torch.from_numpy(high_img).to(DEV)
    want = PR.parse_opened(low, c["off"] % np.uint64(HI), c["len"], c["pn"], c["conn"], c["ok"],
                           31, 40)
    want["body_off"] = want["body_off"] + np.where(high, np.uint64(HI), np.uint64(0))
    d = {name: dview(np.full(901, poison, dtype)) for name, dtype, poison in OUTPUTS}
    cnt = dview(np.full(7, POISON64))
    ctx.parse_opened(big, dview(c["off"]), dview(c["len"]), dview(c["pn"]), dview(c["conn"]), 900,
                     31, 40, d["key"], d["idx"], d["body_off"], d["body_len"], d["hdr"],
                     pkt_ok=dview(c["ok"]), entropy_out=d["entropy"], counts=cnt)
    sync(ctx, bool(want["counts"][PR.N_RANGE]))
    for name, dtype, poison in OUTPUTS:
        same(name, host(d[name], dtype), tail(want[name], dtype, poison))
    same("counts", host(cnt, np.uint64), np.append(want["counts"], POISON64))
    assert (want["hdr"][high] < 8).sum() > 100


@gpu
def test_without_entropy_and_counts(ctx):
    c = Case(random_turn(np.random.default_rng(8400), 700, 40, 31))
    assert c.latches(True)  # (the latch does not hang on counts)
    run(ctx, c, entropy=False)
    run(ctx, c, counts=False)
    run(ctx, c, entropy=False, counts=False, with_ok=False)


@gpu
def test_no_packets(ctx):
    """n_packets == 0: six zeroes, before the buffers are looked at"""
    cnt = dview(np.full(7, POISON64))
    ctx.parse_opened(None, None, None, None, None, 0, 31, 40, None, None, None, None, None,
                     counts=cnt)
    ctx.parse_opened(None, None, None, None, None, 0, 31, 40, None, None, None, None, None)
    assert ctx.sync() == qfec.QFEC_OK
    assert host(cnt, np.uint64).tolist() == [0] * 6 + [int(POISON64)]


@gpu
def test_hint_flags_change_nothing(ctx):
    c = Case(random_turn(np.random.default_rng(8500), 300, 40, 31))
    run(ctx, c, flags=qfec.QFEC_CACHED | qfec.QFEC_SMALL_GROUPS)


@gpu
def test_three_launches_identical(ctx):
    c = Case(random_turn(np.random.default_rng(8600), 40 * TILE + 3, 40, 31))
    runs = [launch(ctx, c) for _ in range(3)]
    sync(ctx, c.latches(True))
    for d in runs:
        compare(c, d)


@gpu
def test_entropy_feeds_the_cumulative_call(ctx):
    """entropy_out handed to entropy_cumulative_batch gives what the same call
    gives on hashes computed on the host from the flags"""
    rng = np.random.default_rng(8700)
    n = 5 * TILE + 9
    c = random_turn(rng, n, 40, 31)
    c["conn"] = np.sort(rng.integers(0, 6, n)).astype(np.uint32)
    case = Case(c)
    d = run(ctx, case)
    hdr = case.want[True]["hdr"]
    hashes = np.where(hdr < 8, (hdr & 1).astype(np.uint64) << (c["pn"] % np.uint64(8)),
                      0).astype(np.uint8)
    assert len(set(hashes.tolist())) > 5
    conn_ptr = dview(np.searchsorted(c["conn"], np.arange(7)).astype(np.uint64))
    cum = [dview(np.full(n, POISON8)) for _ in range(2)]
    ctx.entropy_cumulative(d["entropy"], conn_ptr, None, 6, cum[0], n_packets=n)
    ctx.entropy_cumulative(dview(hashes), conn_ptr, None, 6, cum[1], n_packets=n)
    assert ctx.sync() == qfec.QFEC_OK
    assert torch.equal(cum[0], cum[1]) and len(set(host(cum[0], np.uint8).tolist())) > 5


NAMES = ["data", "off", "len", "pn", "conn", "ok", "n", "version", "shift", "key", "idx",
         "body_off", "body_len", "hdr", "entropy", "cnt", "flags"]
REFUSALS = [
    ("QFEC_PTR_HOST", dict(flags=qfec.QFEC_PTR_HOST), "device pointers only"),
    ("QFEC_PTR_MAPPED", dict(flags=qfec.QFEC_PTR_MAPPED), "device pointers only"),
    ("QFEC_ASYNC", dict(flags=qfec.QFEC_ASYNC), "QFEC_ASYNC"),
    ("bytes NULL", dict(data=None), "null buffer"),
    ("pkt_off NULL", dict(off=None), "null buffer"),
    ("pkt_len NULL", dict(len=None), "null buffer"),
    ("packet_number NULL", dict(pn=None), "null buffer"),
    ("pkt_conn NULL", dict(conn=None), "null buffer"),
    ("pkt_key_out NULL", dict(key=None), "null buffer"),
    ("pkt_idx_out NULL", dict(idx=None), "null buffer"),
    ("body_off_out NULL", dict(body_off=None), "null buffer"),
    ("body_len_out NULL", dict(body_len=None), "null buffer"),
    ("hdr_out NULL", dict(hdr=None), "null buffer"),
    ("key_shift 0", dict(shift=0), "key_shift"),
    ("key_shift 64", dict(shift=64), "key_shift"),
    ("quic_version 0", dict(version=0), "quic_version"),
    ("quic_version 34", dict(version=34), "quic_version"),
    ("2^32 packets", dict(n=1 << 32), "2^32"),
    ("launch failure injected", dict(inject=True), "launch failure injected"),
]


@gpu
@pytest.mark.parametrize("name,fault,fragment", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refused_on_the_host(ctx, name, fault, fragment):
    """Every refusal leaves the poisoned outputs as they were.  Should a check
    go missing and the call launch: every buffer is sized for the good call."""
    n = 9
    c = random_turn(np.random.default_rng(8800), n, 40, 31)
    bufs = dict(data=dview(np.concatenate([c["data"], BEYOND])), off=dview(c["off"]),
                len=dview(c["len"]), pn=dview(c["pn"]), conn=dview(c["conn"]), ok=dview(c["ok"]),
                cnt=dview(np.full(6, POISON64)))
    for out, dtype, poison in OUTPUTS:
        bufs[out] = dview(np.full(n, poison, dtype))
    before = {key: t.cpu() for key, t in bufs.items()}
    a = dict(bufs, n=n, version=31, shift=40, flags=0)
    a.update(fault)
    inject = a.pop("inject", False)
    if inject:
        assert ctx.lib.qfec_debug_fail_launches(ctx.ctx, 1) == 0
    try:
        rc = ctx.lib.qfec_parse_opened(ctx.ctx, *[qfec._ptr(a[x]) for x in NAMES])
    finally:
        if inject:
            assert ctx.lib.qfec_debug_fail_launches(ctx.ctx, 0) == 0
    msg = ctx.lib.qfec_last_error(ctx.ctx).decode()
    assert rc == qfec.QFEC_ERR_INTERNAL and fragment in msg and "parse opened" in msg, (rc, msg)
    assert ctx.sync() == qfec.QFEC_OK
    for key, t in bufs.items():
        assert torch.equal(t.cpu(), before[key]), key
