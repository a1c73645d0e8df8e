"""The rule of qfec_parse_opened (tests/parse_rule.py) pinned on the CPU: its
packet-by-packet and its whole-array form agree on random turns; on every row
of tests/golden/wire_ref.npz it says what the reference's own QuicFramer said
(accept / reject, the entropy and FEC bits, the class of a rejected header);
and it equals the host parser (qfec_wire_parse_private_header) on all of
wire_cases.private_header_cases().  The fixture and the cases hold no EMPTY
and no RANGE (their bodies are padded to 8 bytes or cut to the flags byte, the
packet numbers are small): key_shift 40, connection 0.
Also here: random_turn, the generator the GPU tests share.
"""
import numpy as np

import parse_rule as PR
import wire_cases as W
from conftest import load_npz

KEY_SHIFT = 40


def random_turn(rng, n, key_shift=KEY_SHIFT, quic_version=31, with_ok=True, gap=20):
    """n packets in one arena of random bytes, each at its own offset (gaps of
    0..gap bytes, so every alignment occurs and the byte behind a packet looks
    like a header), lengths 0..60 with the short ones frequent, flags mostly
    legal, offsets around the packet number, packet numbers and connections
    around what the key holds."""
    ln = np.where(rng.random(n) < 0.3, rng.integers(0, 4, n), rng.integers(4, 61, n))
    gaps = rng.integers(0, gap + 1, n)
    off = np.cumsum(gaps + ln) - ln
    size = int(off[-1] + ln[-1]) if n else 0
    data = rng.integers(0, 256, size, dtype=np.uint8)
    top = (1 << key_shift) - 1
    pn = rng.integers(max(1, top - 300), top + 300, n, dtype=np.uint64, endpoint=True)
    small = rng.random(n)
    pn[small < 0.5] = rng.integers(1, 600, n, dtype=np.uint64)[small < 0.5]
    pn[small < 0.2] = rng.integers(1, 6, n, dtype=np.uint64)[small < 0.2]
    conn_top = min((1 << (64 - key_shift)) - 1, 0xFFFFFFFF)
    conn = np.where(rng.random(n) < 0.8, rng.integers(0, min(conn_top, 50) + 1, n),
                    rng.integers(max(0, conn_top - 2), min(conn_top + 2, 0xFFFFFFFF), n,
                                 endpoint=True)).astype(np.uint32)
    flags = np.where(rng.random(n) < 0.85, rng.integers(0, 8, n), rng.integers(0, 256, n))
    fo = np.where(rng.random(n) < 0.5, rng.integers(0, 256, n),
                  np.clip(pn.astype(np.float64) + rng.integers(-3, 3, n), 0, 255).astype(np.int64))
    data[off[ln >= 1]] = flags[ln >= 1]
    data[off[ln >= 2] + 1] = fo[ln >= 2]
    ok = (rng.random(n) < 0.9).astype(np.uint8) if with_ok else None
    return dict(data=data, off=off.astype(np.uint64), len=ln.astype(np.uint16), pn=pn, conn=conn,
                ok=ok, version=quic_version, shift=key_shift)


def rule(c, form=PR.parse_opened):
    return form(c["data"], c["off"], c["len"], c["pn"], c["conn"], c["ok"], c["version"],
                c["shift"])


def test_the_two_forms_agree():
    seen = set()
    for i, (shift, version) in enumerate([(1, 31), (40, 31), (63, 30), (40, 32), (32, 33),
                                          (31, 31), (33, 31), (40, 31)]):
        rng = np.random.default_rng(7000 + i)
        c = random_turn(rng, 3000, shift, version, with_ok=i % 2 == 0)
        a, b = rule(c), rule(c, PR.parse_opened_np)
        for name in a:
            assert np.array_equal(a[name], b[name]), (shift, version, name)
        assert a["counts"].sum() == 3000
        seen |= set(a["hdr"].tolist())
    # every class and every accepted flags byte occurred
    assert seen == set(range(8)) | set(range(0x80, 0x87))


def fixture_turn():
    """All of wire_ref.npz as one arena per version: {version: (turn, rows)}"""
    g = load_npz("wire_ref.npz")
    out = {}
    for v in W.VERSIONS:
        rows = np.flatnonzero(g["version"] == v)
        ln = g["body_len"][rows].astype(np.int64)
        off = np.cumsum(ln) - ln
        data = np.concatenate([g["body"][r, :g["body_len"][r]] for r in rows])
        out[v] = (dict(data=data, off=off.astype(np.uint64), len=ln.astype(np.uint16),
                       pn=g["pn"][rows].astype(np.uint64), conn=np.zeros(len(rows), np.uint32),
                       ok=None, version=v, shift=KEY_SHIFT), rows)
    return g, out


def check_against_reference(g, rows, out):
    """a parse's outputs over the fixture rows `rows` against the reference
    framer's committed verdicts"""
    hdr = out["hdr"]
    seen = g["header_seen"][rows] != 0
    assert np.array_equal(hdr < 0x80, seen)
    assert np.array_equal((hdr[seen] & PR.ENTROPY_BIT) != 0, g["entropy"][rows][seen] != 0)
    assert np.array_equal((hdr[seen] & PR.FEC_BIT) != 0, g["fec"][rows][seen] != 0)
    want = np.array([PR.DETAIL[d.decode()] for d in g["detail"][rows][~seen]], np.uint8)
    assert np.array_equal(hdr[~seen], want)
    pn = g["pn"][rows].astype(np.uint64)
    ent = np.where(seen, (hdr & 1).astype(np.uint64) << (pn % np.uint64(8)), 0)
    assert np.array_equal(out["entropy"], ent.astype(np.uint8))


def test_rule_equals_the_reference_framer_on_the_fixture():
    g, turns = fixture_turn()
    total = 0
    for v, (c, rows) in turns.items():
        for form in (PR.parse_opened, PR.parse_opened_np):
            out = rule(c, form)
            check_against_reference(g, rows, out)
            assert out["counts"][PR.N_RANGE] == 0 and not np.any(out["hdr"] == PR.EMPTY)
        total += len(rows)
    assert total == len(g["version"]) > 30000
    # the reference knows every class it can: all four rejections occur
    rejected = g["detail"][g["header_seen"] == 0]
    assert {d.decode() for d in rejected} == set(PR.DETAIL)


def test_rule_equals_the_host_parser():
    from libquic_amd import qfec
    n = 0
    for v, pn, body in W.private_header_cases():
        data = np.frombuffer(body, np.uint8)
        hdr, key, idx, body_off, body_len, entropy = PR.parse_one(data, 0, len(body), pn, 0,
                                                                  True, v, KEY_SHIFT)
        used, h = qfec.wire_parse_private_header(body, v, pn)
        if used == 0:
            assert hdr == PR.DETAIL[h], (v, pn, body.hex(), hdr, h)
            assert (key, idx, body_off, body_len, entropy) == (PR.NO_KEY, 0, 0, 0, 0)
        else:
            assert hdr == body[0] and body_off == used and body_len == len(body) - used
            assert (h.entropy_flag, h.in_fec_group, h.fec_flag) == (hdr & 1, hdr >> 1 & 1, hdr >> 2)
            assert entropy == h.entropy_flag << (pn % 8)
            if h.in_fec_group:
                assert idx == h.fec_group_offset and key == pn - h.fec_group_offset
            else:
                assert idx == 0 and key == PR.NO_KEY
        n += 1
    assert n > 30000


def test_writer_rule_equals_the_host_writer():
    from libquic_amd import qfec
    for v in (31, 32):
        for h in range(256):
            for fo in (0, 1, 254, 255):
                data = np.full(4, 0xEE, np.uint8)
                body_off, counts = PR.write_private_headers(data, [1], [h], [fo], v)
                want = b"" if h > 7 else qfec.wire_write_private_header(h & 1, h >> 2 & 1,
                                                                        h >> 1 & 1, fo)
                if v > 31 and h > 1:
                    want = b""  # (the host writer knows no version; the framer refuses these)
                assert bytes(data[1:1 + len(want)]) == want and body_off[0] == 1 + len(want)
                assert np.all(data[1 + len(want):] == 0xEE) and data[0] == 0xEE
                assert counts.tolist() == ([1, 0] if want else [0, 1])
