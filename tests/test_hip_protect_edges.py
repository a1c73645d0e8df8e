"""The packet-protection kernels (qpp_kernels.hip: NULL / FNV-1a-128,
ChaCha20-Poly1305, AES-128-GCM-12) and their host-pointer path (protect_host,
qfec_capi.cpp) on the batches of tests/protect_cases.py: short ciphertexts and
the first valid lane of a wave, key runs against the wave, the 64-bit nonce,
the length / alignment grid, offsets in any order, in place, and host
pointers.  tests/test_protect_cases.py proves on the CPU that every batch
holds the edge it is built for.

Every output buffer starts as 0xA5 and the WHOLE buffer is compared, bit for
bit, with the oracle's (oracle/oracle_c.py) started from the same fill: gaps,
failed packets and short packets all count.
"""
import numpy as np
import pytest
import torch

import protect_cases as PC
from protect_cases import AEADS, CIPHERS, FILL

from test_hip_aead import DEV, dv

pytestmark = pytest.mark.gpu


def run(ctx, cipher, b, *, host=False, scratch_out=False, inplace=False, fill=FILL):
    """One call on Batch b.  Returns the whole output buffer (inplace: the
    bytes buffer, which is the output too) and ok (None for a seal)."""
    pl, n = b.plain, b.n
    conv = (lambda a: a) if host else dv
    if host:
        out = b.data.copy() if inplace else np.full(b.size, fill, np.uint8)
        data = out if inplace else b.data
        ok = np.full(n, 7, np.uint8)
    else:
        out = dv(b.data) if inplace else torch.full((b.size,), fill, dtype=torch.uint8, device=DEV)
        data = out if inplace else dv(b.data)
        ok = torch.full((n,), 7, dtype=torch.uint8, device=DEV)
    io = [data, conv(b.ad_off), conv(b.ad_len), conv(b.in_off), conv(b.in_len), n, out,
          conv(b.out_off)]
    kw = dict(host=host)
    if b.decrypt:
        io.append(ok)
        kw["scratch_out"] = scratch_out
    if cipher == "null":
        (ctx.null_decrypt if b.decrypt else ctx.null_encrypt)(*io, **kw)
    else:
        keys, pre = pl.keys(cipher)
        head = [conv(keys), conv(pre), conv(pl.kidx), conv(pl.pn),
                None if pl.path is None else conv(pl.path)]
        getattr(ctx, cipher + ("_open" if b.decrypt else "_seal"))(*head, *io, **kw)
    if host:
        return out, ok if b.decrypt else None
    ctx.sync()
    torch.cuda.synchronize()
    return out.cpu().numpy(), ok.cpu().numpy() if b.decrypt else None


def same(got, want):
    """Whole-buffer equality, the first differing offsets in the message."""
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError(f"{bad.size} bytes differ, first at {bad[:8].tolist()}")


_cache = {}


def cached(key, make):
    """The oracle's result for a batch, computed once per session and left unchanged."""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def seal_and_open(ctx, cipher, key, seal, opn, **kw):
    want = cached((key, cipher, "seal"), lambda: PC.oracle_seal(cipher, seal))
    same(run(ctx, cipher, seal, **kw)[0], want)
    w_out, w_ok = cached((key, cipher, "open"), lambda: PC.oracle_open(cipher, opn))
    assert w_ok.all()
    out, ok = run(ctx, cipher, opn, **kw)
    assert np.array_equal(ok, w_ok)
    same(out, w_out)


# ---- a. short ciphertexts and the first valid lane --------------------------------------
SHORT_RUNS = [(1, False, False), (1, False, True), (3, False, False), (3, False, True),
              (3, True, False)]


@pytest.mark.parametrize("cipher", CIPHERS)
@pytest.mark.parametrize("nkeys,tamper,scratch", SHORT_RUNS)
def test_short_ciphertexts(ctx, cipher, nkeys, tamper, scratch):
    """581 ciphertexts, those below the tag's 12 bytes placed so that the first
    valid lane of a wave is 7, none, 63, 1 and 0: ok as the oracle's, and the
    outputs of short (and, two-pass, of tampered) packets and every gap still
    0xA5.  One key: the GCM table path with round keys broadcast from a lane
    other than 0; three keys: the per-lane path."""
    c = PC.short_open(nkeys, tamper)
    b = PC.open_batch(c.plain, cipher, short=c.short, tamper=c.tampered, gap=3, out_gap=5)
    w_out, w_ok = PC.oracle_open(cipher, b)
    assert np.array_equal(w_ok, c.ok)
    out, ok = run(ctx, cipher, b, scratch_out=scratch)
    assert np.array_equal(ok, w_ok)
    same(out, w_out)
    for p in np.flatnonzero(c.ok == 0):  # (the whole-buffer compare, spelled out)
        o = int(b.out_off[p])
        assert np.all(out[o:o + int(b.slot_len[p])] == FILL), p


# ---- b. key runs ----------------------------------------------------------------------------
@pytest.mark.parametrize("cipher", AEADS)
@pytest.mark.parametrize("variant", ["wave", "lane", "dup", "sparse", "tail"])
def test_key_runs(ctx, cipher, variant):
    """Key-uniform and mixed waves side by side (aes128gcm_kernel decides by
    key_idx and keeps one table per wave of a block): keys that change with
    the wave, at a lane inside it, equal key bytes under two indices, sparse
    indices into a 70,001-entry table, a mixed partial last wave."""
    c = PC.key_runs(variant)
    seal = PC.seal_batch(c.plain, gap=1, out_gap=2)
    opn = PC.open_batch(c.plain, cipher, gap=1, out_gap=2)
    seal_and_open(ctx, cipher, ("runs", variant), seal, opn)
    if variant == "dup":
        ones = PC.seal_batch(c.plain.with_kidx(np.ones(c.plain.n)), gap=1, out_gap=2)
        same(run(ctx, cipher, ones)[0], run(ctx, cipher, seal)[0])


# ---- c. the nonce ---------------------------------------------------------------------------
@pytest.mark.parametrize("cipher", AEADS)
@pytest.mark.parametrize("nkeys", [1, 3])
def test_nonce(ctx, cipher, nkeys):
    """nonce = prefix || LE64(path_id << 56 | packet_number) over packet
    numbers up to 2^64 - 1 and path ids up to 0xFF, in uniform (nkeys 1) and
    mixed waves; path_id = None is an all-zero path_id array."""
    c = PC.nonce_grid(nkeys)
    pl = c.plain
    seal_and_open(ctx, cipher, ("nonce", nkeys), PC.seal_batch(pl, out_gap=1),
                  PC.open_batch(pl, cipher, out_gap=1))
    none = PC.seal_batch(pl.with_path(None), out_gap=1)
    zero = PC.seal_batch(pl.with_path(np.zeros(pl.n, np.uint8)), out_gap=1)
    want = PC.oracle_seal(cipher, none)
    same(run(ctx, cipher, none)[0], want)
    same(run(ctx, cipher, zero)[0], want)
    o_none = PC.open_batch(pl.with_path(None), cipher, out_gap=1)
    w_out, w_ok = PC.oracle_open(cipher, o_none)
    out, ok = run(ctx, cipher, o_none)
    assert w_ok.all() and np.array_equal(ok, w_ok)
    same(out, w_out)


# ---- d. the length and alignment grid -----------------------------------------------------
@pytest.fixture(scope="module")
def grid():
    return PC.length_grid()


@pytest.mark.parametrize("cipher", CIPHERS)
def test_length_grid(ctx, grid, cipher):
    """Payload length % 16 x full chunks x input offset % 16 x output offset %
    16 (49,152 packets), the lengths around 1,350 and 1,452 at every pair of
    residues and two skewed waves: seal, and open of what was sealed."""
    c = grid
    seal = PC.seal_batch(c.plain, c.ad_res, c.in_res, c.out_res)
    opn = PC.open_batch(c.plain, cipher, ad_res=c.ad_res, in_res=c.in_res, out_res=c.out_res)
    seal_and_open(ctx, cipher, "grid", seal, opn)


# ---- e. offsets in any order, and in place ---------------------------------------------------
@pytest.fixture(scope="module")
def reduced():
    return PC.reduced_grid()


@pytest.mark.parametrize("cipher", CIPHERS)
def test_offsets_in_any_order(ctx, reduced, cipher):
    """out_off a random permutation of the output slots, in_off and ad_off
    permuted independently (stage_store writes through other lanes' dst)."""
    c = reduced
    n = c.plain.n
    rng = np.random.default_rng(5)
    kw = dict(ad_res=c.ad_res, in_res=c.in_res, out_res=c.out_res, gap=1, out_gap=3)
    seal = PC.seal_batch(c.plain, in_order=rng.permutation(2 * n), out_order=rng.permutation(n),
                         **kw)
    opn = PC.open_batch(c.plain, cipher, in_order=rng.permutation(2 * n),
                        out_order=rng.permutation(n), **kw)
    seal_and_open(ctx, cipher, "perm", seal, opn)


def in_place_want(b, cipher):
    want = b.data.copy()
    PC.put(want, b.out_off, b.out_len, b.plain.sealed(cipher))
    return want


@pytest.mark.parametrize("cipher", CIPHERS)
def test_seal_in_place_records(ctx, reduced, cipher):
    """[header | payload | 12 spare] records sealed in place at every alignment
    of the payload: every record's ciphertext and tag as the oracle's, headers
    and the bytes between records unchanged."""
    b = PC.inplace_batch(reduced.plain, reduced.in_res)
    got = run(ctx, cipher, b, inplace=True)[0]
    want = in_place_want(b, cipher)
    ct, at = b.plain.sealed(cipher), PC.starts(b.out_len)
    for p in range(b.n):  # record by record first: a failure names the packet
        o, l = int(b.out_off[p]), int(b.out_len[p])
        assert np.array_equal(got[o:o + l], ct[at[p]:at[p] + l]), p
    same(got, want)


# ---- f. host pointers -----------------------------------------------------------------------
@pytest.mark.parametrize("cipher", CIPHERS)
def test_host_descending_and_interleaved(ctx, reduced, cipher):
    """protect_host rebases every offset to the span it stages and seeds the
    output span from the caller's bytes: descending out_off, and headers,
    payloads and outputs interleaved in one offset space; the 0xA5 between the
    outputs survives."""
    c = reduced
    n = c.plain.n
    down = PC.seal_batch(c.plain, c.ad_res, c.in_res, c.out_res, out_order=np.arange(n)[::-1],
                         out_gap=3)
    same(run(ctx, cipher, down, host=True)[0], PC.oracle_seal(cipher, down))
    sh = PC.shared_batch(c.plain, np.random.default_rng(6).permutation(3 * n))
    same(run(ctx, cipher, sh, host=True)[0], PC.oracle_seal(cipher, sh))
    opn = PC.open_batch(c.plain, cipher, ad_res=c.ad_res, in_res=c.in_res, out_res=c.out_res,
                        out_order=np.arange(n)[::-1], out_gap=3)
    w_out, w_ok = PC.oracle_open(cipher, opn)
    out, ok = run(ctx, cipher, opn, host=True)
    assert w_ok.all() and np.array_equal(ok, w_ok)
    same(out, w_out)


@pytest.mark.parametrize("cipher", CIPHERS)
def test_host_short_and_tampered(ctx, cipher):
    """The outputs of failed and short packets survive the host path too."""
    c = PC.short_open(3, True)
    b = PC.open_batch(c.plain, cipher, short=c.short, tamper=c.tampered, gap=3, out_gap=5)
    w_out, w_ok = PC.oracle_open(cipher, b)
    assert np.array_equal(w_ok, c.ok)
    out, ok = run(ctx, cipher, b, host=True)
    assert np.array_equal(ok, w_ok)
    same(out, w_out)


@pytest.mark.parametrize("cipher", CIPHERS)
def test_host_seal_in_place(ctx, reduced, cipher):
    """out and bytes the same host array."""
    b = PC.inplace_batch(reduced.plain, reduced.in_res)
    same(run(ctx, cipher, b, host=True, inplace=True)[0], in_place_want(b, cipher))
