"""The batches of tests/protect_cases.py through the oracle alone (seal, then
open), and every promise of their designs checked on the CPU: the GPU tests
of test_hip_protect_edges.py cannot pass because a batch silently lost the
edge it was built for."""
import itertools

import numpy as np
import pytest

import protect_cases as PC
from protect_cases import AEADS, CIPHERS, FILL, TAG


def written(b, ok=None):
    """Mask of the bytes of the output buffer that the call writes."""
    m = np.zeros(b.size, bool)
    l = b.out_len if ok is None else b.out_len * ok.astype(np.int64)
    m[PC.positions(b.out_off, l)] = True
    return m


def check_seal_open(cipher, seal, opn, ok_want=None):
    """Oracle seal of `seal`, oracle open of `opn` (the same Plain): the
    ciphertexts opened are the ones sealed, ok is as designed, the plaintext
    comes back and every byte outside a passing packet's output stays FILL."""
    pl = seal.plain
    out = PC.oracle_seal(cipher, seal)
    assert np.all(out[~written(seal)] == FILL)
    assert np.array_equal(PC.take(out, seal.out_off, seal.out_len), pl.sealed(cipher))
    dec, ok = PC.oracle_open(cipher, opn)
    ok_want = np.ones(pl.n, np.uint8) if ok_want is None else ok_want
    assert np.array_equal(ok, ok_want)
    w = written(opn, ok_want)
    assert np.all(dec[~w] == FILL)
    good = ok_want.astype(bool)
    sel = np.repeat(good, pl.pt_len.astype(np.int64))
    assert np.array_equal(PC.take(dec, opn.out_off[good], opn.out_len[good]), pl.pt[sel])
    return out, dec


def check_layout(b):
    assert PC.disjoint(b.out_off, b.slot_len), "output slots overlap"
    lens = np.concatenate([b.ad_len.astype(np.int64), b.in_len.astype(np.int64)])
    assert PC.disjoint(np.concatenate([b.ad_off, b.in_off]), lens), "input spans overlap"
    assert int((b.out_off.astype(np.int64) + b.slot_len).max()) <= b.size
    assert int((b.in_off.astype(np.int64) + b.in_len).max()) <= b.data.size
    assert int((b.ad_off.astype(np.int64) + b.ad_len).max()) <= b.data.size


# ---- a. short ciphertexts ------------------------------------------------------------
@pytest.mark.parametrize("cipher", CIPHERS)
@pytest.mark.parametrize("nkeys,tamper", [(1, False), (3, False), (3, True)])
def test_short_open(cipher, nkeys, tamper):
    c = PC.short_open(nkeys, tamper)
    assert c.plain.n == 581 and c.short[:8].tolist() == [0, 1, 5, 11, 11, 3, 0, -1]
    assert c.first_valid == [7, None, 63, 1, 0, 0, 0, 0, 0, 1]
    assert not c.valid[64:128].any() and c.valid[128:192].sum() == 1
    assert c.valid[192:256].tolist() == [False, True] * 32 and c.valid[256:576].all()
    assert c.valid[576:].tolist() == [False, True, True, True, True]
    assert set(c.plain.pt_len[c.valid].tolist()) == set(PC.LENGTHS)
    assert set(c.short[~c.valid].tolist()) == set(range(12))
    if nkeys == 1:
        assert c.uniform.all()
    else:  # every wave with two valid packets mixes keys
        assert c.uniform.tolist() == [False, True, True] + [False] * 7
    if tamper:
        assert c.tampered.size == 9 and np.unique(c.tampered // 64).size == 9
        assert c.valid[c.tampered].all()
    b = PC.open_batch(c.plain, cipher, short=c.short, tamper=c.tampered, gap=3, out_gap=5)
    assert np.array_equal(b.in_len < TAG, ~c.valid)
    check_layout(b)
    dec, ok = PC.oracle_open(cipher, b)
    assert np.array_equal(ok, c.ok)  # 0 exactly on the short and the tampered packets
    assert np.array_equal(ok == 0, ~c.valid | np.isin(np.arange(581), c.tampered))
    assert np.all(dec[~written(b, c.ok)] == FILL)
    good = c.ok.astype(bool)
    assert np.array_equal(PC.take(dec, b.out_off[good], b.out_len[good]),
                          c.plain.pt[np.repeat(good, c.plain.pt_len.astype(np.int64))])


# ---- b. key runs -----------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["wave", "lane", "dup", "sparse", "tail"])
def test_key_runs(variant):
    c = PC.key_runs(variant)
    k = c.plain.kidx.astype(np.int64)
    n = k.size
    assert n == 1061 and set(c.plain.pt_len.tolist()) == set(PC.LENGTHS)
    change = np.flatnonzero(np.diff(k)) + 1
    inside = change[change % 64 != 0]
    if variant == "wave":
        assert c.uniform.all() and inside.size == 0
        assert np.all(k[::64][1:] != k[::64][:-1])  # neighbouring waves hold different tables
    elif variant == "lane":
        assert inside.tolist() == c.edges == [64 * w + b for w, b in PC.KEY_RUN_LANES]
        assert sorted(b for _, b in PC.KEY_RUN_LANES) == [1, 15, 16, 17, 32, 63]
        assert np.flatnonzero(~c.uniform).tolist() == [w for w, _ in PC.KEY_RUN_LANES]
    elif variant == "dup":
        t = c.plain.table
        assert np.array_equal(t[1], t[3]) and not np.array_equal(t[1], t[0])
        assert np.flatnonzero(~c.uniform).tolist() == [2]
        assert k[128:192].tolist() == [1, 3] * 32 and np.all(np.delete(k, np.s_[128:192]) == 1)
    elif variant == "sparse":
        assert set(k.tolist()) == set(PC.SPARSE) and c.plain.table.shape[0] == 70001
        assert np.flatnonzero(~c.uniform).tolist() == [5, 9]
    else:
        assert np.flatnonzero(~c.uniform).tolist() == [16] and n % 64 == 37
        assert np.unique(k[1024:]).size == 4
    for cipher in AEADS:
        seal = PC.seal_batch(c.plain, gap=1, out_gap=2)
        opn = PC.open_batch(c.plain, cipher, gap=1, out_gap=2)
        check_layout(seal)
        check_layout(opn)
        out, _ = check_seal_open(cipher, seal, opn)
        if variant == "dup":  # equal key bytes under two indices: the bytes of index 1 alone
            ones = PC.seal_batch(c.plain.with_kidx(np.ones(n)), gap=1, out_gap=2)
            assert np.array_equal(PC.oracle_seal(cipher, ones), out)


# ---- c. nonces -------------------------------------------------------------------------
@pytest.mark.parametrize("nkeys", [1, 3])
def test_nonce_grid(nkeys):
    c = PC.nonce_grid(nkeys)
    pl = c.plain
    assert pl.n >= 64 and len(c.uniform) == 3
    assert c.uniform.all() if nkeys == 1 else not c.uniform.any()
    pairs = set(zip(pl.pn.tolist(), pl.path.tolist()))
    assert pairs == set(itertools.product(PC.PACKET_NUMBERS, PC.PATH_IDS)) and len(pairs) == 45
    assert 2**64 - 1 in pl.pn.tolist() and pl.pn.dtype == np.uint64
    for pair in pairs:  # each on three different lanes
        at = np.flatnonzero((pl.pn == np.uint64(pair[0])) & (pl.path == pair[1]))
        assert np.unique(at % 64).size == 3
    for cipher in AEADS:
        seal, opn = PC.seal_batch(pl, out_gap=1), PC.open_batch(pl, cipher, out_gap=1)
        out, _ = check_seal_open(cipher, seal, opn)
        # the high word and the path id both reach the nonce: without either the
        # ciphertexts differ
        low = pl.with_path(None)
        low.pn = pl.pn & np.uint64(0xFFFFFFFF)
        assert not np.array_equal(PC.oracle_seal(cipher, PC.seal_batch(low, out_gap=1)), out)
        zero = pl.with_path(np.zeros(pl.n, np.uint8))
        assert np.array_equal(PC.oracle_seal(cipher, PC.seal_batch(zero, out_gap=1)),
                              PC.oracle_seal(cipher, PC.seal_batch(pl.with_path(None), out_gap=1)))


# ---- d. the length and alignment grid ---------------------------------------------------
@pytest.fixture(scope="module")
def grid():
    return PC.length_grid()


def test_length_grid_cells(grid):
    c = grid
    pl = c.plain
    assert pl.n == 49152 + 1280 + 128 and c.n_grid == 49152 and pl.n % 64 == 0
    assert set(pl.ad_len.tolist()) == set(range(48))
    want = set(itertools.product(range(16), PC.GRID_CHUNKS, range(16), range(16)))
    long = set((l % 16, l // 16, i, o) for l in PC.GRID_LONG for i in range(16)
               for o in range(16))
    assert len(want) == 49152
    seal = PC.seal_batch(pl, c.ad_res, c.in_res, c.out_res)
    for b in (seal, PC.open_batch(pl, "null", ad_res=c.ad_res, in_res=c.in_res,
                                  out_res=c.out_res)):
        check_layout(b)
        cells = [tuple(x) for x in PC.cells_of(b)[:-128].tolist()]
        assert len(cells) == len(set(cells)) and set(cells) == want | long
        assert np.array_equal(b.ad_off.astype(np.int64) % 16, c.ad_res)
    # a wave holds mixed lengths (the loops trim against the wave's longest)
    per_wave = pl.pt_len[:-128].reshape(-1, 64) // 16
    assert np.all(per_wave.max(axis=1) > per_wave.min(axis=1))
    a, z = c.skew
    wa, wz = pl.pt_len[a:a + 64], pl.pt_len[z:z + 64]
    assert a % 64 == 0 and wa[37] == 1452 and set(np.delete(wa, 37).tolist()) == {0, 1, 15}
    assert wz.tolist().count(1452) == 63 and wz[20] == 0
    assert PC.uniform_waves(pl.kidx).all()


@pytest.mark.parametrize("cipher", CIPHERS)
def test_length_grid_oracle(grid, cipher):
    c = grid
    seal = PC.seal_batch(c.plain, c.ad_res, c.in_res, c.out_res)
    opn = PC.open_batch(c.plain, cipher, ad_res=c.ad_res, in_res=c.in_res, out_res=c.out_res)
    check_seal_open(cipher, seal, opn)


# ---- e, f. offsets in any order, in place, interleaved ----------------------------------
@pytest.fixture(scope="module")
def reduced():
    return PC.reduced_grid()


def test_reduced_grid_layouts(reduced):
    c = reduced
    pl = c.plain
    n = pl.n
    assert 2000 <= n <= 8000 and n % 64 == 0
    want = set(itertools.product(PC.REDUCED_REMS, PC.REDUCED_CHUNKS, range(16), range(16)))
    rng = np.random.default_rng(5)
    perm = PC.seal_batch(pl, c.ad_res, c.in_res, c.out_res, in_order=rng.permutation(2 * n),
                         out_order=rng.permutation(n), gap=1, out_gap=3)
    down = PC.seal_batch(pl, c.ad_res, c.in_res, c.out_res, out_order=np.arange(n)[::-1],
                         out_gap=3)
    for b in (perm, down):
        check_layout(b)
        assert want <= set(tuple(x) for x in PC.cells_of(b).tolist())
    d = np.diff(perm.out_off.astype(np.int64))
    assert 0.4 < np.mean(d > 0) < 0.6 and 0.4 < np.mean(np.diff(perm.in_off.astype(np.int64)) > 0)
    assert np.mean(perm.ad_off > perm.in_off) > 0.4  # headers and payloads permuted apart
    assert np.all(np.diff(down.out_off.astype(np.int64)) < 0)
    rec = PC.inplace_batch(pl, c.in_res)
    assert PC.disjoint(rec.rec_off, rec.rec_len)  # and a packet's spans lie inside its record
    assert np.array_equal(rec.in_off, rec.out_off)
    assert np.array_equal(rec.ad_off + rec.ad_len.astype(np.uint64), rec.in_off)
    assert set((rec.in_off % np.uint64(16)).tolist()) == set(range(16))
    assert int((rec.rec_off.astype(np.int64) + rec.rec_len).max()) <= rec.size
    sh = PC.shared_batch(pl, rng.permutation(3 * n))
    allo = np.concatenate([sh.ad_off, sh.in_off, sh.out_off])
    alll = np.concatenate([sh.ad_len.astype(np.int64), sh.in_len.astype(np.int64), sh.out_len])
    assert PC.disjoint(allo, alll)  # no output range on an input another packet needs
    lo, hi = int(sh.out_off.min()), int(sh.out_off.max())
    assert np.mean((sh.in_off > lo) & (sh.in_off < hi)) > 0.99  # the spans interleave
    for cipher in CIPHERS:
        ct = pl.sealed(cipher)
        for b in (perm, down, sh):
            out = PC.oracle_seal(cipher, b)
            assert np.array_equal(PC.take(out, b.out_off, b.out_len), ct)
        opn = PC.open_batch(pl, cipher, ad_res=c.ad_res, in_res=c.in_res, out_res=c.out_res,
                            in_order=rng.permutation(2 * n), out_order=rng.permutation(n),
                            gap=1, out_gap=3)
        check_layout(opn)
        check_seal_open(cipher, perm, opn)
