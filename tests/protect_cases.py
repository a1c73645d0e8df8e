"""Batches for the packet-protection kernels (qpp_kernels.hip) built to sit on
their wave, key, nonce, length / alignment and offset edges, with what each
design promises about itself.  NumPy and the C oracle only: test_protect_cases.py
checks every promise on the CPU, test_hip_protect_edges.py runs the same
batches on the GPU and compares whole output buffers with the oracle.

A Plain is what is protected (headers, payloads, key indices, packet numbers,
path ids, the key table); seal_batch / open_batch / inplace_batch /
shared_batch lay it out in memory for one call (a Batch).  The builders below
(short_open, key_runs, nonce_grid, length_grid, reduced_grid) return a Plain
plus the promises of the design.
"""
from concurrent.futures import ThreadPoolExecutor
from types import SimpleNamespace

import numpy as np

from oracle import oracle_c as OC

TAG = 12
FILL = 0xA5
CIPHERS = ("null", "chacha20poly1305", "aes128gcm")
AEADS = CIPHERS[1:]
KLEN = {"chacha20poly1305": 32, "aes128gcm": 16}
LENGTHS = (0, 1, 15, 16, 17, 100, 1350, 1452)
THREADS = 8


# ---- bytes in and out of scattered spans ---------------------------------------
def positions(off, lens):
    l = lens.astype(np.int64)
    return np.repeat(off.astype(np.int64) - (np.cumsum(l) - l), l) + np.arange(int(l.sum()))


def put(buf, off, lens, src):
    """src: the spans' bytes one after another, in span order."""
    buf[positions(off, lens)] = src


def take(buf, off, lens):
    return buf[positions(off, lens)]


def starts(lens):
    l = lens.astype(np.int64)
    return np.cumsum(l) - l


def place(lens, res=None, order=None, gap=0):
    """Offsets of spans of lens[i] bytes laid one behind the other in `order`
    (default: as numbered), `gap` bytes apart, span i at res[i] mod 16 where
    res is given.  Returns the offsets (uint64) and the end of the last span."""
    L = [int(x) for x in lens]
    R = None if res is None else [int(x) for x in res]
    off = np.zeros(len(L), np.uint64)
    cur = 0
    for i in (range(len(L)) if order is None else [int(x) for x in order]):
        cur += gap
        if R is not None:
            cur += (R[i] - cur) % 16
        off[i] = cur
        cur += L[i]
    return off, cur


def disjoint(off, lens):
    """No two of the (non-empty) ranges overlap."""
    keep = lens.astype(np.int64) > 0
    o, l = off.astype(np.int64)[keep], lens.astype(np.int64)[keep]
    s = np.argsort(o, kind="stable")
    return bool(np.all(o[s][:-1] + l[s][:-1] <= o[s][1:]))


# ---- what is protected -------------------------------------------------------------
class Plain:
    """dup: pairs (a, b), entry b of the key table a copy of entry a (key and
    prefix).  The table has 36 bytes per entry: a 32-byte key (AES-128-GCM uses
    the first 16) and the 4-byte nonce prefix."""

    def __init__(self, ad_len, pt_len, kidx, pn, path, nkeys, seed, dup=()):
        rng = np.random.default_rng(seed)
        self.n = len(pt_len)
        self.ad_len = np.asarray(ad_len, np.uint16)
        self.pt_len = np.asarray(pt_len, np.uint16)
        self.kidx = np.asarray(kidx, np.uint32)
        self.pn = np.asarray(pn, np.uint64)
        self.path = None if path is None else np.asarray(path, np.uint8)
        self.ad = rng.integers(0, 256, int(self.ad_len.astype(np.int64).sum()), dtype=np.uint8)
        self.pt = rng.integers(0, 256, int(self.pt_len.astype(np.int64).sum()), dtype=np.uint8)
        self.table = rng.integers(0, 256, (nkeys, 36), dtype=np.uint8)
        for a, b in dup:
            self.table[b] = self.table[a]
        assert int(self.kidx.max()) < nkeys
        self.seed = seed
        self._sealed = {}

    def keys(self, cipher):
        return (np.ascontiguousarray(self.table[:, :KLEN[cipher]]).ravel(),
                np.ascontiguousarray(self.table[:, 32:]).ravel())

    def with_kidx(self, kidx):
        """The same packets and key table under other key indices."""
        q = Plain.__new__(Plain)
        q.__dict__.update(self.__dict__)
        q.kidx = np.asarray(kidx, np.uint32)
        q._sealed = {}
        return q

    def with_path(self, path):
        q = Plain.__new__(Plain)
        q.__dict__.update(self.__dict__)
        q.path = None if path is None else np.asarray(path, np.uint8)
        q._sealed = {}
        return q

    def sealed(self, cipher):
        """The oracle's ciphertexts (with tags), one after another."""
        if cipher not in self._sealed:
            b = seal_batch(self)
            out = oracle_seal(cipher, b)
            self._sealed[cipher] = take(out, b.out_off, b.out_len)
        return self._sealed[cipher]


class Batch:
    """The arrays of one call.  out_len: the bytes the call writes for a packet
    that passes; slot_len: the room laid out for it (>= out_len)."""

    def __init__(self, plain, decrypt, data, ad_off, in_off, in_len, out_off, out_len, slot_len,
                 size, cipher=None):
        self.plain, self.decrypt, self.cipher = plain, decrypt, cipher
        self.n = plain.n
        self.data = data
        self.ad_off, self.ad_len = ad_off, plain.ad_len
        self.in_off, self.in_len = in_off, np.asarray(in_len, np.uint16)
        self.out_off, self.size = out_off, size
        self.out_len = np.asarray(out_len, np.int64)
        self.slot_len = np.asarray(slot_len, np.int64)


def _inputs(plain, in_len, in_bytes, ad_res, in_res, order, gap, seed):
    n = plain.n
    lens = np.empty(2 * n, np.int64)
    lens[0::2], lens[1::2] = plain.ad_len, in_len
    res = None
    if ad_res is not None or in_res is not None:
        res = np.empty(2 * n, np.int64)
        res[0::2] = np.arange(n) * 5 % 16 if ad_res is None else ad_res
        res[1::2] = np.arange(n) * 3 % 16 if in_res is None else in_res
    off, end = place(lens, res, order, gap)
    data = np.random.default_rng(seed).integers(0, 256, end + 1, dtype=np.uint8)
    ad_off, in_off = off[0::2].copy(), off[1::2].copy()
    put(data, ad_off, plain.ad_len, plain.ad)
    put(data, in_off, in_len, in_bytes)
    return data, ad_off, in_off


def seal_batch(plain, ad_res=None, in_res=None, out_res=None, in_order=None, out_order=None,
               gap=0, out_gap=0):
    """in_order: an order of the 2n input spans (2p the header, 2p + 1 the
    payload of packet p); out_order: an order of the n output slots."""
    data, ad_off, in_off = _inputs(plain, plain.pt_len, plain.pt, ad_res, in_res, in_order, gap,
                                   plain.seed + 1)
    out_len = plain.pt_len.astype(np.int64) + TAG
    out_off, end = place(out_len, out_res, out_order, out_gap)
    return Batch(plain, False, data, ad_off, in_off, plain.pt_len, out_off, out_len, out_len,
                 end + out_gap + 1)


def open_batch(plain, cipher, short=None, tamper=(), ad_res=None, in_res=None, out_res=None,
               in_order=None, out_order=None, gap=0, out_gap=0, short_slot=16):
    """The oracle's ciphertexts of `plain` laid out for an open.  short: per
    packet -1 or a ciphertext length below the tag's 12 bytes (its payload in
    `plain` is empty: the ciphertext is the tag, cut); tamper: packets with
    one bit flipped, in the ciphertext or in the tag."""
    ct = plain.sealed(cipher)
    full = plain.pt_len.astype(np.int64) + TAG
    ct_len = full.copy()
    if short is not None:
        cut = short >= 0
        assert np.all(plain.pt_len[cut] == 0) and np.all(short[cut] < TAG)
        ct_len[cut] = short[cut]
        keep = np.arange(ct.size) - np.repeat(starts(full), full) < np.repeat(ct_len, full)
        ct = ct[keep]
    ct = ct.copy()
    at = starts(ct_len)
    for j, p in enumerate(tamper):
        assert ct_len[p] >= TAG
        ct[at[p] + (j * 7 + 5) % ct_len[p]] ^= 1 << (j % 8)
    data, ad_off, in_off = _inputs(plain, ct_len, ct, ad_res, in_res, in_order, gap,
                                   plain.seed + 2)
    out_len = np.maximum(ct_len - TAG, 0)
    slot = out_len.copy()
    if short is not None:
        slot[short >= 0] = short_slot
    out_off, end = place(slot, out_res, out_order, out_gap)
    return Batch(plain, True, data, ad_off, in_off, ct_len, out_off, out_len, slot,
                 end + out_gap + 1, cipher)


def inplace_batch(plain, pay_res=None, gap=2):
    """[header | payload | 12 spare] records, the output on the payload
    (QuicPacketCreator::EncryptInPlace), the payload at pay_res[p] mod 16."""
    ad, pt = plain.ad_len.astype(np.int64), plain.pt_len.astype(np.int64)
    res = None if pay_res is None else (np.asarray(pay_res, np.int64) - ad) % 16
    rec, end = place(ad + pt + TAG, res, None, gap)
    data = np.random.default_rng(plain.seed + 3).integers(0, 256, end + gap + 1, dtype=np.uint8)
    in_off = rec + ad.astype(np.uint64)
    put(data, rec, plain.ad_len, plain.ad)
    put(data, in_off, plain.pt_len, plain.pt)
    b = Batch(plain, False, data, rec, in_off, plain.pt_len, in_off.copy(), pt + TAG, pt + TAG,
              data.size)
    b.rec_off, b.rec_len = rec, ad + pt + TAG
    return b


def shared_batch(plain, order, res=None, gap=1):
    """A seal whose headers, payloads and output slots share one offset space
    (span 3p the header, 3p + 1 the payload, 3p + 2 the output of packet p, laid
    in `order`): input and output spans interleave.  bytes and out are two
    arrays of the same size."""
    n = plain.n
    lens = np.empty(3 * n, np.int64)
    lens[0::3], lens[1::3] = plain.ad_len, plain.pt_len
    lens[2::3] = plain.pt_len.astype(np.int64) + TAG
    off, end = place(lens, res, order, gap)
    data = np.random.default_rng(plain.seed + 4).integers(0, 256, end + gap, dtype=np.uint8)
    put(data, off[0::3], plain.ad_len, plain.ad)
    put(data, off[1::3], plain.pt_len, plain.pt)
    return Batch(plain, False, data, off[0::3].copy(), off[1::3].copy(), plain.pt_len,
                 off[2::3].copy(), lens[2::3], lens[2::3], data.size)


# ---- the oracle on a Batch -------------------------------------------------------------
def _split(n, threads):
    t = max(1, min(threads, n // 64))
    return [(n * i // t, n * (i + 1) // t) for i in range(t)]


def oracle_seal(cipher, b, out=None):
    """out: the buffer to seal into (default: b.size bytes of FILL)."""
    out = np.full(b.size, FILL, np.uint8) if out is None else out
    if cipher == "null":
        OC.null_encrypt_batch(b.data, b.ad_off, b.ad_len, b.in_off, b.in_len, b.out_off, out.size,
                              threads=THREADS, out=out)
        return out
    keys, pre = b.plain.keys(cipher)
    fn = (OC.quic_c20p1305_encrypt_batch if cipher == "chacha20poly1305"
          else OC.quic_aes128gcm_encrypt_batch)
    fn(keys, pre, b.plain.kidx, b.plain.pn, b.plain.path, b.data, b.ad_off, b.ad_len, b.in_off,
       b.in_len, b.out_off, out.size, threads=THREADS, out=out)
    return out


def oracle_open(cipher, b, out=None):
    """null_decrypt_batch / quic_*_decrypt_batch of oracle_c on slices of the
    batch side by side, into one buffer that starts as FILL.  Returns out, ok."""
    out = np.full(b.size, FILL, np.uint8) if out is None else out
    ok = np.full(b.n, 7, np.uint8)
    L, P = OC.lib(), OC._p
    if cipher != "null":
        keys, pre = b.plain.keys(cipher)
        fn = (L.qo_quic_c20p1305_decrypt_batch if cipher == "chacha20poly1305"
              else L.qo_quic_aes128gcm_decrypt_batch)
        pl = b.plain

    def run(r):
        s = slice(*r)
        m = r[1] - r[0]
        if cipher == "null":
            L.qo_null_decrypt_batch(P(b.data), P(b.ad_off[s]), P(b.ad_len[s]), P(b.in_off[s]),
                                    P(b.in_len[s]), m, P(out), P(b.out_off[s]), P(ok[s]))
        else:
            fn(P(keys), P(pre), P(pl.kidx[s]), P(pl.pn[s]),
               None if pl.path is None else P(pl.path[s]), P(b.data), P(b.ad_off[s]),
               P(b.ad_len[s]), P(b.in_off[s]), P(b.in_len[s]), m, P(out), P(b.out_off[s]),
               P(ok[s]))

    parts = _split(b.n, THREADS)
    if cipher == "aes128gcm":
        OC.aes128_encrypt(np.zeros(16, np.uint8), np.zeros(16, np.uint8))  # tables, one thread
    if len(parts) == 1:
        run(parts[0])
    else:
        with ThreadPoolExecutor(len(parts)) as ex:
            list(ex.map(run, parts))
    return out, ok


# ---- the designs -----------------------------------------------------------------------
def numbers(n, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 1 << 62, n, dtype=np.uint64), rng.integers(0, 256, n).astype(np.uint8)


def uniform_waves(kidx, valid=None):
    """Per wave of 64 packets: do all its (valid) packets carry one key index?"""
    n = kidx.size
    out = []
    for w in range(0, n, 64):
        k = kidx[w:w + 64] if valid is None else kidx[w:w + 64][valid[w:w + 64]]
        out.append(np.unique(k).size <= 1)
    return np.array(out)


def short_open(nkeys, tamper=False):
    """581 ciphertexts to open (a 512-thread block, one more wave and five
    lanes), the short ones (below the tag's 12 bytes) placed by lane:
    wave 0 lanes 0-6 of 0, 1, 5, 11, 11, 3, 0 bytes (first valid lane 7); wave
    1 all short; wave 2 only lane 63 valid; wave 3 the even lanes short; waves
    4-8 valid; lane 0 of the tail wave short.  nkeys 1: one key; 3: every wave
    with two valid packets mixes keys.  tamper: one valid packet of every wave
    that has one fails its tag as well."""
    n = 581
    p = np.arange(n)
    short = np.full(n, -1, np.int64)
    short[:7] = [0, 1, 5, 11, 11, 3, 0]
    short[64:128] = np.arange(64) % 12
    short[128:191] = np.arange(63) * 5 % 12
    short[192:256:2] = np.arange(32) * 7 % 12
    short[576] = 4
    valid = short < 0
    pt_len = np.where(valid, np.array(LENGTHS)[p * 3 % 8], 0)
    kidx = np.zeros(n, np.uint32) if nkeys == 1 else (p % 3).astype(np.uint32)
    pn, path = numbers(n, 70 + nkeys)
    plain = Plain(p * 29 % 48, pt_len, kidx, pn, path, nkeys, 71 + nkeys)
    bad = []
    if tamper:
        for w in range(0, n, 64):
            v = np.flatnonzero(valid[w:w + 64])
            if v.size:
                bad.append(w + int(v[(w // 64 * 5) % v.size]))
    ok = valid.copy()
    ok[bad] = False
    first = [int(np.argmax(valid[w:w + 64])) if valid[w:w + 64].any() else None
             for w in range(0, n, 64)]
    return SimpleNamespace(plain=plain, short=short, valid=valid, tampered=np.array(bad, np.int64),
                           ok=ok.astype(np.uint8), first_valid=first,
                           uniform=uniform_waves(kidx, valid))


KEY_RUN_LANES = ((1, 1), (3, 15), (5, 16), (8, 17), (10, 32), (13, 63))  # (wave, lane)
SPARSE = (0, 1000, 70000)


def key_runs(variant):
    """1,061 packets (16 waves and 37 lanes; two 512-thread blocks and a
    part), 4 keys.
      wave:   kidx = (p // 64) % 4: every wave uniform, neighbours differ
      lane:   as wave, but the key changes at lane b of wave w instead of at
              the wave's end, for the (w, b) of KEY_RUN_LANES
      dup:    table entries 1 and 3 hold the same key and prefix; wave 2
              alternates between them, every other packet uses entry 1
      sparse: indices 0, 1,000 and 70,000 of a 70,001-entry table, by wave,
              waves 5 and 9 mixed
      tail:   as wave, the partial last wave mixed"""
    n = 1024 + 37
    p = np.arange(n)
    w, lane = p // 64, p % 64
    nkeys, dup, edges = 4, (), []
    if variant == "wave":
        kidx = w % 4
    elif variant == "lane":
        kidx = w % 4
        for ww, b in KEY_RUN_LANES:
            kidx = np.where((w == ww) & (lane >= b), (ww + 1) % 4, kidx)
            edges.append(64 * ww + b)
    elif variant == "dup":
        kidx = np.where((w == 2) & (lane % 2 == 1), 3, 1)
        dup = ((1, 3),)
    elif variant == "sparse":
        nkeys = SPARSE[-1] + 1
        kidx = np.array(SPARSE)[np.where((w == 5) | (w == 9), lane % 3, w % 3)]
    elif variant == "tail":
        kidx = np.where(w == 16, lane % 4, w % 4)
    else:
        raise ValueError(variant)
    rng = np.random.default_rng(80)
    pn, path = numbers(n, 81)
    plain = Plain(p * 29 % 48, rng.choice(LENGTHS, n), kidx, pn, path, nkeys, 82, dup)
    return SimpleNamespace(plain=plain, edges=edges, uniform=uniform_waves(plain.kidx))


PACKET_NUMBERS = (0, 1, 2**32 - 1, 2**32, 2**48, 2**56 - 1, 2**56, 2**63, 2**64 - 1)
PATH_IDS = (0, 1, 0x7F, 0x80, 0xFF)


def nonce_grid(nkeys):
    """135 packets: every (packet_number, path_id) of the two lists three
    times, on different lanes.  nkeys 1: uniform waves; 3: mixed waves."""
    n = 3 * len(PACKET_NUMBERS) * len(PATH_IDS)
    p = np.arange(n)
    c = p % 45
    pn = np.array(PACKET_NUMBERS, np.uint64)[c % 9]
    path = np.array(PATH_IDS, np.uint8)[c // 9]
    kidx = np.zeros(n, np.uint32) if nkeys == 1 else p % 3
    plain = Plain(p * 29 % 48, np.array((0, 1, 15, 16, 17, 100))[p % 6], kidx, pn, path, nkeys,
                  90 + nkeys)
    return SimpleNamespace(plain=plain, uniform=uniform_waves(plain.kidx))


GRID_CHUNKS = (0, 1, 3, 4, 7, 8, 9, 15, 16, 17, 32, 33)
GRID_LONG = (1349, 1350, 1351, 1451, 1452)


def _grid(chunks, rems, long, seed):
    cells = [(16 * c + r, i, o) for c in chunks for r in rems for i in range(16)
             for o in range(16)]
    cells += [(l, i, o) for l in long for i in range(16) for o in range(16)]
    cells = np.array(cells)
    cells = cells[np.random.default_rng(seed).permutation(len(cells))]  # mixed lengths per wave
    assert len(cells) % 64 == 0
    return cells


def length_grid():
    """The product of payload length % 16 (0..15), full 16-byte chunks
    (GRID_CHUNKS: both sides of the 128-byte GCM slab, the 256-byte ChaCha slab
    and the 4-chunk step), input offset % 16 and output offset % 16: 49,152
    packets; GRID_LONG at every pair of residues; shuffled, so a wave holds
    mixed lengths.  Behind them two skewed waves: lane 37 of 1,452 bytes among
    lanes of 0, 1 or 15, and a wave of 1,452 with one empty packet.  Header
    lengths cycle through 0..47 (stride 29), the header at its own residue.
    Keys by wave, (p // 64) % 4."""
    cells = _grid(GRID_CHUNKS, range(16), GRID_LONG, 100)
    lane = np.arange(64)
    skew = [np.where(lane == 37, 1452, np.array((0, 1, 15))[lane % 3]),
            np.where(lane == 20, 0, 1452)]
    pt_len = np.concatenate([cells[:, 0]] + skew)
    n = pt_len.size
    p = np.arange(n)
    in_res = np.concatenate([cells[:, 1], p[-128:] * 5 % 16])
    out_res = np.concatenate([cells[:, 2], p[-128:] * 11 % 16])
    pn, path = numbers(n, 101)
    plain = Plain(p * 29 % 48, pt_len, p // 64 % 4, pn, path, 4, 102)
    return SimpleNamespace(plain=plain, in_res=in_res, out_res=out_res, ad_res=(p * 7 + 3) % 16,
                           n_grid=len(cells) - 256 * len(GRID_LONG), skew=(n - 128, n - 64))


REDUCED_CHUNKS = (0, 1, 8, 16, 33)
REDUCED_REMS = (0, 1, 7, 15)


def reduced_grid():
    """5,120 cells of the grid (REDUCED_REMS x REDUCED_CHUNKS x 16 x 16) and
    1,350 / 1,452 at every pair of residues: 5,632 packets, keys by wave and
    wave 3 mixed, for the layouts whose offsets run in any order."""
    cells = _grid(REDUCED_CHUNKS, REDUCED_REMS, (1350, 1452), 110)
    n = len(cells)
    p = np.arange(n)
    pn, path = numbers(n, 111)
    kidx = np.where(p // 64 == 3, p % 3, p // 64 % 3)
    plain = Plain(p * 29 % 48, cells[:, 0], kidx, pn, path, 3, 112)
    return SimpleNamespace(plain=plain, in_res=cells[:, 1], out_res=cells[:, 2],
                           ad_res=(p * 7 + 3) % 16)


def cells_of(b):
    """The (length % 16, full chunks, input offset % 16, output offset % 16) of
    every packet of a Batch, from its own arrays."""
    plen = b.out_len - TAG if not b.decrypt else b.out_len
    return np.stack([plen % 16, plen // 16, b.in_off.astype(np.int64) % 16,
                     b.out_off.astype(np.int64) % 16], axis=1)
