"""The staging budgets of the host-pointer FEC paths (ragged_host / fixed_host in
libquic_amd/csrc/qfec_capi.cpp), a plain restatement of their chunk planners,
and the seeded batches with which the GPU tests run both paths past one trip
of the slot rotation.  tests/test_host_chunks.py pins the constants to the
sources and proves on the CPU that every batch holds the edge it is built for.

A host-pointer call cuts its batch into chunks of whole groups and rotates
them over SLOTS slots (pinned + device staging buffers and a stream each):
chunk c is gathered into slot c % SLOTS once chunk c - SLOTS has been
scattered out of it.  A slot stages STAGE bytes of input, STAGE // 4 of
output and, on the fixed-shape recover, STAGE // 8 of redundancy + lost
indices.  Whatever the planner does, a batch that stages more than
SLOTS * STAGE bytes (or returns more than SLOTS * STAGE // 4) takes more than
SLOTS chunks, so every slot is used twice: the GPU tests rest on these byte
bounds alone; the modelled plan only says which chunk meets which edge.
"""
import numpy as np

SLOTS = 3                 # kSlots
STAGE = 64 << 20          # kStageBytes: staged input per slot
OUT_STAGE = STAGE // 4    # staged output per slot
AUX_STAGE = STAGE // 8    # fixed recover: redundancy rows + lost indices per slot
SMALL_GROUP_BYTES = 4096  # kRaggedSmallGroupBytes: below it on average, two groups per wave
MAX_PACKET = 1452         # QFEC_MAX_PACKET_SIZE
SLOT_BYTES = 1460         # the callers' parity / output slot in the ragged tests
SLOT_BASE = 5             # ... which start at an odd offset
FILL = 0xA5               # every output buffer starts as this
LEN_SENTINEL = 0xBEEF     # parity_len_out starts as this
FAR_OFF = 1 << 60         # pkt_off of a lost packet: never read, and far outside any arena


def align_up(x, a):
    return (x + a - 1) // a * a


def ragged_totals(n, npk, nbytes, nout, npar, recover):
    """RaggedLayout's in_total / out_total for a chunk of n groups with npk
    packet entries, nbytes staged packet bytes, nout output bytes and (recover)
    npar redundancy bytes."""
    off = align_up(nbytes, 16)
    ln = off + npk * 8
    ptr = align_up(ln + npk * 2, 8)
    poff = align_up(ptr + (n + 1) * 4, 8)
    par = align_up(poff + n * 8, 16)
    plen = align_up(par + (npar if recover else 0), 8)
    miss = plen + (n * 2 if recover else 0)
    ooff = align_up(miss + (n if recover else 0), 8)
    in_total = ooff + (n * 8 if recover else 0)
    out_total = align_up(nout, 8) + (0 if recover else n * 2)
    return in_total, out_total


def group_sums(pkt_len, grp_ptr, missing=None):
    """per group: packets, staged bytes and longest packet (recover: the lost
    packet is not staged); grp_ptr need not start at 0"""
    ptr = np.asarray(grp_ptr).astype(np.int64)
    ln = np.asarray(pkt_len).astype(np.int64)[:ptr[-1]].copy()
    ks = np.diff(ptr)
    mx = np.maximum.reduceat(ln, ptr[:-1])
    if missing is not None:
        ln[ptr[:-1] + np.asarray(missing).astype(np.int64)] = 0
    return ks, np.add.reduceat(ln, ptr[:-1]), mx


def plan_ragged(pkt_len, grp_ptr, recover=False, missing=None, parity_len=None):
    """ragged_host's plan: whole groups, cut before the group that would exceed
    the input or the output budget.  A list of dicts: g0, n, npk, nbytes, nout,
    npar, small (the two-groups-per-wave rule) and cut: "in", "out", "both"
    (which budget the next group would have exceeded) or "end"."""
    ks, gb, mx = group_sums(pkt_len, grp_ptr, missing if recover else None)
    gout = np.asarray(parity_len).astype(np.int64) if recover else mx
    ks, gb, gout = ks.tolist(), gb.tolist(), gout.tolist()
    n, g, chunks = len(ks), 0, []
    while g < n:
        c = dict(g0=g, n=0, npk=0, nbytes=0, nout=0, npar=0, cut="end")
        while g < n:
            t = (c["n"] + 1, c["npk"] + ks[g], c["nbytes"] + gb[g], c["nout"] + gout[g],
                 c["npar"] + (gout[g] if recover else 0))
            it, ot = ragged_totals(*t, recover)
            if c["n"] > 0 and (it > STAGE or ot > OUT_STAGE):
                c["cut"] = "both" if it > STAGE and ot > OUT_STAGE else \
                    "in" if it > STAGE else "out"
                break
            c["n"], c["npk"], c["nbytes"], c["nout"], c["npar"] = t
            g += 1
        c["small"] = c["nbytes"] < SMALL_GROUP_BYTES * c["n"]
        chunks.append(c)
    return chunks


def fixed_chunk_groups(L, group_stride, recover):
    """fixed_host's groups per chunk; 0 is its "staging too small" refusal"""
    cg = min(STAGE // group_stride, OUT_STAGE // L)
    return min(cg, AUX_STAGE // (L + 1)) if recover else cg


# ---- ragged batches --------------------------------------------------------
ARENA = 8 << 20
# (groups, kmin, kmax, lmin, lmax): 200 MB of full-size k = 15 groups for the
# input budget, 36,000 groups of one or two full-size packets (52 MB of
# outputs from 78 MB of packets) for the output budget, and 60,000 tiny groups
# that fit one chunk beside the rest of either stretch
STRETCHES = ((9_700, 15, 15, 1_300, 1_452), (36_000, 1, 2, 1_440, 1_452), (60_000, 2, 4, 16, 100))


def ragged_batch(seed, stretches=STRETCHES, order=None, arena=ARENA):
    """A seeded CSR batch of the stretches in `order` (default: as listed).
    Every packet lies at a random offset of one shared arena, overlapping the
    others, so the caller's memory stays small however much is staged.  Each
    stretch is drawn from its own generator: it is the same groups wherever
    it stands.  Returns data, pkt_off, pkt_len, grp_ptr, missing, ks and
    stretch (the stretch of every group)."""
    order = range(len(stretches)) if order is None else order
    ks, ln, off, miss, sid = [], [], [], [], []
    for s in order:
        n, kmin, kmax, lmin, lmax = stretches[s]
        rng = np.random.default_rng([seed, s])
        k = rng.integers(kmin, kmax + 1, n)
        ks.append(k)
        ln.append(rng.integers(lmin, lmax + 1, int(k.sum())).astype(np.uint16))
        off.append(rng.integers(0, arena - MAX_PACKET, int(k.sum())).astype(np.uint64))
        miss.append((rng.integers(0, 1 << 30, n) % k).astype(np.uint8))
        sid.append(np.full(n, s))
    ks = np.concatenate(ks)
    ptr = np.zeros(ks.size + 1, np.uint32)
    ptr[1:] = np.cumsum(ks)
    data = np.random.default_rng([seed, 99]).integers(0, 256, arena, dtype=np.uint8)
    return dict(data=data, pkt_off=np.concatenate(off), pkt_len=np.concatenate(ln), grp_ptr=ptr,
                missing=np.concatenate(miss), ks=ks, stretch=np.concatenate(sid))


def from_groups(groups, seed, missing=None):
    """A small batch from explicit packet lengths per group, over a gapped,
    unaligned arena of its own."""
    rng = np.random.default_rng(seed)
    ln = np.array([l for g in groups for l in g], np.uint16)
    ks = np.array([len(g) for g in groups])
    ptr = np.zeros(len(groups) + 1, np.uint32)
    ptr[1:] = np.cumsum(ks)
    off = np.zeros(ln.size, np.uint64)
    off[1:] = np.cumsum(ln[:-1].astype(np.uint64) + rng.integers(0, 40, ln.size - 1).astype(np.uint64))
    data = rng.integers(0, 256, int(off[-1]) + int(ln[-1]) + 7, dtype=np.uint8)
    if missing is None:
        missing = (rng.integers(0, 1 << 30, ks.size) % ks).astype(np.uint8)
    return dict(data=data, pkt_off=off, pkt_len=ln, grp_ptr=ptr,
                missing=np.asarray(missing, np.uint8), ks=ks, stretch=np.zeros(ks.size, np.int64))


def slot_offsets(n, seed):
    """parity_off / out_off: a random permutation of n SLOT_BYTES slots from an
    odd base, so the scatter order is not the group order; and the buffer size"""
    perm = np.random.default_rng([seed, 7]).permutation(n).astype(np.uint64)
    return perm * np.uint64(SLOT_BYTES) + np.uint64(SLOT_BASE), n * SLOT_BYTES + SLOT_BASE


def parity_lengths(b):
    """the encode's parity_len_out: the longest packet of every group"""
    return group_sums(b["pkt_len"], b["grp_ptr"])[2].astype(np.uint16)


def recover_offsets(b):
    """pkt_off with every lost packet's entry far outside the arena"""
    off = b["pkt_off"].copy()
    off[b["grp_ptr"][:-1].astype(np.int64) + b["missing"]] = FAR_OFF
    return off


def staged_bytes(b, recover):
    """(input bytes, output bytes) a call must stage whatever its plan: the
    packets it reads (recover: the received ones plus the redundancy) and the
    parity_len[g] bytes per group it returns"""
    _, gb, mx = group_sums(b["pkt_len"], b["grp_ptr"], b["missing"] if recover else None)
    return int(gb.sum()) + (int(mx.sum()) if recover else 0), int(mx.sum())


def plans(b):
    """the modelled plan of the encode and of the recover from its outputs"""
    return (plan_ragged(b["pkt_len"], b["grp_ptr"]),
            plan_ragged(b["pkt_len"], b["grp_ptr"], True, b["missing"], parity_lengths(b)))


# the large ragged batches of tests/test_hip_host_ragged.py: (seed, order)
LARGE = {"forward": (1, (0, 1, 2)),   # input-budget chunks first
         "reverse": (2, (2, 1, 0))}   # tiny groups first: every stretch meets another slot


def large(name):
    seed, order = LARGE[name]
    return ragged_batch(seed, order=order)


# ---- fixed shapes past the slot rotation ----------------------------------------
# Full-size rows (L = 1,452) make the cheapest chunks: the recover's aux budget
# holds AUX_STAGE // 1453 = 5,773 groups whatever k is, the encode's output
# budget OUT_STAGE // 1452 = 11,554.  n = SLOTS * cg + a few: SLOTS full chunks
# and a tail of a few groups, which is gathered into slot 0 after its first
# chunk left it and leaves nearly all of that chunk's bytes stale behind it.
# k = 2 keeps a test's pinned buffers near 100 MB (rows 2 x 25 MB, parity and
# output 25 MB each); the pageable case affords k = 3.  The encode needs twice
# the groups for a fourth chunk: k = 1 keeps its pinned case at 2 x 51 MB.
FIXED_L = MAX_PACKET
FIXED_ROW_STRIDE = 1456    # > L
FIXED_FREE_EXTRA = 48      # group_stride = k * row_stride + 48
FIXED_OUT_STRIDE = 1460    # > L, parity and output
N_RECOVER = SLOTS * 5_773 + 5
N_ENCODE = SLOTS * 11_554 + 7
# name: (recover, k, n, rows way); rows ways as in tests/test_hip_host_fixed.py
FIXED_MULTI = {
    "recover-pinned-uniform": (True, 2, N_RECOVER, "pinned-uniform"),
    "recover-pinned-free": (True, 2, N_RECOVER, "pinned-free"),
    "recover-pageable-strided": (True, 3, N_RECOVER, "pageable-free"),
    "encode-pinned-uniform": (False, 1, N_ENCODE, "pinned-uniform"),
    "encode-pageable-strided": (False, 2, N_ENCODE, "pageable-free"),
}


def row_strides(way, k, L, row_stride=None):
    """(row_stride, group_stride) of a way to lay the rows out"""
    rs = (L + 4 if row_stride is None else row_stride)
    layout = way.split("-", 1)[1]
    if layout == "packed":
        return L, k * L
    if layout == "uniform":
        return rs, k * rs
    if layout == "free":
        return rs, k * rs + FIXED_FREE_EXTRA
    if layout == "rowpacked":          # rows back to back, groups apart
        return L, k * L + FIXED_FREE_EXTRA
    raise ValueError(way)


def fixed_multi(name):
    recover, k, n, way = FIXED_MULTI[name]
    rs, gs = row_strides(way, k, FIXED_L, FIXED_ROW_STRIDE)
    return dict(recover=recover, k=k, L=FIXED_L, n=n, way=way, row_stride=rs, group_stride=gs,
                parity_stride=FIXED_OUT_STRIDE, out_stride=FIXED_OUT_STRIDE,
                cg=fixed_chunk_groups(FIXED_L, gs, recover))
