// qturn_kernels.hip — gfx950 (CDNA4) kernels for the table passes of the
// receiver's turn: what a turn decides about its packets and groups before and
// after the XOR kernels (qfec_kernels.hip) touch the payloads.  Most of these
// passes read no packet byte.
//
//  * Revive from receive maps (qfec_revive_batch): classify / scan / emit build
//    a packed list of the revivable groups on the device, and the recover
//    body runs over that list only (revive_xor_kernel, qfec_kernels.hip); for
//    ragged batches (qfec_revive_ragged) the same three kernels with k per
//    group and the ragged block body over the list (revive_ragged_kernel); for
//    the receiver's close (qfec_revive_accumulated) with k per group from
//    group_k and the gather over the list (close_gather_kernel).  The three
//    passes are launch_revive_passes below; the kernel over the list is
//    launched by its caller in qfec_kernels.hip.
//  * The receive maps on the device (qfec_admit_ragged / qfec_revive_tracked):
//    one running map per slot; decide / scan / scatter filter a turn's
//    candidates against it and the open call's ok flags into the tables the
//    accumulate folds (admit_*_kernel), and the receiver's close reads K and
//    the map by slot (the classify kernels instantiated for TrackedCloseArgs).
//  * The rest of the turn, a section each below: a turn's CSR tables
//    (qfec_bin_arrivals), each packet's group found or opened
//    (qfec_assign_slots), retention and forced closes (qfec_retire_groups),
//    the private headers parsed and written (qfec_parse_opened,
//    qfec_write_private_headers), the ack state and its wire bytes
//    (qfec_record_received, qfec_build_acks, qfec_write_ack_frames) and the
//    frame walk (qfec_scan_frames).
#include "qfec_device.h"

#include <algorithm>

namespace qfec {
namespace {

// ---------------------------------------------------------------------------
// Workgroup primitives of the turn passes.
// ---------------------------------------------------------------------------
// The scans, sums and ranks in which the passes of the receiver's turn (revive,
// admit, bin, assign) are written; the first four (lane_id, lane_read,
// wave_incl_scan, block_excl_scan) are in qfec_device.h, because the ragged
// kernels use them too.  One contract for all of them: they are called from
// block-uniform control flow with every lane of every wave active (they
// shuffle, ballot or meet at a barrier), lane and wave are tid & 63 and
// tid >> 6, and they shift 32-bit words only (the gfx950 64-bit shift hazard,
// DESIGN.md §4).  One that takes an LDS array s_w ends with the barrier that
// makes s_w free again: the caller puts none between two of them.
constexpr int kTurnWaves = kReviveTile / 64;  // waves of a per-tile or per-packet workgroup
constexpr int kRvScanBlock = 1024;            // lanes of a one-workgroup scan kernel

// put(i, the sum of get(0 .. i - 1)) for every i < n by one workgroup of
// kRvScanBlock lanes, a trip per kRvScanBlock elements with the running base in
// a register; returns the sum of all.  An element is a 32-bit count and so is
// the sum of a trip; s_w: kRvScanBlock / 64 words.  get(i) is called exactly
// once for every i < n, by the lane that then puts i and before it does: in
// place is fine, and a get may keep sums of its own per lane on the way (the
// side totals of the revive's and the admit's scan).  No barrier if n == 0.
template <typename Get, typename Put>
__device__ __forceinline__ uint64_t tile_scan(uint64_t n, uint32_t* s_w, Get get, Put put) {
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  uint64_t base = 0;
  for (uint64_t t0 = 0; t0 < n; t0 += kRvScanBlock) {
    const uint64_t i = t0 + tid;
    uint32_t tot;
    const uint32_t before =
        block_excl_scan<kRvScanBlock / 64>(i < n ? get(i) : 0u, lane, wave, s_w, tot);
    if (i < n) put(i, base + before);
    base += tot;
  }
  return base;
}
// ... over the n words of v in place (sums that fit 32 bits: packets or slots)
__device__ __forceinline__ uint32_t tile_scan_in_place(uint32_t* v, uint64_t n, uint32_t* s_w) {
  return (uint32_t)tile_scan(
      n, s_w, [=](uint64_t i) { return v[i]; }, [=](uint64_t i, uint64_t x) { v[i] = (uint32_t)x; });
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

// Every wave of a kTurnWaves-wave workgroup brings CH counts (uniform in the
// wave: ballot popcounts, wave_sums); lane ch < CH of every wave gets the
// workgroup's sum of count ch (the lanes above it that of the last: a clamped
// read, not a masked one).  s_w: kTurnWaves * CH words.
template <int CH>
__device__ __forceinline__ uint32_t block_sum(const uint32_t (&c)[CH], uint32_t lane,
                                              uint32_t wave, uint32_t* s_w) {
  if (lane == 0u) {
#pragma unroll
    for (int ch = 0; ch < CH; ++ch) s_w[wave * CH + ch] = c[ch];
  }
  __syncthreads();
  const uint32_t ch = min(lane, (uint32_t)(CH - 1));
  uint32_t t = 0;
#pragma unroll
  for (int w = 0; w < kTurnWaves; ++w) t += s_w[w * CH + ch];
  __syncthreads();  // s_w free again
  return t;
}
__device__ __forceinline__ uint32_t block_sum(uint32_t c, uint32_t lane, uint32_t wave,
                                              uint32_t* s_w) {
  const uint32_t one[1] = {c};
  return block_sum(one, lane, wave, s_w);
}

// The set bits of ballot b below this lane (v_mbcnt: no shift, no lane).
__device__ __forceinline__ uint32_t ballot_rank(uint64_t b) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32),
                                   __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
}

// ... and below it in the whole kTurnWaves-wave workgroup, b being each wave's
// ballot of one predicate; total: the workgroup's set bits.
__device__ __forceinline__ uint32_t block_ballot_rank(uint64_t b, uint32_t lane, uint32_t wave,
                                                      uint32_t* s_w, uint32_t& total) {
  if (lane == 0u) s_w[wave] = (uint32_t)__popcll(b);
  __syncthreads();
  uint32_t r = ballot_rank(b), tot = 0;
#pragma unroll
  for (int w = 0; w < kTurnWaves; ++w) {
    const uint32_t v = s_w[w];
    r += (uint32_t)w < wave ? v : 0u;
    tot += v;
  }
  total = tot;
  __syncthreads();  // s_w free again
  return r;
}
__device__ __forceinline__ uint32_t block_ballot_rank(uint64_t b, uint32_t lane, uint32_t wave,
                                                      uint32_t* s_w) {
  uint32_t total;
  return block_ballot_rank(b, lane, wave, s_w, total);
}

// Runs of neighbouring lanes with one key, so that a run's first lane can make
// one atomic or one probe for all of it.  eligible: the lane takes part; same:
// its key equals that of the lane below.  THE RULE for `same`: every lane
// executes every shuffle before anything is compared.  A __shfl_up under the &&
// of a comparison, or under `eligible`, runs only in the lanes that got that
// far and reads 0 from a neighbour that is not among them, which equals the
// high half of a small key: 4 of 81,999 packets took the wrong slot that way.
// head: the lane is the first of a run; first: the head of the lane's run (its
// last head at or below); end: the lane after the run (the next head or
// ineligible lane, or 64).  first and end mean something in eligible lanes only.
struct LaneRun {
  bool head;
  uint32_t first, end;
};
__device__ __forceinline__ LaneRun lane_runs(bool eligible, bool same, uint32_t lane) {
  LaneRun r;
  r.head = eligible && (lane == 0u || !same);
  const uint64_t heads = __ballot(r.head), enders = heads | ~__ballot(eligible);
  // the lanes at or below this one, as 32-bit words
  const uint32_t m_lo = lane < 32u ? (2u << lane) - 1u : 0xFFFFFFFFu;
  const uint32_t m_hi = lane < 32u ? 0u : (2u << (lane - 32u)) - 1u;
  const uint32_t h_lo = (uint32_t)heads & m_lo, h_hi = (uint32_t)(heads >> 32) & m_hi;
  const uint32_t e_lo = (uint32_t)enders & ~m_lo, e_hi = (uint32_t)(enders >> 32) & ~m_hi;
  r.first = h_hi ? 63u - (uint32_t)__builtin_clz(h_hi)
                 : (h_lo ? 31u - (uint32_t)__builtin_clz(h_lo) : 0u);
  r.end = e_lo ? (uint32_t)__builtin_ctz(e_lo)
               : (e_hi ? 32u + (uint32_t)__builtin_ctz(e_hi) : 64u);
  return r;
}
static_assert(kReviveTile % 64 == 0 && kRvScanBlock % 64 == 0, "whole waves");

// ---------------------------------------------------------------------------
// Revive from per-group receive maps (qfec_revive_batch).
// ---------------------------------------------------------------------------
// A batch in which most groups need nothing: classify every group from its
// receive map (k + 1 bits), then run the recover body over a packed work list
// of the revivable groups only, so the HBM traffic is that of the revived
// groups plus the maps.  Four kernels on the stream, ordered by the kernel
// boundaries alone -- no workgroup ever waits on another:
//   classify : one lane per group, status / revived_idx out, each tile of 256
//              groups leaves its revived and complete counts (ballots) in
//              scratch;
//   scan     : one workgroup, an exclusive scan over the tile counts: every
//              tile's position in the work list, and the three totals;
//   emit     : the classification again (the maps are 2 B per group at
//              k = 10), every revived group's (g, m) into the work list and g
//              into revived_list at its scanned position: ascending, no sort;
//   revive   : fixed_xor_kernel's recover body with g and m from work-list
//              entry i, a grid-stride loop over the list whose length the
//              kernel reads from scratch (the host never learns it).

// Status of the group whose map starts at mp; m: its one clear data bit
// (revived groups only, else 0xFF).  All shifts are 32-bit (the gfx950 64-bit
// shift hazard).
__device__ __forceinline__ uint32_t revive_classify(const uint8_t* mp, uint32_t k, uint32_t& m) {
  uint32_t miss, first, fec;
  if (k < 64u) {
    // k + 1 <= 64 bits: the map as two 32-bit words
    const uint32_t nb = k / 8u + 1u;
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (uint32_t j = 0; j < 8u; ++j) {
      const uint32_t b = j < nb ? (uint32_t)mp[j] : 0u;
      if (j < 4u) lo |= b << (8u * j);
      else hi |= b << (8u * (j - 4u));
    }
    const uint32_t lom = k >= 32u ? 0xFFFFFFFFu : (1u << k) - 1u;
    const uint32_t him = k > 32u ? (1u << (k - 32u)) - 1u : 0u;
    const uint32_t zl = ~lo & lom, zh = ~hi & him;
    miss = __popc(zl) + __popc(zh);
    first = zl ? (uint32_t)__builtin_ctz(zl) : 32u + (zh ? (uint32_t)__builtin_ctz(zh) : 0u);
    fec = k < 32u ? (lo >> k) & 1u : (hi >> (k - 32u)) & 1u;
  } else {
    miss = 0;
    first = 0;
    const uint32_t nfull = k / 8u, rem = k % 8u;
    for (uint32_t b = 0; b < nfull; ++b) {
      const uint32_t z = ~(uint32_t)mp[b] & 0xFFu;
      if (z != 0u && miss == 0u) first = 8u * b + (uint32_t)__builtin_ctz(z);
      miss += __popc(z);
    }
    const uint32_t last = mp[nfull];
    const uint32_t z = ~last & ((1u << rem) - 1u);
    if (z != 0u && miss == 0u) first = 8u * nfull + (uint32_t)__builtin_ctz(z);
    miss += __popc(z);
    fec = (last >> rem) & 1u;
  }
  m = 0xFFu;
  if (miss == 0u) return kGroupComplete;
  if (miss == 1u && fec != 0u) {
    m = first;
    return kGroupRevived;
  }
  return kGroupUnrevivable;
}

// EMIT = false: status, revived_idx and the tile's counts.  EMIT = true: the
// work list and revived_list, at tile_off[tile] + the group's rank among the
// tile's revived groups (wave ballots, the waves' counts through LDS).
// Args: ReviveArgs (one k for the batch, every group legal) or
// ReviveRaggedArgs (k per group from grp_ptr; a group of 0 or more than 255
// packets, or whose k + 1 bits do not fit map_stride, is unrevivable and
// latches kErrGroupSize -- its map is not read).
__device__ __forceinline__ bool revive_group_k(const ReviveArgs& a, uint64_t, uint32_t& k) {
  k = a.k;
  return true;
}
__device__ __forceinline__ bool revive_group_k(const ReviveRaggedArgs& a, uint64_t g,
                                               uint32_t& k) {
  k = a.grp_ptr[g + 1] - a.grp_ptr[g];  // a non-monotone grp_ptr shows up as k > 255
  return k >= 1u && k <= 255u && (uint64_t)(k / 8u + 1u) <= a.map_stride;
}
__device__ __forceinline__ void revive_bad_group(const ReviveArgs&, uint64_t) {}
__device__ __forceinline__ void revive_bad_group(const ReviveRaggedArgs& a, uint64_t) {
  atomicOr(a.err, kErrGroupSize);
}
// The EMIT pass's look at every group of the batch (st 3: past it); returns
// bits to OR into a revived group's work-list entry.  Nothing for the two
// revives above.
__device__ __forceinline__ uint64_t revive_emit_group(const ReviveArgs&, uint64_t, uint32_t) {
  return 0ull;
}
__device__ __forceinline__ uint64_t revive_emit_group(const ReviveRaggedArgs&, uint64_t,
                                                      uint32_t) {
  return 0ull;
}

// CloseArgs (qfec_revive_accumulated): k per group from group_k; a group whose
// slot is out of range (kErrMissingIndex), whose k is 0 or whose k + 1 bits do
// not fit map_stride (kErrGroupSize) is unrevivable -- its map and its slot's
// length are not read.  (close_slot, the group's slot: qfec_device.h, the
// gather uses it too.)
__device__ __forceinline__ bool close_k_ok(const CloseArgs& a, uint32_t k) {
  return k >= 1u && (uint64_t)(k / 8u + 1u) <= a.map_stride;
}
__device__ __forceinline__ bool revive_group_k(const CloseArgs& a, uint64_t g, uint32_t& k) {
  k = a.group_k[g];
  return close_slot(a, g) < a.n_slots && close_k_ok(a, k);
}
__device__ __forceinline__ void revive_bad_group(const CloseArgs& a, uint64_t g) {
  if (close_slot(a, g) >= a.n_slots) atomicOr(a.err, kErrMissingIndex);
  if (!close_k_ok(a, a.group_k[g])) atomicOr(a.err, kErrGroupSize);
}
// Where a valid group's map starts: by group for the three argument structs
// above, by slot for TrackedCloseArgs.
template <typename Args>
__device__ __forceinline__ const uint8_t* revive_map(const Args& a, uint64_t g) {
  return a.received + g * a.map_stride;
}

// TrackedCloseArgs (qfec_revive_tracked): CloseArgs's rules with K =
// group_k[s] and the map of slot s.  A slot out of range (kErrMissingIndex; K,
// map and length not read) or a bad K (kErrGroupSize; map and length not read)
// is unrevivable, and so is a FRESH slot, acc_len[s] == 0: its map counts as
// all clear whatever it holds, which is no error and is not read either.
__device__ __forceinline__ bool revive_group_k(const TrackedCloseArgs& a, uint64_t g,
                                               uint32_t& k) {
  const uint32_t s = close_slot(a, g);
  k = 0;
  if (s >= a.n_slots) return false;
  k = a.group_k[s];
  return close_k_ok(a, k) && a.acc_len[s] != 0;
}
__device__ __forceinline__ void revive_bad_group(const TrackedCloseArgs& a, uint64_t g) {
  const uint32_t s = close_slot(a, g);
  if (s >= a.n_slots) atomicOr(a.err, kErrMissingIndex);
  else if (!close_k_ok(a, a.group_k[s])) atomicOr(a.err, kErrGroupSize);
}
__device__ __forceinline__ const uint8_t* revive_map(const TrackedCloseArgs& a, uint64_t g) {
  return a.received + (uint64_t)close_slot(a, g) * a.map_stride;
}

// The K of group g, which sits in slot s: the one thing the EMIT pass below
// reads differently for the two closes.
__device__ __forceinline__ uint32_t close_group_k(const CloseArgs& a, uint64_t g, uint32_t) {
  return a.group_k[g];
}
__device__ __forceinline__ uint32_t close_group_k(const TrackedCloseArgs& a, uint64_t,
                                                  uint32_t s) {
  return a.group_k[s];
}
// The EMIT pass's look for CloseArgs and TrackedCloseArgs (the two revives
// further up have overloads of their own): out_len and the release, one lane
// per group.  A revived group's length is read here, ONCE, and travels in its
// work-list entry (the gather never reads acc_len), so the zero stored below
// cannot reach the copy.  A revived group whose length is 0 or above the limit
// latches kErrParityLength: out_len 0, entry length 0 (nothing copied), no
// release.  Invalid groups: out_len 0, no release.  A fresh slot of
// TrackedCloseArgs arrives here unrevivable, its length 0 already.
template <typename Args>
__device__ __forceinline__ uint64_t revive_emit_group(const Args& a, uint64_t g, uint32_t st) {
  if (st > kGroupUnrevivable) return 0ull;
  const uint32_t s = close_slot(a, g);
  uint32_t len = 0;
  if (s < a.n_slots && close_k_ok(a, close_group_k(a, g, s))) {
    bool ok = true;
    if (st == kGroupRevived) {
      const uint32_t l = a.acc_len[s];
      ok = l >= 1u && l <= a.lim;
      if (ok) len = l;
      else atomicOr(a.err, kErrParityLength);
    }
    if (ok && ((a.release >> st) & 1u) != 0u) a.acc_len[s] = 0;
  }
  a.out_len[g] = (uint16_t)len;
  return (uint64_t)len << kCloseLenShift;
}

template <bool EMIT, typename Args>
__global__ __launch_bounds__(kReviveTile) void revive_classify_kernel(Args a) {
  __shared__ uint32_t s_w[kTurnWaves];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint64_t ntile = (a.n_groups + kReviveTile - 1) / kReviveTile;
  for (uint64_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
    const uint64_t g = tile * kReviveTile + tid;
    uint32_t st = 3u, m = 0xFFu;  // 3: past the batch
    if (g < a.n_groups) {
      uint32_t k;
      if (revive_group_k(a, g, k)) {
        st = revive_classify(revive_map(a, g), k, m);
      } else {
        st = kGroupUnrevivable;
        if constexpr (!EMIT) revive_bad_group(a, g);
      }
    }
    const uint64_t brev = __ballot(st == kGroupRevived);
    if constexpr (!EMIT) {
      const uint64_t bcomp = __ballot(st == kGroupComplete);
      if (g < a.n_groups) {
        a.status[g] = (uint8_t)st;
        if (a.revived_idx) a.revived_idx[g] = (uint8_t)m;
      }
      const uint32_t t = block_sum(
          (uint32_t)__popcll(brev) | ((uint32_t)__popcll(bcomp) << 16), lane, wave, s_w);
      if (tid == 0u) a.tile_cnt[tile] = t;
    } else {
      // (its loads and stores go out in front of the rank's two barriers)
      const uint64_t ex = revive_emit_group(a, g, st);
      const uint32_t rank = block_ballot_rank(brev, lane, wave, s_w);
      if (st == kGroupRevived) {
        const uint64_t pos = a.tile_off[tile] + rank;
        a.work[pos] = (g << 8) | m | ex;
        if (a.revived_list) a.revived_list[pos] = g;
      }
    }
  }
}

// One workgroup: tile_off[i] = revived groups in tiles before i, then the
// totals.  The complete groups are a sum per lane, then per wave through s_w
// (a wave's sixteenth of the groups fits 32 bits: the work list of 2^36 groups
// would be 512 GiB).
template <typename Args>
__global__ __launch_bounds__(kRvScanBlock) void revive_scan_kernel(Args a) {
  __shared__ uint32_t s_w[kRvScanBlock / 64];
  const uint32_t tid = threadIdx.x;
  uint32_t comp = 0;
  const uint64_t base_rev = tile_scan(
      (a.n_groups + kReviveTile - 1) / kReviveTile, s_w,
      [&](uint64_t i) {
        const uint32_t c = a.tile_cnt[i];
        comp += c >> 16;
        return c & 0xFFFFu;
      },
      [&](uint64_t i, uint64_t x) { a.tile_off[i] = x; });
  comp = wave_sum(comp);
  if ((tid & 63u) == 0u) s_w[tid >> 6] = comp;
  __syncthreads();
  if (tid == 0u) {
    uint64_t base_comp = 0;
    for (uint32_t w = 0; w < kRvScanBlock / 64; ++w) base_comp += s_w[w];
    const uint64_t unrev = a.n_groups - base_rev - base_comp;
    a.totals[kGroupComplete] = base_comp;
    a.totals[kGroupRevived] = base_rev;
    a.totals[kGroupUnrevivable] = unrev;
    if (a.counts) {
      a.counts[kGroupComplete] = base_comp;
      a.counts[kGroupRevived] = base_rev;
      a.counts[kGroupUnrevivable] = unrev;
    }
  }
}

// ---------------------------------------------------------------------------
// Admission to running rows (qfec_admit_ragged): the group's received-packets
// set on the device, consulted before the fold.
// ---------------------------------------------------------------------------
// Three kernels on the stream, the pattern of the revive above (tile counts,
// a one-workgroup scan, ranks from the scanned counts); none reads a payload
// byte:
//   decide  : one lane per group walks its candidates in CSR order with the
//             slot's map (bits 0..K, all clear for a fresh slot) in eight LDS
//             words of its own: verdict[p], the group's admitted count, the
//             tile's four verdict counts, and the map back if anything was
//             admitted.  The first candidate of an index wins because the walk
//             is serial: deterministic, no sort, no atomics on the map;
//   scan    : one workgroup, an exclusive scan over the tiles' admitted
//             counts, the four totals and grp_ptr_out[n_groups];
//   scatter : a scan of the tile's 256 group counts gives grp_ptr_out[g]; the
//             lane walks its group's verdicts again and copies the admitted
//             packets' table entries in order.
// All map arithmetic is on 32-bit words (the gfx950 64-bit shift hazard).
constexpr uint32_t kPktAdmitted = 0, kPktFailed = 1, kPktDuplicate = 2, kPktInvalid = 3;
constexpr uint32_t kAdmitMapWords = 8;  // bits 0..K, K <= 255

__global__ __launch_bounds__(kReviveTile) void admit_decide_kernel(AdmitArgs a) {
  __shared__ uint32_t s_map[kAdmitMapWords][kReviveTile];  // word-major: no bank conflicts
  __shared__ uint32_t s_w[kTurnWaves * 4];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint64_t ntile = (a.n_groups + kReviveTile - 1) / kReviveTile;
  for (uint64_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
    const uint64_t g = tile * kReviveTile + tid;
    uint32_t c_adm = 0, c_fail = 0, c_dup = 0, c_inv = 0;
    if (g < a.n_groups) {
      const uint32_t p0 = a.grp_ptr[g];
      const uint32_t kg = a.grp_ptr[g + 1] - p0;  // a non-monotone grp_ptr shows up as kg > 255
      uint32_t bad = 0;
      if (kg > 255u) {
        bad = kErrGroupSize;  // its verdicts are not written
      } else {
        const uint32_t s = a.slot ? a.slot[g] : (uint32_t)g;
        uint32_t K = 0, old = 0;
        if (s >= a.n_slots) {
          bad = kErrMissingIndex;
        } else {
          K = a.slot_k[s];
          old = a.acc_len[s];
          if (K == 0u || (uint64_t)(K / 8u + 1u) > a.map_stride) bad |= kErrGroupSize;
          if (old > a.lim) bad |= kErrParityLength;
        }
        if (bad != 0u) {
          for (uint32_t j = 0; j < kg; ++j) a.verdict[p0 + j] = (uint8_t)kPktInvalid;
          c_inv = kg;
        } else {
          uint8_t* mp = a.acc_map + (uint64_t)s * a.map_stride;
          const uint32_t nb = K / 8u + 1u, nbit = K + 1u;
          // base: the map's bits 0..K, or nothing for a fresh slot
#pragma unroll
          for (uint32_t w = 0; w < kAdmitMapWords; ++w) {
            uint32_t x = 0;
            if (old != 0u && 4u * w < nb) {
#pragma unroll
              for (uint32_t b = 0; b < 4u; ++b)
                if (4u * w + b < nb) x |= (uint32_t)mp[4u * w + b] << (8u * b);
              if (nbit < 32u * w + 32u) x &= (1u << (nbit - 32u * w)) - 1u;  // shift 1..31
            }
            s_map[w][tid] = x;
          }
          uint32_t pkt_bad = 0;
          for (uint32_t j = 0; j < kg; ++j) {
            const uint32_t p = p0 + j;
            const uint32_t idx = a.pkt_idx[p], len = a.pkt_len[p];
            const uint32_t okp = a.pkt_ok ? (uint32_t)a.pkt_ok[p] : 1u;
            uint32_t e = 0;
            if (idx > K) e |= kErrMissingIndex;
            if (len == 0u || len > a.lim) e |= kErrPacketLength;
            uint32_t v;
            if (e != 0u) {
              v = kPktInvalid;
              pkt_bad |= e;
            } else if (okp == 0u) {
              v = kPktFailed;
            } else {
              const uint32_t w = idx >> 5, bit = 1u << (idx & 31u);
              const uint32_t cur = s_map[w][tid];
              v = (cur & bit) != 0u ? kPktDuplicate : kPktAdmitted;
              s_map[w][tid] = cur | bit;
            }
            a.verdict[p] = (uint8_t)v;
            c_adm += v == kPktAdmitted ? 1u : 0u;
            c_fail += v == kPktFailed ? 1u : 0u;
            c_dup += v == kPktDuplicate ? 1u : 0u;
            c_inv += v == kPktInvalid ? 1u : 0u;
          }
          if (c_adm != 0u)  // base | new, zero above bit K
            for (uint32_t b = 0; b < nb; ++b)
              mp[b] = (uint8_t)(s_map[b >> 2][tid] >> (8u * (b & 3u)));
          if (pkt_bad != 0u) atomicOr(a.err, pkt_bad);
        }
      }
      if (bad != 0u) atomicOr(a.err, bad);
      a.grp_cnt[g] = c_adm;
    }
    // (in the order of the verdicts: kPktAdmitted, Failed, Duplicate, Invalid)
    const uint32_t c[4] = {wave_sum(c_adm), wave_sum(c_fail), wave_sum(c_dup), wave_sum(c_inv)};
    const uint32_t t = block_sum(c, lane, wave, s_w);
    if (tid < 4u) a.tile_v[tile * 4u + tid] = t;
  }
}

// One workgroup: tile_off[i] = packets admitted in the tiles before i, then
// the totals.  The other three verdicts are sums per lane, met in LDS at the end.
__global__ __launch_bounds__(kRvScanBlock) void admit_scan_kernel(AdmitArgs a) {
  __shared__ uint32_t s_w[kRvScanBlock / 64];
  __shared__ unsigned long long s_tot[3];
  const uint32_t tid = threadIdx.x;
  if (tid < 3u) s_tot[tid] = 0ull;  // (the scan's barriers lie between this and the
                                    // sums: n_groups > 0, the launcher's guard)
  uint64_t fail = 0, dup = 0, inv = 0;
  const uint64_t base = tile_scan(
      (a.n_groups + kReviveTile - 1) / kReviveTile, s_w,
      [&](uint64_t i) {
        fail += a.tile_v[i * 4u + kPktFailed];
        dup += a.tile_v[i * 4u + kPktDuplicate];
        inv += a.tile_v[i * 4u + kPktInvalid];
        return a.tile_v[i * 4u + kPktAdmitted];
      },
      [&](uint64_t i, uint64_t x) { a.tile_off[i] = x; });
  if (fail != 0ull) atomicAdd(&s_tot[0], (unsigned long long)fail);
  if (dup != 0ull) atomicAdd(&s_tot[1], (unsigned long long)dup);
  if (inv != 0ull) atomicAdd(&s_tot[2], (unsigned long long)inv);
  __syncthreads();
  if (tid == 0u) {
    a.grp_ptr_out[a.n_groups] = (uint32_t)base;
    if (a.counts) {
      a.counts[kPktAdmitted] = base;
      a.counts[kPktFailed] = s_tot[0];
      a.counts[kPktDuplicate] = s_tot[1];
      a.counts[kPktInvalid] = s_tot[2];
    }
  }
}

// grp_ptr_out[g] and the admitted packets' table entries, stable.  `room`:
// the candidates the tables list, grp_ptr[n_groups] - grp_ptr[0] -- with a
// grp_ptr that is not monotone (latched by the decide pass) the valid groups
// can claim more, and no entry is written past it.
__global__ __launch_bounds__(kReviveTile) void admit_scatter_kernel(AdmitArgs a) {
  __shared__ uint32_t s_w[kTurnWaves];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint64_t ntile = (a.n_groups + kReviveTile - 1) / kReviveTile;
  const uint32_t room = a.grp_ptr[a.n_groups] - a.grp_ptr[0];
  for (uint64_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
    const uint64_t g = tile * kReviveTile + tid;
    const uint32_t cnt = g < a.n_groups ? a.grp_cnt[g] : 0u;
    uint32_t tot;
    const uint32_t pos =
        (uint32_t)a.tile_off[tile] + block_excl_scan<kTurnWaves>(cnt, lane, wave, s_w, tot);
    uint32_t p0 = 0, kg = 0;
    if (g < a.n_groups) {
      a.grp_ptr_out[g] = pos;
      p0 = a.grp_ptr[g];
      kg = a.grp_ptr[g + 1] - p0;
    }
    // Every group of the tile valid in size: their candidates are one
    // contiguous run of the tables, each with a verdict, and an admitted
    // packet's place is the tile's plus the admitted packets before it in the
    // run -- one lane per PACKET, loads and stores coalesced (a lane per group
    // touches a cache line per lane and store: 6x the time on 2^20 groups).
    if (__syncthreads_and(kg <= 255u ? 1 : 0)) {  // (the vote; s_w is free since the scan)
      const uint64_t gend = min((tile + 1) * (uint64_t)kReviveTile, a.n_groups);
      const uint32_t first = a.grp_ptr[tile * kReviveTile], end = a.grp_ptr[gend];
      uint32_t base = (uint32_t)a.tile_off[tile];
      for (uint64_t q = first; q < end; q += kReviveTile) {  // (uniform; 64-bit: no wrap)
        const uint64_t p = q + tid;
        const bool adm = p < end && a.verdict[p] == (uint8_t)kPktAdmitted;
        const uint32_t r = base + block_ballot_rank(__ballot(adm), lane, wave, s_w, tot);
        if (adm && r < room) {
          a.pkt_off_out[r] = a.pkt_off[p];
          a.pkt_len_out[r] = a.pkt_len[p];
        }
        base += tot;
      }
    } else {
      // a group of more than 255 candidates in the tile (its verdicts are not
      // written, and grp_ptr need not be monotone around it): group by group
      if (cnt != 0u) {
        for (uint32_t j = 0, r = 0; j < kg && r < cnt; ++j) {
          if (a.verdict[p0 + j] != (uint8_t)kPktAdmitted) continue;
          if (pos + r < room) {
            a.pkt_off_out[pos + r] = a.pkt_off[p0 + j];
            a.pkt_len_out[pos + r] = a.pkt_len[p0 + j];
          }
          ++r;
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Arrival order to per-slot CSR tables (qfec_bin_arrivals): a stable counting
// sort keyed by slot, in front of the admit.
// ---------------------------------------------------------------------------
// Six kernels on the stream behind one memset of the tallies and the per-slot
// counters; none reads a payload byte or dereferences pkt_off:
//   count   : one lane per packet classifies its slot (none, out of range,
//             binned) and takes a provisional rank from an atomic on the slot's
//             counter, one atomic per run of neighbouring lanes with one
//             slot; the three tallies per wave by ballot, per workgroup
//             through LDS, one atomic per workgroup and class;
//   tile    : the sum of every tile of kReviveTile slot counters;
//   scan    : one workgroup, an exclusive scan over the tile sums in place,
//             grp_ptr_out[n_slots] and counts;
//   ptr     : a scan of the tile's 256 counters gives grp_ptr_out[s];
//   scatter : one lane per packet, ONE aligned 16-B record (off, len | idx <<
//             16 | ok << 24, p) to scratch at grp_ptr_out[s] + provisional rank;
//   order   : a workgroup per tile of slots owns one contiguous run of
//             records: one lane per RECORD finds its slot by bisection over the
//             tile's 257 pointers in LDS, its final rank as the number of
//             records of the slot with a smaller p (segments of at most 255;
//             longer ones stay as they lie: nothing here grows faster than the
//             segment), and writes the five tables.
// The atomics decide only the provisional place inside a segment; the order
// pass removes that freedom.  Every index formed from pkt_slot is checked
// against n_slots first, and every place against n_packets.
__global__ __launch_bounds__(kReviveTile) void bin_count_kernel(BinArgs a) {
  __shared__ uint32_t s_w[kTurnWaves * 3];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  uint32_t n[3] = {0, 0, 0};  // the wave's binned, slotless and out-of-range packets (uniform)
  const uint64_t step = (uint64_t)gridDim.x * kReviveTile;
  for (uint64_t p0 = (uint64_t)blockIdx.x * kReviveTile; p0 < a.n_packets; p0 += step) {
    const uint64_t p = p0 + tid;
    const bool in = p < a.n_packets;
    const uint32_t s = a.pkt_slot[in ? p : a.n_packets - 1u];  // (clamped, not masked)
    const bool binned = in && s < a.n_slots;
    const bool none = in && s == kBinNoSlot;
    const bool bad = in && !binned && !none;
    // One atomic per RUN of neighbouring lanes with one slot (a burst of one
    // group's packets), taken by the run's first lane for all of it: arrivals
    // already grouped cost a tenth of the atomics, a random order what it did.
    // (a binned lane's slot differs from any lane's that is not binned)
    const uint32_t prev = __shfl_up(s, 1);
    const LaneRun run = lane_runs(binned, prev == s, lane);
    uint32_t base = 0;
    if (run.head) base = atomicAdd(&a.cnt[s], run.end - lane);
    base = __shfl(base, run.first);
    if (binned) a.rank[p] = base + (lane - run.first);
    n[0] += (uint32_t)__popcll(__ballot(binned));
    n[1] += (uint32_t)__popcll(__ballot(none));
    n[2] += (uint32_t)__popcll(__ballot(bad));
  }
  const uint32_t t = block_sum(n, lane, wave, s_w);
  if (tid < 3u) {
    if (t != 0u) atomicAdd(&a.tally[tid], (unsigned long long)t);
    if (tid == 2u && t != 0u) atomicOr(a.err, kErrMissingIndex);
  }
}

__global__ __launch_bounds__(kReviveTile) void bin_tile_kernel(BinArgs a) {
  __shared__ uint32_t s_w[kTurnWaves];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint64_t ntile = ((uint64_t)a.n_slots + kReviveTile - 1) / kReviveTile;
  for (uint64_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
    const uint64_t s = tile * kReviveTile + tid;
    const uint32_t t = block_sum(wave_sum(s < a.n_slots ? a.cnt[s] : 0u), lane, wave, s_w);
    if (tid == 0u) a.tile_off[tile] = t;
  }
}

// One workgroup: tile_off[i] = packets binned to the tiles before i (in place
// over the tile sums), then the totals.  All sums fit 32 bits: n_packets < 2^32.
__global__ __launch_bounds__(kRvScanBlock) void bin_scan_kernel(BinArgs a) {
  __shared__ uint32_t s_w[kRvScanBlock / 64];
  const uint32_t base = tile_scan_in_place(
      a.tile_off, ((uint64_t)a.n_slots + kReviveTile - 1) / kReviveTile, s_w);
  if (threadIdx.x == 0u) {
    a.grp_ptr_out[a.n_slots] = base;
    if (a.counts) {
      a.counts[0] = a.tally[0];
      a.counts[1] = a.tally[1];
      a.counts[2] = a.tally[2];
    }
  }
}

__global__ __launch_bounds__(kReviveTile) void bin_ptr_kernel(BinArgs a) {
  __shared__ uint32_t s_w[kTurnWaves];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint64_t ntile = ((uint64_t)a.n_slots + kReviveTile - 1) / kReviveTile;
  for (uint64_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
    const uint64_t s = tile * kReviveTile + tid;
    uint32_t tot;
    const uint32_t before =
        block_excl_scan<kTurnWaves>(s < a.n_slots ? a.cnt[s] : 0u, lane, wave, s_w, tot);
    if (s < a.n_slots) a.grp_ptr_out[s] = a.tile_off[tile] + before;
  }
}

__global__ __launch_bounds__(kReviveTile) void bin_scatter_kernel(BinArgs a) {
  const uint32_t tid = threadIdx.x;
  const uint64_t step = (uint64_t)gridDim.x * kReviveTile;
  for (uint64_t p0 = (uint64_t)blockIdx.x * kReviveTile; p0 < a.n_packets; p0 += step) {
    const uint64_t p = p0 + tid;
    const bool in = p < a.n_packets;
    const uint64_t pc = in ? p : a.n_packets - 1u;  // (clamped, not masked)
    const uint32_t s = a.pkt_slot[pc];
    const uint64_t off = a.pkt_off[pc];
    const uint32_t len = a.pkt_len[pc], idx = a.pkt_idx[pc];
    const uint32_t okp = a.pkt_ok ? (uint32_t)a.pkt_ok[pc] : 0u;
    if (in && s < a.n_slots) {
      const uint64_t pos = (uint64_t)a.grp_ptr_out[s] + a.rank[p];
      if (pos < a.n_packets)
        a.rec[pos] = make_uint4((uint32_t)off, (uint32_t)(off >> 32), len | (idx << 16) | (okp << 24),
                                (uint32_t)p);
    }
  }
}

__global__ __launch_bounds__(kReviveTile) void bin_order_kernel(BinArgs a) {
  __shared__ uint32_t s_ptr[kReviveTile + 1];
  const uint32_t tid = threadIdx.x;
  const uint64_t ntile = ((uint64_t)a.n_slots + kReviveTile - 1) / kReviveTile;
  for (uint64_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
    // (slots past n_slots: empty segments at the run's end)
    s_ptr[tid] = a.grp_ptr_out[min(tile * kReviveTile + tid, (uint64_t)a.n_slots)];
    if (tid == 0u)
      s_ptr[kReviveTile] = a.grp_ptr_out[min((tile + 1) * kReviveTile, (uint64_t)a.n_slots)];
    __syncthreads();
    const uint32_t first = s_ptr[0];
    const uint32_t end = min(s_ptr[kReviveTile], (uint32_t)a.n_packets);
    for (uint64_t q = (uint64_t)first + tid; q < end; q += kReviveTile) {
      uint32_t lo = 0, hi = kReviveTile;  // s_ptr[lo] <= q < s_ptr[hi]
#pragma unroll
      for (uint32_t i = 0; i < 8u; ++i) {
        const uint32_t mid = (lo + hi) >> 1;
        if (s_ptr[mid] <= (uint32_t)q) lo = mid;
        else hi = mid;
      }
      const uint32_t seg = s_ptr[lo], k = s_ptr[lo + 1u] - seg;
      const uint4 r = a.rec[q];
      uint32_t place = (uint32_t)q;
      if (k <= 255u) {
        uint32_t before = 0;
        for (uint32_t j = 0; j < k; ++j) before += a.rec[seg + j].w < r.w ? 1u : 0u;
        place = seg + before;
      }
      a.pkt_off_out[place] = (uint64_t)r.x | ((uint64_t)r.y << 32);
      a.pkt_len_out[place] = (uint16_t)r.z;
      a.pkt_idx_out[place] = (uint8_t)(r.z >> 16);
      if (a.pkt_ok) a.pkt_ok_out[place] = (uint8_t)(r.z >> 24);
      if (a.src_out) a.src_out[place] = r.w;
    }
    __syncthreads();  // s_ptr is reused by the next tile
  }
}
static_assert(kReviveTile == 256, "eight bisection steps");

// ---------------------------------------------------------------------------
// Group keys to slots (qfec_assign_slots): find each packet's open group or
// open one in a free slot, in front of the bin.
// ---------------------------------------------------------------------------
// Seven kernels on the stream behind one memset to 0xFF of an open-addressing
// table that lives for this call only (entry: 64-bit key, 32-bit value, 32-bit
// first arrival; all ones = empty, and QFEC_NO_KEY is never inserted):
//   slots : one lane per slot; an open slot (acc_len > 0) inserts its key and
//           takes atomicMin(value, s), so the lowest slot wins; the free slots
//           of every tile are counted; workgroup 0 zeroes counts;
//   probe : one lane per packet, one probe per run of neighbouring lanes with
//           one key: an entry with a value is an open group, complete since
//           the slots pass; any other is claimed and takes atomicMin(first, p);
//           the entry index is kept per packet, nothing probes twice;
//   tile  : the openers (first == p) of every tile of kReviveTile packets;
//   scan  : one workgroup, exclusive scans over both tile tables in place, the
//           number of free slots and counts[3];
//   free  : the ascending list of free slots;
//   open  : the r-th opener by p takes free[r]: the entry's value, slot_key,
//           slot_k;
//   emit  : one lane per packet, pkt_slot_out from the entry's value and the
//           four packet tallies by ballot, LDS, one atomic per workgroup.
// The atomics decide only WHICH entry a key lands in; every output is read
// through the key's own entry, so neither the hash nor the order shows.  Every
// probe ends after cap steps; every entry index is at most cap_mask by
// construction (masked) or checked where it is read back from scratch, and
// every slot read from the table or the free list is checked against n_slots.
__device__ __forceinline__ uint32_t assign_hash(const AssignArgs& a, unsigned long long k) {
  k ^= k >> 33;  // (the 64-bit finaliser of MurmurHash3: every key bit reaches the low bits)
  k *= 0xFF51AFD7ED558CCDull;
  k ^= k >> 33;
  k *= 0xC4CEB9FE1A85EC53ull;
  k ^= k >> 33;
  return a.probe_last ? a.cap_mask : (uint32_t)k & a.cap_mask;
}
__device__ __forceinline__ uint32_t* assign_value(const AssignArgs& a, uint32_t e) {
  return reinterpret_cast<uint32_t*>(a.table + 2ull * e + 1u);
}
__device__ __forceinline__ uint32_t* assign_first(const AssignArgs& a, uint32_t e) {
  return reinterpret_cast<uint32_t*>(a.table + 2ull * e + 1u) + 1;
}
// The entry that holds key, claimed if no entry does; kAssignNone after cap
// steps without one (a full table: impossible at load 0.5).  The load in front
// of the compare-and-swap may be stale only as "empty", which the swap corrects.
__device__ __forceinline__ uint32_t assign_find_or_claim(const AssignArgs& a,
                                                         unsigned long long key) {
  uint32_t e = assign_hash(a, key);
  const uint64_t cap = (uint64_t)a.cap_mask + 1u;
  for (uint64_t i = 0; i < cap; ++i) {
    unsigned long long cur =
        __hip_atomic_load(&a.table[2ull * e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == kAssignNoKey) cur = atomicCAS(&a.table[2ull * e], kAssignNoKey, key);
    if (cur == kAssignNoKey || cur == key) return e;
    e = (e + 1u) & a.cap_mask;
  }
  return kAssignNone;
}

__global__ __launch_bounds__(kReviveTile) void assign_slots_kernel(AssignArgs a) {
  __shared__ uint32_t s_w[kTurnWaves];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  if (blockIdx.x == 0u && tid < 5u && a.counts) a.counts[tid] = 0ull;
  const uint64_t ntile = ((uint64_t)a.n_slots + kReviveTile - 1) / kReviveTile;
  for (uint64_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
    const uint64_t s = tile * kReviveTile + tid;
    const bool in = s < a.n_slots;
    const uint64_t sc = in ? s : a.n_slots - 1u;  // (clamped, not masked)
    const bool open = in && a.acc_len[sc] != 0;
    const unsigned long long key = a.slot_key[sc];
    if (open && key != kAssignNoKey) {
      const uint32_t e = assign_find_or_claim(a, key);
      if (e <= a.cap_mask) atomicMin(assign_value(a, e), (uint32_t)s);
      else atomicOr(a.err, kErrMissingIndex);
    }
    const uint32_t t = block_sum((uint32_t)__popcll(__ballot(in && !open)), lane, wave, s_w);
    if (tid == 0u) a.free_tile[tile] = t;
  }
}

__global__ __launch_bounds__(kReviveTile) void assign_probe_kernel(AssignArgs a) {
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  const uint64_t step = (uint64_t)gridDim.x * kReviveTile;
  for (uint64_t p0 = (uint64_t)blockIdx.x * kReviveTile; p0 < a.n_packets; p0 += step) {
    const uint64_t p = p0 + tid;
    const bool in = p < a.n_packets;
    const unsigned long long key = a.pkt_key[in ? p : a.n_packets - 1u];  // (clamped, not masked)
    const bool keyed = in && key != kAssignNoKey;
    // One probe per RUN of neighbouring lanes with one key (a burst of one
    // group's packets), made by the run's first lane, which is also the run's
    // lowest p: the only one whose atomicMin on the first arrival can matter.
    // (both halves shuffled before either is compared: lane_runs' rule)
    const uint32_t k_lo = (uint32_t)key, k_hi = (uint32_t)(key >> 32);
    const uint32_t below_lo = __shfl_up(k_lo, 1), below_hi = __shfl_up(k_hi, 1);
    const LaneRun run = lane_runs(keyed, below_lo == k_lo && below_hi == k_hi, lane);
    uint32_t e = kAssignNone;
    if (run.head) {
      e = assign_find_or_claim(a, key);
      if (e <= a.cap_mask) {
        // (the value is final since the slots pass: this kernel never writes it)
        if (*assign_value(a, e) >= a.n_slots) atomicMin(assign_first(a, e), (uint32_t)p);
      } else {
        atomicOr(a.err, kErrMissingIndex);
      }
    }
    e = __shfl(e, run.first);  // (a keyed lane's run has a head: itself or one below it)
    if (in) a.ent[p] = keyed ? e : kAssignNone;
  }
}

// a packet opens a group if it is the first arrival of an entry that has one
// (an open group's entry never gets a first arrival)
__device__ __forceinline__ bool assign_opener(const AssignArgs& a, uint64_t p, uint32_t& e) {
  e = p < a.n_packets ? a.ent[p] : kAssignNone;
  return e <= a.cap_mask && *assign_first(a, e) == (uint32_t)p;
}

__global__ __launch_bounds__(kReviveTile) void assign_tile_kernel(AssignArgs a) {
  __shared__ uint32_t s_w[kTurnWaves];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint64_t ntile = (a.n_packets + kReviveTile - 1) / kReviveTile;
  for (uint64_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
    uint32_t e;
    const uint32_t opening =
        (uint32_t)__popcll(__ballot(assign_opener(a, tile * kReviveTile + tid, e)));
    const uint32_t t = block_sum(opening, lane, wave, s_w);
    if (tid == 0u) a.open_tile[tile] = t;
  }
}

__global__ __launch_bounds__(kRvScanBlock) void assign_scan_kernel(AssignArgs a) {
  __shared__ uint32_t s_w[kRvScanBlock / 64];
  const uint32_t n_free = tile_scan_in_place(
      a.free_tile, ((uint64_t)a.n_slots + kReviveTile - 1) / kReviveTile, s_w);
  const uint32_t n_open = tile_scan_in_place(
      a.open_tile, (a.n_packets + kReviveTile - 1) / kReviveTile, s_w);
  if (threadIdx.x == 0u) {
    a.totals[0] = n_free;
    if (a.counts) a.counts[3] = min(n_free, n_open);  // (zeroed by the slots pass)
  }
}

__global__ __launch_bounds__(kReviveTile) void assign_free_kernel(AssignArgs a) {
  __shared__ uint32_t s_w[kTurnWaves];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint64_t ntile = ((uint64_t)a.n_slots + kReviveTile - 1) / kReviveTile;
  for (uint64_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
    const uint64_t s = tile * kReviveTile + tid;
    const bool in = s < a.n_slots;
    const bool is_free = in && a.acc_len[in ? s : a.n_slots - 1u] == 0;
    // the free slots of the tiles and of the tile's lanes below this one
    const uint64_t r =
        (uint64_t)a.free_tile[tile] + block_ballot_rank(__ballot(is_free), lane, wave, s_w);
    if (is_free && r < a.n_slots) a.free_list[r] = (uint32_t)s;
  }
}

__global__ __launch_bounds__(kReviveTile) void assign_open_kernel(AssignArgs a) {
  __shared__ uint32_t s_w[kTurnWaves];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint64_t ntile = (a.n_packets + kReviveTile - 1) / kReviveTile;
  const uint32_t n_free = min(a.totals[0], a.n_slots);
  for (uint64_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
    const uint64_t p = tile * kReviveTile + tid;
    uint32_t e;
    const bool opener = assign_opener(a, p, e);
    // its rank among the openers, by p
    const uint64_t r =
        (uint64_t)a.open_tile[tile] + block_ballot_rank(__ballot(opener), lane, wave, s_w);
    if (opener && r < n_free) {
      const uint32_t s = a.free_list[r];
      if (s < a.n_slots) {
        *assign_value(a, e) = s;  // (no other lane reads this entry's value in this kernel)
        a.slot_key[s] = a.pkt_key[p];
        a.slot_k[s] = a.pkt_k[p];
      }
    }
  }
}

__global__ __launch_bounds__(kReviveTile) void assign_emit_kernel(AssignArgs a) {
  __shared__ uint32_t s_w[kTurnWaves * 4];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  // the wave's packets (uniform): to an open group, to a new one, keyless, turned away
  uint32_t n[4] = {0, 0, 0, 0};
  const uint64_t step = (uint64_t)gridDim.x * kReviveTile;
  for (uint64_t p0 = (uint64_t)blockIdx.x * kReviveTile; p0 < a.n_packets; p0 += step) {
    const uint64_t p = p0 + tid;
    const bool in = p < a.n_packets;
    const uint64_t pc = in ? p : a.n_packets - 1u;  // (clamped, not masked)
    const bool keyed = in && a.pkt_key[pc] != kAssignNoKey;
    const uint32_t e = a.ent[pc];
    uint32_t s = kAssignNone;
    bool opened = false;
    if (keyed && e <= a.cap_mask) {
      // one 8-byte load: the value and the first arrival
      const unsigned long long vf = a.table[2ull * e + 1u];
      s = (uint32_t)vf;
      opened = (uint32_t)(vf >> 32) != kAssignNone;
    }
    const bool placed = s < a.n_slots;
    if (in) a.pkt_slot_out[p] = placed ? s : kAssignNone;
    n[0] += (uint32_t)__popcll(__ballot(placed && !opened));
    n[1] += (uint32_t)__popcll(__ballot(placed && opened));
    n[2] += (uint32_t)__popcll(__ballot(in && !keyed));
    n[3] += (uint32_t)__popcll(__ballot(keyed && !placed));
  }
  const uint32_t t = block_sum(n, lane, wave, s_w);
  // counts[0..2] and counts[4]; counts[3] is the scan's
  if (tid < 4u && a.counts && t != 0u)
    atomicAdd(&a.counts[tid < 3u ? tid : 4u], (unsigned long long)t);
}

// ---------------------------------------------------------------------------
// Group retention and forced closes (qfec_retire_groups): the watermark of
// QuicFecReceiver::CloseFecGroupsBefore and the kMaxFecGroups eviction of
// GetFecGroup, in front of the assign.
// ---------------------------------------------------------------------------
// The one call that reads a key: conn = key >> key_shift, number = the bits
// below.  Behind one memset of the tallies and the round words:
//   raise    : one lane per raise, a 64-bit atomicMax into conn_mark;
//   round r  : (max_groups + 1 of them, only with max_groups > 0) one lane per
//              slot, then per packet; a live number (at or above its mark)
//              below round r - 1's result goes by atomicMax, as number + 1,
//              into the connection's word of round r: the r-th largest
//              distinct live number, 0 if there is none.  One atomic per run of
//              neighbouring lanes with one key, and none where the word
//              already holds as much;
//   mark     : one lane per connection; where round max_groups found a
//              number, more than max_groups are live and conn_mark becomes
//              round max_groups - 1's, the max_groups-th largest;
//   filter   : one lane per packet, pkt_key_out and the four packet tallies;
//   classify : one lane per slot, the slots to close counted per tile;
//   scan     : one workgroup, an exclusive scan over the tile counts, counts;
//   close    : the classification again, acc_len = 0 and closed_list at the
//              scanned position: ascending, no sort.
// A maximum does not depend on the order of its operands, so the atomics show
// nowhere.  Every connection index is checked against n_conns before it
// indexes conn_mark or a round word, every place in closed_list against
// n_slots.  All variable shifts are 32-bit (the gfx950 64-bit shift hazard).
__device__ __forceinline__ bool retire_split(const RetireArgs& a, unsigned long long key,
                                             uint32_t& conn, unsigned long long& number) {
  const uint32_t lo = (uint32_t)key, hi = (uint32_t)(key >> 32), sh = a.key_shift;
  uint32_t c_lo, c_hi, n_lo, n_hi;
  if (sh >= 32u) {
    const uint32_t t = sh - 32u;  // 0 .. 31
    c_lo = hi >> t;
    c_hi = 0u;
    n_lo = lo;
    n_hi = hi & ((1u << t) - 1u);
  } else {  // 1 .. 31
    c_lo = (lo >> sh) | (hi << (32u - sh));
    c_hi = hi >> sh;
    n_lo = lo & ((1u << sh) - 1u);
    n_hi = 0u;
  }
  conn = c_lo;
  number = (unsigned long long)n_lo | ((unsigned long long)n_hi << 32);
  return c_hi == 0u && c_lo < a.n_conns;
}

// a 64-bit maximum into *w that skips the atomic where it cannot win (a stale
// load can only be too small, and then the atomic decides)
__device__ __forceinline__ void retire_max(unsigned long long* w, unsigned long long v) {
  if (__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < v) atomicMax(w, v);
}

// One lane's key offered to round a.round; keyed: the lane holds a key that
// counts (an open slot's or a packet's, not QFEC_NO_KEY).
__device__ __forceinline__ void retire_offer(const RetireArgs& a, unsigned long long key,
                                             bool keyed, uint32_t lane) {
  uint32_t conn;
  unsigned long long num;
  bool live = retire_split(a, key, conn, num) && keyed;
  if (live) live = num >= a.conn_mark[conn];
  if (live && a.round != 0u)  // (0 = nothing left below: num + 1 >= 1)
    live = num + 1u < a.top[(uint64_t)(a.round - 1u) * a.n_conns + conn];
  // (all three shuffled before anything is compared: lane_runs' rule; a live
  // lane under a lane that is not live heads a run whatever the keys are)
  const uint32_t k_lo = (uint32_t)key, k_hi = (uint32_t)(key >> 32);
  const uint32_t below_lo = __shfl_up(k_lo, 1), below_hi = __shfl_up(k_hi, 1);
  const uint32_t below_live = __shfl_up((uint32_t)live, 1);
  const LaneRun run =
      lane_runs(live, below_live != 0u && below_lo == k_lo && below_hi == k_hi, lane);
  if (run.head) retire_max(&a.top[(uint64_t)a.round * a.n_conns + conn], num + 1u);
}

__global__ __launch_bounds__(kReviveTile) void retire_raise_kernel(RetireArgs a) {
  __shared__ uint32_t s_w[kTurnWaves];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  uint32_t n_bad = 0;  // the wave's raises out of range (uniform)
  const uint64_t step = (uint64_t)gridDim.x * kReviveTile;
  for (uint64_t i0 = (uint64_t)blockIdx.x * kReviveTile; i0 < a.n_raise; i0 += step) {
    const uint64_t i = i0 + tid;
    const bool in = i < a.n_raise;
    const uint64_t ic = in ? i : a.n_raise - 1u;  // (clamped, not masked)
    const uint32_t conn = a.raise_conn[ic];
    const unsigned long long mark = a.raise_mark[ic];
    if (in && conn < a.n_conns) retire_max(&a.conn_mark[conn], mark);
    n_bad += (uint32_t)__popcll(__ballot(in && conn >= a.n_conns));
  }
  const uint32_t t = block_sum(n_bad, lane, wave, s_w);
  if (tid == 0u && t != 0u) {
    atomicAdd(&a.tally[4], (unsigned long long)t);
    atomicOr(a.err, kErrMissingIndex);
  }
}

__global__ __launch_bounds__(kReviveTile) void retire_round_kernel(RetireArgs a) {
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  const uint64_t step = (uint64_t)gridDim.x * kReviveTile;
  for (uint64_t s0 = (uint64_t)blockIdx.x * kReviveTile; s0 < a.n_slots; s0 += step) {
    const uint64_t s = s0 + tid;
    const bool in = s < a.n_slots;
    const uint64_t sc = in ? s : a.n_slots - 1u;  // (clamped, not masked)
    const unsigned long long key = a.slot_key[sc];
    retire_offer(a, key, in && a.acc_len[sc] != 0 && key != kAssignNoKey, lane);
  }
  for (uint64_t p0 = (uint64_t)blockIdx.x * kReviveTile; p0 < a.n_packets; p0 += step) {
    const uint64_t p = p0 + tid;
    const bool in = p < a.n_packets;
    const unsigned long long key = a.pkt_key[in ? p : a.n_packets - 1u];  // (clamped)
    retire_offer(a, key, in && key != kAssignNoKey, lane);
  }
}

__global__ __launch_bounds__(kReviveTile) void retire_mark_kernel(RetireArgs a) {
  const uint64_t step = (uint64_t)gridDim.x * kReviveTile;
  for (uint64_t c = (uint64_t)blockIdx.x * kReviveTile + threadIdx.x; c < a.n_conns; c += step) {
    // more than max_groups live numbers: the max_groups-th largest is the mark
    // (it is live, so at or above the old one)
    const unsigned long long kept = a.top[(uint64_t)(a.max_groups - 1u) * a.n_conns + c];
    if (a.top[(uint64_t)a.max_groups * a.n_conns + c] != 0ull && kept != 0ull)
      a.conn_mark[c] = kept - 1u;
  }
}

__global__ __launch_bounds__(kReviveTile) void retire_filter_kernel(RetireArgs a) {
  __shared__ uint32_t s_w[kTurnWaves * 4];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  // the wave's packets (uniform): refused, keyless, passed, connection out of range
  uint32_t n[4] = {0, 0, 0, 0};
  const uint64_t step = (uint64_t)gridDim.x * kReviveTile;
  for (uint64_t p0 = (uint64_t)blockIdx.x * kReviveTile; p0 < a.n_packets; p0 += step) {
    const uint64_t p = p0 + tid;
    const bool in = p < a.n_packets;
    const unsigned long long key = a.pkt_key[in ? p : a.n_packets - 1u];  // (clamped, not masked)
    const bool keyed = in && key != kAssignNoKey;
    uint32_t conn;
    unsigned long long num;
    const bool known = retire_split(a, key, conn, num) && keyed;
    const bool refused = known && num < a.conn_mark[conn];
    const bool passed = known && !refused;
    if (in) a.pkt_key_out[p] = passed ? key : kAssignNoKey;
    n[0] += (uint32_t)__popcll(__ballot(refused));
    n[1] += (uint32_t)__popcll(__ballot(in && !keyed));
    n[2] += (uint32_t)__popcll(__ballot(passed));
    n[3] += (uint32_t)__popcll(__ballot(keyed && !known));
  }
  const uint32_t t = block_sum(n, lane, wave, s_w);
  if (tid < 4u && t != 0u) {
    atomicAdd(&a.tally[1u + tid], (unsigned long long)t);
    if (tid == 3u) atomicOr(a.err, kErrMissingIndex);
  }
}

// what the close does with slot s: 1 it closes it (open, keyed, below its
// connection's mark), 2 its connection is out of range, 0 anything else
__device__ __forceinline__ uint32_t retire_slot_class(const RetireArgs& a, uint64_t s) {
  const bool in = s < a.n_slots;
  const uint64_t sc = in ? s : a.n_slots - 1u;  // (clamped, not masked)
  const unsigned long long key = a.slot_key[sc];
  const bool keyed = in && a.acc_len[sc] != 0 && key != kAssignNoKey;
  uint32_t conn;
  unsigned long long num;
  const bool known = retire_split(a, key, conn, num);
  if (!keyed) return 0u;
  if (!known) return 2u;
  return num < a.conn_mark[conn] ? 1u : 0u;
}

__global__ __launch_bounds__(kReviveTile) void retire_classify_kernel(RetireArgs a) {
  __shared__ uint32_t s_w[kTurnWaves];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  uint32_t n_bad = 0;  // the wave's open slots with a connection out of range (uniform)
  const uint64_t ntile = ((uint64_t)a.n_slots + kReviveTile - 1) / kReviveTile;
  for (uint64_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
    const uint32_t cls = retire_slot_class(a, tile * kReviveTile + tid);
    n_bad += (uint32_t)__popcll(__ballot(cls == 2u));
    const uint32_t t = block_sum((uint32_t)__popcll(__ballot(cls == 1u)), lane, wave, s_w);
    if (tid == 0u) a.tile_off[tile] = t;
  }
  const uint32_t t = block_sum(n_bad, lane, wave, s_w);
  if (tid == 0u && t != 0u) {
    atomicAdd(&a.tally[4], (unsigned long long)t);
    atomicOr(a.err, kErrMissingIndex);
  }
}

// One workgroup: tile_off[i] = slots closed in the tiles before i (in place
// over the tile counts), then counts.  The sum fits 32 bits: n_slots < 2^32.
__global__ __launch_bounds__(kRvScanBlock) void retire_scan_kernel(RetireArgs a) {
  __shared__ uint32_t s_w[kRvScanBlock / 64];
  const uint32_t closed = tile_scan_in_place(
      a.tile_off, ((uint64_t)a.n_slots + kReviveTile - 1) / kReviveTile, s_w);
  if (threadIdx.x == 0u && a.counts) {
    a.counts[0] = closed;
    for (uint32_t i = 1; i < 5u; ++i) a.counts[i] = a.tally[i];
  }
}

__global__ __launch_bounds__(kReviveTile) void retire_close_kernel(RetireArgs a) {
  __shared__ uint32_t s_w[kTurnWaves];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint64_t ntile = ((uint64_t)a.n_slots + kReviveTile - 1) / kReviveTile;
  for (uint64_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
    const uint64_t s = tile * kReviveTile + tid;
    // (a lane reads and writes the length of its own slot only)
    const bool closing = retire_slot_class(a, s) == 1u;
    // the closed slots of the tiles and of the tile's lanes below this one
    const uint64_t r =
        (uint64_t)a.tile_off[tile] + block_ballot_rank(__ballot(closing), lane, wave, s_w);
    if (closing) {
      a.acc_len[s] = 0;
      if (a.closed_list && r < a.n_slots) a.closed_list[r] = (uint32_t)s;
    }
  }
}

// ---------------------------------------------------------------------------
// Private headers on the device (qfec_parse_opened,
// qfec_write_private_headers): QuicFramer::ProcessAuthenticatedHeader and
// WriteFecPrivateHeader over a turn's opened packets, in front of the retire.
// ---------------------------------------------------------------------------
// One pass, one lane per packet: the record (clamped for the lanes past the
// end, which then classify the last packet once more and store nothing), at
// most two bytes of the packet, the class, six stores.  A byte is loaded only
// under the predicate that puts it inside [pkt_off, pkt_off + pkt_len) of a
// packet that verified; the two are byte loads, so no alignment matters.  The
// key is built, and its range checked, in 32-bit halves as retire_split takes
// it apart (the gfx950 64-bit shift hazard).  Tallies by ballot, block_sum and
// one atomic per workgroup and class into counts, zeroed in front of the pass.
__global__ __launch_bounds__(kReviveTile) void parse_opened_kernel(ParseArgs a) {
  __shared__ uint32_t s_w[kTurnWaves * 6];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  // the wave's packets (uniform): data, FEC, outside a group, failed, rejected, range
  uint32_t n[6] = {0, 0, 0, 0, 0, 0};
  const uint32_t sh = a.key_shift;
  const uint64_t step = (uint64_t)gridDim.x * kReviveTile;
  for (uint64_t p0 = (uint64_t)blockIdx.x * kReviveTile; p0 < a.n_packets; p0 += step) {
    const uint64_t p = p0 + tid;
    const bool in = p < a.n_packets;
    const uint64_t pc = in ? p : a.n_packets - 1u;  // (clamped, not masked)
    const uint64_t off = a.pkt_off[pc];
    const uint32_t len = a.pkt_len[pc];
    const unsigned long long pn = a.packet_number[pc];
    const uint32_t conn = a.pkt_conn[pc];
    const bool ok = a.pkt_ok == nullptr || a.pkt_ok[pc] != 0;
    uint32_t b0 = 0u, b1 = 0u;
    if (ok && len >= 1u) b0 = a.bytes[off];
    if (ok && len >= 2u) b1 = a.bytes[off + 1u];
    const bool grouped = (b0 & kPrivateFlagFecGroup) != 0u;
    // the key, and whether its parts fit: conn below 2^(64 - sh), group below 2^sh
    const unsigned long long group = pn - b1;  // (read only where b1 < pn)
    const uint32_t g_lo = (uint32_t)group, g_hi = (uint32_t)(group >> 32);
    uint32_t k_lo, k_hi;
    bool fits;
    if (sh >= 32u) {
      const uint32_t t = sh - 32u;  // 0 .. 31
      fits = (t == 0u || (conn >> (32u - t)) == 0u) && (g_hi >> t) == 0u;
      k_lo = g_lo;
      k_hi = (conn << t) | g_hi;
    } else {  // 1 .. 31: any 32-bit connection fits the 64 - sh bits above
      fits = g_hi == 0u && (g_lo >> sh) == 0u;
      k_lo = (conn << sh) | g_lo;
      k_hi = conn >> (32u - sh);
    }
    const unsigned long long key = (unsigned long long)k_lo | ((unsigned long long)k_hi << 32);
    uint32_t cls;
    if (!ok) cls = kHdrFailed;
    else if (len == 0u) cls = kHdrNoFlags;
    else if (b0 > a.max_flags) cls = kHdrIllegalFlags;
    else if (!grouped) cls = b0;
    else if (len < 2u) cls = kHdrNoOffset;
    else if ((unsigned long long)b1 >= pn) cls = kHdrBadOffset;
    else if (len == 2u) cls = kHdrEmpty;
    else if (!fits || key == kAssignNoKey) cls = kHdrRange;
    else cls = b0;
    const bool accepted = cls < kHdrFailed, keyed = accepted && grouped;
    const uint32_t used = keyed ? 2u : accepted ? 1u : 0u;
    if (in) {
      a.pkt_key_out[p] = keyed ? key : kAssignNoKey;
      a.pkt_idx_out[p] = (uint8_t)(keyed ? b1 : 0u);
      a.body_off_out[p] = off + used;
      a.body_len_out[p] = (uint16_t)(accepted ? len - used : 0u);
      a.hdr_out[p] = (uint8_t)cls;
      if (a.entropy_out)
        a.entropy_out[p] =
            (uint8_t)(accepted ? (b0 & kPrivateFlagEntropy) << ((uint32_t)pn & 7u) : 0u);
    }
    const bool fec = (b0 & kPrivateFlagFec) != 0u;
    n[0] += (uint32_t)__popcll(__ballot(in && keyed && !fec));
    n[1] += (uint32_t)__popcll(__ballot(in && keyed && fec));
    n[2] += (uint32_t)__popcll(__ballot(in && accepted && !keyed));
    n[3] += (uint32_t)__popcll(__ballot(in && cls == kHdrFailed));
    n[4] += (uint32_t)__popcll(__ballot(in && !accepted && cls != kHdrFailed && cls != kHdrRange));
    n[5] += (uint32_t)__popcll(__ballot(in && cls == kHdrRange));
  }
  const uint32_t t = block_sum(n, lane, wave, s_w);
  if (tid < 6u && t != 0u) {
    if (a.counts) atomicAdd(&a.counts[tid], (unsigned long long)t);
    if (tid == 5u) atomicOr(a.err, kErrMissingIndex);
  }
}

// The sender's mirror, one lane per record: the flags byte and, in a group,
// the offset byte behind it; a record WriteFecPrivateHeader refuses (FEC
// without a group, flags above the version's maximum) stores no byte.
__global__ __launch_bounds__(kReviveTile) void write_headers_kernel(WriteHeadersArgs a) {
  __shared__ uint32_t s_w[kTurnWaves * 2];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  uint32_t n[2] = {0, 0};  // the wave's records (uniform): written, refused
  const uint64_t step = (uint64_t)gridDim.x * kReviveTile;
  for (uint64_t p0 = (uint64_t)blockIdx.x * kReviveTile; p0 < a.n_packets; p0 += step) {
    const uint64_t p = p0 + tid;
    const bool in = p < a.n_packets;
    const uint64_t pc = in ? p : a.n_packets - 1u;  // (clamped, not masked)
    const uint64_t off = a.pkt_off[pc];
    const uint32_t h = a.hdr[pc], fo = a.fec_offset[pc];
    const bool grouped = (h & kPrivateFlagFecGroup) != 0u;
    const bool refused = h > a.max_flags || ((h & kPrivateFlagFec) != 0u && !grouped);
    const bool writes = in && !refused;
    if (writes) a.bytes[off] = (uint8_t)h;
    if (writes && grouped) a.bytes[off + 1u] = (uint8_t)fo;
    if (in && a.body_off_out) a.body_off_out[p] = off + (refused ? 0u : grouped ? 2u : 1u);
    n[0] += (uint32_t)__popcll(__ballot(writes));
    n[1] += (uint32_t)__popcll(__ballot(in && refused));
  }
  const uint32_t t = block_sum(n, lane, wave, s_w);
  if (tid < 2u && t != 0u) {
    if (a.counts) atomicAdd(&a.counts[tid], (unsigned long long)t);
    if (tid == 1u) atomicOr(a.err, kErrMissingIndex);
  }
}

// ---------------------------------------------------------------------------
// Ack state on the device (qfec_record_received, qfec_build_acks):
// QuicReceivedPacketManager and its EntropyTracker over a turn, behind the
// revive.
// ---------------------------------------------------------------------------
// The record, behind a memset of counts and of the per-connection maxima:
//   classify : one lane per packet against the state as the call found it;
//              rcv_out, six tallies, a 64-bit atomicMax of every RECORDED
//              number into its connection's word of the scratch;
//   advance  : one lane per connection; where the maximum passed the largest
//              observed, the wave clears the cells the ring now takes in (a
//              lane's range broadcast, 64 byte stores a trip) and the largest
//              becomes the maximum.  No other pass stores a cell's byte;
//   set      : one lane per packet, RECORDED ones OR received | flag << 1 into
//              their cell by a 32-bit atomic on the word that holds it; the
//              cell was new where the word that came back lacked the bit;
//   revived  : one lane per group, 4 OR-ed into the cell of a revived packet
//              that is live, below the largest and not received;
//   raises   : one wave per STOP_WAITING over the cells the raise drops.
// An OR and a maximum do not depend on the order of their operands, and no two
// raises name one connection, so the atomics show nowhere.  The build is three
// launches: one wave per ack over its live cells that counts (and writes the
// ack's scalars), one workgroup that scans the counts into the two CSR
// pointers, and the walk again that fills the tables.  Every connection index
// is checked against n_conns before it indexes the state, every ring index is
// masked with window - 1, a walk is at most window cells long whatever the
// state holds, and a table entry is stored only below max_ranges or
// max_revived of its ack.  All variable shifts are 32-bit (the gfx950 64-bit
// shift hazard); keys are split in halves as retire_split does it.
__device__ __forceinline__ uint64_t ack_cell_index(uint32_t conn, uint32_t window, uint32_t pn_lo) {
  return (uint64_t)conn * window + (pn_lo & (window - 1u));
}

__global__ __launch_bounds__(kReviveTile) void record_classify_kernel(RecordArgs a) {
  __shared__ uint32_t s_w[kTurnWaves * 6];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  uint32_t n[6] = {0, 0, 0, 0, 0, 0};  // the wave's packets per class (uniform)
  const uint64_t step = (uint64_t)gridDim.x * kReviveTile;
  for (uint64_t p0 = (uint64_t)blockIdx.x * kReviveTile; p0 < a.n_packets; p0 += step) {
    const uint64_t p = p0 + tid;
    const bool in = p < a.n_packets;
    const uint64_t pc = in ? p : a.n_packets - 1u;  // (clamped, not masked)
    const unsigned long long pn = a.packet_number[pc];
    const uint32_t conn = a.pkt_conn[pc];
    const uint32_t h = a.hdr ? a.hdr[pc] : 0u;
    const bool known = conn < a.n_conns;
    const uint32_t cc = known ? conn : 0u;  // (clamped; nothing to load with no connection)
    unsigned long long least = 0, largest = 0;
    uint32_t cell = 0;
    if (a.n_conns != 0u) {
      least = a.rcv_least[cc];
      largest = a.rcv_largest[cc];
      cell = a.rcv_cells[ack_cell_index(cc, a.window, (uint32_t)pn)];
    }
    const unsigned long long lo = least ? least : 1ull;
    uint32_t cls;
    if (h >= kHdrFailed) cls = kRcvNotAccepted;
    else if (!known) cls = kRcvRange;
    else if (pn == 0ull || pn < least) cls = kRcvStale;
    else if (pn - lo >= a.window) cls = kRcvOverflow;
    else if (pn <= largest && (cell & kCellReceived) != 0u) cls = kRcvDuplicate;
    else cls = kRcvRecorded;
    if (in) {
      a.rcv_out[p] = (uint8_t)cls;
      if (cls == kRcvRecorded) retire_max(&a.seen[conn], pn);
    }
#pragma unroll
    for (uint32_t c = 0; c < 6u; ++c) n[c] += (uint32_t)__popcll(__ballot(in && cls == c));
  }
  const uint32_t t = block_sum(n, lane, wave, s_w);
  if (tid < 6u && t != 0u) {
    if (a.counts) atomicAdd(&a.counts[tid], (unsigned long long)t);
    if (tid == kRcvRange) atomicOr(a.err, kErrMissingIndex);
  }
}

__global__ __launch_bounds__(kReviveTile) void record_advance_kernel(RecordArgs a) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t step = (uint64_t)gridDim.x * kReviveTile;
  for (uint64_t c0 = (uint64_t)blockIdx.x * kReviveTile; c0 < a.n_conns; c0 += step) {
    const uint64_t c = c0 + threadIdx.x;
    const bool in = c < a.n_conns;
    const uint32_t cc = (uint32_t)(in ? c : a.n_conns - 1u);  // (clamped, not masked)
    const unsigned long long largest = a.rcv_largest[cc], seen = a.seen[cc],
                             least = a.rcv_least[cc];
    const unsigned long long lo = least ? least : 1ull;
    const bool moved = in && seen > largest;
    // the cells of (max(largest, lo - 1), seen]: at most window, seen being RECORDED
    const unsigned long long from = (largest >= lo ? largest : lo - 1u) + 1u;
    const uint32_t cnt =
        moved && seen >= from ? (uint32_t)min(seen - from + 1u, (unsigned long long)a.window) : 0u;
    if (moved) a.rcv_largest[cc] = seen;
    // (the ballot is the wave's: the loop and every lane_read in it are uniform)
    for (uint64_t m = __ballot(cnt != 0u); m != 0ull; m &= m - 1ull) {
      const uint32_t src = (uint32_t)__builtin_ctzll(m);
      const uint32_t c_s = lane_read(cc, src), f_s = lane_read((uint32_t)from, src),
                     n_s = lane_read(cnt, src);
      for (uint32_t j = lane; j < n_s; j += 64u)
        a.rcv_cells[ack_cell_index(c_s, a.window, f_s + j)] = 0;
    }
  }
}

__global__ __launch_bounds__(kReviveTile) void record_set_kernel(RecordArgs a) {
  __shared__ uint32_t s_w[kTurnWaves];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  uint32_t n_new = 0;  // the wave's cells newly set (uniform)
  uint32_t* const words = reinterpret_cast<uint32_t*>(a.rcv_cells);
  const uint64_t step = (uint64_t)gridDim.x * kReviveTile;
  for (uint64_t p0 = (uint64_t)blockIdx.x * kReviveTile; p0 < a.n_packets; p0 += step) {
    const uint64_t p = p0 + tid;
    const bool in = p < a.n_packets;
    const uint64_t pc = in ? p : a.n_packets - 1u;  // (clamped, not masked)
    const uint32_t pn_lo = (uint32_t)a.packet_number[pc], conn = a.pkt_conn[pc];
    const uint32_t flag = a.entropy ? (uint32_t)(a.entropy[pc] != 0) : 0u;
    bool fresh = false;
    if (in && a.rcv_out[pc] == kRcvRecorded) {  // (RECORDED: conn < n_conns)
      const uint64_t idx = ack_cell_index(conn, a.window, pn_lo);
      const uint32_t sh = ((uint32_t)idx & 3u) * 8u;
      const uint32_t old = atomicOr(&words[idx >> 2], (kCellReceived | flag << 1) << sh);
      fresh = ((old >> sh) & kCellReceived) == 0u;
    }
    n_new += (uint32_t)__popcll(__ballot(fresh));
  }
  const uint32_t t = block_sum(n_new, lane, wave, s_w);
  if (tid == 0u && t != 0u && a.counts) atomicAdd(&a.counts[6], (unsigned long long)t);
}

// key >> sh and key & ((1 << sh) - 1) in 32-bit halves, sh in 1..63
__device__ __forceinline__ void ack_split_key(unsigned long long key, uint32_t sh, uint32_t& c_lo,
                                              uint32_t& c_hi, unsigned long long& number) {
  const uint32_t lo = (uint32_t)key, hi = (uint32_t)(key >> 32);
  uint32_t n_lo, n_hi;
  if (sh >= 32u) {
    const uint32_t t = sh - 32u;  // 0 .. 31
    c_lo = hi >> t;
    c_hi = 0u;
    n_lo = lo;
    n_hi = hi & ((1u << t) - 1u);
  } else {  // 1 .. 31
    c_lo = (lo >> sh) | (hi << (32u - sh));
    c_hi = hi >> sh;
    n_lo = lo & ((1u << sh) - 1u);
    n_hi = 0u;
  }
  number = (unsigned long long)n_lo | ((unsigned long long)n_hi << 32);
}

__global__ __launch_bounds__(kReviveTile) void record_revived_kernel(RecordArgs a) {
  __shared__ uint32_t s_w[kTurnWaves * 2];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  uint32_t n[2] = {0, 0};  // the wave's revived groups (uniform): recorded, not missing
  uint32_t* const words = reinterpret_cast<uint32_t*>(a.rcv_cells);
  const uint64_t step = (uint64_t)gridDim.x * kReviveTile;
  for (uint64_t g0 = (uint64_t)blockIdx.x * kReviveTile; g0 < a.n_groups; g0 += step) {
    const uint64_t g = g0 + tid;
    const bool in = g < a.n_groups;
    const uint64_t gc = in ? g : a.n_groups - 1u;  // (clamped, not masked)
    const uint32_t st = a.status[gc], ri = a.revived_idx[gc];
    const uint32_t s = a.slot ? a.slot[gc] : (uint32_t)gc;
    const bool cand = in && st == 1u /* QFEC_GROUP_REVIVED */ && s < a.n_slots;
    unsigned long long key = kAssignNoKey;
    if (a.n_slots != 0u) key = a.slot_key[s < a.n_slots ? s : 0u];  // (clamped)
    uint32_t c_lo, c_hi;
    unsigned long long first;
    ack_split_key(key, a.key_shift, c_lo, c_hi, first);
    const bool known = key != kAssignNoKey && c_hi == 0u && c_lo < a.n_conns;
    const uint32_t cc = known ? c_lo : 0u;  // (clamped)
    const unsigned long long pn = first + ri;
    unsigned long long least = 0, largest = 0;
    uint32_t cell = 0;
    if (a.n_conns != 0u) {
      least = a.rcv_least[cc];
      largest = a.rcv_largest[cc];
      cell = a.rcv_cells[ack_cell_index(cc, a.window, (uint32_t)pn)];
    }
    const unsigned long long lo = least ? least : 1ull;
    // RecordPacketRevived's IsMissing; (largest - lo < window: the index is the cell's)
    const bool missing =
        cand && known && pn >= lo && pn < largest && (cell & kCellReceived) == 0u;
    if (missing) {
      const uint64_t idx = ack_cell_index(cc, a.window, (uint32_t)pn);
      atomicOr(&words[idx >> 2], kCellRevived << (((uint32_t)idx & 3u) * 8u));
    }
    n[0] += (uint32_t)__popcll(__ballot(missing));
    n[1] += (uint32_t)__popcll(__ballot(cand && !missing));
  }
  const uint32_t t = block_sum(n, lane, wave, s_w);
  if (tid < 2u && t != 0u && a.counts) atomicAdd(&a.counts[7u + tid], (unsigned long long)t);
}

__device__ __forceinline__ uint32_t wave_xor(uint32_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v ^= __shfl_xor(v, d);
  return v;
}

// One wave per raise (no two of a call name one connection: the caller's).
__global__ __launch_bounds__(kReviveTile) void record_raise_kernel(RecordArgs a) {
  __shared__ uint32_t s_w[kTurnWaves * 4];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  uint32_t n[4] = {0, 0, 0, 0};  // the wave's raises (uniform): applied, dropped one, jumps, range
  const uint64_t step = (uint64_t)gridDim.x * kTurnWaves;
  for (uint64_t i = (uint64_t)blockIdx.x * kTurnWaves + wave; i < a.n_raise; i += step) {
    const uint32_t conn = a.raise_conn[i];
    const unsigned long long up = a.raise_least[i];
    const uint32_t frame_hash = a.raise_hash[i];
    if (conn >= a.n_conns) {
      ++n[3];
      continue;
    }
    const unsigned long long least = a.rcv_least[conn], largest = a.rcv_largest[conn];
    if (up <= least) continue;
    ++n[0];
    uint32_t hash = frame_hash;
    if (up > largest + 1u) {
      ++n[2];  // a jump: nothing of the ring is left below it
    } else {
      const unsigned long long lo = least ? least : 1ull;
      const uint32_t len = (uint32_t)min(up - lo, (unsigned long long)a.window), lo32 = (uint32_t)lo;
      uint32_t x = 0, gone = 0;
      for (uint32_t j0 = 0; j0 < len; j0 += 64u) {
        const uint32_t j = j0 + lane;
        const uint32_t jc = j < len ? j : len - 1u;  // (clamped, not masked)
        const uint32_t cell = a.rcv_cells[ack_cell_index(conn, a.window, lo32 + jc)];
        const bool got = (cell & kCellReceived) != 0u;
        if (j < len && got) x ^= ((cell >> 1) & 1u) << ((lo32 + j) & 7u);
        if (j < len && !got) gone = 1u;
      }
      x = wave_xor(x);
      const bool lost = __ballot(gone != 0u) != 0ull;
      if (lost) ++n[1];
      else hash = (uint32_t)a.rcv_hash[conn] ^ x;
    }
    if (lane == 0u) {
      a.rcv_hash[conn] = (uint8_t)hash;
      a.rcv_least[conn] = up;
    }
  }
  const uint32_t t = block_sum(n, lane, wave, s_w);
  if (tid < 4u && t != 0u) {
    if (tid < 3u && a.counts) atomicAdd(&a.counts[9u + tid], (unsigned long long)t);
    if (tid == 3u) atomicOr(a.err, kErrMissingIndex);
  }
}

// One ack's walk over its live cells, by one wave.  FILL == false: the ack's
// scalars and its two counts; FILL == true: the same walk again, the tables.
template <bool FILL>
__device__ __forceinline__ void ack_walk(const AcksArgs& a, uint64_t i, uint32_t lane) {
  const uint32_t conn = a.ack_conn[i];
  unsigned long long least = 0, largest = 0;
  uint32_t hash = 0;
  const bool known = conn < a.n_conns;  // (uniform, as everything read per ack)
  if (known) {
    least = a.rcv_least[conn];
    largest = a.rcv_largest[conn];
    hash = a.rcv_hash[conn];
  }
  const unsigned long long lo = least ? least : 1ull;
  uint32_t kept = 0, n_revd = 0, cut = 0;
  if (known && largest >= lo) {
    const uint32_t len = (uint32_t)min(largest - lo + 1u, (unsigned long long)a.window),
                   lo32 = (uint32_t)lo;
    uint32_t rp = 0, vp = 0, keep_from = 0;
    if (FILL) {
      rp = a.range_ptr[i];
      vp = a.rev_ptr[i];
      const uint32_t all = a.n_rev[i];
      keep_from = all - min(all, a.max_revived);
    }
    uint32_t n_start = 0, x = 0, carry = 0;  // (carry: the cell below this trip's was missing)
    for (uint32_t j0 = 0; j0 < len && cut == 0u; j0 += 64u) {
      const uint32_t j = j0 + lane;
      const bool inr = j < len;
      const uint32_t jc = inr ? j : len - 1u;  // (clamped, not masked)
      const uint32_t cell = a.rcv_cells[ack_cell_index(conn, a.window, lo32 + jc)];
      const uint32_t miss = (uint32_t)(inr && (cell & kCellReceived) == 0u);
      // (every lane shuffles before anything is compared)
      const uint32_t below = lane_read(miss, lane ? lane - 1u : 0u);
      const uint32_t last = lane_read(miss, 63u);
      const bool prev = (lane ? below : carry) != 0u;
      const bool start = miss != 0u && !prev, end = inr && miss == 0u && prev;
      const uint64_t bs = __ballot(start);
      const uint32_t sidx = n_start + ballot_rank(bs);  // starts below this cell
      // the first interval that does not fit cuts the ack off below its first packet
      const uint64_t bt = __ballot(start && sidx == a.max_ranges);
      uint32_t lim = len;
      if (bt != 0ull) {
        cut = 1u;
        lim = j0 + (uint32_t)__builtin_ctzll(bt);
        largest = lo + lim - 1u;
      }
      const bool live = j < lim;
      if (live && miss == 0u) x ^= ((cell >> 1) & 1u) << ((lo32 + j) & 7u);
      const bool revd = live && miss != 0u && (cell & kCellRevived) != 0u;
      const uint64_t br = __ballot(revd);
      const uint32_t ridx = n_revd + ballot_rank(br);
      if (FILL) {
        if (start && sidx < a.max_ranges) a.range_lo[(uint64_t)rp + sidx] = lo + j;
        if (end && sidx != 0u && sidx - 1u < a.max_ranges)
          a.range_hi[(uint64_t)rp + sidx - 1u] = lo + j;
        if (revd && ridx >= keep_from && ridx - keep_from < a.max_revived)
          a.rev_pn[(uint64_t)vp + ridx - keep_from] = lo + j;
      }
      n_start += (uint32_t)__popcll(bs);
      n_revd += (uint32_t)__popcll(br);
      carry = last;
    }
    kept = min(n_start, a.max_ranges);
    hash ^= wave_xor(x);
  }
  if (!FILL && lane == 0u) {
    a.largest_observed[i] = largest;
    a.entropy_hash[i] = (uint8_t)hash;
    a.truncated[i] = (uint8_t)cut;
    a.n_rng[i] = kept;
    a.n_rev[i] = n_revd;
    if (!known) atomicOr(a.err, kErrMissingIndex);
  }
}

template <bool FILL>
__global__ __launch_bounds__(kReviveTile) void acks_walk_kernel(AcksArgs a) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint64_t step = (uint64_t)gridDim.x * kTurnWaves;
  for (uint64_t i = (uint64_t)blockIdx.x * kTurnWaves + wave; i < a.n_acks; i += step)
    ack_walk<FILL>(a, i, lane);
}

// One workgroup: the two CSR pointers from the per-ack counts.  The sums fit
// 32 bits: n_acks * max(max_ranges, max_revived) < 2^32.
__global__ __launch_bounds__(kRvScanBlock) void acks_scan_kernel(AcksArgs a) {
  __shared__ uint32_t s_w[kRvScanBlock / 64];
  const uint64_t rng = tile_scan(
      a.n_acks, s_w, [=](uint64_t i) { return a.n_rng[i]; },
      [=](uint64_t i, uint64_t x) { a.range_ptr[i] = (uint32_t)x; });
  const uint64_t rev = tile_scan(
      a.n_acks, s_w, [=](uint64_t i) { return min(a.n_rev[i], a.max_revived); },
      [=](uint64_t i, uint64_t x) { a.rev_ptr[i] = (uint32_t)x; });
  if (threadIdx.x == 0u) {
    a.range_ptr[a.n_acks] = (uint32_t)rng;
    a.rev_ptr[a.n_acks] = (uint32_t)rev;
  }
}

// ---------------------------------------------------------------------------
// The ack frame's wire bytes (qfec_write_ack_frames): AppendAckFrameAndTypeByte
// with GetAckFrameInfo over the build's tables, one wave per ack.
// ---------------------------------------------------------------------------
// Two walks over the ack's intervals, 64 a trip and four trips at the most (255
// intervals of an ack are read, whatever range_ptr says).  The first sums the
// nack ranges (an interval of n numbers is ceil(n / 256) of them) and takes the
// wave maximum of the gaps' minimal lengths: mm, and with the room the number
// of ranges kept.  The second scans the per-interval counts again: range k, the
// k-th from below, lies (kept - 1 - k) * (mm + 1) bytes behind the range count,
// so every lane stores its intervals' ranges with no order among the lanes, and
// the lane whose interval holds range number `kept` names the largest observed
// of a cut ack.  Only then lane 0 writes the head.  A cut ack's hash needs the
// cells between the two largest, 64 a trip, at most window of them.  Nothing is
// stored before the frame's mandatory length is known to be within out_cap, and
// every store after that lies below that length plus the revived numbers
// counted into the same room.  Every connection index is checked before it
// indexes the ring and every ring index is masked.  64-bit values are compared
// and subtracted whole but shifted in 32-bit halves only (the gfx950 64-bit
// shift hazard): the numbers' bytes, the ufloat16 and the interval lengths.
__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = max(v, (uint32_t)__shfl_xor(v, d));
  return v;
}

// GetMinSequenceNumberLength
__device__ __forceinline__ uint32_t ackw_length(unsigned long long n) {
  const uint32_t lo = (uint32_t)n, hi = (uint32_t)(n >> 32);
  return hi != 0u ? 6u : lo >= 0x10000u ? 4u : lo >= 0x100u ? 2u : 1u;
}

// The low `length` (<= 6) bytes of n, little-endian, by byte stores.
__device__ __forceinline__ void ackw_put(uint8_t* p, uint32_t length, unsigned long long n) {
  const uint32_t lo = (uint32_t)n, hi = (uint32_t)(n >> 32);
#pragma unroll
  for (uint32_t b = 0; b < 4u; ++b)
    if (b < length) p[b] = (uint8_t)(lo >> (8u * b));
#pragma unroll
  for (uint32_t b = 4; b < 6u; ++b)
    if (b < length) p[b] = (uint8_t)(hi >> (8u * (b - 4u)));
}

// QuicDataWriter::WriteUFloat16
__device__ __forceinline__ uint32_t ackw_ufloat16(unsigned long long v) {
  const uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
  if (hi == 0u && lo < 4096u) return lo;
  if (hi > 0x3FFu || (hi == 0x3FFu && lo >= 0xC0000000u)) return 0xFFFFu;  // kUFloat16MaxValue
  // the highest bit, at 12 .. 41, goes to bit 11; the exponent is the distance
  const uint32_t top = hi != 0u ? 63u - (uint32_t)__clz((int)hi) : 31u - (uint32_t)__clz((int)lo);
  const uint32_t sh = top - 11u;  // 1 .. 30
  const uint32_t mant = (lo >> sh) | (hi << (32u - sh));
  return (mant & 0xFFFu) + (sh << 11);
}

// The nack ranges of [lo, hi); a live interval is at most a window long.
__device__ __forceinline__ uint32_t ackw_span(unsigned long long lo, unsigned long long hi) {
  return hi > lo ? (uint32_t)min(hi - lo, (unsigned long long)kAckMaxWindow) : 0u;
}

__device__ __forceinline__ uint32_t ack_write(const AckWireArgs& a, uint64_t i, uint32_t lane) {
  const uint32_t conn = a.ack_conn[i];
  const bool known = conn < a.n_conns;  // (uniform, as everything read per ack)
  const unsigned long long given = a.largest_observed[i];
  const uint32_t given_hash = a.entropy_hash[i];
  const bool cut_before = a.truncated[i] != 0;
  const uint32_t rp = a.range_ptr[i], n_int = min(a.range_ptr[i + 1u] - rp, 255u);
  const uint32_t cap = a.out_cap[i];
  uint8_t* const frame = a.out + a.out_off[i];

  // GetAckFrameInfo
  uint32_t my_runs = 0, my_mm = 1;
  unsigned long long below = 0;  // (the end of the interval under this trip's first)
  for (uint32_t t0 = 0; t0 < n_int; t0 += 64u) {
    const uint32_t idx = t0 + lane;
    const bool in = idx < n_int;
    const uint32_t ic = in ? idx : n_int - 1u;  // (clamped, not masked)
    const unsigned long long lo = a.range_lo[(uint64_t)rp + ic], hi = a.range_hi[(uint64_t)rp + ic];
    // (every lane shuffles before anything is compared)
    const uint32_t src = lane ? lane - 1u : 0u;
    const uint32_t p_lo = lane_read((uint32_t)hi, src), p_hi = lane_read((uint32_t)(hi >> 32), src);
    const uint32_t e_lo = lane_read((uint32_t)hi, 63u), e_hi = lane_read((uint32_t)(hi >> 32), 63u);
    const unsigned long long prev = lane ? ((unsigned long long)p_hi << 32 | p_lo) : below;
    if (in) {
      my_runs += (ackw_span(lo, hi) + 255u) >> 8;
      if (idx != 0u) my_mm = max(my_mm, ackw_length(lo - (prev - 1u)));
      if (idx == n_int - 1u) my_mm = max(my_mm, ackw_length(given - (hi - 1u)));
    }
    below = (unsigned long long)e_hi << 32 | e_lo;
  }
  const uint32_t n_runs = wave_sum(my_runs), mm = wave_max(my_mm), ll = ackw_length(given);
  // (the framer subtracts unsigned: with less room than the minimum every range
  // "fits", and the frame fails at a later byte)
  const uint32_t fixed = 6u + ll;
  const uint32_t max_num = cap < fixed ? 255u : min(255u, (cap - fixed) / (mm + 1u));
  const bool cut = n_runs > max_num, trunc = cut || cut_before;
  const uint32_t kept = min(n_runs, max_num);
  const uint32_t first_range = 4u + ll + (trunc ? 0u : 1u) + 1u;  // behind the range count
  const uint32_t rev_at = first_range + kept * (mm + 1u);         // the revived count
  const uint32_t mandatory = n_runs != 0u ? rev_at + 1u : first_range - 1u;
  const bool fits = known && mandatory <= cap;

  unsigned long long largest = given;
  uint32_t hash = given_hash, length = 0;
  if (fits) {
    length = mandatory;
    if (n_runs != 0u) {
      uint32_t base = 0;  // the ranges below this trip's intervals
      for (uint32_t t0 = 0; t0 < n_int; t0 += 64u) {
        const uint32_t idx = t0 + lane;
        const bool in = idx < n_int;
        const uint32_t ic = in ? idx : n_int - 1u;  // (clamped, not masked)
        const unsigned long long lo = a.range_lo[(uint64_t)rp + ic],
                                 hi = a.range_hi[(uint64_t)rp + ic];
        // what lies above the interval's last number: the next interval, or the largest
        const unsigned long long above =
            ic + 1u < n_int ? a.range_lo[(uint64_t)rp + ic + 1u] : given + 1u;
        const uint32_t span = ackw_span(lo, hi);
        const uint32_t runs = in ? (span + 255u) >> 8 : 0u;
        const uint32_t incl = wave_incl_scan(runs, lane);
        const uint32_t first = base + incl - runs;  // my interval's first range
        // the first range dropped starts the cut
        const uint64_t bc = __ballot(cut && first <= kept && kept < first + runs);
        const unsigned long long at = lo + ((kept - first) << 8);
        const uint32_t src = bc != 0ull ? (uint32_t)__builtin_ctzll(bc) : 0u;
        const uint32_t c_lo = lane_read((uint32_t)at, src), c_hi = lane_read((uint32_t)(at >> 32), src);
        if (bc != 0ull) largest = ((unsigned long long)c_hi << 32 | c_lo) - 1u;
        for (uint32_t j = 0; j < runs && first + j < kept; ++j) {
          const uint32_t len = min(256u, span - (j << 8));
          uint8_t* const p = frame + first_range + (kept - 1u - (first + j)) * (mm + 1u);
          ackw_put(p, mm, j + 1u == runs ? above - hi : 0ull);
          p[mm] = (uint8_t)(len - 1u);
        }
        base += lane_read(incl, 63u);
      }
      if (cut) {  // EntropyHash(largest): take the numbers above it out of the hash
        const uint32_t len = (uint32_t)min(given - largest, (unsigned long long)a.window);
        const uint32_t from = (uint32_t)largest + 1u;
        uint32_t x = 0;
        for (uint32_t j0 = 0; j0 < len; j0 += 64u) {
          const uint32_t j = j0 + lane;
          const uint32_t jc = j < len ? j : len - 1u;  // (clamped, not masked)
          const uint32_t cell = a.rcv_cells[ack_cell_index(conn, a.window, from + jc)];
          if (j < len && (cell & kCellReceived) != 0u) x ^= ((cell >> 1) & 1u) << ((from + j) & 7u);
        }
        hash ^= wave_xor(x);
      }
      // the revived tail: the newest at or below the largest written, newest first
      const uint32_t vp = a.rev_ptr[i];
      const uint32_t n_rev = a.rev_pn ? min(a.rev_ptr[i + 1u] - vp, 255u) : 0u;
      uint32_t at_or_below = 0;
      for (uint32_t t0 = 0; t0 < n_rev; t0 += 64u) {
        const uint32_t idx = t0 + lane;
        const uint32_t ic = idx < n_rev ? idx : n_rev - 1u;  // (clamped, not masked)
        const unsigned long long pn = a.rev_pn[(uint64_t)vp + ic];
        at_or_below += (uint32_t)__popcll(__ballot(idx < n_rev && pn <= largest));
      }
      const uint32_t n_out = min(at_or_below, min(255u, (cap - mandatory) / ll));
      for (uint32_t t = lane; t < n_out; t += 64u)
        ackw_put(frame + rev_at + 1u + t * ll, ll, a.rev_pn[(uint64_t)vp + at_or_below - 1u - t]);
      if (lane == 0u) {
        frame[first_range - 1u] = (uint8_t)kept;
        frame[rev_at] = (uint8_t)n_out;
      }
      length += n_out * ll;
    }
    if (lane == 0u) {
      frame[0] = (uint8_t)(0x40u | (n_runs != 0u ? 0x20u : 0u) | (trunc ? 0x10u : 0u) |
                           (ll >> 1) << 2 | mm >> 1);
      frame[1] = (uint8_t)hash;
      ackw_put(frame + 2, ll, largest);
      const uint32_t delay = a.ack_delay_us ? ackw_ufloat16(a.ack_delay_us[i]) : 0xFFFFu;
      frame[2u + ll] = (uint8_t)delay;
      frame[3u + ll] = (uint8_t)(delay >> 8);
      if (!trunc) frame[4u + ll] = 0;  // no receipt times
    }
  }
  const uint32_t status = !known ? 3u /* QFEC_ACKW_RANGE */
                          : !fits ? 2u /* QFEC_ACKW_NO_ROOM */
                                  : (uint32_t)cut /* QFEC_ACKW_CUT : QFEC_ACKW_WRITTEN */;
  if (lane == 0u) {
    a.out_len[i] = (uint16_t)(fits ? a.prefix_len + length : 0u);
    a.wire_largest[i] = largest;
    a.wire_hash[i] = (uint8_t)hash;
    a.ack_status[i] = (uint8_t)status;
  }
  return status;
}

__global__ __launch_bounds__(kReviveTile) void ack_write_kernel(AckWireArgs a) {
  __shared__ uint32_t s_w[kTurnWaves * 4];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  uint32_t n[4] = {0, 0, 0, 0};  // the wave's acks per status (uniform)
  const uint64_t step = (uint64_t)gridDim.x * kTurnWaves;
  for (uint64_t i = (uint64_t)blockIdx.x * kTurnWaves + wave; i < a.n_acks; i += step) {
    const uint32_t status = ack_write(a, i, lane);
#pragma unroll
    for (uint32_t c = 0; c < 4u; ++c) n[c] += (uint32_t)(status == c);
  }
  const uint32_t t = block_sum(n, lane, wave, s_w);
  if (tid < 4u && t != 0u) {
    if (a.counts) atomicAdd(&a.counts[tid], (unsigned long long)t);
    if (tid == 3u) atomicOr(a.err, kErrMissingIndex);
  }
}

// ---------------------------------------------------------------------------
// Frames on the device (qfec_scan_frames): QuicFramer::ProcessFrameData over a
// turn's packets, behind the parse, and the newest STOP_WAITING per connection.
// ---------------------------------------------------------------------------
// One lane per packet walks its packet's frames, twice:
//   count : the verdict, the frames the packet lists (n_frm), its last
//           STOP_WAITING (pkt_least, pkt_hash) and, where that one is newer
//           than the connection's, a 64-bit atomicMax of the packet number into
//           the connection's word of the scratch;
//           nine tallies, and the frames of the trip's 256 packets, a tile;
//   scan  : one workgroup over the tiles' sums; the total and the overflow;
//   fill  : frm_ptr[p] from the tile's offset and a workgroup scan of n_frm,
//           then the walk again over the OK packets, every frame stored at
//           frm_ptr[p] + its rank where that lies below frm_cap; a packet whose
//           number is its connection's maximum offers its arrival index to a
//           32-bit atomicMin;
//   set   : one lane per connection takes the picked packet's frame.
// A maximum and a minimum do not depend on the order of their operands, so the
// atomics show nowhere.  The lanes of a wave follow packets of their own: the
// walk's loop diverges and holds no shuffle, ballot or barrier; the tallies are
// taken behind it, where the wave is whole again.  A byte is loaded only under
// the bounds check that puts it inside [body_off, body_off + body_len), always
// as a byte, so no alignment matters; a trip consumes at least the type byte
// and the loop ends at max_frames, so a walk is at most min(max_frames,
// body_len) trips.  Values are assembled from bytes in 32-bit halves with
// constant shifts (the gfx950 64-bit shift hazard).

// n <= 8 bytes at p, little-endian; the caller has checked that they lie inside
__device__ __forceinline__ void frm_get(const uint8_t* p, uint32_t n, uint32_t& lo, uint32_t& hi) {
  lo = 0u;
  hi = 0u;
#pragma unroll
  for (uint32_t b = 0; b < 4u; ++b)
    if (b < n) lo |= (uint32_t)p[b] << (8u * b);
#pragma unroll
  for (uint32_t b = 4; b < 8u; ++b)
    if (b < n) hi |= (uint32_t)p[b] << (8u * (b - 4u));
}

// ReadSequenceNumberLength: 1, 2, 4, 6
__device__ __forceinline__ uint32_t frm_length(uint32_t c) { return c == 3u ? 6u : 1u << c; }

struct FrmWalk {
  uint32_t status;  // the verdict
  uint32_t n;       // frames walked before it
  uint32_t n_stream, n_ack, n_sw;  // of those
  bool has_sw;                  // a STOP_WAITING among them whose last has least_unacked > 0
  unsigned long long sw_least;  // the last one's
  uint32_t sw_hash;
};

// Packet p's frames: len > 0 bytes at body, packet number pn in pn_len bytes on
// the wire.  FILL: frame k goes to entry base + k of the table.
template <bool FILL>
__device__ __forceinline__ FrmWalk frames_walk(const FramesArgs& a, const uint8_t* body,
                                               uint64_t off, uint32_t len, unsigned long long pn,
                                               uint32_t pn_len, uint32_t p, uint32_t base) {
  FrmWalk w{kFrmOk, 0u, 0u, 0u, 0u, false, 0ull, 0u};
  uint32_t o = 0;
  while (o < len) {
    if (w.n == a.max_frames) {
      w.status = kFrmTooMany;
      break;
    }
    const uint32_t at = o, t = body[o];
    o += 1u;
    const uint32_t room = len - o;
    uint32_t type = t, flags = 0, f_off = 0, f_len = 0, id = 0, v_lo = 0, v_hi = 0, code = 0;
    uint32_t bad = 0, x;
    bool placed = false;  // the kind names an offset
    if ((t & 0x80u) != 0u) {  // ProcessStreamFrame: 1 fin len ooo ss
      const uint32_t idl = (t & 3u) + 1u, ob = (t >> 2) & 7u, ofl = ob != 0u ? ob + 1u : 0u;
      const bool has_len = (t & 0x20u) != 0u;
      const uint32_t head = idl + ofl + (has_len ? 2u : 0u);
      if (room < head) {
        bad = kFrmStream;
      } else {
        frm_get(body + o, idl, id, x);
        frm_get(body + o + idl, ofl, v_lo, v_hi);
        uint32_t n = room - head;
        if (has_len) {
          uint32_t l;
          frm_get(body + o + idl + ofl, 2u, l, x);
          if (l > n) bad = kFrmStream;
          n = l;
        }
        type = kFrameStream;
        flags = ((t >> 6) & 1u) | (has_len ? 2u : 0u);
        placed = true;
        f_off = o + head;
        f_len = n;
        o = f_off + n;
      }
    } else if ((t & 0x40u) != 0u) {  // ProcessAckFrame, stepped over
      const uint32_t mm = frm_length(t & 3u), ll = frm_length((t >> 2) & 3u);
      uint32_t q = o;
      bool whole = room >= 3u + ll;  // hash, largest, delay
      if (whole) {
        code = body[q];
        frm_get(body + q + 1u, ll, v_lo, v_hi);
        q += 3u + ll;
        if ((t & 0x10u) == 0u) {  // ProcessTimestampsInAckFrame
          whole = q < len;
          if (whole) {
            const uint32_t n = body[q];
            const uint32_t need = n != 0u ? 5u + (n - 1u) * 3u : 0u;
            q += 1u;
            whole = len - q >= need;
            q += need;
          }
        }
        if (whole && (t & 0x20u) != 0u) {
          whole = q < len;
          if (whole) {
            const uint32_t need = (uint32_t)body[q] * (mm + 1u);
            q += 1u;
            whole = len - q >= need;
            q += need;
          }
          if (whole && a.revived_tail != 0u) {
            whole = q < len;
            if (whole) {
              const uint32_t need = (uint32_t)body[q] * ll;
              q += 1u;
              whole = len - q >= need;
              q += need;
            }
          }
        }
      }
      if (!whole) bad = kFrmAck;
      type = kFrameAck;
      flags = t & 0x3Fu;
      placed = true;
      f_off = at;
      f_len = q - at;
      o = q;
    } else if ((t & 0x20u) != 0u) {
      bad = kFrmIllegalType;
    } else if (t == 0u) {  // PADDING: the rest of the packet
      placed = true;
      f_off = o;
      f_len = room;
      o = len;
    } else if (t == 1u) {  // RST_STREAM
      if (room < 16u) {
        bad = kFrmRst;
      } else {
        frm_get(body + o, 4u, id, x);
        frm_get(body + o + 4u, 8u, v_lo, v_hi);
        frm_get(body + o + 12u, 4u, code, x);
        o += 16u;
      }
    } else if (t == 2u || t == 3u) {  // CONNECTION_CLOSE, GOAWAY
      const uint32_t head = t == 2u ? 6u : 10u, cls = t == 2u ? kFrmClose : kFrmGoaway;
      if (room < head) {
        bad = cls;
      } else {
        uint32_t n;
        frm_get(body + o, 4u, code, x);
        if (t == 3u) frm_get(body + o + 4u, 4u, id, x);
        frm_get(body + o + head - 2u, 2u, n, x);
        if (n > room - head) bad = cls;
        placed = true;
        f_off = o + head;
        f_len = n;
        o = f_off + n;
      }
    } else if (t == 4u) {  // WINDOW_UPDATE
      if (room < 12u) {
        bad = kFrmWindowUpdate;
      } else {
        frm_get(body + o, 4u, id, x);
        frm_get(body + o + 4u, 8u, v_lo, v_hi);
        o += 12u;
      }
    } else if (t == 5u) {  // BLOCKED
      if (room < 4u) {
        bad = kFrmBlocked;
      } else {
        frm_get(body + o, 4u, id, x);
        o += 4u;
      }
    } else if (t == kFrameStopWaiting) {  // (the entropy byte: every version up to 33)
      if (room < 1u + pn_len) {
        bad = kFrmStopWaiting;
      } else {
        uint32_t d_lo, d_hi;
        code = body[o];
        frm_get(body + o + 1u, pn_len, d_lo, d_hi);
        const unsigned long long delta = (unsigned long long)d_hi << 32 | d_lo;
        if (delta > pn) bad = kFrmBadLeast;
        const unsigned long long least = pn - delta;
        v_lo = (uint32_t)least;
        v_hi = (uint32_t)(least >> 32);
        o += 1u + pn_len;
      }
    } else if (t == 7u) {  // PING
    } else if (t == 8u) {  // PATH_CLOSE
      if (room < 1u) {
        bad = kFrmPathClose;
      } else {
        id = body[o];
        o += 1u;
      }
    } else {
      bad = kFrmIllegalType;
    }
    if (bad != 0u) {
      w.status = bad;
      break;
    }
    const unsigned long long val = (unsigned long long)v_hi << 32 | v_lo;
    if (FILL) {
      const uint32_t e = base + w.n;
      if (e < a.frm_cap) {
        a.frm_pkt[e] = p;
        a.frm_type[e] = (uint8_t)type;
        a.frm_flags[e] = (uint8_t)flags;
        a.frm_off[e] = placed ? off + f_off : 0ull;
        a.frm_len[e] = (uint16_t)f_len;
        a.frm_id[e] = id;
        a.frm_val[e] = val;
        a.frm_code[e] = code;
      }
    }
    w.n_stream += (uint32_t)(type == kFrameStream);
    w.n_ack += (uint32_t)(type == kFrameAck);
    if (type == kFrameStopWaiting) {
      w.n_sw += 1u;
      w.has_sw = val != 0ull;
      w.sw_least = val;
      w.sw_hash = code;
    }
    w.n += 1u;
  }
  return w;
}

template <bool FILL>
__global__ __launch_bounds__(kReviveTile) void frames_walk_kernel(FramesArgs a) {
  __shared__ uint32_t s_w[kTurnWaves * 9];
  __shared__ uint32_t s_t[kTurnWaves];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  // the wave's packets (uniform): OK, skipped, rejected, too many, caller errors;
  // and this lane's frames listed: stream, ack, stop waiting, other
  uint32_t n[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  uint32_t mine[4] = {0, 0, 0, 0};
  const uint64_t step = (uint64_t)gridDim.x * kReviveTile;
  for (uint64_t p0 = (uint64_t)blockIdx.x * kReviveTile; p0 < a.n_packets; p0 += step) {
    const uint64_t p = p0 + tid;
    const bool in = p < a.n_packets;
    const uint64_t pc = in ? p : a.n_packets - 1u;  // (clamped, not masked)
    const uint64_t off = a.body_off[pc];
    const uint32_t len = a.body_len[pc];
    const unsigned long long pn = a.packet_number[pc];
    const uint32_t conn = a.pkt_conn[pc], pn_len = a.pkt_pn_len[pc];
    if (FILL) {
      const bool ok = in && a.frm_status[pc] == kFrmOk;  // (OK: conn < n_conns, len > 0)
      // frm_ptr: the frames of the tiles in front, and of the tile's packets in front
      uint32_t in_tile;
      const uint32_t base = a.tile_off[p0 / kReviveTile] +
                            block_excl_scan<kTurnWaves>(in ? a.n_frm[pc] : 0u, lane, wave, s_t, in_tile);
      if (in) a.frm_ptr[p] = base;
      if (ok) {
        const FrmWalk w =
            frames_walk<true>(a, a.bytes + off, off, len, pn, pn_len, (uint32_t)p, base);
        if (w.has_sw && pn == a.top[conn]) atomicMin(&a.pick[conn], (uint32_t)p);
      }
    } else {
      const uint32_t h = a.hdr ? a.hdr[pc] : 0u;
      uint32_t status;
      if (h >= kHdrFailed || (h & kPrivateFlagFec) != 0u) status = kFrmSkipped;
      else if (pn_len != 1u && pn_len != 2u && pn_len != 4u && pn_len != 6u) status = kFrmPnLen;
      else if (conn >= a.n_conns) status = kFrmRange;
      else if (len == 0u) status = kFrmNoFrames;
      else status = kFrmOk;
      FrmWalk w{status, 0u, 0u, 0u, 0u, false, 0ull, 0u};
      if (in && status == kFrmOk)
        w = frames_walk<false>(a, a.bytes + off, off, len, pn, pn_len, (uint32_t)p, 0u);
      const bool ok = in && w.status == kFrmOk;
      const uint32_t listed = ok ? w.n : 0u;
      if (in) {
        a.frm_status[p] = (uint8_t)w.status;
        a.n_frm[p] = listed;
      }
      // (behind the walk: the wave is whole again)  The trip's packets are one
      // tile of the scan: its frames, for the one-workgroup pass over the tiles.
      const uint32_t in_tile = block_sum(wave_sum(listed), lane, wave, s_t);
      if (tid == 0u) a.tile_off[p0 / kReviveTile] = in_tile;
      if (ok) {
        mine[0] += w.n_stream;
        mine[1] += w.n_ack;
        mine[2] += w.n_sw;
        mine[3] += w.n - w.n_stream - w.n_ack - w.n_sw;
        if (w.has_sw) {
          a.pkt_least[p] = w.sw_least;
          a.pkt_hash[p] = (uint8_t)w.sw_hash;
          if (pn > a.sw_seen[conn]) retire_max(&a.top[conn], pn);
        }
      }
      const uint32_t s = w.status;
      n[0] += (uint32_t)__popcll(__ballot(ok));
      n[1] += (uint32_t)__popcll(__ballot(in && s == kFrmSkipped));
      n[2] += (uint32_t)__popcll(__ballot(in && s >= kFrmNoFrames && s <= kFrmBadLeast));
      n[3] += (uint32_t)__popcll(__ballot(in && s == kFrmTooMany));
      n[4] += (uint32_t)__popcll(__ballot(in && (s == kFrmPnLen || s == kFrmRange)));
    }
  }
  if (!FILL) {
#pragma unroll
    for (uint32_t c = 0; c < 4u; ++c) n[5u + c] = wave_sum(mine[c]);
    const uint32_t t = block_sum(n, lane, wave, s_w);
    if (tid < 9u && t != 0u) {
      if (a.counts) atomicAdd(&a.counts[tid], (unsigned long long)t);
      if (tid == 4u) atomicOr(a.err, kErrMissingIndex);
    }
  }
}

__global__ __launch_bounds__(kRvScanBlock) void frames_scan_kernel(FramesArgs a) {
  __shared__ uint32_t s_w[kRvScanBlock / 64];
  const uint64_t total =
      tile_scan_in_place(a.tile_off, (a.n_packets + kReviveTile - 1u) / kReviveTile, s_w);
  if (threadIdx.x == 0u) {
    a.frm_ptr[a.n_packets] = (uint32_t)total;
    if (a.counts) {
      a.counts[9] = total;
      a.counts[10] = total > a.frm_cap ? total - a.frm_cap : 0ull;
    }
  }
}

__global__ __launch_bounds__(kReviveTile) void frames_set_kernel(FramesArgs a) {
  __shared__ uint32_t s_w[kTurnWaves * 2];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  uint32_t n[2] = {0, 0};  // the wave's connections (uniform): replaced, and with a lower least
  const uint64_t step = (uint64_t)gridDim.x * kReviveTile;
  for (uint64_t c0 = (uint64_t)blockIdx.x * kReviveTile; c0 < a.n_conns; c0 += step) {
    const uint64_t c = c0 + tid;
    const bool in = c < a.n_conns;
    const uint32_t cc = (uint32_t)(in ? c : a.n_conns - 1u);  // (clamped, not masked)
    const uint32_t pick = a.pick[cc];
    const bool won = in && pick != 0xFFFFFFFFu;  // (a pick is a packet: below n_packets)
    bool lower = false;
    if (in) a.sw_conn[cc] = cc;
    if (won) {
      const unsigned long long least = a.pkt_least[pick];
      lower = least < a.sw_least[cc];
      a.sw_seen[cc] = a.top[cc];
      a.sw_least[cc] = least;
      a.sw_hash[cc] = a.pkt_hash[pick];
    }
    n[0] += (uint32_t)__popcll(__ballot(won));
    n[1] += (uint32_t)__popcll(__ballot(lower));
  }
  const uint32_t t = block_sum(n, lane, wave, s_w);
  if (tid < 2u && t != 0u && a.counts) atomicAdd(&a.counts[11u + tid], (unsigned long long)t);
}

// ---------------------------------------------------------------------------
// The launches.
// ---------------------------------------------------------------------------
// The grids of the turn passes, in workgroups of kReviveTile lanes that loop.
// Per tile, where a workgroup scans or ranks a tile of n elements at a time:
inline uint32_t tile_grid(uint64_t n) {
  return (uint32_t)std::min<uint64_t>(revive_tiles(n), kMaxBlocks256);
}
// per packet, where it keeps tallies or only streams: sixteen per CU, so that
// the tallies cost a few atomics per workgroup and not per 256 packets
inline uint32_t per_packet_grid(uint64_t n, uint32_t ncu) {
  return (uint32_t)std::min<uint64_t>(revive_tiles(n), (uint64_t)(ncu ? ncu : 256u) * 16u);
}

// One kernel of a call's chain, launched on s unless a launch before it failed
// (e, what the launch before returned); returns the chain's first failure.
template <typename Args>
hipError_t launch_pass(hipError_t e, void (*kernel)(Args), uint32_t grid, uint32_t block,
                       hipStream_t s, const Args& a) {
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, s, a);
  return hipGetLastError();
}

// The first three launches of every revive (classify, scan, emit), for any of
// the revive argument structs.
template <typename Args>
hipError_t launch_revive_passes_as(const Args& a, hipStream_t s) {
  hipError_t e = launch_pass(hipSuccess, revive_classify_kernel<false, Args>,
                             tile_grid(a.n_groups), kReviveTile, s, a);
  e = launch_pass(e, revive_scan_kernel<Args>, 1, kRvScanBlock, s, a);
  e = launch_pass(e, revive_classify_kernel<true, Args>, tile_grid(a.n_groups), kReviveTile, s, a);
  return e;
}

}  // namespace

// ... by name for each struct: their callers launch an XOR kernel over the
// work list next and sit with those kernels, in qfec_kernels.hip.
hipError_t launch_revive_passes(const ReviveArgs& a, hipStream_t s) {
  return launch_revive_passes_as(a, s);
}
hipError_t launch_revive_passes(const ReviveRaggedArgs& a, hipStream_t s) {
  return launch_revive_passes_as(a, s);
}
hipError_t launch_revive_passes(const CloseArgs& a, hipStream_t s) {
  return launch_revive_passes_as(a, s);
}
hipError_t launch_revive_passes(const TrackedCloseArgs& a, hipStream_t s) {
  return launch_revive_passes_as(a, s);
}

hipError_t launch_admit_ragged(const AdmitArgs& a, hipStream_t s) {
  if (a.n_groups == 0) return hipSuccess;
  hipError_t e = launch_pass(hipSuccess, admit_decide_kernel, tile_grid(a.n_groups), kReviveTile, s, a);
  e = launch_pass(e, admit_scan_kernel, 1, kRvScanBlock, s, a);
  e = launch_pass(e, admit_scatter_kernel, tile_grid(a.n_groups), kReviveTile, s, a);
  return e;
}

hipError_t launch_bin_arrivals(const BinArgs& a, hipStream_t s) {
  if (a.n_packets == 0 || a.n_slots == 0) return hipSuccess;
  hipError_t e = hipMemsetAsync(a.tally, 0, bin_scratch_zeroed(a.n_slots), s);
  const uint32_t pgrid = per_packet_grid(a.n_packets, a.ncu), sgrid = tile_grid(a.n_slots);
  e = launch_pass(e, bin_count_kernel, pgrid, kReviveTile, s, a);
  e = launch_pass(e, bin_tile_kernel, sgrid, kReviveTile, s, a);
  e = launch_pass(e, bin_scan_kernel, 1, kRvScanBlock, s, a);
  e = launch_pass(e, bin_ptr_kernel, sgrid, kReviveTile, s, a);
  e = launch_pass(e, bin_scatter_kernel, pgrid, kReviveTile, s, a);
  e = launch_pass(e, bin_order_kernel, sgrid, kReviveTile, s, a);
  return e;
}

hipError_t launch_assign_slots(const AssignArgs& a, hipStream_t s) {
  if (a.n_packets == 0) return hipSuccess;
  hipError_t e = hipMemsetAsync(a.table, 0xFF, ((uint64_t)a.cap_mask + 1u) * 16u, s);
  const uint32_t pgrid = per_packet_grid(a.n_packets, a.ncu), ptiles = tile_grid(a.n_packets);
  // (no slots: one workgroup still zeroes counts)
  const uint32_t stiles = std::max(tile_grid(a.n_slots), 1u);
  e = launch_pass(e, assign_slots_kernel, stiles, kReviveTile, s, a);
  e = launch_pass(e, assign_probe_kernel, pgrid, kReviveTile, s, a);
  e = launch_pass(e, assign_tile_kernel, ptiles, kReviveTile, s, a);
  e = launch_pass(e, assign_scan_kernel, 1, kRvScanBlock, s, a);
  e = launch_pass(e, assign_free_kernel, stiles, kReviveTile, s, a);
  e = launch_pass(e, assign_open_kernel, ptiles, kReviveTile, s, a);
  e = launch_pass(e, assign_emit_kernel, pgrid, kReviveTile, s, a);
  return e;
}

hipError_t launch_retire_groups(const RetireArgs& a0, hipStream_t s) {
  if (a0.n_packets == 0 && a0.n_slots == 0 && a0.n_raise == 0) return hipSuccess;
  RetireArgs a = a0;
  hipError_t e = hipMemsetAsync(a.tally, 0, retire_scratch_zeroed(a.n_conns, a.max_groups), s);
  const uint32_t pgrid = per_packet_grid(a.n_packets, a.ncu), stiles = tile_grid(a.n_slots);
  if (a.n_raise != 0)
    e = launch_pass(e, retire_raise_kernel, per_packet_grid(a.n_raise, a.ncu), kReviveTile, s, a);
  if (a.max_groups != 0 && a.n_conns != 0 && (a.n_packets != 0 || a.n_slots != 0)) {
    const uint32_t rgrid = per_packet_grid(std::max<uint64_t>(a.n_packets, a.n_slots), a.ncu);
    for (a.round = 0; a.round <= a.max_groups; ++a.round)
      e = launch_pass(e, retire_round_kernel, rgrid, kReviveTile, s, a);
    a.round = 0;
    e = launch_pass(e, retire_mark_kernel, per_packet_grid(a.n_conns, a.ncu), kReviveTile, s, a);
  }
  if (a.n_packets != 0) e = launch_pass(e, retire_filter_kernel, pgrid, kReviveTile, s, a);
  if (a.n_slots != 0) e = launch_pass(e, retire_classify_kernel, stiles, kReviveTile, s, a);
  e = launch_pass(e, retire_scan_kernel, 1, kRvScanBlock, s, a);  // (counts, whatever is empty)
  if (a.n_slots != 0) e = launch_pass(e, retire_close_kernel, stiles, kReviveTile, s, a);
  return e;
}

hipError_t launch_parse_opened(const ParseArgs& a, hipStream_t s) {
  if (a.n_packets == 0) return hipSuccess;
  hipError_t e = a.counts ? hipMemsetAsync(a.counts, 0, 6 * sizeof(uint64_t), s) : hipSuccess;
  return launch_pass(e, parse_opened_kernel, per_packet_grid(a.n_packets, a.ncu), kReviveTile, s, a);
}

hipError_t launch_write_private_headers(const WriteHeadersArgs& a, hipStream_t s) {
  if (a.n_packets == 0) return hipSuccess;
  hipError_t e = a.counts ? hipMemsetAsync(a.counts, 0, 2 * sizeof(uint64_t), s) : hipSuccess;
  return launch_pass(e, write_headers_kernel, per_packet_grid(a.n_packets, a.ncu), kReviveTile, s, a);
}

hipError_t launch_record_received(const RecordArgs& a, hipStream_t s) {
  if (a.n_packets == 0 && a.n_groups == 0 && a.n_raise == 0) return hipSuccess;
  hipError_t e =
      a.counts ? hipMemsetAsync(a.counts, 0, kRecordCounts * sizeof(uint64_t), s) : hipSuccess;
  if (a.n_packets != 0) {
    const uint32_t pgrid = per_packet_grid(a.n_packets, a.ncu);
    if (e == hipSuccess && a.n_conns != 0)
      e = hipMemsetAsync(a.seen, 0, record_scratch_bytes(a.n_conns), s);
    e = launch_pass(e, record_classify_kernel, pgrid, kReviveTile, s, a);
    if (a.n_conns != 0) {  // (else nothing was RECORDED)
      e = launch_pass(e, record_advance_kernel, per_packet_grid(a.n_conns, a.ncu), kReviveTile, s, a);
      e = launch_pass(e, record_set_kernel, pgrid, kReviveTile, s, a);
    }
  }
  if (a.n_groups != 0)
    e = launch_pass(e, record_revived_kernel, per_packet_grid(a.n_groups, a.ncu), kReviveTile, s, a);
  if (a.n_raise != 0)  // (a wave per raise)
    e = launch_pass(e, record_raise_kernel, per_packet_grid((uint64_t)a.n_raise * 64u, a.ncu),
                    kReviveTile, s, a);
  return e;
}

hipError_t launch_build_acks(const AcksArgs& a, hipStream_t s) {
  if (a.n_acks == 0) return hipSuccess;
  const uint32_t wgrid = per_packet_grid((uint64_t)a.n_acks * 64u, a.ncu);  // (a wave per ack)
  hipError_t e = launch_pass(hipSuccess, acks_walk_kernel<false>, wgrid, kReviveTile, s, a);
  e = launch_pass(e, acks_scan_kernel, 1, kRvScanBlock, s, a);
  return launch_pass(e, acks_walk_kernel<true>, wgrid, kReviveTile, s, a);
}

hipError_t launch_write_ack_frames(const AckWireArgs& a, hipStream_t s) {
  if (a.n_acks == 0) return hipSuccess;
  hipError_t e =
      a.counts ? hipMemsetAsync(a.counts, 0, kAckWireCounts * sizeof(uint64_t), s) : hipSuccess;
  const uint32_t wgrid = per_packet_grid((uint64_t)a.n_acks * 64u, a.ncu);  // (a wave per ack)
  return launch_pass(e, ack_write_kernel, wgrid, kReviveTile, s, a);
}

hipError_t launch_scan_frames(const FramesArgs& a, hipStream_t s) {
  if (a.n_packets == 0) return hipSuccess;
  hipError_t e =
      a.counts ? hipMemsetAsync(a.counts, 0, kFramesCounts * sizeof(uint64_t), s) : hipSuccess;
  if (e == hipSuccess && a.n_conns != 0)
    e = hipMemsetAsync(a.top, 0, (size_t)a.n_conns * sizeof(uint64_t), s);
  if (e == hipSuccess && a.n_conns != 0)
    e = hipMemsetAsync(a.pick, 0xFF, (size_t)a.n_conns * sizeof(uint32_t), s);
  const uint32_t pgrid = per_packet_grid(a.n_packets, a.ncu);
  e = launch_pass(e, frames_walk_kernel<false>, pgrid, kReviveTile, s, a);
  e = launch_pass(e, frames_scan_kernel, 1, kRvScanBlock, s, a);
  e = launch_pass(e, frames_walk_kernel<true>, pgrid, kReviveTile, s, a);
  if (a.n_conns != 0)
    e = launch_pass(e, frames_set_kernel, per_packet_grid(a.n_conns, a.ncu), kReviveTile, s, a);
  return e;
}

}  // namespace qfec
