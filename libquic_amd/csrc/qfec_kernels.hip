// qfec_kernels.hip — gfx950 (CDNA4) kernels for the QUIC FEC XOR path.
//
// What they compute (the historical QuicFecGroup whose
// sources are gone from the snapshot, evidence /root/reference/Makefile:5332-5384):
//   encode : parity[j]  = XOR_i p_i[j]                       (zero padded rows)
//   recover: revived[j] = parity[j] XOR_{i != m} p_i[j]
// Both are one streaming pass over HBM with one integer op per byte: the
// roofline is HBM bandwidth (no MFMA — this is a byte-wise XOR reduction).
//
// Layout and mapping:
//  * Fixed shape [G][k][L] (L = 1350 in the headline config).  A row is split
//    into C = ceil(L/16) 16-byte windows; lane t of a group owns the window at
//    byte min(16t, L-16), so the last window ends exactly at the row end and
//    overlaps its neighbour (both lanes store identical bytes there).  No lane
//    ever touches memory outside its rows, no tail branch, no masking.
//    A 256-lane workgroup owns floor(256/C) whole groups (3 at L = 1350), so a
//    wave-instruction reads ~1 KiB of contiguous row bytes and workgroups never
//    split a group.
//  * Rows are only 2-byte aligned at L = 1350 (1350 = 2 mod 4).  gfx950 runs
//    global loads in unaligned-access mode, so every row load is ONE
//    global_load_dwordx4 regardless of alignment (checked in the .s); the
//    L2/TA handle the line crossing.
//  * Recover reads the parity row *in place of* the lost row: k loads per lane,
//    every one unconditional — the lost slot is never read and no lane idles.
//  * Batches of >= 6 phases (about 184K groups at L = 1350) run
//    phase_xor_kernel instead: the same lanes and loads in a persistent
//    one-workgroup-per-CU grid that separates the row reads and the parity
//    writes into grid-wide phases (0.80 of 8 TB/s on any buffer placement).
//  * Revive from receive maps (qfec_revive_batch): classify / scan / emit build
//    a packed list of the revivable groups on the device, and the recover
//    body above runs over that list only (revive_xor_kernel); for ragged
//    batches (qfec_revive_ragged) the same three kernels with k per group and
//    the ragged block body over the list (revive_ragged_kernel).
//  * Ragged CSR batches: eight groups per 4-wave block in one flat window
//    space (ragged_block_kernel; the one-group body below is its exact
//    fallback; two groups per wave, ragged_multi_kernel, for large batches of
//    small groups), lanes own 16-byte
//    windows of the packets; a window shorter than 16 bytes is loaded as the
//    16 bytes that end at the packet's last byte and shifted down (zero
//    fill), so again no load leaves the packet.
//  * Running group parities (qfec_accumulate_ragged): the same block body in a
//    third mode beside encode and recover -- the accumulators start from the
//    caller's rows (zero past their old lengths) and are stored back in place,
//    the lengths the running maxima (accumulate_ragged_kernel).
//  * Closing those rows (qfec_emit_accumulated / qfec_revive_accumulated): a
//    gather, one wave per row, chunks cut where the destination is 16-B
//    aligned (close_gather_kernel) -- over every group for the emit, over the
//    revive's work list (classify / scan / emit with k per group from group_k)
//    for the receiver's close.
//  * The receive maps on the device (qfec_admit_ragged / qfec_revive_tracked):
//    one running map per slot; decide / scan / scatter filter a turn's
//    candidates against it and the open call's ok flags into the tables the
//    accumulate folds (admit_*_kernel), and the receiver's close reads K and
//    the map by slot (the classify kernels instantiated for TrackedCloseArgs).
#include "qfec_internal.h"

#include <algorithm>
#include <type_traits>
#include <cstdlib>

namespace qfec {
namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr uint32_t kMaxPacket = 1452;  // kMaxPacketSize, quic_protocol.h:66
constexpr int kBlock = 256;

__device__ __forceinline__ u32x4 ld16(const uint8_t* p) {
  u32x4 v;
  __builtin_memcpy(&v, p, 16);
  return v;
}

template <bool NT>
__device__ __forceinline__ u32x4 ld16t(const uint8_t* p) {
  if constexpr (NT) {
    return __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
  } else {
    return ld16(p);
  }
}

__device__ __forceinline__ void st16(uint8_t* p, u32x4 v) { __builtin_memcpy(p, &v, 16); }

template <bool NT>
__device__ __forceinline__ void st16t(uint8_t* p, u32x4 v) {
  if constexpr (NT) {
    __builtin_nontemporal_store(v, reinterpret_cast<u32x4*>(p));
  } else {
    st16(p, v);
  }
}

// Wave max of 11-bit values by ballots, MSB first (no LDS round trips).
__device__ __forceinline__ uint32_t wave_max11(uint32_t v) {
  uint32_t mx = 0;
#pragma unroll
  for (int b = 10; b >= 0; --b) {
    const uint32_t cand = mx | (1u << b);
    if (__ballot(v >= cand) != 0ull) mx = cand;
  }
  return mx;
}

__device__ __forceinline__ bool wave_any(bool p) { return __ballot(p) != 0ull; }

// N rows r .. r+N-1 of a group, all N loads in flight before the first XOR
// (recover: row m is the parity row `par`).  The runtime-k bodies use it for
// their full batches AND their remainder (a switch on k - r picks N): round
// 4's remainder was a rolled loop, one load in flight per lane, which made
// the runtime-k phased kernel 1.1-2.5x slower than one-pass
// (profiles/round4/phase_k_table_nontemplated_r4o.txt, k = 6: 0.27 vs 0.69).
template <int N, bool RECOVER, bool NT>
__device__ __forceinline__ void xor_rows_n(u32x4& acc, const uint8_t* src, uint64_t row_stride,
                                           uint32_t r, uint32_t m, const uint8_t* par) {
  u32x4 v[N];
#pragma unroll
  for (int w = 0; w < N; ++w) {
    const uint8_t* q = (RECOVER && r + (uint32_t)w == m) ? par : src + (uint64_t)(r + w) * row_stride;
    v[w] = ld16t<NT>(q);
  }
#pragma unroll
  for (int w = 0; w < N; ++w) acc ^= v[w];
}

// Rows [0, k) of a group at runtime k: ceil(k / B) batches of loads in
// flight, their sizes as even as possible (k = 40, B = 32: 20 + 20, not
// 32 + 8 -- a batch is a round trip).  The phased kernel (one wave per SIMD:
// a lane's loads in flight are all the CU has) takes B = 32: round 5's
// B = 16 split k = 20 into 10 + 10 and read at 0.743 / 0.683 of 8 TB/s
// against 0.781 / 0.741 at k = 32 (16 + 16) (profiles/round5/
// phase_k_table_r5b.txt; round 6: profiles/round6/phase_k_table_r6*.txt).
template <int B, bool RECOVER, bool NT>
__device__ __forceinline__ void xor_rows_rt(u32x4& acc, const uint8_t* src, uint64_t row_stride,
                                            uint32_t k, uint32_t m, const uint8_t* par) {
  static_assert(B == 8 || B == 16 || B == 32, "batch of 8, 16 or 32 rows");
  const uint32_t nb = (k + B - 1) / B;
  const uint32_t base = nb ? k / nb : 0u, extra = k - base * nb;
  uint32_t r = 0;
  for (uint32_t b = 0; b < nb; ++b) {
    const uint32_t n = base + (b < extra ? 1u : 0u);
#define QFEC_REM(N)                                                 \
  case N:                                                           \
    xor_rows_n<N, RECOVER, NT>(acc, src, row_stride, r, m, par);    \
    break;
    if (B == 8 || n <= 8u) {
      switch (n) {
        QFEC_REM(1) QFEC_REM(2) QFEC_REM(3) QFEC_REM(4) QFEC_REM(5) QFEC_REM(6) QFEC_REM(7)
        QFEC_REM(8)
        default:
          break;
      }
    } else if constexpr (B >= 16) {
      if (B == 16 || n <= 16u) {
        switch (n) {
          QFEC_REM(9) QFEC_REM(10) QFEC_REM(11) QFEC_REM(12) QFEC_REM(13) QFEC_REM(14)
          QFEC_REM(15) QFEC_REM(16)
          default:
            break;
        }
      } else if constexpr (B == 32) {
        switch (n) {
          QFEC_REM(17) QFEC_REM(18) QFEC_REM(19) QFEC_REM(20) QFEC_REM(21) QFEC_REM(22)
          QFEC_REM(23) QFEC_REM(24) QFEC_REM(25) QFEC_REM(26) QFEC_REM(27) QFEC_REM(28)
          QFEC_REM(29) QFEC_REM(30) QFEC_REM(31) QFEC_REM(32)
          default:
            break;
        }
      }
    }
#undef QFEC_REM
    r += n;
  }
}

// ---------------------------------------------------------------------------
// Fixed shape, L >= 16.
// ---------------------------------------------------------------------------
// SM (recover, gpb <= 8): lost-slot indices by scalar loads, see below.
// INPL (encode form only): the in-slot recover written in place -- the
// group's output row is its own row missing[g] (which held the redundancy);
// a barrier between the loads and the stores keeps a wave from overwriting
// the bytes the overlapping last window of a neighbouring wave still reads.
//
// Variant measured and removed (the kernel with it as the template switch XCD,
// and the block mapping itself, are in git history at ace3ed3): XCD-aware
// workgroup order -- the blocks b, b + 8, ... that share an XCD and its L2
// take one contiguous share of the groups.  Fixed encode 0.99x, recover 1.00x
// (profiles/round1/tune_xcd_t2.txt); it does not change a buffer pair's
// placement mode either, +-1-5% (profiles/round1/place_order_p{1,2}.txt;
// DESIGN.md §4).  The only reuse between workgroups is one boundary line each.
template <int KC, bool RECOVER, bool NT, bool SM, bool INPL = false>
__global__ __launch_bounds__(kBlock) void fixed_xor_kernel(FixedArgs a, uint32_t C,
                                                           uint32_t gpb) {
  static_assert(!(INPL && RECOVER), "in place: the encode form over the k rows");
  const uint32_t tid = threadIdx.x;
  const uint32_t gl = tid / C;  // group within the workgroup
  const uint32_t t = tid - gl * C;
  const uint64_t gb = (uint64_t)blockIdx.x * gpb;
  const uint64_t g = gb + gl;
  if constexpr (INPL) {
    // no early return before the barrier: every wave reaches it
    const bool on = gl < gpb && g < a.n_groups;
    const uint64_t gg = on ? g : 0;
    const uint32_t off = min(t * 16u, a.L - 16u);
    const uint8_t* src = a.rows + gg * a.group_stride + off;
    const uint32_t k = KC > 0 ? (uint32_t)KC : a.k;
    const uint32_t m = on ? (uint32_t)a.inplace_missing[gg] : 0u;
    u32x4 acc = {0u, 0u, 0u, 0u};
    if constexpr (KC > 0) {
      xor_rows_n<(KC > 0 ? KC : 1), false, NT>(acc, src, a.row_stride, 0, 0, nullptr);
    } else {
      xor_rows_rt<8, false, NT>(acc, src, a.row_stride, k, 0, nullptr);
    }
    __syncthreads();
    if (on && m < k) st16t<NT>(const_cast<uint8_t*>(src) + (uint64_t)m * a.row_stride, acc);
    if (on && m >= k && t == 0) atomicOr(a.err, kErrMissingIndex);
    return;
  }
  uint64_t mw0 = 0, mw1 = 0;
  if constexpr (RECOVER) {
    // SM: the block's lost-slot indices by (at most) two SCALAR loads of the
    // aligned 8-byte words covering missing[gb .. gb+gpb) (gpb <= 8): every
    // row address below depends on m, and a per-lane byte load here would
    // put a vector-memory round trip in front of all of them (-7% measured).
    // An aligned word holding a valid byte never crosses a page: no fault.
    if constexpr (SM) {
      const uint8_t* mp = a.missing + gb;
      const uint32_t mis = (uint32_t)((uintptr_t)mp & 7u);  // pointer math keeps addrspace(1)
      const uint64_t* wp = reinterpret_cast<const uint64_t*>(mp - mis);
      mw0 = wp[0];
      if (gb + 8u - mis < a.n_groups) mw1 = wp[1];
    }
  }
  if (gl >= gpb || g >= a.n_groups) return;
  const uint32_t off = min(t * 16u, a.L - 16u);
  const uint8_t* src = a.rows + g * a.group_stride + off;
  const uint32_t k = KC > 0 ? (uint32_t)KC : a.k;

  u32x4 acc = {0u, 0u, 0u, 0u};
  if constexpr (RECOVER) {
    uint32_t m;
    if constexpr (SM) {
      const uint32_t sh = gl + (uint32_t)((uintptr_t)(a.missing + gb) & 7u);
      m = (uint32_t)((sh < 8u ? mw0 >> (8u * sh) : mw1 >> (8u * (sh - 8u))) & 0xFFu);
    } else {
      m = a.missing[g];
    }
    if (m >= k) {
      if (t == 0) atomicOr(a.err, kErrMissingIndex);
      return;
    }
    const uint8_t* par = a.parity + g * a.parity_stride + off;
    if constexpr (KC > 0) {
#pragma unroll
      for (uint32_t i = 0; i < (uint32_t)KC; ++i) {
        const uint8_t* p = (i == m) ? par : src + i * a.row_stride;
        acc ^= ld16t<NT>(p);
      }
    } else {
      xor_rows_rt<8, true, NT>(acc, src, a.row_stride, k, m, par);
    }
  } else {
    if constexpr (KC > 0) {
#pragma unroll
      for (uint32_t i = 0; i < (uint32_t)KC; ++i) acc ^= ld16t<NT>(src + i * a.row_stride);
    } else {
      xor_rows_rt<8, false, NT>(acc, src, a.row_stride, k, 0, nullptr);
    }
  }
  st16t<NT>(a.out + g * a.out_stride + off, acc);
}

// ---------------------------------------------------------------------------
// Fixed shape, large batches: the same lanes and loads, phased.
// ---------------------------------------------------------------------------
// The fixed kernel above runs at 0.69-0.81 of 8 TB/s depending on where the
// caller's rows and parity buffers sit in the DRAM relative to each other
// (a property of the (rows, parity) PAIR — the read and write
// streams meeting in the DRAM).  Here a persistent grid of one workgroup per
// CU walks the batch in phases: in phase p every workgroup XORs kPhSteps x gpb
// groups into LDS (160 KiB — the whole CU), the grid meets, every workgroup
// stores its parity rows and goes on to the next phase.  The HBM then sees
// (mostly) separate phases of reads and writes, whatever the placement
// (tools/tune/tune_phase.hip).
// The meetings only shape timing: no workgroup reads what another wrote, so
// every wait is bounded — a workgroup that waits longer than kPhTimeout
// (e.g. the GPU shared with other work, so not all workgroups are resident)
// raises an abandon flag and every workgroup stops waiting for the rest of the
// launch; results are identical either way.
constexpr int kPhSteps = 40;         // 40 x 256 lanes x 16 B = 160 KiB of LDS
// k = 10 (the headline shape): 32 more steps per phase held in VGPRs (one
// wave per SIMD has the register file to itself): 19 phases instead of 35 at
// 2^20 groups, encode +1.6%; recover +0.1-1.3%, +1.7% with the register
// steps' parity rows loaded first (RPF) (tools/tune/tune_phase.hip "40+32",
// profiles/round3/phase/tune_phase_rs*.txt; 40 + 40 / 48 / 64 spill into
// AGPRs and lose).
constexpr int kPhRegSteps = 32;
constexpr uint64_t kPhTimeout = 20000;  // s_memrealtime ticks (100 MHz): 200 us

// sync words, 256 B apart: [0] top, [1..16] sub-counters, [17] exits, [18] abandon,
// [19] abandoned launches so far (never reset: qfec_phase_abandons)
__device__ __forceinline__ uint32_t* ph_word(uint32_t* ps, uint32_t i) { return ps + 64u * i; }

__device__ __forceinline__ uint32_t ph_load(uint32_t* w) {
  return __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Meeting number `epoch` (1, 2, ...), in two parts.
// Arrive: thread 0 adds its workgroup to one of 16 sub-counters (one counter
// for every workgroup cost ~60 us per meeting at 1,024 adders); the add's
// return value tells the last arriver of a sub-counter in this epoch
// (old + 1 == epoch * nsub), which adds to the top counter (phase_arrived).
// Wait: the workgroup polls the top counter until it holds epoch * min(B, 16).
// With kPhEarly = 0 the two run back to back after the phase's last step,
// behind a read of the abandon flag: three dependent round trips plus the
// poll, during which the CU neither reads nor writes.  With kPhEarly = E > 0
// the kernel arrives E steps before the phase's last step, while its loads
// are in flight, and looks at the returned value one step later, when it is
// back; phase_wait is then the poll alone (and the top add when the arrival
// came with the last step).  The fastest workgroups may then start storing
// while the slowest have up to E steps of reads to go.
// Invariant (what keeps the epoch arithmetic right with early arrivals): a
// workgroup arrives for meeting p + 1 only after it has left phase_wait(p),
// and nobody leaves phase_wait(p) before the top counter says every workgroup
// has arrived for p, so a sub-counter never holds arrivals of two meetings
// that are both still open.  The one way out of phase_wait without that is
// the abandon flag, and a workgroup that has seen it (`gone`, thread 0's)
// neither arrives nor waits again in this launch.
// E = 0 / 1 / 2 / 4 at 2^20 groups x 10 x 1350 B, six buffer pairs, fraction
// of 8 TB/s: encode 0.8268 / 0.8277 / 0.8332 / 0.8415, recover 0.7854 /
// 0.7898 / 0.7940 / 0.8009; by the stamps a workgroup's wait, summed over a
// launch's 19 meetings, falls from 100 to 45 us (encode) and from 131 to
// 103 us (recover), E = 0 to 4; most of it is the workgroups' skew, not the
// meeting's own round trips (tools/tune/tune_phase.hip,
// profiles/phase_arrive/tune_phase_arrive.txt).
constexpr int kPhEarly = 4;  // E: steps before a phase's last step at which a workgroup arrives

__device__ __forceinline__ uint32_t phase_arrive(uint32_t* ps) {
  return __hip_atomic_fetch_add(ph_word(ps, 1u + (blockIdx.x & 15u)), 1u, __ATOMIC_RELAXED,
                                __HIP_MEMORY_SCOPE_AGENT);
}

// The early arrival's add: its address passes through a VGPR the compiler
// cannot see through.  With a uniform address the atomic optimizer rewrites
// the add as one lane's add of the active-lane count and a readfirstlane of
// what it returned, with a wait for it right behind the add (found in the
// assembly: s_waitcnt vmcnt(0) in the arrival step) -- the round trip this
// arrival is there to hide.
__device__ __forceinline__ uint32_t phase_arrive_early(uint32_t* ps) {
  typedef __attribute__((address_space(1))) uint32_t* gptr;  // stays a global access, not flat
  gptr w = (gptr)ph_word(ps, 1u + (blockIdx.x & 15u));
  asm volatile("" : "+v"(w));
  return __hip_atomic_fetch_add(w, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// what this workgroup's sub-counter holds when all its workgroups have arrived
// for meeting `epoch`
__device__ __forceinline__ uint32_t phase_full(uint32_t epoch) {
  const uint32_t B = gridDim.x, sub = blockIdx.x & 15u, nsub = (B - sub + 15u) / 16u;
  return epoch * nsub;
}

__device__ __forceinline__ void phase_top(uint32_t* ps) {
  __hip_atomic_fetch_add(ph_word(ps, 0), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// `old`: what this workgroup's phase_arrive for meeting `epoch` returned
__device__ __forceinline__ void phase_arrived(uint32_t* ps, uint32_t epoch, uint32_t old) {
  if (old + 1u == phase_full(epoch)) phase_top(ps);
}

// thread 0: polls the top counter; true when the launch has abandoned its
// meetings (this workgroup waited kPhTimeout, or another one did)
__device__ __forceinline__ bool phase_poll(uint32_t* ps, uint32_t epoch) {
  const uint32_t target = epoch * min(gridDim.x, 16u);
  const uint64_t t0 = wall_clock64();
  while (ph_load(ph_word(ps, 0)) < target) {
    if (wall_clock64() - t0 > kPhTimeout) {
      if (__hip_atomic_fetch_or(ph_word(ps, 18), 1u, __ATOMIC_RELAXED,
                                __HIP_MEMORY_SCOPE_AGENT) == 0u)  // count abandoned launches
        __hip_atomic_fetch_add(ph_word(ps, 19), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      return true;
    }
    if (ph_load(ph_word(ps, 18)) != 0u) return true;
    __builtin_amdgcn_s_sleep(1);
  }
  return false;
}

// E = 0: arrive and wait here.  E > 0: the kernel has arrived (`old`); `late`:
// it has not looked at `old` yet (the arrival came with the phase's last step).
// T0, T1 (tools/tune only, null in the product): thread 0's clock after the
// workgroup's last load has returned and when it leaves the meeting.
template <int E>
__device__ __forceinline__ void phase_wait(uint32_t* ps, uint32_t epoch, uint32_t old, bool late,
                                           bool& gone, uint64_t* T0 = nullptr,
                                           uint64_t* T1 = nullptr) {
  __syncthreads();
  if (T0 && threadIdx.x == 0) *T0 = wall_clock64();
  if constexpr (E == 0) {
    if (threadIdx.x == 0 && ph_load(ph_word(ps, 18)) == 0u) {
      phase_arrived(ps, epoch, phase_arrive(ps));
      gone = phase_poll(ps, epoch);
    }
  } else {
    if (threadIdx.x == 0 && !gone) {
      if (late) phase_arrived(ps, epoch, old);
      gone = phase_poll(ps, epoch);
    }
  }
  if (T1 && threadIdx.x == 0) *T1 = wall_clock64();
  __syncthreads();
}

// The whole meeting in one call, arrive and wait after the last step: what
// the persistent kernels of tools/tune that include this file meet with.
[[maybe_unused]] __device__ __forceinline__ void phase_meet(uint32_t* ps, uint32_t epoch) {
  bool gone = false;
  phase_wait<0>(ps, epoch, 0u, false, gone);
}

// The last workgroup out zeroes the sync words for the next launch on the
// stream (vector atomics; the launch boundary orders them before it) and
// copies the abandoned-launch count into the context's host-mapped word
// (a vector store at system scope), where the host reads it at the next
// launch without waiting for this one.
__device__ __forceinline__ void phase_exit(uint32_t* ps, uint32_t* host) {
  __syncthreads();
  if (threadIdx.x == 0 &&
      __hip_atomic_fetch_add(ph_word(ps, 17), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ==
          gridDim.x - 1u) {
    for (uint32_t i = 0; i < 19u; ++i)
      __hip_atomic_store(ph_word(ps, i), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (host)
      __hip_atomic_store(host, ph_load(ph_word(ps, 19)), __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// One phase of one workgroup: the first kPhSteps steps keep their parity in
// LDS, RS more (templated k only) in registers; a step is gpb groups, its k
// row loads (nontemporal) in flight per lane, one step at a time.  The grid
// meets once, then every workgroup stores the phase's parity rows; a
// workgroup arrives at that meeting kPhEarly steps before its last step
// (with step max(SP - kPhEarly, 0) of the launch's SP steps, in the LDS loop
// or in the register steps) and only waits for the others at the phase's end
// (phase_arrive / phase_wait above), so the fastest workgroups store while
// the slowest read their last kPhEarly steps.  Step i of
// phase p covers one contiguous window of B x gpb groups (the fixed kernel's
// sliding window), workgroup b its gpb groups at b x gpb.
//   encode, templated k: the k rows of a step loaded together, XORed.
//   recover, templated k: the phase's parity rows first, as one stream over
//     the parity buffer (LDS steps into LDS, then the register steps' into
//     registers), then per step the k-1 received rows in order, r + (r >= m),
//     so no load instruction runs with the lost row's lanes masked off.
//   runtime k (> 16, or > 25 for recover): batches of up to RTB loads in
//     flight, as even as possible (xor_rows_rt); recover loads the parity in
//     place of the lost row (parity first with compact received rows measured
//     2-6% slower for k = 17-48, profiles/round6/phase_k_table_r6c.txt
//     against r6b).
//   INPL: the encode form over the k rows of a group whose lost row holds
//     zeroes, the result written into that row.
// Which of these a launch gets is phase_body()'s decision, below.
//
// Variants measured and removed (tools/tune/tune_phase.hip of that time; the
// kernel with all of them as template switches is in git history at 2677a57).
// profiles/round2/phase/tune_phase8.txt: a second meeting per phase, after the
// stores (MEET2) -3%; two steps' loads in flight per lane (kPhU = 2) -4%; row
// pointers as generic pointers, flat loads (FLAT) no change; XCD-aware block
// order in the window (XCDW) +0.5% encode / -3% recover.  Other lanes x steps
// (NTHR, STEPS) against 256 x 40's 0.79-0.81: 512 x 20 0.74, 1024 x 10 0.68
// (tune_phase9.txt), 128 x 80 0.50, 192 x 53 0.77 (tune_phase10.txt).
// tune_phase12.txt: recover's parity rows first (PARFIRST) +2.7% over the
// parity loaded in place of the lost row.  tune_phase_compact.txt: the compact
// received rows (COMPACT) +2.5% over every row's load with the lost row's
// lanes masked off (17 loads and 22 exec branches per step instead of 18 and
// 32), 0.780 vs 0.761 on six buffer pairs.  Default-policy loads everywhere
// (NTLD off) -3%, 0.755-0.790 vs 0.781-0.811 (tune_phase13.txt), or only in a
// row's first and last 128-B line (EDGE) as slow, 0.761-0.784
// (tune_phase14.txt); DESIGN.md §5.
// profiles/round3/phase/tune_phase_rs{4,5}.txt: recover's register steps
// loading each parity row with its step instead of all of them first (RPF
// off) 0.798-0.805 / 0.793-0.798 vs 0.801-0.808 / 0.797-0.803.
// profiles/round4/tune_phase_recover_r4l.txt: the register steps' parity rows
// right after the LDS steps' ones, one parity stream per phase (RPFE), 0.789
// vs 0.791.
//
// QFEC_PHASE_TUNE (tools/tune/tune_phase.hip only; the product build never
// defines it): E becomes a template parameter, so one process can run several
// values side by side, and STAMP makes thread 0 of every workgroup write four
// wall_clock64() stamps per phase into g_phase_stamps[block][phase][4] --
// 0 the workgroup's last load has returned, 1 it has left the meeting, 2 its
// last store is issued, 3 the phase's first loads are issued (written at the
// phase's start, so stamp 2 of phase p pairs with stamp 3 of phase p + 1).
//
// The one exception to kPhEarly: the templated recover at k = 24 and 25.  Its
// 32 unrolled register steps sit just below the size at which the compiler
// stops unrolling a loop; with the two compares per step of the early
// arrival it stops, indexes the steps' accumulators at run time and puts them
// in scratch (528 B; tests/test_isa_guard.py).  These two keep E = 0.
__host__ __device__ constexpr int phase_early(int kc, bool recover, int rs) {
  return recover && rs > 0 && kc >= 24 ? 0 : kPhEarly;
}
#ifdef QFEC_PHASE_TUNE
__device__ uint64_t* g_phase_stamps = nullptr;
#define QFEC_PH_TUNE_TPARAMS , int E = kPhEarly, bool STAMP = false
#else
#define QFEC_PH_TUNE_TPARAMS
#endif
template <int KC, bool RECOVER, int RS = 0, bool INPL = false, int RTB = 32 QFEC_PH_TUNE_TPARAMS>
__global__ __launch_bounds__(kBlock) void phase_xor_kernel(FixedArgs a, uint32_t C, uint32_t gpb,
                                                             uint32_t nphase) {
#ifdef QFEC_PHASE_TUNE
  uint64_t* const stamps =
      STAMP && threadIdx.x == 0 ? g_phase_stamps + (uint64_t)blockIdx.x * nphase * 4u : nullptr;
#else
  constexpr int E = phase_early(KC, RECOVER, RS);
  uint64_t* const stamps = nullptr;
#endif
  static_assert(E >= 0, "arrival E steps before the phase's last step");
  static_assert(!(INPL && RECOVER), "in place: the encode form over the k rows");
  static_assert(kPhSteps <= 64, "recover: bad-step masks are 64 bits");
  static_assert(RS == 0 || (KC > 0 && RS <= 64), "register steps: templated k, 64-bit lane-on mask");
  constexpr bool PF = RECOVER && KC > 0;  // parity rows first, compact received rows
  constexpr int TS = kPhSteps + RS;       // steps per phase (at most)
  // the launch's steps per phase (launch_fixed spreads the batch evenly over
  // its phases, so the last phase is not a sliver); the LDS steps come first
  const int SP = a.phase_steps != 0u ? min((int)a.phase_steps, TS) : TS;
  const int NL = min(kPhSteps, SP);  // LDS steps in use
  __shared__ u32x4 s_par[kPhSteps][kBlock];  // lane tid's parity of each step
  const uint32_t tid = threadIdx.x, gl = tid / C, t = tid - gl * C;
  const bool lane_on = gl < gpb;
  const uint32_t off = min(t * 16u, a.L - 16u);
  const uint32_t k = KC > 0 ? (uint32_t)KC : a.k;
  const uint64_t B = gridDim.x;
  // the meeting (above): thread 0 arrives with step `arr`, once that step's
  // loads are issued, and looks at what the add returned with step arr + 1 (a
  // wave-uniform compare per step; in a VGPR all the way, no readfirstlane of
  // a lane-0-only atomic's result: DESIGN.md §13 lesson 8)
  const int arr = max(SP - E, 0);
  uint32_t ph_old = 0u;  // thread 0: its arrival's return value
  bool ph_gone = false;  // thread 0: the launch has abandoned its meetings
  for (uint32_t p = 0; p < nphase; ++p) {
    // (the step number as this phase's own value: compared with a value that
    // is the same in every phase, the unrolled register steps' 2 x 32 compare
    // results are computed once before the phase loop and kept -- 130 more
    // SGPRs spilled into VGPR lanes, and scratch in the k = 24, 25 recover)
    int arr_p = arr;
    if constexpr (E > 0) asm volatile("" : "+s"(arr_p));
    // (everything a step's share of the meeting needs, once per phase: the
    // unrolled register steps of the k = 24, 25 recover sit just below the
    // size at which the compiler stops unrolling them)
    const bool ph_on = tid == 0u && !ph_gone;
    const uint32_t ph_full = phase_full(p + 1u);
    auto early = [&](int step) {
      if constexpr (E > 0) {
        if (step == arr_p) {
          if (ph_on) ph_old = phase_arrive_early(a.phase_sync);
        } else if (step == arr_p + 1) {
          if (ph_on && ph_old + 1u == ph_full) phase_top(a.phase_sync);
        }
      }
    };
    const uint64_t base = ((uint64_t)p * (uint64_t)SP * B + blockIdx.x) * gpb + gl;
    // recover: steps whose lost-slot index is out of range (bit i of lo/hi:
    // 32-bit shifts only)
    uint32_t bad_lo = 0, bad_hi = 0;
    auto gidx = [&](int i) { return base + (uint64_t)i * B * gpb; };
    // recover: the lost-slot indices of the next steps are loaded one
    // iteration ahead (every row address depends on them)
    uint32_t m_reg[RS > 0 && RECOVER ? RS : 1];  // register steps' lost slots, loaded early
    if constexpr (RS > 0 && RECOVER) {
#pragma unroll
      for (int j = 0; j < RS; ++j) {
        const uint64_t g = gidx(kPhSteps + j);
        m_reg[j] = lane_on && g < a.n_groups && kPhSteps + j < SP ? a.missing[g] : 0u;
      }
    }
    // The LDS steps go one at a time, in the shape the loop had when U steps'
    // loads could be in flight together (U = 2 measured -4%, above): with the
    // one-element arrays as scalars and the one-trip loops gone the compiler
    // lays the loop's blocks out differently (a branch's sense flips in every
    // instantiation, registers move in the runtime-k recover), and the code
    // that was measured is the code that is kept.
    constexpr int U = 1;
    uint32_t m_next[U];
    if constexpr (RECOVER) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const uint64_t g = gidx(u);
        m_next[u] = lane_on && g < a.n_groups ? a.missing[g] : 0u;
      }
    }
    u32x4 racc[RS > 0 ? RS : 1];
    if constexpr (PF) {
      // the LDS steps' parity rows, into the accumulators
#pragma unroll 1
      for (int i = 0; i < kPhSteps; i += 8) {
        u32x4 w[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const uint64_t g = gidx(i + j < NL ? i + j : 0);
          const bool on = i + j < NL && lane_on && g < a.n_groups;
          w[j] = ld16t<true>(a.parity + (on ? g : 0) * a.parity_stride + off);
        }
        if (stamps && i == 0) stamps[p * 4u + 3u] = wall_clock64();
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (i + j < kPhSteps) s_par[i + j][tid] = w[j];
      }
    }
#pragma unroll 1
    for (int i = 0; i < NL; i += U) {
      u32x4 acc[U];
      uint32_t m[U];
      const uint8_t* src[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const uint64_t g = gidx(i + u);
        const bool on = lane_on && g < a.n_groups;
        src[u] = a.rows + (on ? g : 0) * a.group_stride + off;
        acc[u] = u32x4{0u, 0u, 0u, 0u};
        m[u] = k;  // encode: no slot replaced
        if constexpr (RECOVER) {
          m[u] = m_next[u];
          if (m[u] >= k) {
            if (on) {
              if (i + u < 32) bad_lo |= 1u << (i + u);
              else bad_hi |= 1u << (i + u - 32);
            }
            m[u] = 0u;  // read something valid; the group is not stored
          }
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if constexpr (PF) {
          // the k-1 received rows in order, every lane on every load
          u32x4 v[KC];
#pragma unroll
          for (int r = 0; r + 1 < KC; ++r)
            v[r] = ld16t<true>(src[u] + ((uint32_t)r + ((uint32_t)r >= m[u] ? 1u : 0u)) * a.row_stride);
          v[KC - 1] = u32x4{0u, 0u, 0u, 0u};
          early(i + u);
          acc[u] = s_par[i + u][tid];
#pragma unroll
          for (int r = 0; r < KC; ++r) acc[u] ^= v[r];
        } else if constexpr (KC > 0) {
          u32x4 v[KC];
#pragma unroll
          for (int r = 0; r < KC; ++r) v[r] = ld16t<true>(src[u] + r * a.row_stride);
          if (stamps && i + u == 0) stamps[p * 4u + 3u] = wall_clock64();
          early(i + u);
#pragma unroll
          for (int r = 0; r < KC; ++r) acc[u] ^= v[r];
        } else {
          // (runtime k: the step's loads go in batches, so the arrival is
          // issued ahead of them)
          if (stamps && i + u == 0) stamps[p * 4u + 3u] = wall_clock64();
          early(i + u);
          const uint64_t g = gidx(i + u);
          const uint8_t* par = RECOVER ? a.parity + (lane_on && g < a.n_groups ? g : 0) * a.parity_stride + off
                                       : nullptr;
          xor_rows_rt<RTB, RECOVER, true>(acc[u], src[u], a.row_stride, k, m[u], par);
        }
      }
      if constexpr (RECOVER) {
        if (i + U < NL) {
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const uint64_t g = gidx(i + U + u);
            m_next[u] = lane_on && g < a.n_groups ? a.missing[g] : 0u;
          }
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) s_par[i + u][tid] = acc[u];
    }
    uint32_t ron[2] = {0u, 0u};  // step j's lane is on: bit j % 32 of word j / 32
    bool rbad = false;           // recover: a register step's lost slot out of range
    if constexpr (RS > 0) {
      // one live row address, advanced step by step (the compiler would
      // otherwise keep every step's address live across the unrolled steps)
      const uint64_t g0r = gidx(kPhSteps);
      const uint8_t* q = a.rows + g0r * a.group_stride + off;
      const uint64_t dq = B * gpb * a.group_stride;
      // (recover: qp, the step's parity address, is no longer loaded from --
      // the parity rows are loaded before the steps -- but it is still
      // advanced and fenced with q: the fences are kept exactly as measured)
      const uint8_t* qp = RECOVER ? a.parity + g0r * a.parity_stride + off : nullptr;
      const uint64_t dqp = RECOVER ? B * gpb * a.parity_stride : 0u;
      if constexpr (RECOVER) {
        // every register step's parity row first (one stream, as the LDS
        // steps'), then the received rows step by step
#pragma unroll
        for (int j = 0; j < RS; ++j) {
          const uint64_t g = g0r + (uint64_t)j * B * gpb;
          const bool on = lane_on && g < a.n_groups && kPhSteps + j < SP;
          racc[j] = ld16t<true>(a.parity + (on ? g : 0) * a.parity_stride + off);
        }
      }
#pragma unroll
      for (int j = 0; j < RS; ++j) {
        const uint64_t g = g0r + (uint64_t)j * B * gpb;
        bool on = lane_on && g < a.n_groups && kPhSteps + j < SP;
        u32x4 v[KC];
        if constexpr (RECOVER) {
          uint32_t mj = m_reg[j];
          if (mj >= k) {  // out-of-range lost slot: the group is not stored
            rbad = rbad || on;
            on = false;
            mj = 0u;
          }
          const uint8_t* qq = on ? q : a.rows + off;
          // the parity row, then the k-1 received rows in order (compact)
          v[0] = racc[j];
#pragma unroll
          for (int r = 0; r + 1 < KC; ++r)
            v[r + 1] = ld16t<true>(qq + ((uint32_t)r + ((uint32_t)r >= mj ? 1u : 0u)) * a.row_stride);
        } else {
          const uint8_t* qq = on ? q : a.rows + off;
#pragma unroll
          for (int r = 0; r < KC; ++r) v[r] = ld16t<true>(qq + r * a.row_stride);
        }
        early(kPhSteps + j);
        ron[j / 32] |= on ? 1u << (j % 32) : 0u;
        u32x4 x = v[0];
#pragma unroll
        for (int r = 1; r < KC; ++r) x ^= v[r];
        racc[j] = x;
        q += dq;
        // the next step's address waits for this step's XOR: one step's k
        // loads in flight, as in the LDS steps
        asm volatile("" : "+v"(q) : "v"(x));
        if constexpr (RECOVER) {
          qp += dqp;
          asm volatile("" : "+v"(qp) : "v"(x));
        }
      }
    }
    if constexpr (RECOVER) {
      if (((bad_lo | bad_hi) != 0u || rbad) && t == 0u) atomicOr(a.err, kErrMissingIndex);
    }
    phase_wait<E>(a.phase_sync, p + 1u, ph_old, arr + 1 >= SP, ph_gone, stamps ? stamps + p * 4u : nullptr,
                  stamps ? stamps + p * 4u + 1u : nullptr);
    // INPL: the output row of group g is its own row missing[g] (the in-slot
    // recover written in place; every read of the phase is done by now, and
    // no other workgroup reads this group).  It runs at 0.73-0.76 of 8 TB/s
    // against 0.80-0.82 out of place: its stores land inside the rows' own
    // allocation, the DRAM placement DESIGN.md §4 measured slow for the
    // one-pass kernel's parity too (prefetching the lost indices before the
    // meeting measured no better: profiles/round5/bench_r5{b,c}.json).
    bool ibad = false;
    auto dst = [&](uint64_t g, bool& on) -> uint8_t* {
      if constexpr (INPL) {
        const uint32_t m = a.inplace_missing[g];
        if (m >= k) {
          ibad = ibad || on;
          on = false;
        }
        return const_cast<uint8_t*>(a.rows) + g * a.group_stride + (uint64_t)m * a.row_stride + off;
      } else {
        return a.out + g * a.out_stride + off;
      }
    };
#pragma unroll 4
    for (int i = 0; i < kPhSteps; ++i) {
      const uint64_t g = gidx(i);
      const uint32_t skip = RECOVER ? ((i < 32 ? bad_lo >> i : bad_hi >> (i - 32)) & 1u) : 0u;
      bool on = lane_on && g < a.n_groups && !skip && i < NL;
      uint8_t* d = dst(on ? g : 0, on);
      if (on) st16t<true>(d, s_par[i][tid]);
    }
    if constexpr (RS > 0) {
#pragma unroll
      for (int j = 0; j < RS; ++j) {
        const uint64_t g = gidx(kPhSteps + j);
        bool on = ((ron[j / 32] >> (j % 32)) & 1u) != 0u;
        uint8_t* d = dst(on ? g : 0, on);
        if (on) st16t<true>(d, racc[j]);
      }
    }
    if constexpr (INPL) {
      if (ibad && t == 0u) atomicOr(a.err, kErrMissingIndex);
    }
    if (stamps) stamps[p * 4u + 2u] = wall_clock64();
  }
  phase_exit(a.phase_sync, a.phase_host);
}

// Fixed shape, L < 16 (degenerate tiny packets): one lane per output byte.
template <bool RECOVER>
__global__ __launch_bounds__(kBlock) void fixed_small_kernel(FixedArgs a) {
  const uint64_t e = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  const uint64_t g = e / a.L;
  const uint32_t j = (uint32_t)(e - g * a.L);
  if (g >= a.n_groups) return;
  uint8_t acc = 0;
  const uint8_t* src = a.rows + g * a.group_stride + j;
  if (RECOVER) {
    const uint32_t m = a.missing[g];
    if (m >= a.k) {
      if (j == 0) atomicOr(a.err, kErrMissingIndex);
      return;
    }
    acc = a.parity[g * a.parity_stride + j];
    for (uint32_t i = 0; i < a.k; ++i)
      if (i != m) acc ^= src[i * a.row_stride];
  } else {
    for (uint32_t i = 0; i < a.k; ++i) acc ^= src[i * a.row_stride];
  }
  if (a.inplace_missing) {
    // in-slot recover in place: this lane alone reads and writes byte j
    const uint32_t m = a.inplace_missing[g];
    if (m >= a.k) {
      if (j == 0) atomicOr(a.err, kErrMissingIndex);
      return;
    }
    const_cast<uint8_t*>(src)[(uint64_t)m * a.row_stride] = acc;
    return;
  }
  a.out[g * a.out_stride + j] = acc;
}

// ---------------------------------------------------------------------------
// Workgroup primitives of the turn passes.
// ---------------------------------------------------------------------------
// The scans, sums and ranks in which the passes of the receiver's turn (revive,
// admit, bin, assign) are written; the ragged kernels further down use the
// first four.  One contract for all of them: they are called from
// block-uniform control flow with every lane of every wave active (they
// shuffle, ballot or meet at a barrier), lane and wave are tid & 63 and
// tid >> 6, and they shift 32-bit words only (the gfx950 64-bit shift hazard,
// DESIGN.md §4).  One that takes an LDS array s_w ends with the barrier that
// makes s_w free again: the caller puts none between two of them.
constexpr int kTurnWaves = kReviveTile / 64;  // waves of a per-tile or per-packet workgroup
constexpr int kRvScanBlock = 1024;            // lanes of a one-workgroup scan kernel

__device__ __forceinline__ uint32_t lane_id() {
  return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
}

// Lane src's x (ds_bpermute; src in [0, 64)).  The shuffles below take the
// caller's lane instead of HIP's __shfl*, which recompute it (mbcnt) and
// whose lane-derived addresses the compiler hoists out of a resident loop:
// in the service worker they stayed live through the whole job body and
// spilled to scratch at 256 VGPRs (round 6).
__device__ __forceinline__ uint32_t lane_read(uint32_t x, uint32_t src) {
  return (uint32_t)__builtin_amdgcn_ds_bpermute((int)(src << 2), (int)x);
}

// Inclusive prefix sum over the wave.
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t x, uint32_t lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t y = lane_read(x, lane >= (uint32_t)d ? lane - (uint32_t)d : lane);
    if (lane >= (uint32_t)d) x += y;
  }
  return x;
}

// Exclusive prefix sum over a workgroup of WAVES waves, and the sum of all.
template <int WAVES>
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t x, uint32_t lane, uint32_t wv,
                                                    uint32_t* s_w, uint32_t& total) {
  const uint32_t incl = wave_incl_scan(x, lane);
  if (lane == 63u) s_w[wv] = incl;
  __syncthreads();
  uint32_t base = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < WAVES; ++w) {
    const uint32_t v = s_w[w];
    base += (uint32_t)w < wv ? v : 0u;
    tot += v;
  }
  total = tot;
  __syncthreads();  // s_w free again
  return base + incl - x;
}

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
constexpr uint32_t kGroupComplete = 0, kGroupRevived = 1, kGroupUnrevivable = 2;

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
// length are not read.
__device__ __forceinline__ uint32_t close_slot(const CloseArgs& a, uint64_t g) {
  return a.slot ? a.slot[g] : (uint32_t)g;
}
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

// The recover body over the work list, L >= 16: lanes, windows and loads as
// fixed_xor_kernel; workgroup step i takes entries [i * gpb, (i + 1) * gpb).
// `work` and `totals` are separate restrict parameters so that their loads
// stay SCALAR in the loop although the loop stores: every row address depends
// on the entry, and a per-lane load of it would put a vector-memory round trip
// in front of all of them (fixed_xor_kernel's SM path, -7% measured there).
// SM (gpb <= 8): the workgroup's entries are eight uniform loads (the list is
// readable kReviveListPad entries past the count) and a select by the lane's
// group; smaller packets load their entry per lane.  (A template switch, not
// a branch: with both forms in one loop the compiler waits for every vector
// access, the previous step's store included, before a step's first load.)
// In place (out == nullptr) the result goes to row m of the group's own rows:
// the recover form never reads row m, and the clamped last window
// min(t * 16, L - 16) stays inside row m, so no lane overwrites a byte another
// lane still reads and, unlike the in-slot INPL body, no barrier is needed.
template <int KC, bool NT, bool SM>
__global__ __launch_bounds__(kBlock) void revive_xor_kernel(ReviveArgs a,
                                                            const uint64_t* __restrict__ work,
                                                            const uint64_t* __restrict__ totals,
                                                            uint32_t C, uint32_t gpb) {
  static_assert(kReviveListPad >= 8, "eight entries are loaded unconditionally");
  const uint32_t tid = threadIdx.x;
  const uint32_t gl = tid / C;  // entry within the workgroup's step
  const uint32_t t = tid - gl * C;
  const uint32_t off = min(t * 16u, a.L - 16u);
  const uint32_t k = KC > 0 ? (uint32_t)KC : a.k;
  const uint64_t count = totals[kGroupRevived];
  const uint64_t nstep = (count + gpb - 1) / gpb;
  for (uint64_t i = blockIdx.x; i < nstep; i += gridDim.x) {
    const uint64_t eb = i * gpb;
    uint64_t e;
    if constexpr (SM) {
      uint64_t w[8];
#pragma unroll
      for (uint32_t j = 0; j < 8u; ++j) w[j] = work[eb + j];
      e = w[0];
#pragma unroll
      for (uint32_t j = 1; j < 8u; ++j) e = gl == j ? w[j] : e;
    } else {
      e = gl < gpb && eb + gl < count ? work[eb + gl] : 0ull;
    }
    if (gl >= gpb || eb + gl >= count) continue;
    const uint64_t g = e >> 8;
    const uint32_t m = (uint32_t)e & 0xFFu;
    const uint8_t* src = a.rows + g * a.group_stride + off;
    const uint8_t* par = a.parity + g * a.parity_stride + off;
    u32x4 acc = {0u, 0u, 0u, 0u};
    if constexpr (KC > 0) {
#pragma unroll
      for (uint32_t r = 0; r < (uint32_t)KC; ++r) {
        const uint8_t* p = (r == m) ? par : src + r * a.row_stride;
        acc ^= ld16t<NT>(p);
      }
    } else {
      xor_rows_rt<8, true, NT>(acc, src, a.row_stride, k, m, par);
    }
    uint8_t* dst = a.out ? a.out + g * a.out_stride + off
                         : const_cast<uint8_t*>(src) + (uint64_t)m * a.row_stride;
    st16t<NT>(dst, acc);
  }
}

// L < 16: one lane per revived byte, as fixed_small_kernel.
__global__ __launch_bounds__(kBlock) void revive_small_kernel(ReviveArgs a,
                                                              const uint64_t* __restrict__ work,
                                                              const uint64_t* __restrict__ totals) {
  const uint64_t nbyte = totals[kGroupRevived] * a.L;
  for (uint64_t x = (uint64_t)blockIdx.x * kBlock + threadIdx.x; x < nbyte;
       x += (uint64_t)gridDim.x * kBlock) {
    const uint64_t i = x / a.L;
    const uint32_t j = (uint32_t)(x - i * a.L);
    const uint64_t e = work[i];
    const uint64_t g = e >> 8;
    const uint32_t m = (uint32_t)e & 0xFFu;
    uint8_t* src = a.rows + g * a.group_stride + j;
    uint8_t acc = a.parity[g * a.parity_stride + j];
    for (uint32_t r = 0; r < a.k; ++r)
      if (r != m) acc ^= src[r * a.row_stride];
    if (a.out) a.out[g * a.out_stride + j] = acc;
    else src[(uint64_t)m * a.row_stride] = acc;
  }
}

// ---------------------------------------------------------------------------
// Ragged CSR: the per-group body (one wave per group) and, below it, the
// two-groups-per-wave product kernel.
// ---------------------------------------------------------------------------
// Bytes [o, o+16) of the 32 bytes lo || hi (o in 0..15), branch-free, in
// 32-bit lanes: two 2-way dword selects (by 8 and by 4 bytes), then one byte
// funnel v_alignbyte_b32 per dword.  No variable 64-bit shift on purpose: on
// gfx950 a v_lshlrev_b64 / v_lshrrev_b64 whose amount sits in the wave's last
// allocated VGPR can shift by v0's value instead (the build
// refuses such code, libquic_amd/isa_guard.py).  Written without multi-way
// selects: the compiler turns those into divergent branches, each of which
// waits for the load (vmcnt(0)) and serialises rows.
__device__ __forceinline__ u32x4 bytes16_at(u32x4 lo, u32x4 hi, uint32_t o) {
  // (named scalars, not arrays: an array here was placed in scratch memory)
  const bool b8 = (o & 8u) != 0u, b4 = (o & 4u) != 0u;
  const uint32_t f0 = b8 ? lo.z : lo.x, f1 = b8 ? lo.w : lo.y, f2 = b8 ? hi.x : lo.z,
                 f3 = b8 ? hi.y : lo.w, f4 = b8 ? hi.z : hi.x, f5 = b8 ? hi.w : hi.y;
  const uint32_t g0 = b4 ? f1 : f0, g1 = b4 ? f2 : f1, g2 = b4 ? f3 : f2, g3 = b4 ? f4 : f3,
                 g4 = b4 ? f5 : f4;
  const uint32_t r = o & 3u;
  return u32x4{__builtin_amdgcn_alignbyte(g1, g0, r), __builtin_amdgcn_alignbyte(g2, g1, r),
               __builtin_amdgcn_alignbyte(g3, g2, r), __builtin_amdgcn_alignbyte(g4, g3, r)};
}

// Right shift of a 16-byte vector by sh bytes (0..15), zero fill.
__device__ __forceinline__ u32x4 shr_bytes_bf(u32x4 v, uint32_t sh) {
  return bytes16_at(v, u32x4{0u, 0u, 0u, 0u}, sh);
}

// Bytes [win, win+16) of a zero-padded packet of `len` bytes, len >= 16.
// Always ONE 16-byte load inside the packet (no exec-masked branch): a window
// that crosses the packet end loads the 16 bytes ending at its last byte and
// shifts them down; a window past the end is zeroed by a select.
template <bool NT>
__device__ __forceinline__ u32x4 window16(const uint8_t* row, uint32_t len, uint32_t win) {
  const bool full = win + 16u <= len;
  const u32x4 v = ld16t<NT>(row + (full ? win : len - 16u));
  // sh = 0 for a full window (shift is then the identity); all-zero mask past the end.
  const uint32_t sh = full ? 0u : min(win + 16u - len, 15u);
  const uint32_t keep = win < len ? 0xFFFFFFFFu : 0u;
  return shr_bytes_bf(v, sh) & keep;
}

// Same for len < 16 (wave-uniform branch per packet; rare).
__device__ __forceinline__ u32x4 window16_small(const uint8_t* row, uint32_t len, uint32_t win) {
  uint8_t b[16];
#pragma unroll
  for (uint32_t x = 0; x < 16; ++x) b[x] = (win + x < len) ? row[win + x] : (uint8_t)0;
  u32x4 v;
  __builtin_memcpy(&v, b, 16);
  return v;
}

// Flat-window ragged kernel: one wave per group.
//
// A group's received packets are cut into 16-byte windows (packet i has
// n_i = ceil(len_i/16); window t covers bytes [16t, 16t+16), the last one
// loaded as the 16 bytes ending at the packet end and shifted down, zero
// filled).  The windows of all packets are numbered consecutively
// (flat index f; packet i owns [S_i, S_i + n_i)) and lane l takes
// f = l, l+64, l+128, ...: every lane of every wave-instruction loads, and
// consecutive lanes read consecutive bytes — across packet boundaries too in a
// packed CSR batch.  Each loaded window is XORed into the group's parity
// accumulator in LDS at byte 16t (ds_xor_b64; two packets' windows can meet
// at the same t inside one instruction, hence the atomic).  The lane's packet
// comes from a bitmask of packet starts (bit S_i set): with M the mask word of
// the wave's 64 windows, packet = starts before + inclusive popcount(M) - 1
// (v_mbcnt), then its offset/length/S from an LDS table.
//
// LDS per wave: accumulator 92 x 16 B, start mask 92 x 8 B, packet table
// 64 x 16 B (3.2 KiB).  Groups of more than 64 received packets run in chunks
// of 64 with the same accumulator.
constexpr int kFlatWaves = kBlock / 64;
constexpr int kPairGroups = 2;  // ragged_multi_kernel: groups per wave
constexpr int kPairWaves = kFlatWaves;  // ragged_multi_kernel: waves per block (4)
constexpr int kRaggedU = 2;     // flat-window loops: iterations' loads in flight
constexpr int kWindowPB = 16;   // ragged_window_kernel: load slots per trip
constexpr int kParWin = 92;  // ceil(1452/16) = 91 windows (+1 spare)

// The group's LDS state (accumulator, start mask, packet table) passes data
// between lanes of one wave.  The LDS executes a wave's accesses in program
// order; wavefront-scope fences around a wave barrier keep the compiler from
// moving one lane's access across another lane's (no s_waitcnt emitted).
__device__ __forceinline__ void wave_lds_order() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// (lane_id, lane_read, wave_incl_scan and block_excl_scan: the workgroup
// primitives above the revive passes)

// The accumulator is only ever accessed as uint32_t (plain and atomic): one
// type, so the compiler cannot reorder the plain initialisation / final reads
// across the atomic XORs on type-based alias grounds.
// Component-major: dword c of window t at c*kParWin + t (ds_xor_b32 x4; lanes
// on consecutive windows hit consecutive banks: conflict-free).
// Layouts removed (template switch ACC, in git history at ace3ed3): window t's
// four dwords at 4t .. 4t+3 (lanes on consecutive windows hit every 4th bank:
// 4-way conflicts), and the same interleaved layout with 2 x ds_xor_b64, no
// faster than component-major.  The latter's U = 4 build was wrong in ~1% of
// recover groups -- not the atomics: that build's 64-bit funnel shift took its
// amount from the last VGPR (profiles/round2/anomaly/); the
// funnels are 32-bit now.
__device__ __forceinline__ uint32_t acc_idx(uint32_t t, uint32_t c) {
  return c * (uint32_t)kParWin + t;
}
// SCOPE: the lanes that share the accumulator -- one wave (the per-group
// body) or every wave of the block (ragged_block_kernel: 4 waves XOR into the
// same groups).  The DS atomic is the same instruction either way; the scope
// states who may race on the word.
template <int SCOPE = __HIP_MEMORY_SCOPE_WAVEFRONT>
__device__ __forceinline__ void lds_xor_u32(uint32_t* p, uint32_t v) {
  __hip_atomic_fetch_xor(p, v, __ATOMIC_RELAXED, SCOPE);
}
template <int SCOPE = __HIP_MEMORY_SCOPE_WAVEFRONT>
__device__ __forceinline__ void lds_xor16(uint32_t* acc, uint32_t t, u32x4 v) {
  lds_xor_u32<SCOPE>(acc + acc_idx(t, 0), v.x);
  lds_xor_u32<SCOPE>(acc + acc_idx(t, 1), v.y);
  lds_xor_u32<SCOPE>(acc + acc_idx(t, 2), v.z);
  lds_xor_u32<SCOPE>(acc + acc_idx(t, 3), v.w);
}
__device__ __forceinline__ void lds_put16(uint32_t* acc, uint32_t t, u32x4 v) {
  acc[acc_idx(t, 0)] = v.x;
  acc[acc_idx(t, 1)] = v.y;
  acc[acc_idx(t, 2)] = v.z;
  acc[acc_idx(t, 3)] = v.w;
}
__device__ __forceinline__ u32x4 lds_get16(const uint32_t* acc, uint32_t t) {
  return u32x4{acc[acc_idx(t, 0)], acc[acc_idx(t, 1)], acc[acc_idx(t, 2)], acc[acc_idx(t, 3)]};
}

// Bytes [16t, 16t+16) of a zero-padded packet (any len >= 1, 16t < len).
template <bool NT>
__device__ __forceinline__ u32x4 packet_window(const uint8_t* row, uint32_t len, uint32_t t) {
  const uint32_t win = 16u * t;
  if (len >= 16u) {
    const bool full = win + 16u <= len;
    const u32x4 v = ld16t<NT>(row + (full ? win : len - 16u));
    return shr_bytes_bf(v, full ? 0u : win + 16u - len);
  }
  return window16_small(row, len, 0u);  // t == 0 (rare: packets below 16 B)
}

// Window t of a zero-padded row of len >= 16 bytes without a branch: a window
// at or past len loads the row's last 16 bytes and returns zero.
template <bool NT>
__device__ __forceinline__ u32x4 parity_window_bf(const uint8_t* row, uint32_t len, uint32_t t) {
  const uint32_t win = 16u * t;
  const bool in = win < len;
  const bool full = win + 16u <= len;
  const uint32_t at = in && full ? win : len - 16u;
  u32x4 v = shr_bytes_bf(ld16t<NT>(row + at), in && !full ? win + 16u - len : 0u);
  const uint32_t keep = in ? 0xFFFFFFFFu : 0u;
  v.x &= keep;
  v.y &= keep;
  v.z &= keep;
  v.w &= keep;
  return v;
}

// Per-group inputs a wave can fetch one group ahead: the group scalars and,
// for the first 64 received packets, lane r's packet length / offset (and for
// recover the parity row's two windows per lane).
struct GroupPrefetch {
  uint32_t p0, k, m, plen;       // wave-uniform
  uint64_t dst_off;              // parity_off (encode) / out_off (recover)
  uint32_t len, offlo, offhi;    // lane r = received packet r (r < 64)
  u32x4 pw0, pw1;                // recover: parity windows lane, lane + 64
  // accumulate only: the slot and its length on entry.  The old length stays
  // a value of its own (plen becomes the new one): the row is zero from `old`
  // on whatever the new maximum is.  kAccBadSlot: slot >= n_slots, acc_len
  // not read.
  uint32_t slot, old;
};
constexpr uint32_t kAccBadSlot = 0xFFFFFFFFu;

// Work-list entry g << 8 | m of a ragged revive (g < 2^32), taken apart with
// 32-bit shifts.
__device__ __forceinline__ void list_entry(uint64_t e, uint64_t& g, uint32_t& m) {
  const uint32_t lo = (uint32_t)e, hi = (uint32_t)(e >> 32);
  g = (uint64_t)((lo >> 8) | (hi << 24));
  m = lo & 0xFFu;
}

// LIST (recover): m is the work-list entry's (qfec_revive_ragged), a.missing is
// not read.
// ACCUM (encode form, qfec_accumulate_ragged; x its arguments): the slot, its
// length on entry (not read for a slot out of range) and the row's offset
// s * acc_stride -- a multiply, no shift.
template <bool RECOVER, bool LIST = false, bool ACCUM = false>
__device__ __forceinline__ void group_scalars(const RaggedArgs& a, uint64_t g, GroupPrefetch& f,
                                              uint32_t list_m = 0,
                                              const AccumulateRaggedArgs* x = nullptr) {
  static_assert(!ACCUM || !RECOVER, "accumulate is the encode form: no packet is skipped");
  f.p0 = a.grp_ptr[g];
  f.k = a.grp_ptr[g + 1] - f.p0;
  f.m = 0xFFFFFFFFu;
  f.plen = 0;
  if constexpr (ACCUM) {
    const uint32_t s = x->slot ? x->slot[g] : x->slot_base + (uint32_t)g;
    f.slot = s;
    f.old = s < x->n_slots ? (uint32_t)x->acc_len[s] : kAccBadSlot;
    f.dst_off = (uint64_t)s * x->acc_stride;
  } else if constexpr (RECOVER) {
    if constexpr (LIST) f.m = list_m;
    else f.m = a.missing[g];
    f.plen = a.parity_len[g];
    f.dst_off = a.out_off[g];
  } else {
    f.dst_off = a.parity_off[g];
  }
}

// Vector part (needs the scalars).  Invalid groups load nothing.
// ACCUM: the slot's row up to its old length is the "parity row"; a fresh slot
// (old == 0) loads nothing of it.
template <bool RECOVER, bool ACCUM = false>
__device__ __forceinline__ void group_vectors(const RaggedArgs& a, uint64_t g, uint32_t lane,
                                              GroupPrefetch& f,
                                              const AccumulateRaggedArgs* x = nullptr) {
  f.len = f.offlo = f.offhi = 0;
  const u32x4 zero = {0u, 0u, 0u, 0u};
  f.pw0 = f.pw1 = zero;
  bool ok = f.k >= 1u && f.k <= 255u && (!RECOVER || (f.m < f.k && f.plen >= 1u &&
                                                       f.plen <= kMaxPacket));
  if constexpr (ACCUM) ok = ok && f.old <= x->lim;  // (kAccBadSlot is above any limit)
  if (!ok) return;
  const uint32_t kr = RECOVER ? f.k - 1u : f.k;
  if (lane < kr) {
    const uint32_t p = f.p0 + lane + (lane >= f.m ? 1u : 0u);
    f.len = a.pkt_len[p];
    const uint64_t o = a.pkt_off[p];
    f.offlo = (uint32_t)o;
    f.offhi = (uint32_t)(o >> 32);
  }
  if constexpr (RECOVER) {
    const uint8_t* prow = a.parity + a.parity_off[g];
    if (16u * lane < f.plen) f.pw0 = packet_window<true>(prow, f.plen, lane);
    if (16u * (lane + 64u) < f.plen) f.pw1 = packet_window<true>(prow, f.plen, lane + 64u);
  }
  if constexpr (ACCUM) {
    const uint8_t* prow = a.parity + f.dst_off;
    if (16u * lane < f.old) f.pw0 = packet_window<true>(prow, f.old, lane);
    if (16u * (lane + 64u) < f.old) f.pw1 = packet_window<true>(prow, f.old, lane + 64u);
  }
}

// One group, one wave (see the flat-window description above).
//
// ACCUM (qfec_accumulate_ragged, x its arguments): the encode form whose
// accumulator starts from the slot's own row (zero from its old length on) and
// whose output goes back to that row, its length the running maximum.  In
// place is safe because every load of the row precedes every store to it: the
// row is read only by the prefetch (group_vectors), whose windows are in LDS
// before the first store below, and the unaligned tail store ("the 16 bytes
// ending at the length") overlaps the previous window's store with identical
// bytes.  A group that latches an error returns before any store, to the row
// or to its length; a group of no packets is a no-op.
//
// Loads and stores are nontemporal, kRaggedU iterations' loads are in flight
// before the first XOR, the accumulator is component-major (acc_idx).
// Variants measured and removed (template switches NT, U, ACC, BF of this
// body and of ragged_pair_xor, in git history at ace3ed3; DESIGN.md §4,
// profiles/round2/ragged_store/): default-policy (write-back) stores 0.500 /
// 0.494 against 0.624 / 0.625; U = 1 / 2 / 3 / 4 encode 0.614 / 0.624 /
// 0.629 / 0.625, recover 0.602 / 0.615 / 0.614 / 0.616, flat above 2
// (tune_rw_diag7.txt); the other accumulator layouts, at acc_idx; a
// branch-free XOR loop (BF: lanes past the last window XOR zero into window
// `lane`) 0.615 / 0.602 against 0.625 / 0.616 strided, 0.618 / 0.587 against
// 0.633 / 0.605 packed (tune_rw_diag6*.txt).
template <bool RECOVER, bool ACCUM = false>
__device__ __forceinline__ void ragged_group(const RaggedArgs& a, uint64_t g, uint32_t lane,
                                             const GroupPrefetch& f, uint32_t* par,
                                             uint64_t* head, u32x4* meta,
                                             const AccumulateRaggedArgs* x = nullptr) {
  const uint32_t p0 = f.p0, k = f.k, m = f.m;
  uint32_t plen = f.plen;
  if ((!ACCUM && k == 0u) || k > 255u) {  // grp_ptr not monotone shows up as k > 255 too
    if (lane == 0) atomicOr(a.err, kErrGroupSize);
    return;
  }
  const u32x4 zero = {0u, 0u, 0u, 0u};
  if constexpr (ACCUM) {
    if (f.old == kAccBadSlot) {  // slot >= n_slots
      if (lane == 0) atomicOr(a.err, kErrMissingIndex);
      return;
    }
    if (f.old > x->lim) {
      if (lane == 0) atomicOr(a.err, kErrParityLength);
      return;
    }
    if (k == 0u) return;  // nothing to fold this turn
    // accumulator := the slot's row (zero from its old length on)
    lds_put16(par, lane, f.pw0);
    if (lane + 64u < kParWin) lds_put16(par, lane + 64u, f.pw1);
  } else if constexpr (RECOVER) {
    if (m >= k) {
      if (lane == 0) atomicOr(a.err, kErrMissingIndex);
      return;
    }
    if (plen == 0u || plen > kMaxPacket) {
      if (lane == 0) atomicOr(a.err, kErrParityLength);
      return;
    }
    // accumulator := the parity row (zero past plen), prefetched windows
    lds_put16(par, lane, f.pw0);
    if (lane + 64u < kParWin) lds_put16(par, lane + 64u, f.pw1);
  } else {
    for (uint32_t t = lane; t < kParWin; t += 64u) lds_put16(par, t, zero);
  }
  const uint32_t kr = RECOVER ? k - 1u : k;  // received packets
  uint32_t lim = RECOVER ? plen : kMaxPacket;
  if constexpr (ACCUM) lim = x->lim;
  constexpr int U = kRaggedU;
  uint32_t mx = 0;
  for (uint32_t c = 0; c < kr; c += 64u) {
    // packet table of this chunk: lane j = received packet c + j
    const uint32_t r = c + lane;
    uint32_t len = f.len, offlo = f.offlo, offhi = f.offhi;
    if (c > 0) {  // groups of more than 64 received packets: load inline
      len = offlo = offhi = 0;
      if (r < kr) {
        const uint32_t p = p0 + r + (r >= m ? 1u : 0u);
        len = a.pkt_len[p];
        const uint64_t o = a.pkt_off[p];
        offlo = (uint32_t)o;
        offhi = (uint32_t)(o >> 32);
      }
    }
    const bool bad = r < kr && (len == 0u || len > lim);
    if (wave_any(bad)) {
      if (lane == 0) atomicOr(a.err, kErrPacketLength);
      return;
    }
    mx = max(mx, len);
    const uint32_t n = (len + 15u) >> 4;
    const uint32_t incl = wave_incl_scan(n, lane);
    const uint32_t S = incl - n;
    const uint32_t W = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    const uint32_t nit = (W + 63u) >> 6;
    wave_lds_order();  // accumulator initialised / previous chunk's table reads done
    for (uint32_t q = lane; q < nit; q += 64u) head[q] = 0ull;
    wave_lds_order();
    if (r < kr) {
      meta[lane] = u32x4{offlo, offhi, len, S};
      __hip_atomic_fetch_or(&head[S >> 6], 1ull << (S & 63u), __ATOMIC_RELAXED,
                            __HIP_MEMORY_SCOPE_WAVEFRONT);
    }
    wave_lds_order();  // packet table and start mask complete
    const uint64_t below = lane == 63u ? ~0ull : ((2ull << lane) - 1ull);
    const uint32_t last = min(kr - c, 64u) - 1u;
    uint32_t before = 0;  // packet starts in earlier wave-iterations
    if (!wave_any(r < kr && len < 16u)) {
      // Every packet >= 16 B: every lane loads 16 in-packet bytes each
      // iteration (lanes past W re-read their packet's last window and drop
      // it), U iterations' loads in flight before the first XOR.
      for (uint32_t it = 0; it < nit; it += U) {
        // phase 1: the U start-mask words (independent LDS reads)
        uint64_t M[U];
#pragma unroll
        for (int u = 0; u < U; ++u) M[u] = it + u < nit ? head[it + u] : 0ull;
        // phase 2: packet of each window, its table entry
        u32x4 md[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const uint32_t pi = min(before + (uint32_t)__popcll(M[u] & below) - 1u, last);
          before += (uint32_t)__popcll(M[u]);
          md[u] = meta[pi];
        }
        // phase 3: U in-packet 16-B loads, all in flight
        u32x4 v[U];
        uint32_t tt[U], sh[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const uint32_t fl = 64u * (it + u) + lane;
          const uint32_t win = 16u * (fl - md[u].w);
          const bool full = win + 16u <= md[u].z;
          v[u] = ld16t<true>(a.bytes + (((uint64_t)md[u].y << 32) | md[u].x) +
                           (full ? win : md[u].z - 16u));
          sh[u] = full ? 0u : min(win + 16u - md[u].z, 15u);
          tt[u] = fl < W ? fl - md[u].w : 0xFFFFFFFFu;
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
          if (tt[u] != 0xFFFFFFFFu) lds_xor16(par, tt[u], shr_bytes_bf(v[u], sh[u]));
      }
    } else {
      // Some packet below 16 B (rare): generic per-lane windows.
      for (uint32_t it = 0; it < nit; ++it) {
        const uint64_t M = head[it];
        const uint32_t fl = 64u * it + lane;
        const uint32_t pi = min(before + (uint32_t)__popcll(M & below) - 1u, last);
        before += (uint32_t)__popcll(M);
        if (fl < W) {
          const u32x4 md = meta[pi];
          const uint32_t t = fl - md.w;
          lds_xor16(par, t, packet_window<false>(a.bytes + (((uint64_t)md.y << 32) | md.x),
                                                  md.z, t));
        }
      }
    }
  }
  if constexpr (ACCUM) {
    plen = max(wave_max11(mx), f.old);
    if (lane == 0) x->acc_len[f.slot] = (uint16_t)plen;
  } else if constexpr (!RECOVER) {
    plen = wave_max11(mx);
    if (lane == 0) a.parity_len_out[g] = (uint16_t)plen;
  }
  wave_lds_order();  // every lane's XORs into the accumulator done
  uint8_t* dst = a.out + f.dst_off;
  if (plen >= 16u) {
    const uint32_t nw = (plen + 15u) >> 4;
    for (uint32_t t = lane; t < nw; t += 64u) {
      if (16u * t + 16u <= plen) {
        st16t<true>(dst + 16u * t, lds_get16(par, t));
      } else {
        // tail: the 16 bytes ending at plen, from windows t-1 and t
        const uint32_t o = plen - 16u * t;  // 1..15
        const u32x4 lo = lds_get16(par, t - 1u), hi = lds_get16(par, t);
        st16t<true>(dst + plen - 16u, bytes16_at(lo, hi, o));
      }
    }
  } else if (lane < plen) {
    dst[lane] = (uint8_t)(par[acc_idx(0, lane >> 2)] >> (8u * (lane & 3u)));
  }
}

// One group's parity accumulator in LDS, component-major (ACC = 1).
constexpr uint32_t kAccWords = 4 * kParWin;

// Ragged CSR, large batches — the PRODUCT kernel (launch_ragged), round 3:
// BLOCK-flat windows.  A short-lived block of WAVES waves owns GPB consecutive
// groups and numbers the 16-B windows of ALL their received packets
// consecutively (the flat-window mapping of ragged_group, widened from one
// wave to the block); lane tid of iteration i takes window NT i + tid
// (NT = 64 WAVES), so one block instruction reads NT/4 KiB of the batch, in
// batch order.  Why: without its parity stores ragged_multi_kernel (each wave
// its own pair of groups, the waves 14 KB apart) read its packets at
// 5.56 TB/s, where 16 waves streaming one chunk (the chunk-phased experiment)
// read at ~6.3 TB/s — fewer, wider streams.  4 waves x 8 groups measured
// +2.5% encode / +4.5% recover over ragged_multi_kernel on three boxes;
// 2 x 4, 2 x 6, 4 x 6, 4 x 10, 4 x 12 less, 8 x 16 and 16 x 32 slower (block
// barriers), U = 1 / 3 no better (profiles/round3/ragged_block/, DESIGN.md
// §4).  One pass of setup per block: the group scalars (wave 0), one
// received packet per lane, a block scan for each packet's first window S, a
// start bitmask and per 64-window block the number of packets starting
// before it (a second block scan).  Blocks that do not fit (more than NT
// received packets or CAPW windows, a packet below 16 B, any invalid field)
// run the per-group body, one wave per group, so outputs and error bits are
// exactly those of the per-group kernel.  Encode parity lengths come from an
// LDS atomicMax.
//
// Recover and accumulate load their rows' windows into the accumulators before
// the packet table, so their round trip overlaps the table's; kRaggedU
// iterations' loads are in flight; a last window whose start is 16-B aligned
// is loaded in place and masked (below); loads and stores are nontemporal.
// DIAG (tools/tune only; bits): 1 = no parity stores (not exact); 2 = output
// rows stored as whole 128-B lines (zeros past the parity length up to the
// line end: the zero-padded parity of SURVEY.md Appendix A, for output slots
// that have the room -- the write-granularity probe of round 6); 4 = no tail
// logic (every window XORed whole, in place: the VALU probe of round 6, not
// exact).  The three are what the open store-schedule item is measured with
// (DESIGN.md §13).
// LIST (recover, qfec_revive_ragged): group slot j of the block is not group
// g0 + j with m = a.missing[g0 + j] but work-list entry step * GPB + j
// (g << 8 | m) of a list of `count` entries; a.missing and a.n_groups are not
// used.  The list is readable past the count but holds nothing there: only
// slots below the count are ever turned into a group.  Every return of the
// body is block-uniform, so a kernel may call it once per list step with a
// barrier between the steps (revive_ragged_kernel).
// ACCUM (encode form, qfec_accumulate_ragged; x its arguments): group slot j
// folds into accumulator row s = slot[g] (or g) of the caller's buffer, in
// place.  The LDS accumulator starts from that row up to its OLD length
// (s_old, zero from there on; nothing is loaded for a fresh slot, old == 0),
// the packets' lengths are limited by x->lim as in an encode, and the NEW
// length -- s_pl, which starts at the old one and takes the atomicMax of the
// packet lengths -- is written back to acc_len[s].  Two values on purpose: the
// row preload below reads the length with no barrier before the atomicMax.
// In place is safe because every load of a row precedes every store to it:
// the rows are read only by the preload, whose windows are in LDS before the
// barriers that follow it, and stored only after the last barrier; the
// unaligned tail store ("the 16 bytes ending at the length") overlaps the
// previous window's store with identical bytes.  Steps the block path does
// not take (an old length of 1..15, a group of no packets, any invalid field,
// and the cases above) run the per-group body, which leaves the row and the
// length of a group it rejects untouched.
//
// Variants measured and removed (template switches U, PF, AL and DIAG bits 8,
// 16 and 5-7, with the inline-assembly stores behind bits 5-7, in git history
// at ace3ed3; DESIGN.md §4, rounds 3 and 6): U = 1 / 3 no better than 2
// (profiles/round3/ragged_block/); the rows' windows loaded after the scan (PF
// off) measured equal (profiles/round3/ragged_block/block3.txt); every last
// window loaded as the 16 bytes ending at the packet end (AL off), the form
// before the aligned payload arena; the round-6 cache-policy probe, all exact
// (profiles/round6/tune_rblock_cache_r6p_{a16,a1}.txt, tune_rblock_pol_r6q.txt;
// encode, arena layout) -- payload loads through the caches (16) 0.713 against
// 0.736-0.739, parity stores through the caches (8) 0.530, stores with an
// explicit policy (5-7) sc1 / sc0 sc1 0.531 / 0.532, nt sc1 / nt sc0 sc1
// 0.656 / 0.665 against 0.691: the nontemporal loads and stores stay best.
template <bool RECOVER, int WAVES, int GPB, int DIAG = 0, bool LIST = false, bool ACCUM = false>
__device__ __forceinline__ void ragged_block_body(const RaggedArgs& a,
                                                  const uint64_t* __restrict__ work = nullptr,
                                                  uint64_t count = 0, uint64_t step = 0,
                                                  const AccumulateRaggedArgs* x = nullptr) {
  static_assert(GPB >= 2 && GPB <= 64, "group slots are lanes of wave 0");
  static_assert(!LIST || RECOVER, "the work list is a receiver's");
  static_assert(!ACCUM || (!RECOVER && !LIST), "accumulate: the encode form");
  static_assert((DIAG & ~7) == 0, "DIAG bits: 1 no stores, 2 whole-line stores, 4 no tail logic");
  constexpr int U = kRaggedU;
  constexpr bool ROWIN = RECOVER || ACCUM;  // the accumulators start from a row
  constexpr uint32_t NT = 64u * WAVES;
  constexpr uint32_t NBLK = NT;        // 64-window blocks: CAPW = 64 NT windows
  constexpr uint32_t CAPW = 64u * NBLK;
  // per-wave fallback scratch (ragged_group): accumulator, start mask, table
  constexpr uint32_t kFbWords = 4u * kParWin + 2u * kParWin + 4u * 64u;
  constexpr uint32_t kMainWords = GPB * kAccWords + 4u * NT;  // accumulators + packet table
  constexpr uint32_t kRawWords = kMainWords > WAVES * kFbWords ? kMainWords : WAVES * kFbWords;
  __shared__ uint32_t s_raw[kRawWords];
  __shared__ uint64_t s_head[NBLK];
  __shared__ uint32_t s_cnt[NBLK];
  __shared__ uint32_t s_rb[GPB + 1], s_kb[GPB], s_m[GPB], s_pl[GPB], s_ob[GPB + 1];
  __shared__ uint64_t s_doff[GPB], s_poff[GPB];
  __shared__ uint32_t s_w[WAVES], s_fit;
  __shared__ uint32_t s_old[GPB], s_slot[GPB];  // ACCUM only (else never referenced)
  uint32_t* acc = s_raw;
  u32x4* pk = reinterpret_cast<u32x4*>(s_raw + GPB * kAccWords);
  const uint32_t tid = threadIdx.x;
  const uint32_t lane = lane_id();
  const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane(tid >> 6);
  // LIST: g0 is the step's first list entry and the entries number `count`
  const uint64_t g0 = LIST ? step * GPB : (uint64_t)blockIdx.x * GPB;
  const uint64_t gn = LIST ? count : a.n_groups;
  if (g0 >= gn) return;  // block-uniform
  const uint32_t ng = (uint32_t)min<uint64_t>((uint64_t)GPB, gn - g0);
  s_head[tid] = 0ull;  // NBLK == NT
  // ---- 1. group scalars (wave 0, lane j = group slot j)
  if (wv == 0u) {
    uint32_t k = 0, m = 0xFFFFFFFFu, pl = 0, r = 0, p0 = 0;
    uint64_t d = 0, po = 0;
    bool ok = true;
    if (lane < ng) {
      uint64_t g = g0 + lane;
      if constexpr (LIST) list_entry(work[g0 + lane], g, m);
      p0 = a.grp_ptr[g];
      k = a.grp_ptr[g + 1] - p0;
      if constexpr (ACCUM) {
        const uint32_t s = x->slot ? x->slot[g] : x->slot_base + (uint32_t)g;
        const bool sok = s < x->n_slots;
        pl = sok ? (uint32_t)x->acc_len[s] : 0u;  // the old length
        d = po = (uint64_t)s * x->acc_stride;
        ok = sok && pl <= x->lim && (pl == 0u || pl >= 16u);
        s_slot[lane] = s;
        s_old[lane] = pl;
      } else if constexpr (RECOVER) {
        if constexpr (!LIST) m = a.missing[g0 + lane];
        pl = a.parity_len[g];
        d = a.out_off[g];
        po = a.parity_off[g];
        ok = m < k && pl >= 16u && pl <= kMaxPacket;
      } else {
        d = a.parity_off[g];
      }
      ok = ok && k >= 1u && k <= 255u;
      r = ok ? (RECOVER ? k - 1u : k) : 0u;
    }
    const uint32_t incl = wave_incl_scan(r, lane);
    const uint32_t R = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    if (lane < (uint32_t)GPB) {
      s_rb[lane] = incl - r;
      s_kb[lane] = p0;
      s_m[lane] = m;
      s_pl[lane] = pl;
      s_doff[lane] = d;
      s_poff[lane] = po;
    }
    const bool all_ok = !wave_any(lane < ng && !ok);  // every lane of wave 0
    if (lane == 0u) {
      s_rb[GPB] = R;
      s_fit = (all_ok && R <= NT) ? 1u : 0u;
    }
  }
  __syncthreads();
  const uint32_t R = s_rb[GPB];
  bool fit = s_fit != 0u;
  // ---- 2. one received packet per lane
  if (ROWIN && fit) {
    for (uint32_t q = tid; q < GPB * (uint32_t)kParWin; q += NT) {
      const uint32_t jq = q / (uint32_t)kParWin, t = q - jq * (uint32_t)kParWin;
      u32x4 w = {0u, 0u, 0u, 0u};
      if constexpr (ACCUM) {
        // (s_old, not s_pl: the atomicMax below may already have raised that)
        if (jq < ng && s_old[jq] != 0u)
          w = parity_window_bf<true>(a.parity + s_poff[jq], s_old[jq], t);
      } else {
        if (jq < ng) w = parity_window_bf<true>(a.parity + s_poff[jq], s_pl[jq], t);
      }
      lds_put16(acc + jq * kAccWords, t, w);
    }
  }
  uint32_t len = 0, offlo = 0, offhi = 0, j = 0;
  if (fit && tid < R) {
#pragma unroll
    for (int q = 1; q < GPB; ++q) j += tid >= s_rb[q] ? 1u : 0u;
    const uint32_t i = tid - s_rb[j];
    const uint32_t p = s_kb[j] + i + (RECOVER && i >= s_m[j] ? 1u : 0u);
    len = a.pkt_len[p];
    const uint64_t o = a.pkt_off[p];
    offlo = (uint32_t)o;
    offhi = (uint32_t)(o >> 32);
    uint32_t lim = kMaxPacket;
    if constexpr (RECOVER) lim = s_pl[j];
    if constexpr (ACCUM) lim = x->lim;
    if (len < 16u || len > lim) s_fit = 0u;  // benign race: every writer stores 0
    if (!RECOVER) atomicMax(&s_pl[j], len);
  }
  const uint32_t n = (len + 15u) >> 4;
  uint32_t W;
  const uint32_t S = block_excl_scan<WAVES>(n, lane, wv, s_w, W);  // (barriers publish s_fit)
  fit = fit && s_fit != 0u && W <= CAPW;
  if (!fit) {
    // per-group body, one wave per group (exact outputs and error bits)
    uint32_t* fb = s_raw + wv * kFbWords;
    for (uint32_t jj = wv; jj < ng; jj += WAVES) {
      GroupPrefetch f;
      uint64_t g = g0 + jj;
      uint32_t lm = 0;
      if constexpr (LIST) list_entry(work[g0 + jj], g, lm);  // jj < ng: below the count
      group_scalars<RECOVER, LIST, ACCUM>(a, g, f, lm, x);
      group_vectors<RECOVER, ACCUM>(a, g, lane, f, x);
      wave_lds_order();
      ragged_group<RECOVER, ACCUM>(a, g, lane, f, fb,
                                   reinterpret_cast<uint64_t*>(fb + 4u * kParWin),
                                   reinterpret_cast<u32x4*>(fb + 6u * kParWin), x);
      wave_lds_order();
    }
    return;
  }
  if (tid < R) {
    pk[tid] = u32x4{offlo, offhi, len | (j << 16), S};
    __hip_atomic_fetch_or(&s_head[S >> 6], 1ull << (S & 63u), __ATOMIC_RELAXED,
                          __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  // accumulators of an encode: zero, windows of all groups
  if (!ROWIN) {
    for (uint32_t q = tid; q < GPB * (uint32_t)kParWin; q += NT) {
      const uint32_t jq = q / (uint32_t)kParWin, t = q - jq * (uint32_t)kParWin;
      const u32x4 w = {0u, 0u, 0u, 0u};
      lds_put16(acc + jq * kAccWords, t, w);
    }
  }
  __syncthreads();  // packet table, start mask, accumulators, parity lengths
  const uint32_t nblk = (W + 63u) >> 6;
  uint32_t tot;
  const uint32_t c = block_excl_scan<WAVES>(tid < nblk ? (uint32_t)__popcll(s_head[tid]) : 0u,
                                            lane, wv, s_w, tot);
  s_cnt[tid] = c;
  if (wv == 0u) {  // output windows per group (encode: the max lengths are final)
    uint32_t nw = lane < ng ? (s_pl[lane] + 15u) >> 4 : 0u;
    if (DIAG & 2) nw = lane < ng ? ((s_pl[lane] + 127u) >> 7) << 3 : 0u;
    const uint32_t incl = wave_incl_scan(nw, lane);
    if (lane < (uint32_t)GPB) s_ob[lane] = incl - nw;
    if (lane == 0u) s_ob[GPB] = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    if constexpr (ACCUM) {
      if (lane < ng) x->acc_len[s_slot[lane]] = (uint16_t)s_pl[lane];
    } else {
      if (!RECOVER && lane < ng) a.parity_len_out[g0 + lane] = (uint16_t)s_pl[lane];
    }
  }
  __syncthreads();
  // ---- 3. the flat windows, U iterations' loads in flight
  const uint64_t below = lane == 63u ? ~0ull : ((2ull << lane) - 1ull);
  const uint32_t nit = (W + NT - 1u) / NT;
  for (uint32_t it = 0; it < nit; it += U) {
    u32x4 md[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t f = (it + (uint32_t)u) * NT + tid;
      const uint32_t b = min(f >> 6, nblk - 1u);
      const uint64_t M = s_head[b];
      const uint32_t pi = min(s_cnt[b] + (uint32_t)__popcll(M & below) - 1u, R - 1u);
      md[u] = pk[pi];
    }
    u32x4 v[U];
    uint32_t tt[U], sh[U];
    bool inp[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t f = (it + (uint32_t)u) * NT + tid;
      const uint32_t ln = md[u].z & 0xFFFFu;
      const uint32_t win = 16u * (f - md[u].w);
      const bool full = win + 16u <= ln;
      const uint64_t at = (((uint64_t)md[u].y << 32) | md[u].x) + win;
      // A last window whose start is 16-B aligned (payloads on 16-B
      // boundaries, the payload arena's layout) is loaded in place and its
      // bytes past the packet masked: an aligned 16-B load holding one packet
      // byte cannot leave that byte's page.  Otherwise the 16 bytes ending at
      // the packet end, shifted down.
      inp[u] = full || (win < ln && (at & 15u) == 0u) || (DIAG & 4);
      v[u] = ld16t<true>(a.bytes + (inp[u] ? at : at - win + ln - 16u));
      sh[u] = full ? 0u : min(win + 16u - ln, 15u);
      tt[u] = f < W ? (md[u].z >> 16) * kAccWords + (f - md[u].w) : 0xFFFFFFFFu;
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (tt[u] != 0xFFFFFFFFu) {
        u32x4 w;
        if constexpr ((DIAG & 4) != 0) {
          w = v[u];
        } else {
          // in place: v & (ones >> sh); shifted: v >> sh (sh = 0 when full)
          const u32x4 ones = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
          const u32x4 m = shr_bytes_bf(inp[u] ? ones : v[u], sh[u]);
          w = inp[u] ? (m & v[u]) : m;
        }
        lds_xor16<__HIP_MEMORY_SCOPE_WORKGROUP>(acc, tt[u], w);
      }
  }
  __syncthreads();  // every lane's XORs done
  // ---- 4. stores, flattened over the groups' output windows
  const uint32_t NW = s_ob[GPB];
  for (uint32_t q = tid; q < NW; q += NT) {
    uint32_t jq = 0;
#pragma unroll
    for (int i = 1; i < GPB; ++i) jq += q >= s_ob[i] ? 1u : 0u;
    const uint32_t t = q - s_ob[jq];
    const uint32_t plen = s_pl[jq];
    uint8_t* dst = a.out + s_doff[jq];
    const uint32_t* ac = acc + jq * kAccWords;
    if ((DIAG & 1) && plen != 0xFFFFFu) continue;  // never a real length: no stores
    if (DIAG & 2) {  // whole lines: the accumulator is zero past plen
      const u32x4 z = {0u, 0u, 0u, 0u};
      st16t<true>(dst + 16u * t, t < (uint32_t)kParWin ? lds_get16(ac, t) : z);
      continue;
    }
    if (16u * t + 16u <= plen) {
      st16t<true>(dst + 16u * t, lds_get16(ac, t));
    } else {
      const uint32_t o = plen - 16u * t;  // 1..15
      const u32x4 x = bytes16_at(lds_get16(ac, t - 1u), lds_get16(ac, t), o);
      st16t<true>(dst + plen - 16u, x);
    }
  }
}


// Completion signal for a host that spins on mapped memory instead of
// waiting on an event (~6 us less per flush, tools/tune/tune_latency): every
// thread's stores (outputs in mapped host memory) are made visible
// system-wide, the block is counted, and the last block to finish resets the
// counter and stores the token into the host-mapped flag.  Block-uniform
// call, after the block's work.
__device__ __forceinline__ void ragged_signal_done(const RaggedArgs& a) {
  if (a.done_flag == nullptr) return;
  __threadfence_system();
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t prev = __hip_atomic_fetch_add(a.done_count, 1u, __ATOMIC_ACQ_REL,
                                                 __HIP_MEMORY_SCOPE_AGENT);
    if (prev == gridDim.x - 1u) {
      __hip_atomic_store(a.done_count, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __threadfence_system();
      __hip_atomic_store(a.done_flag, a.done_token, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

// The block kernel; with done_flag set (mapped batches of any size, round 4)
// it signals completion like the small-batch kernel, so the host neither
// stages the tables nor waits on an event.
template <bool RECOVER, int WAVES, int GPB, int DIAG = 0>
__global__ __launch_bounds__(64 * WAVES) void ragged_block_kernel(RaggedArgs a) {
  ragged_block_body<RECOVER, WAVES, GPB, DIAG>(a);
  ragged_signal_done(a);
}

// qfec_revive_ragged's fourth kernel: the recover block body over the packed
// work list of the revivable groups (classify / scan / emit above), GPB list
// entries per step.  The count stays on the device: the grid is sized by the
// device and its blocks loop over the list steps; the body's early returns end
// a step (all block-uniform), and the barrier keeps a step's LDS from the next
// one's writes.  `work` and `totals` are restrict parameters of their own, as
// for revive_xor_kernel.
template <int WAVES, int GPB>
__global__ __launch_bounds__(64 * WAVES) void revive_ragged_kernel(
    ReviveRaggedArgs v, const uint64_t* __restrict__ work, const uint64_t* __restrict__ totals) {
  RaggedArgs a{};
  a.bytes = v.bytes;
  a.pkt_off = v.pkt_off;
  a.pkt_len = v.pkt_len;
  a.grp_ptr = v.grp_ptr;
  a.parity = v.parity;
  a.parity_off = v.parity_off;
  a.parity_len = v.parity_len;
  a.out = v.out;
  a.out_off = v.out_off;
  a.n_groups = v.n_groups;
  a.err = v.err;
  const uint64_t count = totals[kGroupRevived];
  const uint64_t nstep = (count + GPB - 1) / GPB;
  for (uint64_t step = blockIdx.x; step < nstep; step += gridDim.x) {
    ragged_block_body<true, WAVES, GPB, 0, true>(a, work, count, step);
    __syncthreads();  // the step's LDS reads are done before the next step's writes
  }
}

// qfec_accumulate_ragged: the encode block body in its accumulate mode, GPB
// groups per block.  The accumulator buffer is both the body's "parity" (the
// rows on entry) and its output.
template <int WAVES, int GPB>
__global__ __launch_bounds__(64 * WAVES) void accumulate_ragged_kernel(AccumulateRaggedArgs v) {
  RaggedArgs a{};
  a.bytes = v.bytes;
  a.pkt_off = v.pkt_off;
  a.pkt_len = v.pkt_len;
  a.grp_ptr = v.grp_ptr;
  a.parity = v.acc;
  a.out = v.acc;
  a.n_groups = v.n_groups;
  a.err = v.err;
  ragged_block_body<false, WAVES, GPB, 0, false, true>(a, nullptr, 0, 0, &v);
}

// Lane j's 64-bit value as a scalar (j wave-uniform).
__device__ __forceinline__ uint64_t lane_get64(uint64_t v, uint32_t j) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, (int)j);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), (int)j);
  return (uint64_t)lo | ((uint64_t)hi << 32);
}

// qfec_emit_accumulated (LIST = false: every group, the call's one launch) and
// qfec_revive_accumulated's fourth kernel (LIST = true: the work list, its
// count read from scratch as revive_xor_kernel reads it): copy len bytes of
// row acc + s * acc_stride to out + out_off[g], one wave per row.
// A wave takes `per` consecutive rows at a time -- the rows spread evenly over
// the grid's waves, 64 at most -- and lane j fetches row j's tables (entry or
// group, slot, length, out_off) for all of them at once, so the dependent
// chain entry -> slot -> length in front of a row's bytes is paid once per
// step, not once per row; the rows are then copied one by one with the lane's
// values read back as scalars (v_readlane).  LIST = false does its bookkeeping
// in that per-lane part: out_len, a slot out of range (kErrMissingIndex) or a
// length above the limit (kErrParityLength; both: out_len 0, nothing copied,
// no release) and, with release, acc_len[s] = 0 -- stored after the lane's
// own load of it, and the copy reads the length from the lane, never from
// acc_len.  out_off is read only for rows that are copied.
// A row of 16 bytes or more is cut where the DESTINATION is 16-B aligned (a
// 16-B store across a 16-B boundary costs two): with h
// the bytes up to dst's first boundary, the aligned chunks [h + 16 t,
// h + 16 t + 16), the head [0, 16) if h != 0 and the tail, the 16 bytes ending
// at the length, if the chunks do not end there.  Head and tail overlap their
// neighbours with identical bytes; every chunk lies inside [0, len) of both
// the row and the destination.  At most 90 + 2 chunks (len <= 1452): two per
// lane, both loads issued before the first store; a chunk number past the
// last one loads the tail again and stores nothing.  Shorter rows go a byte
// per lane.
template <bool LIST>
__global__ __launch_bounds__(kBlock) void close_gather_kernel(CloseArgs a,
                                                              const uint64_t* __restrict__ work,
                                                              const uint64_t* __restrict__ totals) {
  constexpr uint32_t kWaves = kBlock / 64;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // (n_groups < 2^32, so the counts and the divisions are 32-bit)
  uint32_t count = (uint32_t)a.n_groups;
  if constexpr (LIST) count = (uint32_t)totals[kGroupRevived];
  if (count == 0u) return;
  const uint32_t nwave = gridDim.x * kWaves;
  const uint32_t per = min(count / nwave + (count % nwave != 0u ? 1u : 0u), 64u);
  const uint32_t nstep = count / per + (count % per != 0u ? 1u : 0u);
  for (uint32_t step = blockIdx.x * kWaves + wave; step < nstep; step += nwave) {
    const uint64_t i = (uint64_t)step * per + lane;
    uint32_t len = 0;
    uint64_t soff = 0, doff = 0;
    if (lane < per && i < (uint64_t)count) {
      uint64_t g;
      uint32_t s;
      if constexpr (LIST) {
        const uint64_t e = work[i];
        uint32_t m;
        list_entry(e, g, m);
        len = ((uint32_t)(e >> 32) >> (kCloseLenShift - 32u)) & 0x7FFu;
        s = close_slot(a, g);  // in range: the emit pass gave the entry a length
      } else {
        g = i;
        s = close_slot(a, g);
        uint32_t bad = s >= a.n_slots ? kErrMissingIndex : 0u;
        if (bad == 0u) {
          len = a.acc_len[s];
          if (len > a.lim) {
            bad = kErrParityLength;
            len = 0;
          }
        }
        a.out_len[g] = (uint16_t)len;
        if (bad != 0u) atomicOr(a.err, bad);
        else if (a.release != 0u) a.acc_len[s] = 0;
      }
      if (len != 0u) {
        soff = (uint64_t)s * a.acc_stride;
        doff = a.out_off[g];
      }
    }
    for (uint64_t todo = __ballot(len != 0u); todo != 0ull; todo &= todo - 1ull) {
      const uint32_t j = (uint32_t)__builtin_ctzll(todo);
      const uint32_t n = (uint32_t)__builtin_amdgcn_readlane((int)len, (int)j);
      const uint8_t* src = a.acc + lane_get64(soff, j);
      uint8_t* dst = a.out + lane_get64(doff, j);
      if (n >= 16u) {
        const uint32_t h = (0u - (uint32_t)reinterpret_cast<uintptr_t>(dst)) & 15u;
        const uint32_t na = (n - h) >> 4;
        const bool tail = h + 16u * na != n;
        uint32_t o[2];
        bool st[2];
#pragma unroll
        for (uint32_t c = 0; c < 2u; ++c) {
          const uint32_t t = lane + 64u * c;
          o[c] = t < na ? h + 16u * t : t == na ? 0u : n - 16u;
          st[c] = t < na || (t == na ? h != 0u : (t == na + 1u && tail));
        }
        const u32x4 v0 = ld16t<true>(src + o[0]), v1 = ld16t<true>(src + o[1]);
        if (st[0]) st16t<true>(dst + o[0], v0);
        if (st[1]) st16t<true>(dst + o[1], v1);
      } else if (lane < n) {
        dst[lane] = src[lane];
      }
    }
  }
}
static_assert((kMaxPacket + 15u) / 16u + 2u <= 128u, "two chunks per lane cover a row");

// Two groups per wave (round 2's product kernel; since round 6 the kernel of
// large batches whose groups are small -- launch_ragged's shape-aware choice,
// below): kPairGroups = 2 consecutive groups in
// ONE flat window space — their received packets fill the 64-lane packet
// table together — so the per-group load chain (group pointer -> packet table
// -> packet bytes), which parks the one-group waves for 70% of their cycles
// (SQ_WAIT_ANY, profiles/round1/sq_stalls_fec_pq.txt), and the partially idle
// last iteration are paid once per pair.  Groups that do not fit (more
// than 64 received packets together, a packet below 16 B, any invalid field)
// run the per-group body above with its exact error semantics.  Measured
// +1.0-1.6% encode and recover over one group per wave in three interleaved
// A/B runs (tune_multi_t2.txt, ragged_slots_p*.txt, tune_multi_sp.txt);
// three groups per wave overflow the table too often (-10%).
//
// Variants measured and removed (template switches NT, GPW, U, WAVES, BF and
// the parity-window form, in git history at ace3ed3; NT, U and BF as for
// ragged_group above): U = 1 / 3 -1.7% / +0.7%, 2 or 8 waves per block
// -0.6% / -0.5...-2.6% (profiles/round1/tune_multi_mu.txt); the recover's
// parity windows loaded under lane masks (round 2's form) recover 0.608
// against 0.615 strided, 0.593 against 0.605 packed
// (profiles/round2/ragged_store/tune_rw_diag5*.txt).

template <int N, typename T>
__device__ __forceinline__ T sel_n(const T (&v)[N], uint32_t j) {
  T r = v[0];
#pragma unroll
  for (int i = 1; i < N; ++i) r = j == (uint32_t)i ? v[i] : r;
  return r;
}

// The kPairGroups groups g0 .. g0+ng-1 of one wave, up to their XOR into the
// LDS accumulators `par` (kPairGroups x kAccWords).  Returns false when the groups took
// the per-group body (odd packets, invalid fields, > 64 received packets):
// then their outputs are already stored; true: ragged_pair_store writes them
// from `par` with lengths pl[] at offsets doff[].

template <bool RECOVER>
__device__ __forceinline__ bool ragged_pair_xor(const RaggedArgs& a, uint64_t g0, uint32_t ng,
                                                uint32_t lane, uint32_t* par, uint64_t* head,
                                                u32x4* meta, uint32_t (&pl)[kPairGroups],
                                                uint64_t (&doff)[kPairGroups]) {
  constexpr int U = kRaggedU;
  // wave-uniform group scalars
  uint32_t kb[kPairGroups + 1], rb[kPairGroups + 1], mm[kPairGroups];
  const uint32_t P0 = a.grp_ptr[g0];
  bool ok = true;
  kb[0] = rb[0] = 0;
#pragma unroll
  for (int j = 0; j < kPairGroups; ++j) {
    uint32_t k = 0, m = 0xFFFFFFFFu, p = 0;
    uint64_t d = 0;
    if ((uint32_t)j < ng) {
      k = a.grp_ptr[g0 + j + 1] - P0 - kb[j];
      if constexpr (RECOVER) {
        m = a.missing[g0 + j];
        p = a.parity_len[g0 + j];
        d = a.out_off[g0 + j];
        ok = ok && m < k && p >= 16u && p <= kMaxPacket;
      } else {
        d = a.parity_off[g0 + j];
      }
      ok = ok && k >= 1u && k <= 255u;
    }
    kb[j + 1] = kb[j] + k;
    rb[j + 1] = rb[j] + (RECOVER && k ? k - 1u : k);
    mm[j] = m;
    pl[j] = p;
    doff[j] = d;
  }
  const uint32_t R = rb[kPairGroups];
  ok = ok && R <= 64u;

  // lane r: received packet r of the wave's groups
  uint32_t jl = 0, base = 0, kbase = 0, ml = 0xFFFFFFFFu, lim = kMaxPacket;
#pragma unroll
  for (int j = 1; j < kPairGroups; ++j) {
    const bool in = lane >= rb[j];
    jl += in ? 1u : 0u;
    base = in ? rb[j] : base;
    kbase = in ? kb[j] : kbase;
  }
  ml = sel_n<kPairGroups>(mm, jl);
  if constexpr (RECOVER) lim = sel_n<kPairGroups>(pl, jl);
  uint32_t len = 0, offlo = 0, offhi = 0;
  if (ok && lane < R) {
    const uint32_t i = lane - base;
    const uint32_t p = P0 + kbase + i + (RECOVER && i >= ml ? 1u : 0u);
    len = a.pkt_len[p];
    const uint64_t o = a.pkt_off[p];
    offlo = (uint32_t)o;
    offhi = (uint32_t)(o >> 32);
  }
  // accumulators: the parity rows (recover) or zero (encode)
  if (ok) {
#pragma unroll
    for (int j = 0; j < kPairGroups; ++j) {
      uint32_t* acc = par + j * kAccWords;
      if constexpr (RECOVER) {
        const uint8_t* prow = a.parity + ((uint32_t)j < ng ? a.parity_off[g0 + j] : 0ull);
        const uint32_t plj = (uint32_t)j < ng ? pl[j] : 0u;
        // branch-free parity windows: every lane loads a window inside the
        // row (lanes past plj re-read its last 16 bytes and keep zero), so
        // neither load runs with lanes masked off.  plj >= 16 whenever the
        // pair takes this path (ok); the branch is wave-uniform.
        const u32x4 zero = {0u, 0u, 0u, 0u};
        u32x4 w0 = zero, w1 = zero;
        if (plj >= 16u) {
          w0 = parity_window_bf<true>(prow, plj, lane);
          w1 = parity_window_bf<true>(prow, plj, lane + 64u);
        }
        lds_put16(acc, lane, w0);
        if (lane + 64u < kParWin) lds_put16(acc, lane + 64u, w1);
      } else {
        const u32x4 zero = {0u, 0u, 0u, 0u};
        for (uint32_t t = lane; t < kParWin; t += 64u) lds_put16(acc, t, zero);
      }
    }
  }
  const bool odd = lane < R && (len < 16u || len > lim);
  if (!ok || wave_any(odd)) {
    // per-group body (exact error semantics of the one-group kernel)
    for (uint32_t j = 0; j < ng; ++j) {
      GroupPrefetch f;
      group_scalars<RECOVER>(a, g0 + j, f);
      group_vectors<RECOVER>(a, g0 + j, lane, f);
      wave_lds_order();
      ragged_group<RECOVER>(a, g0 + j, lane, f, par, head, meta);
      wave_lds_order();
    }
    return false;
  }
  const uint32_t n = (len + 15u) >> 4;
  const uint32_t incl = wave_incl_scan(n, lane);
  const uint32_t S = incl - n;
  const uint32_t W = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
  const uint32_t nit = (W + 63u) >> 6;  // W <= 64 x 91
  for (uint32_t q = lane; q < nit; q += 64u) head[q] = 0ull;
  wave_lds_order();
  if (lane < R) {
    meta[lane] = u32x4{offlo, offhi, len | (jl << 16), S};
    __hip_atomic_fetch_or(&head[S >> 6], 1ull << (S & 63u), __ATOMIC_RELAXED,
                          __HIP_MEMORY_SCOPE_WAVEFRONT);
  }
  wave_lds_order();  // accumulators, packet table and start mask complete
  const uint64_t below = lane == 63u ? ~0ull : ((2ull << lane) - 1ull);
  const uint32_t last = R - 1u;
  uint32_t before = 0;
  for (uint32_t it = 0; it < nit; it += U) {
    uint64_t M[U];
#pragma unroll
    for (int u = 0; u < U; ++u) M[u] = it + u < nit ? head[it + u] : 0ull;
    u32x4 md[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t pi = min(before + (uint32_t)__popcll(M[u] & below) - 1u, last);
      before += (uint32_t)__popcll(M[u]);
      md[u] = meta[pi];
    }
    u32x4 v[U];
    uint32_t tt[U], sh[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t fl = 64u * (it + u) + lane;
      const uint32_t ln = md[u].z & 0xFFFFu;
      const uint32_t win = 16u * (fl - md[u].w);
      const bool full = win + 16u <= ln;
      v[u] = ld16t<true>(a.bytes + (((uint64_t)md[u].y << 32) | md[u].x) + (full ? win : ln - 16u));
      sh[u] = full ? 0u : min(win + 16u - ln, 15u);
      tt[u] = fl < W ? (md[u].z >> 16) * kAccWords + (fl - md[u].w) : 0xFFFFFFFFu;
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (tt[u] != 0xFFFFFFFFu) lds_xor16(par, tt[u], shr_bytes_bf(v[u], sh[u]));
  }
  if constexpr (!RECOVER) {
#pragma unroll
    for (int j = 0; j < kPairGroups; ++j) {
      pl[j] = wave_max11(lane < R && jl == (uint32_t)j ? len : 0u);
      if (lane == 0 && (uint32_t)j < ng) a.parity_len_out[g0 + j] = (uint16_t)pl[j];
    }
  }
  return true;
}

__device__ __forceinline__ void ragged_pair_store(const RaggedArgs& a, uint32_t ng, uint32_t lane,
                                                  const uint32_t* par,
                                                  const uint32_t (&pl)[kPairGroups],
                                                  const uint64_t (&doff)[kPairGroups]) {
  wave_lds_order();  // every lane's XORs done
  // write-out, flattened over the groups' output windows
  uint32_t ob[kPairGroups + 1];
  ob[0] = 0;
#pragma unroll
  for (int j = 0; j < kPairGroups; ++j)
    ob[j + 1] = ob[j] + ((uint32_t)j < ng ? (pl[j] + 15u) >> 4 : 0u);
  const uint32_t NW = ob[kPairGroups];
  for (uint32_t q = lane; q < NW; q += 64u) {
    uint32_t jq = 0, qb = 0;
#pragma unroll
    for (int j = 1; j < kPairGroups; ++j) {
      const bool in = q >= ob[j];
      jq += in ? 1u : 0u;
      qb = in ? ob[j] : qb;
    }
    const uint32_t t = q - qb;
    const uint32_t plen = sel_n<kPairGroups>(pl, jq);
    uint8_t* dst = a.out + sel_n<kPairGroups>(doff, jq);
    const uint32_t* acc = par + jq * kAccWords;
    if (16u * t + 16u <= plen) {
      st16t<true>(dst + 16u * t, lds_get16(acc, t));
    } else {
      const uint32_t o = plen - 16u * t;  // 1..15
      const u32x4 lo = lds_get16(acc, t - 1u), hi = lds_get16(acc, t);
      st16t<true>(dst + plen - 16u, bytes16_at(lo, hi, o));
    }
  }
}

// (with done_flag set -- a direct mapped batch -- it signals completion like
// the block kernel: every wave reaches ragged_signal_done)
template <bool RECOVER>
__global__ __launch_bounds__(64 * kPairWaves) void ragged_multi_kernel(RaggedArgs a) {
  __shared__ uint32_t s_par[kPairWaves][kPairGroups * kAccWords];
  __shared__ uint64_t s_head[kPairWaves][kParWin];
  __shared__ u32x4 s_meta[kPairWaves][64];
  const uint32_t lane = lane_id();
  const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t g0 = ((uint64_t)blockIdx.x * kPairWaves + wv) * kPairGroups;
  if (g0 < a.n_groups) {  // wave-uniform
    const uint32_t ng = (uint32_t)min<uint64_t>((uint64_t)kPairGroups, a.n_groups - g0);
    uint32_t pl[kPairGroups];
    uint64_t doff[kPairGroups];
    if (ragged_pair_xor<RECOVER>(a, g0, ng, lane, s_par[wv], s_head[wv], s_meta[wv], pl, doff))
      ragged_pair_store(a, ng, lane, s_par[wv], pl, doff);
  }
  ragged_signal_done(a);
}


// Ragged CSR, parity-window form — the SMALL-BATCH (latency) kernel: the
// mapped host path runs a batch of <= kDirectGroups groups with it
// (qfec_capi.cpp ragged_mapped), where the payloads are read over PCIe and a
// group's time is its count of dependent round trips, not bandwidth.  (On
// large device-resident batches it is 0.77x ragged_multi_kernel: the
// texture-address unit costs ~64 cycles per 64-lane load whatever its useful
// lanes; profiles/round2/tune_rw_window*.txt, DESIGN.md §4 -- the A/B driver,
// tools/tune/tune_rw.hip, is in git history at ace3ed3.)  Loads and stores
// are nontemporal and kWindowPB = 16 slots are in flight: the library never
// launched another value of the kernel's switches NT and PB (in git history
// at ace3ed3; window_group keeps PB and NP, which the service varies).
// One wave per group, lane l owns the parity
// windows at bytes w0 = min(16l, plen-16) and w1 = min(16(l+64), plen-16) —
// the fixed-shape kernel's mapping (the last window ends exactly at plen and
// overlaps its neighbour with identical bytes), so there is no accumulator in
// LDS, no atomics and no packet search.  The group's packet table is one
// coalesced vector load (lane r = received packet r); packet r's offset and
// length are then wave-uniform (v_readlane), and every lane loads the 16 bytes
// of packet r under its window (a window crossing the packet end loads the 16
// bytes ending at the packet end and shifts them down; a window past it loads
// them too — the same lines as the lane that needs them — and XORs zero).
// Load slots: window w0 of every received packet, then window w1 of the
// packets that reach one (found by a ballot, walked with s_ff1); PB slots'
// loads are in flight before the first XOR, independent of one another, so a
// group costs three dependent round trips (group scalars -> packet table ->
// all packet bytes) instead of one per 2 KiB (ragged_multi_kernel's flat
// windows: profiles/round1/sq_stalls_fec_pq.txt, parked 68-78% of cycles).
// Groups outside the form (more than 64 received packets, a packet < 16 B,
// any invalid field) run the exact per-group body (ragged_group).
// a value every lane holds alike, moved to an SGPR
__device__ __forceinline__ uint32_t uni32(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
}
__device__ __forceinline__ uint64_t uni64(uint64_t v) {
  return ((uint64_t)uni32((uint32_t)(v >> 32)) << 32) | uni32((uint32_t)v);
}

// NP > 1: one group on NP waves (the service's one-group job).  Wave `part`
// takes every NP-th slot and leaves its partial windows in red0 / red1
// [part * 64 + lane]; the caller XORs the NP partials after a barrier and
// stores them where the returned WinOut says (red); a group out of the fast
// form is finished by part 0 alone (!red).  Only part 0 stores the encode length and
// folds in the recover parity.
struct WinOut {
  uint8_t* dst;
  uint32_t w0, w1, nwin;
  bool red;  // partials left in red0 / red1 (false: finished, or NP == 1)
};

template <bool RECOVER, int PB, int NP = 1>
__device__ __forceinline__ WinOut window_group(const RaggedArgs& a, uint64_t g, uint32_t lane,
                                               uint32_t* s_par, uint64_t* s_head, u32x4* s_meta,
                                               uint32_t part = 0, u32x4* red0 = nullptr,
                                               u32x4* red1 = nullptr) {
  static_assert(PB % NP == 0, "slots split evenly over the waves");
  constexpr int PW = PB / NP;                     // loads per wave per chunk
  const uint32_t pt = NP == 1 ? 0u : part;        // (NP == 1: constant slot numbers)
  // trip 1: the group's scalars (s_load; the service's tables sit in LDS
  // behind generic pointers: flat loads into VGPRs, which the compiler takes
  // for per-lane values -- every slot below then became a waterfall loop
  // around its load, ~3 us of issue for one group -- so the scalars are
  // moved to SGPRs explicitly)
  const uint32_t p0 = uni32(a.grp_ptr[g]);
  const uint32_t k = uni32(a.grp_ptr[g + 1]) - p0;
  uint32_t m = 0xFFFFFFFFu, plen = 0;
  uint64_t dst_off, par_off = 0;
  if constexpr (RECOVER) {
    m = uni32(a.missing[g]);
    plen = uni32(a.parity_len[g]);
    dst_off = uni64(a.out_off[g]);
    par_off = uni64(a.parity_off[g]);
  } else {
    dst_off = uni64(a.parity_off[g]);
  }
  const uint32_t kr = RECOVER ? k - 1u : k;  // received packets
  const bool form = k >= 1u && k <= 255u && kr <= 64u &&
                    (!RECOVER || (m < k && plen >= 16u && plen <= kMaxPacket));
  // trip 2: the packet table (lane r = received packet r) and, for recover,
  // the parity windows (they need only the scalars)
  uint32_t len = 0, offlo = 0, offhi = 0;
  if (form && lane < kr) {
    const uint32_t p = p0 + lane + (RECOVER && lane >= m ? 1u : 0u);
    len = a.pkt_len[p];
    const uint64_t o = a.pkt_off[p];
    offlo = (uint32_t)o;
    offhi = (uint32_t)(o >> 32);
  }
  u32x4 acc0 = {0u, 0u, 0u, 0u}, acc1 = {0u, 0u, 0u, 0u};
  uint32_t w0 = 0, w1 = 0;
  if (RECOVER && form) {
    w0 = min(16u * lane, plen - 16u);
    w1 = min(16u * (lane + 64u), plen - 16u);
    if (pt == 0u) {
      const uint8_t* prow = a.parity + par_off;
      acc0 = ld16t<true>(prow + w0);
      if (plen > 1024u) acc1 = ld16t<true>(prow + w1);
    }
  }
  const uint32_t lim = RECOVER ? plen : kMaxPacket;
  if (!form || wave_any(lane < kr && (len < 16u || len > lim))) {
    if (pt == 0u) {
      GroupPrefetch f;
      group_scalars<RECOVER>(a, g, f);
      group_vectors<RECOVER>(a, g, lane, f);
      ragged_group<RECOVER>(a, g, lane, f, s_par, s_head, s_meta);
    }
    return WinOut{nullptr, 0u, 0u, 0u, false};
  }
  if constexpr (!RECOVER) {
    plen = wave_max11(len);
    if (lane == 0 && pt == 0u) a.parity_len_out[g] = (uint16_t)plen;
    w0 = min(16u * lane, plen - 16u);
    w1 = min(16u * (lane + 64u), plen - 16u);
  }
  // second windows: lanes' w1 >= min(1024, plen - 16), so exactly the packets
  // longer than that reach one
  const uint64_t longm = plen > 1024u ? __ballot(lane < kr && len > min(1024u, plen - 16u)) : 0ull;
  const uint32_t ns = kr + (uint32_t)__popcll(longm);
  // slot tables, lane t describing slots t and t + 64: slot j < kr is packet
  // j's first window, slot kr + n the second window of the n-th long packet
  // (the n-th set bit of longm, found by halving), a slot at or past ns none
  // (length 0).  A slot's load then costs three readlanes and its descriptor.
  // (One wave issues an instruction every few cycles: the per-slot search
  // for the next long packet, ~35 instructions a slot, spread a group's 20
  // loads over ~1.5 us of the service's one-group latency.)
  auto slot_packet = [&](uint32_t j) -> uint32_t {
    uint32_t n = j - kr, pos = 0u, w = (uint32_t)longm;
    const uint32_t clo = (uint32_t)__popc((uint32_t)longm);
    const bool up = n >= clo;
    n = up ? n - clo : n;
    pos = up ? 32u : 0u;
    w = up ? (uint32_t)(longm >> 32) : w;
#pragma unroll
    for (uint32_t b = 16u; b >= 1u; b >>= 1) {
      const uint32_t c = (uint32_t)__popc(w & ((1u << b) - 1u));
      const bool ge = n >= c;
      n = ge ? n - c : n;
      pos = ge ? pos + b : pos;
      w = ge ? w >> b : w;
    }
    return j < kr ? j : pos;  // (pos <= 63 for any j: a valid shuffle lane)
  };
  const uint32_t rA = slot_packet(lane), rB = slot_packet(lane + 64u);
  // (every shuffle with the whole wave active: a lane that reads an inactive
  // lane's value gets 0, so none sits under the `< ns` condition)
  const uint32_t shA = lane_read(len, rA);
  const uint32_t shB = lane_read(len, rB);
  const uint32_t lenA = lane < ns ? shA : 0u;
  const uint32_t lenB = lane + 64u < ns ? shB : 0u;
  const uint32_t olA = lane_read(offlo, rA);
  const uint32_t ohA = lane_read(offhi, rA);
  const uint32_t olB = lane_read(offlo, rB);
  const uint32_t ohB = lane_read(offhi, rB);
  // trip 3: every slot's bytes, PB loads in flight per lane.  Branch-free: a
  // slot past the end loads through a descriptor of 0 bytes (its length: the
  // bounds check returns zeros, no memory access; a real slot's load ends
  // inside its packet), so no load sits in a branch and the wait counts stay
  // exact (branches made the compiler drain vmcnt before every load).  A
  // chunk of PB slots reads ONE table (slots base .. base + 63; slots at or
  // past lim none), this wave's PW of them (slot s + pt + NP u).  The first
  // PB slots (every group of up to 12 full-size packets) with the loads
  // issued before any use.
  auto chunk = [&](uint32_t s, uint32_t base, uint32_t lim, uint32_t lenT, uint32_t olT, uint32_t ohT,
                   auto first) __attribute__((always_inline)) {
    u32x4 v[PW];
    uint32_t li[PW];
#pragma unroll
    for (int u = 0; u < PW; ++u) {
      const uint32_t j = s + pt + (uint32_t)(NP * u);
      const int t = (int)min(j - base, 63u);  // (slots past the table: li = 0)
      li[u] = (uint32_t)__builtin_amdgcn_readlane((int)lenT, t);
      // (the first chunk's slots are below 64, where the table is 0 past ns)
      if constexpr (!decltype(first)::value) li[u] = j < lim ? li[u] : 0u;
      const uint64_t o = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)ohT, t) << 32) |
                         (uint32_t)__builtin_amdgcn_readlane((int)olT, t);
      const __amdgpu_buffer_rsrc_t rs =
          __builtin_amdgcn_make_buffer_rsrc((void*)(a.bytes + o), 0, (int)li[u], 0x00020000);
      const uint32_t w = j >= kr ? w1 : w0;
      v[u] = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)min(w, li[u] - 16u), 0, 2);  // nt
      // the first chunk in source order: each slot's descriptor right before
      // its load (hoisting them all holds 4 SGPRs a slot: spills) and every
      // load before any use (the scheduler otherwise interleaves the uses and
      // waits on the first loads before issuing the last)
      if constexpr (decltype(first)::value) __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int u = 0; u < PW; ++u) {
      const bool second = s + pt + (uint32_t)(NP * u) >= kr;
      const uint32_t w = second ? w1 : w0;
      const uint32_t keep = w < li[u] ? 0xFFFFFFFFu : 0u;
      const uint32_t sh = w + 16u > li[u] ? min(w + 16u - li[u], 15u) : 0u;
      const u32x4 x = shr_bytes_bf(v[u], sh) & keep;
      const u32x4 zero = {0u, 0u, 0u, 0u};
      acc0 ^= second ? zero : x;
      acc1 ^= second ? x : zero;
    }
  };
  const uint32_t limA = min(ns, 64u);
  chunk(0u, 0u, limA, lenA, olA, ohA, std::true_type{});
  for (uint32_t s = PB; s < limA; s += PB) chunk(s, 0u, limA, lenA, olA, ohA, std::false_type{});
  for (uint32_t s = 64u; s < ns; s += PB) chunk(s, 64u, ns, lenB, olB, ohB, std::false_type{});
  uint8_t* dst = a.out + dst_off;
  const uint32_t nwin = (plen + 15u) >> 4;
  if constexpr (NP > 1) {
    red0[pt * 64u + lane] = acc0;
    red1[pt * 64u + lane] = acc1;
    return WinOut{dst, w0, w1, nwin, true};
  }
  if (lane < nwin) st16t<true>(dst + w0, acc0);
  if (lane + 64u < nwin) st16t<true>(dst + w1, acc1);
  return WinOut{nullptr, 0u, 0u, 0u, false};
}

// (one workgroup per 4 groups of a small batch: occupancy is no object; the
// default 4-waves-per-SIMD target left the recover body 128 VGPRs and spilled)
template <bool RECOVER>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(1, 2))) void ragged_window_kernel(
    RaggedArgs a) {
  __shared__ uint32_t s_par[kFlatWaves][4 * kParWin];
  __shared__ uint64_t s_head[kFlatWaves][kParWin];
  __shared__ u32x4 s_meta[kFlatWaves][64];
  const uint32_t lane = lane_id();
  const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t g = (uint64_t)blockIdx.x * kFlatWaves + wv;
  if (g < a.n_groups)
    window_group<RECOVER, kWindowPB>(a, g, lane, s_par[wv], s_head[wv], s_meta[wv]);
  ragged_signal_done(a);
}

// The small-batch service worker (qfec_internal.h SvcJob / SvcShared /
// SvcDev): kSvcWgs workgroups of kSvcWaves waves, resident while batches keep
// coming.  The leader's thread 0 polls the host-mapped pub_end and hands the
// turn's end to the followers through device memory; for every published job
// each workgroup copies the job's ring entry -- its header AND its index
// tables, which the host writes inline -- into LDS in one PCIe round trip,
// and each group is then taken by one wave (window_group, as the small-batch
// kernel) with its tables read from LDS: a group costs one dependent PCIe
// round trip (its payload bytes) instead of three (group scalars -> packet
// table -> bytes, round 4).  A job of at most kSvcWaves groups is the
// leader's alone; a larger one is spread over all kSvcWgs x kSvcWaves waves
// (one round of groups for up to 64), each workgroup making its outputs
// visible system-wide before it adds itself to the entry's done counter, and
// the last one stores the token.  Host memory is read after a system-scope
// acquire following each poll (a resident kernel gets no cache invalidation
// from a dispatch).  Exit: idle_ticks without work, or quit (the leader
// decides; the followers leave on its word).  All control stores are vector
// stores.
constexpr int kSvcWaves = 8;
// the leader's poll reads the next job's head with pub_end for this long after
// its last job (100-MHz ticks: 50 us, half the idle time), then pub_end alone
// 
constexpr uint64_t kSvcQuietTicks = 5000;
// Load slots per trip of a group's bytes.  A one-group job (all eight waves,
// three slots each): 24 = every window of a group of up to 12 packets longer
// than 1024 B in ONE PCIe round trip.  A job of several groups (a wave per
// group): 20 = the 10 x 1350 B group (kDefaultMaxPacketsPerFecGroup) in one
// trip (16 made it two; 24 beside the one-group form spilled at 2 waves/SIMD)
constexpr int kSvcPB = 24;
constexpr int kSvcPBw = 20;

__device__ __forceinline__ uint64_t svc_load64(const uint64_t* p) {
  return __hip_atomic_load(p, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ uint32_t svc_load32(const uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// The ring entry's first `bytes` bytes (a multiple of 16) into LDS, every
// thread 16 B per pass (the tables follow the header: one round trip).
__device__ __forceinline__ void svc_copy_entry(const SvcJob* e, uint8_t* dst, uint32_t from,
                                               uint32_t bytes, uint32_t tid) {
  const uint8_t* src = reinterpret_cast<const uint8_t*>(e);
  for (uint32_t o = from + 16u * tid; o < bytes; o += 16u * 64u * kSvcWaves)
    *reinterpret_cast<u32x4*>(dst + o) = ld16(src + o);
}

__global__ __launch_bounds__(64 * kSvcWaves) void ragged_service_kernel(
    SvcShared* sh, SvcDev* dv, const SvcJob* ring, uint32_t* flags, uint64_t idle_ticks,
    uint32_t epoch) {
  __shared__ uint32_t s_par[kSvcWaves][4 * kParWin];
  __shared__ uint64_t s_head[kSvcWaves][kParWin];
  __shared__ u32x4 s_meta[kSvcWaves][64];
  __shared__ u32x4 s_red[2][kSvcWaves * 64];  // a one-group job's partial windows
  __shared__ __attribute__((aligned(16))) uint8_t s_ent[sizeof(SvcJob)];
  __shared__ uint64_t s_from, s_to;
  // the leader: split jobs it has announced; a follower: the next announcement it takes
  __shared__ uint64_t s_split;
  __shared__ uint32_t s_job, s_exit, s_stamp;
  // the job whose entry size is known (s_need bytes; the leader: s_have of
  // them already in LDS from its poll), else no job
  __shared__ uint32_t s_entjob, s_have, s_need;
  static_assert(sizeof(SvcJob) % 16u == 0u, "entry copied in 16-B pieces");
  static_assert(kSvcRing > 3u, "announcement ring: more entries than outstanding jobs");
  constexpr uint32_t kHead = (uint32_t)offsetof(SvcJob, tab);
  constexpr uint32_t kFirst = 4096u;  // first pass: the header and the first tables
  const uint32_t tid = threadIdx.x, lane = lane_id();
  const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane(tid >> 6);
  const uint32_t wg = blockIdx.x;
  const bool lead = wg == 0u;
  const SvcJob& J = *reinterpret_cast<const SvcJob*>(s_ent);
  __shared__ uint64_t st[6];  // measurement hook (sh->stamp_on): the leader's stamps of a job (thread 0; LDS, not 12 VGPRs live through the job)

  // This workgroup's share of job jj, whose entry is in LDS: a split job's
  // group g on wave g / kSvcWgs of workgroup g % kSvcWgs (a 9..64-group job is
  // one round, spread over the workgroups), a smaller one the leader's alone.
  // Then its outputs visible, its count (split) and the token from the last.
  auto run_job = [&](uint32_t jj, bool split) __attribute__((always_inline)) {
    if (tid == 0) st[1] = wall_clock64();
    // the job's tables live in LDS (generic pointers: flat loads)
    RaggedArgs a = J.a;
    a.pkt_off = reinterpret_cast<const uint64_t*>(J.tab + J.t_off);
    a.pkt_len = reinterpret_cast<const uint16_t*>(J.tab + J.t_len);
    a.grp_ptr = reinterpret_cast<const uint32_t*>(J.tab + J.t_ptr);
    a.parity_off = reinterpret_cast<const uint64_t*>(J.tab + J.t_poff);
    if (J.recover) {
      a.parity_len = reinterpret_cast<const uint16_t*>(J.tab + J.t_plen);
      a.missing = J.tab + J.t_miss;
      a.out_off = reinterpret_cast<const uint64_t*>(J.tab + J.t_ooff);
    }
    const uint64_t n = J.a.n_groups;
    const uint64_t step = split ? (uint64_t)kSvcWaves * kSvcWgs : (uint64_t)kSvcWaves;
    if (n <= 2u) {
      // one or two groups: each on 8 / n waves of the leader -- its slots
      // dealt round its waves (a
      // wave issues an instruction every few cycles: one group alone on one
      // wave took ~7.5 us from its entry to its stores, on all 8 waves 3.9,
      // profiles/round6/svc_trace_n_r6t.txt), each group's partial windows
      // XORed out of LDS by two of its waves
      const uint32_t NPn = n == 1u ? (uint32_t)kSvcWaves : 4u;
      const uint32_t q = wv / NPn, part = wv - q * NPn;
      u32x4* const r0 = s_red[0] + q * NPn * 64u;
      u32x4* const r1 = s_red[1] + q * NPn * 64u;
      WinOut o{nullptr, 0u, 0u, 0u, false};
      if (q < n) {
        if (n == 1u)
          o = J.recover ? window_group<true, kSvcPB, kSvcWaves>(
                              a, 0, lane, s_par[wv], s_head[wv], s_meta[wv], part, r0, r1)
                        : window_group<false, kSvcPB, kSvcWaves>(
                              a, 0, lane, s_par[wv], s_head[wv], s_meta[wv], part, r0, r1);
        else
          o = J.recover ? window_group<true, kSvcPB, 4>(
                              a, q, lane, s_par[wv], s_head[wv], s_meta[wv], part, r0, r1)
                        : window_group<false, kSvcPB, 4>(
                              a, q, lane, s_par[wv], s_head[wv], s_meta[wv], part, r0, r1);
      }
      __syncthreads();
      if (q < n && o.red && part < 2u) {
        const u32x4* r = part == 0u ? r0 : r1;
        u32x4 x = r[lane];
        for (uint32_t p = 1; p < NPn; ++p) x ^= r[p * 64u + lane];
        if (lane + 64u * part < o.nwin) st16t<true>(o.dst + (part == 0u ? o.w0 : o.w1), x);
      }
      if (tid == 0) st[2] = wall_clock64();
    } else {
      for (uint64_t g = split ? (uint64_t)wv * kSvcWgs + wg : wv; g < n; g += step) {
        if (J.recover)
          window_group<true, kSvcPBw>(a, g, lane, s_par[wv], s_head[wv], s_meta[wv]);
        else
          window_group<false, kSvcPBw>(a, g, lane, s_par[wv], s_head[wv], s_meta[wv]);
        if (tid == 0 && g == 0) st[2] = wall_clock64();
      }
    }
    // every wave's output stores acknowledged, then ONE system-scope
    // release (thread 0's: its L2 write-back covers the workgroup) before
    // the count / token -- not one per thread
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
      st[3] = wall_clock64();
      __threadfence_system();  // this workgroup's outputs visible before its count
      st[4] = wall_clock64();
      bool last = true;
      if (split) {
        // every workgroup takes every split job (announced to the followers,
        // below), so the count reaches kSvcWgs exactly once per job; the
        // last resets it for the entry's next split job (which the host
        // publishes only after this job's token, stored after the reset)
        last = __hip_atomic_fetch_add(&dv->done[jj % kSvcRing], 1u, __ATOMIC_ACQ_REL,
                                      __HIP_MEMORY_SCOPE_SYSTEM) +
                   1u ==
               kSvcWgs;
        if (last)
          __hip_atomic_store(&dv->done[jj % kSvcRing], 0u, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
      }
      if (last)
        __hip_atomic_store(flags + J.flag_slot, J.token, __ATOMIC_RELEASE,
                           __HIP_MEMORY_SCOPE_SYSTEM);
      if (s_stamp) {
        st[5] = wall_clock64();
        if (lead)
          for (int q = 0; q < 6; ++q)
            __hip_atomic_store(&sh->stamps[q], st[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        const uint64_t row[4] = {st[1], st[3], st[4], st[5]};
        for (int q = 0; q < 4; ++q)
          __hip_atomic_store(&sh->wg_stamps[wg][q], row[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        if (last) {
          __hip_atomic_store(&sh->stamps[6], st[5], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
          __hip_atomic_store(&sh->stamps[7], (uint64_t)wg, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
      }
    }
  };

  // One loop for both roles and one run_job site, round 5's loop nest (a
  // second site, or one job per turn of the outer loop, spilled 72-168 B of
  // scratch at 256 VGPRs): each turn the leader polls and walks the jobs
  // published so far; a follower takes one announcement of a split job.
  // (round 5's followers walked the ring themselves from the
  // host's `consumed`, read at their own start; a follower dispatched late
  // -- the CUs held by another kernel -- started past a split job the leader
  // had already counted and never did its share, so that job's token never
  // came.  Now a follower starts at its own count of announcements taken,
  // kept in device memory across launches, and reads only the entries of
  // split jobs, whose tokens wait for it.)
  if (tid == 0) {
    if (lead) {
      // where the previous worker stopped (stable: it has left): jobs are
      // finished whole and in order, so the next job's number is the count
      s_from = svc_load64(&sh->consumed);
      s_to = s_from;
      s_job = (uint32_t)svc_load64(&sh->jobs);
      s_stamp = svc_load32(&sh->stamp_on);
      s_split = __hip_atomic_load(&dv->nsplit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      // running: a worker queued behind one that cleared `alive` on its way
      // out says so itself (the host then stops it before a phased
      // launch)
      __hip_atomic_store(&sh->alive, 1u, __ATOMIC_SEQ_CST, __HIP_MEMORY_SCOPE_SYSTEM);
    } else {
      // test hook: a follower dispatched late (the hold released)
      while (svc_load32(&sh->hold) != 0u) __builtin_amdgcn_s_sleep(8);
      s_split = __hip_atomic_load(&dv->taken[wg], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      s_stamp = svc_load32(&sh->stamp_on);  // (its own row of wg_stamps)
    }
  }
  __syncthreads();
  // the leader announces split job jj (entry bytes `need`) to the followers (thread 0)
  auto announce = [&](uint32_t jj, uint32_t need) {
    const uint64_t i = s_split;
    __hip_atomic_store(&dv->split[i % kSvcRing], ((uint64_t)jj << 32) | (need >> 4),
                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&dv->nsplit, i + 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    s_split = i + 1u;
  };
  bool miss = false;
  for (;;) {
    // tid and lane redefined (opaquely) every turn of the worker's loop:
    // nothing derived from them is hoisted out of it -- shuffle addresses,
    // head-hash multipliers, slot masks were, live through the whole job
    // body, and spilled to scratch at 256 VGPRs
    if (lead) {
      if (wv == 0u) {
        // Wave 0 polls.  Every look
        // reads pub_end AND the next job's first kSvcHead bytes (16 per lane,
        // relaxed system-scope loads, all in flight together: one PCIe round
        // trip); when the look that sees the job holds it whole -- its head
        // hash, seq and start agree -- the entry copy below is skipped (round
        // 5: one round trip less per job).
        const uint64_t from = s_from;
        const uint32_t job0 = s_job;
        const uint32_t lane2 = 2u * lane;
        const uint64_t* hp = reinterpret_cast<const uint64_t*>(ring + (job0 % kSvcRing)) + lane2;
        uint64_t h0 = 0, h1 = 0;
        uint32_t rot = 0;  // the rotate word, read with every look (same round trip)
        uint32_t wm = 0;   // the host's warm count, likewise
        auto look = [&]() -> uint64_t {
          const uint64_t t = __hip_atomic_load(&sh->pub_end, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
          rot = __hip_atomic_load(&sh->rotate, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
          wm = __hip_atomic_load(&sh->warm, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
          h0 = __hip_atomic_load(hp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
          h1 = __hip_atomic_load(hp + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
          return t;
        };
        // rotated out (wrap-safe epoch compare): leave between turns, the
        // published jobs to the successor queued behind (it starts at consumed)
        auto rotated = [&]() { return (int32_t)(rot - epoch) >= 0; };
        uint64_t to = look();
        uint32_t ex = 0;
        uint64_t t0 = wall_clock64();
        uint32_t warm_seen = wm;
        while (to == from) {
          if (svc_load32(&sh->quit) != 0u) {
            ex = 1;
            break;
          }
          if (wall_clock64() - t0 > idle_ticks) {
            // leaving: say so, then look once more (the host publishes, then
            // reads alive: one of the two sees the other's store)
            __hip_atomic_store(&sh->alive, 0u, __ATOMIC_SEQ_CST, __HIP_MEMORY_SCOPE_SYSTEM);
            __atomic_thread_fence(__ATOMIC_SEQ_CST);
            to = look();
            if (to == from) {
              ex = 1;
              break;
            }
            __hip_atomic_store(&sh->alive, 1u, __ATOMIC_SEQ_CST, __HIP_MEMORY_SCOPE_SYSTEM);
            break;
          }
          if (wall_clock64() - t0 > kSvcQuietTicks) {
            // a quiet stretch: pub_end alone, less often (one 8-B
            // read instead of 1 KiB over the link every look); a job seen
            // this way costs one more round trip for its head
            __builtin_amdgcn_s_sleep(16);
            to = __hip_atomic_load(&sh->pub_end, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            wm = __hip_atomic_load(&sh->warm, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            if (to != from) to = look();
          } else {
            __builtin_amdgcn_s_sleep(2);
            to = look();
          }
          // a warm call (a batch is coming this loop turn): the idle time
          // restarts, so a turn whose batch takes most of it to assemble
          // still finds the worker resident (round 6)
          if (wm != warm_seen) {
            warm_seen = wm;
            t0 = wall_clock64();
          }
        }
        if (!ex && rotated()) ex = 1;
        // the head found whole (its hash, seq and start agree): the entry's
        // size is known -- a small job is all in LDS already, a larger one's
        // header is, and the rest is copied in one pass
        uint32_t have = 0, need = 0;
        if (!ex) {
          uint64_t* sw = reinterpret_cast<uint64_t*>(s_ent);
          sw[lane2] = h0;
          sw[lane2 + 1u] = h1;
          wave_lds_order();
          const uint32_t tbb = J.tab_bytes;
          const uint32_t full = min((kHead + min(tbb, kSvcTab) + 15u) & ~15u, (uint32_t)sizeof(SvcJob));
          const uint32_t nb = min(full, kSvcHead);
          uint64_t part = 0;
          if (lane2 < nb / 8u && lane2 != kSvcHeadSumWord) part += svc_head_word(h0, lane2);
          if (lane2 + 1u < nb / 8u && lane2 + 1u != kSvcHeadSumWord)
            part += svc_head_word(h1, lane2 + 1u);
#pragma unroll
          for (uint32_t d = 32; d > 0; d >>= 1)
            part += ((uint64_t)lane_read((uint32_t)(part >> 32), lane ^ d) << 32) |
                    lane_read((uint32_t)part, lane ^ d);
          const bool whole = (part | 1ull) == J.head_sum && J.seq == job0 && J.start == from &&
                             tbb <= kSvcTab;
          have = whole ? nb : 0u;
          need = whole ? full : 0u;
        }
        if (lane == 0u) {
          st[0] = wall_clock64();
          s_to = to;
          s_exit = ex;
          s_entjob = need != 0u ? job0 : 0xFFFFFFFFu;
          s_have = have;
          s_need = need;
        }
      }
    } else if (tid == 0) {
      // follower: the next announcement, or the leader's exit
      const uint64_t mine = s_split;
      uint64_t ann = 0;
      uint32_t ex = 0;
      for (;;) {
        // the exit word first: the leader stores it after its last
        // announcement, so an exit seen here means nsplit is final
        const uint32_t e = __hip_atomic_load(&dv->exit, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
        if (__hip_atomic_load(&dv->nsplit, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) > mine) {
          ann = __hip_atomic_load(&dv->split[mine % kSvcRing], __ATOMIC_RELAXED,
                                  __HIP_MEMORY_SCOPE_AGENT);
          break;
        }
        if (e == epoch) {
          ex = 1;
          break;
        }
        __builtin_amdgcn_s_sleep(1);
      }
      s_exit = ex;
      s_entjob = (uint32_t)(ann >> 32);
      s_have = 0u;
      s_need = (uint32_t)(ann & 0xFFFFu) << 4;
    }
    __syncthreads();
    if (s_exit) break;
    // every thread: drop cached copies of host memory (ring entries, payloads)
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    // the leader: the published jobs, in order (pub_end moves by whole
    // jobs); a follower: the one announced
    const uint64_t to = s_to;
    uint64_t gi = s_from;
    uint32_t jj = lead ? s_job : s_entjob;
    bool once = true;
    while (lead ? gi < to : once) {
      once = false;
      const SvcJob* e = ring + (jj % kSvcRing);
      // a job of known size in one pass (the leader's poll holds its header
      // and maybe all of it), else the header and first tables, then the rest
      const uint32_t have = jj == s_entjob ? s_have : 0u;
      const uint32_t need = jj == s_entjob ? s_need : 0u;
      // a split job whose header the poll holds: announced before the copy,
      // so the followers' entry copies overlap the leader's
      if (lead && need != 0u && tid == 0 && J.a.n_groups > (uint64_t)kSvcWaves) announce(jj, need);
      if (need == 0u)
        svc_copy_entry(e, s_ent, 0u, min(kFirst, (uint32_t)sizeof(SvcJob)), tid);
      else if (have < need)
        svc_copy_entry(e, s_ent, have, min(need, (uint32_t)sizeof(SvcJob)), tid);
      __syncthreads();
      if (lead && (J.seq != jj || gi != J.start || J.tab_bytes > kSvcTab)) {
        // a malformed ring: nothing of this turn is done
        // (and no announcement of it)
        miss = true;
        break;
      }
      const uint64_t n = J.a.n_groups;
      const bool split = n > (uint64_t)kSvcWaves;
      if (lead && need == 0u) {
        const uint32_t full = (kHead + J.tab_bytes + 15u) & ~15u;
        if (split && tid == 0) announce(jj, full);
        if (full > kFirst) {  // a large job's tables: a second pass
          svc_copy_entry(e, s_ent, kFirst, full, tid);
          __syncthreads();
        }
      }
      // (a follower's entry cannot be wrong while the host keeps its ring:
      // the entry of a split job is reused only after its token, which waits
      // for this workgroup)
      const bool ok = lead || (J.seq == jj && split && J.tab_bytes <= kSvcTab &&
                               kHead + J.tab_bytes <= need);
      if (ok) run_job(jj, split);
      // no share, so no token: the host's wait sees the fault once the
      // worker has left, and fails the job instead of reporting stale output
      if (!ok && tid == 0) __hip_atomic_store(&sh->fault, 1u, __ATOMIC_SEQ_CST, __HIP_MEMORY_SCOPE_SYSTEM);
      gi = J.start + n;
      ++jj;
      __syncthreads();  // s_ent is the next job's
    }
    if (miss) break;
    if (tid == 0) {
      if (lead) {
        s_job = jj;
        s_from = to;
        __hip_atomic_store(&sh->consumed, to, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(&sh->jobs, (uint64_t)jj, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
      } else {
        s_split = s_split + 1u;
      }
    }
    __syncthreads();
  }
  if (tid == 0) {
    if (lead) {
      // latch a malformed ring's fault and leave WITHOUT the job's token --
      // the host's wait sees the stream drained and the fault word and fails
      // the job instead of reporting stale output as finished
      if (miss) __hip_atomic_store(&sh->fault, 1u, __ATOMIC_SEQ_CST, __HIP_MEMORY_SCOPE_SYSTEM);
      // the followers leave once they have taken every announcement (this
      // store is after the last one: release)
      __hip_atomic_store(&dv->exit, epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    } else {
      __hip_atomic_store(&dv->taken[wg], s_split, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  // (no store to `alive` here: an idle exit cleared it before its last look,
  // and a late store could clobber the 1 the host wrote for a worker it has
  // already queued behind this one; stop_service clears it after a quit)
}

// ---------------------------------------------------------------------------
// out ^= in (XorBuffers).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void xor_into_kernel(const uint8_t* in, uint64_t n,
                                                          uint8_t* out) {
  const uint64_t nwin = n / 16u;
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t w = (uint64_t)blockIdx.x * kBlock + threadIdx.x; w < nwin; w += stride) {
    st16(out + 16u * w, ld16(out + 16u * w) ^ ld16(in + 16u * w));
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 15u)) {
    const uint64_t j = 16u * nwin + threadIdx.x;
    out[j] ^= in[j];
  }
}

// ---------------------------------------------------------------------------
// Bandwidth probes (bench.py's measured ceilings): streaming
// read (nt 16-B loads, 8 in flight per lane, XOR-folded) and copy (nt load +
// nt store), grid-stride over n bytes (n a multiple of 16).
// ---------------------------------------------------------------------------
template <bool COPY>
__global__ __launch_bounds__(kBlock) void stream_probe_kernel(const uint8_t* src, uint64_t n,
                                                              uint8_t* dst) {
  constexpr uint32_t U = 8;
  const uint64_t nwin = n / 16u;
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  u32x4 acc = {0u, 0u, 0u, 0u};
  uint64_t w = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  for (; w + (U - 1) * stride < nwin; w += U * stride) {
    u32x4 v[U];
#pragma unroll
    for (uint32_t u = 0; u < U; ++u) v[u] = ld16t<true>(src + 16u * (w + u * stride));
#pragma unroll
    for (uint32_t u = 0; u < U; ++u) {
      if constexpr (COPY) st16t<true>(dst + 16u * (w + u * stride), v[u]);
      else acc ^= v[u];
    }
  }
  for (; w < nwin; w += stride) {
    const u32x4 v = ld16t<true>(src + 16u * w);
    if constexpr (COPY) st16t<true>(dst + 16u * w, v);
    else acc ^= v;
  }
  if constexpr (!COPY) {
    if ((acc.x & acc.y & acc.z & acc.w) == 0xFFFFFFFFu) st16(dst, acc);  // keeps the loads
  }
}

// ---------------------------------------------------------------------------
// Synthetic inputs (counter-based splitmix64).
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
  uint64_t z = x + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__device__ __forceinline__ void synth_word(uint8_t* row, uint64_t key, uint32_t w, uint32_t len) {
  const uint64_t v = splitmix64(key ^ (uint64_t)w);
  const uint32_t j = w * 8u;
  if (j + 8u <= len) {
    __builtin_memcpy(row + j, &v, 8);
  } else {
    for (uint32_t b = 0; j + b < len; ++b) row[j + b] = (uint8_t)(v >> (8u * b));
  }
}

// One workgroup per row (blockIdx.x = row within the launch), lanes = words.
__global__ __launch_bounds__(kBlock) void synth_fixed_kernel(uint8_t* rows, uint32_t k,
                                                             uint32_t L, uint64_t row_stride,
                                                             uint64_t group_stride, uint64_t g0,
                                                             uint64_t row0, uint64_t seed) {
  const uint64_t r = row0 + blockIdx.x;
  const uint64_t g = r / k;
  const uint32_t i = (uint32_t)(r - g * k);
  const uint64_t key = seed ^ (((g0 + g) * 256u + i) << 32);
  uint8_t* row = rows + g * group_stride + i * row_stride;
  const uint32_t words = (L + 7u) / 8u;
  for (uint32_t w = threadIdx.x; w < words; w += kBlock) synth_word(row, key, w, L);
}

// One workgroup per group.
__global__ __launch_bounds__(kBlock) void synth_ragged_kernel(uint8_t* bytes,
                                                              const uint64_t* pkt_off,
                                                              const uint16_t* pkt_len,
                                                              const uint32_t* grp_ptr,
                                                              uint64_t g0, uint64_t gbase,
                                                              uint64_t seed) {
  const uint64_t g = gbase + blockIdx.x;
  const uint32_t p0 = grp_ptr[g], p1 = grp_ptr[g + 1];
  for (uint32_t i = 0; i < p1 - p0; ++i) {
    const uint32_t len = pkt_len[p0 + i];
    const uint64_t key = seed ^ (((g0 + g) * 256u + i) << 32);
    uint8_t* row = bytes + pkt_off[p0 + i];
    const uint32_t words = (len + 7u) / 8u;
    for (uint32_t w = threadIdx.x; w < words; w += kBlock) synth_word(row, key, w, len);
  }
}

// Every group size up to 16 is templated (round 5; round 4 had 2, 4, 5, 8,
// 10, 16 and ran the others through the runtime-k bodies).
#define QFEC_K_ALL(X) \
  X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16)

template <bool RECOVER, bool NT, bool SM, bool INPL = false>
hipError_t launch_fixed_k(const FixedArgs& a, uint32_t C, uint32_t gpb, uint64_t blocks,
                          hipStream_t s) {
  switch (a.k) {
#define QFEC_K_CASE(KV)                                                                       \
  case KV:                                                                                     \
    hipLaunchKernelGGL((fixed_xor_kernel<KV, RECOVER, NT, SM, INPL>),                          \
                       dim3((uint32_t)blocks), dim3(kBlock), 0, s, a, C, gpb);                 \
    break;
    QFEC_K_ALL(QFEC_K_CASE)
#undef QFEC_K_CASE
    default:
      hipLaunchKernelGGL((fixed_xor_kernel<0, RECOVER, NT, SM, INPL>),
                         dim3((uint32_t)blocks), dim3(kBlock), 0, s, a, C, gpb);
  }
  return hipGetLastError();
}

// The group sizes with a templated phased body.  Every templated k takes
// kPhRegSteps register-held steps per phase (round 4; round 3 had
// them for k = 10 only; round 5 templates every k up to 16).  Larger k run
// the runtime-k body with the LDS steps alone.
// Round 6: the phased RECOVER of group sizes 17-25 is templated too (its
// register steps, parity rows first and compact received rows, as k <= 16):
// recover 0.709 / 0.731 / 0.759 (runtime body) -> 0.779 / 0.785 / 0.797 at
// k = 17 / 20 / 24, where the templated encode is no faster than the runtime
// body's batches of 16 (k = 20: 0.804 vs 0.809); from k = 26 the templated
// recover spills (528 B of scratch) and loses (0.70-0.71 against the
// runtime body's 0.76-0.77) (profiles/round6/phase_k_table_r6{i,j}.txt).  So
// encode, the in-place form, recover above 25 and the one-pass kernel keep
// the runtime body above 16.
#define QFEC_K_PHASE_RECOVER(X) X(17) X(18) X(19) X(20) X(21) X(22) X(23) X(24) X(25)
__host__ __device__ constexpr bool phase_k_templated(bool recover, uint32_t k) {
  return (k >= 2u && k <= 16u) || (recover && k >= 17u && k <= 25u);
}

// The runtime-k phased body's load batch (k > 16) by operation and group
// size, from the round-6 per-k table (tools/phase_k_table.py, 2^20 groups up
// to k = 32, 2^18 above; batch 16 / 32, fraction of 8 TB/s,
// profiles/round6/phase_k_table_r6b.txt, r6c.txt): encode 16 at every k
// (k = 20: 0.796 / 0.764, k = 255: 0.804 / 0.780); recover 32 up to k = 32
// (k = 20: 0.679 / 0.720), 16 above (k = 64: 0.765 / 0.725).
__host__ __device__ constexpr uint32_t phase_rt_batch(bool recover, uint32_t k) {
  return recover && k <= 32u ? 32u : 16u;
}

// The body one phased launch gets.  The only place that decides it: phase_plan
// sizes the phases by it and launch_phase_k launches it, so the phase count
// cannot be computed for a phase length the launched body does not have.
struct PhaseBody {
  bool templated;      // KC = k; otherwise the runtime-k body, KC = 0
  uint32_t reg_steps;  // RS: kPhRegSteps or 0 (templated k only)
  uint32_t rt_batch;   // RTB: 16 or 32 (runtime k only)
};
PhaseBody phase_body(const FixedArgs& a) {
  const bool inpl = a.inplace_missing != nullptr, recover = a.parity != nullptr && !inpl;
  // (test hook rt_batch: the runtime-k body with that batch wherever k > 16,
  // the A/B of tools/phase_k_table.py)
  if (phase_k_templated(recover, a.k) && !(a.rt_batch != 0u && a.k > 16u))
    // (test hook no_regsteps: the LDS steps alone; not for the in-place form)
    return {true, a.no_regsteps != 0u && !inpl ? 0u : (uint32_t)kPhRegSteps, 32u};
  return {false, 0u, (a.rt_batch ? a.rt_batch : phase_rt_batch(recover, a.k)) == 16u ? 16u : 32u};
}

template <int KC, bool RECOVER, int RS, bool INPL, int RTB>
hipError_t launch_phase_body(const FixedArgs& a, uint32_t C, uint32_t gpb, uint32_t grid,
                             uint32_t nphase, hipStream_t s) {
  hipLaunchKernelGGL((phase_xor_kernel<KC, RECOVER, RS, INPL, RTB>), dim3(grid), dim3(kBlock), 0, s,
                     a, C, gpb, nphase);
  return hipGetLastError();
}

template <bool RECOVER, bool INPL = false>
hipError_t launch_phase_k(const FixedArgs& a, PhaseBody b, uint32_t C, uint32_t gpb, uint32_t grid,
                          uint32_t nphase, hipStream_t s) {
#define QFEC_PHASE(KC_, RS_, INPL_, RTB_) \
  launch_phase_body<KC_, RECOVER, RS_, INPL_, RTB_>(a, C, gpb, grid, nphase, s)
  if (!b.templated)
    return b.rt_batch == 16u ? QFEC_PHASE(0, 0, INPL, 16) : QFEC_PHASE(0, 0, INPL, 32);
  // (the in-place form has no body without register steps)
  if (INPL && b.reg_steps == 0u) return hipErrorInvalidValue;
  switch (a.k) {
#define QFEC_K_CASE(KV)                                                                          \
  case KV:                                                                                       \
    if constexpr (phase_k_templated(RECOVER, KV))                                                \
      return b.reg_steps ? QFEC_PHASE(KV, kPhRegSteps, INPL, 32) : QFEC_PHASE(KV, 0, false, 32); \
    break;
    QFEC_K_ALL(QFEC_K_CASE)
    QFEC_K_PHASE_RECOVER(QFEC_K_CASE)
#undef QFEC_K_CASE
  }
#undef QFEC_PHASE
  return hipErrorInvalidValue;  // no such instantiation: phase_body and the lists above disagree
}

// The phased kernel for a batch of at least kPhMinPhases phases (about 184K
// groups at L = 1350 on 256 CUs): the two meetings per phase cost ~2-3 us
// each, and below that the one-pass kernel's placement luck matters less
// than they do.  Measured crossover (tools/phase_band.py,
// profiles/round3/phase/phase_band_r3d.txt): one-pass 0.77 vs phased 0.73 of
// 8 TB/s at 131K groups, 0.75 vs 0.76 at 196K, 0.74 vs 0.78 at 262K.
// Returns false when it does not apply.
constexpr uint32_t kPhMinPhases = 6;

// The CU count comes cached from the context (FixedArgs::ncu); the test hook
// phase_extra (tests/test_hip_phase.py) adds workgroups beyond one per CU,
// which cannot all be resident, so the first meeting times out — the abandon
// path.
// Group sizes the phased kernel loses at (round 4, tools/phase_k_table.py,
// profiles/round4/phase_k_table_r4a.txt, 2^20 groups of 1350 B, fraction of
// 8 TB/s phased / one-pass): encode k = 2 0.47 / 0.77, k = 4 0.64 / 0.74,
// k = 5 0.73 / 0.71, k = 8 0.79 / 0.72; recover k = 4 0.54 / 0.72, k = 5
// 0.62 / 0.67, k = 8 0.745 / 0.740, k = 10 0.76 / 0.72 -- a phase of few
// rows per group reads too little between its meetings.  So encode phases
// from k = 5, recover from k = 8.  Round 4 phased only the templated k: the
// runtime-k phased body then loaded the rows past the last batch of 8 one at
// a time (profiles/round4/phase_k_table_nontemplated_r4o.txt: k = 6 0.27 vs
// 0.69 one-pass); round 5 templates every k up to 16 and gives the runtime
// body (k > 16) batches of 16 with a one-batch remainder (xor_rows_rt), so
// the rule is by k alone again (tools/phase_k_table.py); its
// round-5 table moved recover's threshold to k = 7 (phased 0.719 vs one-pass
// 0.697; k = 6 0.684 vs 0.720: profiles/round5/phase_k_table_r5b.txt).  An
// explicit phase_min (test hook) keeps the phase-count rule alone.
constexpr uint32_t kPhMinKEncode = 5, kPhMinKRecover = 7;

bool phase_plan(const FixedArgs& a, uint32_t gpb, uint32_t* grid, uint32_t* nphase) {
  if (a.ncu == 0) return false;
  if (a.phase_min == 0 &&
      a.k < (a.parity != nullptr ? kPhMinKRecover : kPhMinKEncode))
    return false;
  // resident service workers of other contexts hold svc_cus CUs' LDS: the
  // grid leaves them, so every workgroup is resident and the meetings hold
  // (round 6); more than a quarter of the device so held: one-pass
  if (a.svc_cus > a.ncu / 4u) return false;
  // (the test hook phase_extra: that many workgroups beyond one per CU, the
  // other contexts' workers ignored)
  const uint32_t wg =
      a.phase_extra ? a.ncu + std::min<uint32_t>(a.phase_extra, 64u) : a.ncu - a.svc_cus;
  // the threshold counts phases of the LDS steps alone (the measured band);
  // the launch's phases hold the register steps too (k = 10)
  const uint64_t per = (uint64_t)wg * kPhSteps * gpb;
  const uint64_t np = (a.n_groups + per - 1) / per;
  if (np < (a.phase_min ? a.phase_min : kPhMinPhases) || np > 0xFFFFFFFFull) return false;
  const uint64_t per_l = (uint64_t)wg * (kPhSteps + phase_body(a).reg_steps) * gpb;
  *grid = wg;
  *nphase = (uint32_t)((a.n_groups + per_l - 1) / per_l);
  return true;
}

// Steps per phase that spread n_groups evenly over nphase phases (a 393K-group
// batch: 8 phases of 64 steps instead of 7 of 72 and one of 7).
uint32_t phase_steps_for(const FixedArgs& a, uint32_t gpb, uint32_t grid, uint32_t nphase) {
  const uint64_t per_step = (uint64_t)grid * gpb * nphase;
  return (uint32_t)((a.n_groups + per_step - 1) / per_step);
}

// Groups [g, g + at most maxg) of a batch as a launch of their own.
FixedArgs fixed_slice(const FixedArgs& a0, uint64_t g, uint64_t maxg) {
  FixedArgs a = a0;
  a.n_groups = std::min<uint64_t>(maxg, a0.n_groups - g);
  a.rows = a0.rows + g * a0.group_stride;
  if (a0.parity != nullptr) {
    a.parity = a0.parity + g * a0.parity_stride;
    a.missing = a0.missing + g;
  }
  a.out = a0.out + g * a0.out_stride;
  if (a0.inplace_missing) a.inplace_missing = a0.inplace_missing + g;
  return a;
}

}  // namespace

bool fixed_uses_phases(const FixedArgs& a, bool nontemporal, uint32_t* grid) {
  if (!a.phase_sync || !nontemporal || a.L < 16u || a.n_groups == 0) return false;
  uint32_t g = 0, nphase = 0;
  const bool on = phase_plan(a, kBlock / ((a.L + 15u) / 16u), &g, &nphase);
  if (grid) *grid = on ? g : 0u;
  return on;
}

hipError_t launch_fixed(const FixedArgs& a0, bool nontemporal, hipStream_t s) {
  const bool recover = a0.parity != nullptr;
  if (a0.n_groups == 0) return hipSuccess;
  if (a0.L < 16u) {
    const uint64_t maxg = kMaxBlocks256 * kBlock / a0.L;  // one lane per output byte
    for (uint64_t g = 0; g < a0.n_groups; g += maxg) {
      const FixedArgs a = fixed_slice(a0, g, maxg);
      const uint64_t blocks = (a.n_groups * a.L + kBlock - 1) / kBlock;
      if (recover)
        hipLaunchKernelGGL(fixed_small_kernel<true>, dim3((uint32_t)blocks), dim3(kBlock), 0, s, a);
      else
        hipLaunchKernelGGL(fixed_small_kernel<false>, dim3((uint32_t)blocks), dim3(kBlock), 0, s, a);
      hipError_t e = hipGetLastError();
      if (e != hipSuccess) return e;
    }
    return hipSuccess;
  }
  const uint32_t C = (a0.L + 15u) / 16u;  // <= 91 for L <= 1452
  const uint32_t gpb = kBlock / C;         // whole groups per workgroup (>= 2)
  uint32_t grid = 0, nphase = 0;
  if (a0.phase_sync && nontemporal && phase_plan(a0, gpb, &grid, &nphase)) {
    FixedArgs a = a0;
    a.phase_steps = phase_steps_for(a0, gpb, grid, nphase);
    const PhaseBody b = phase_body(a);
    if (a.inplace_missing) return launch_phase_k<false, true>(a, b, C, gpb, grid, nphase, s);
    return recover ? launch_phase_k<true>(a, b, C, gpb, grid, nphase, s)
                   : launch_phase_k<false>(a, b, C, gpb, grid, nphase, s);
  }
  const uint64_t maxg = kMaxBlocks256 * gpb;
  for (uint64_t g = 0; g < a0.n_groups; g += maxg) {
    const FixedArgs a = fixed_slice(a0, g, maxg);
    const uint64_t blocks = (a.n_groups + gpb - 1) / gpb;
    hipError_t e;
    if (a.inplace_missing)
      e = launch_fixed_k<false, true, false, true>(a, C, gpb, blocks, s);
    else if (recover && gpb <= 8u)
      e = nontemporal ? launch_fixed_k<true, true, true>(a, C, gpb, blocks, s)
                      : launch_fixed_k<true, false, true>(a, C, gpb, blocks, s);
    else if (recover)
      e = nontemporal ? launch_fixed_k<true, true, false>(a, C, gpb, blocks, s)
                      : launch_fixed_k<true, false, false>(a, C, gpb, blocks, s);
    else
      e = nontemporal ? launch_fixed_k<false, true, false>(a, C, gpb, blocks, s)
                      : launch_fixed_k<false, false, false>(a, C, gpb, blocks, s);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

namespace {

template <bool NT, bool SM>
hipError_t launch_revive_k(const ReviveArgs& a, uint32_t C, uint32_t gpb, uint32_t grid,
                           hipStream_t s) {
  switch (a.k) {
#define QFEC_K_CASE(KV)                                                                      \
  case KV:                                                                                    \
    hipLaunchKernelGGL((revive_xor_kernel<KV, NT, SM>), dim3(grid), dim3(kBlock), 0, s, a,    \
                       a.work, a.totals, C, gpb);                                             \
    break;
    QFEC_K_ALL(QFEC_K_CASE)
#undef QFEC_K_CASE
    default:
      hipLaunchKernelGGL((revive_xor_kernel<0, NT, SM>), dim3(grid), dim3(kBlock), 0, s, a,
                         a.work, a.totals, C, gpb);
  }
  return hipGetLastError();
}

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
hipError_t launch_revive_passes(const Args& a, hipStream_t s) {
  hipError_t e = launch_pass(hipSuccess, revive_classify_kernel<false, Args>,
                             tile_grid(a.n_groups), kReviveTile, s, a);
  e = launch_pass(e, revive_scan_kernel<Args>, 1, kRvScanBlock, s, a);
  e = launch_pass(e, revive_classify_kernel<true, Args>, tile_grid(a.n_groups), kReviveTile, s, a);
  return e;
}

}  // namespace

hipError_t launch_revive(const ReviveArgs& a, bool nontemporal, hipStream_t s) {
  if (a.n_groups == 0) return hipSuccess;
  hipError_t e = launch_revive_passes(a, s);
  if (e != hipSuccess) return e;
  // revive: the count stays on the device, so the grid is sized by the device
  // (eight workgroups per CU: every wave slot at up to 64 VGPRs) and by the
  // worst case, whichever is smaller; workgroups loop over the list
  const uint64_t resident = (uint64_t)(a.ncu ? a.ncu : 256u) * 8u;
  if (a.L < 16u) {
    const uint64_t blocks = (a.n_groups * a.L + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(revive_small_kernel, dim3((uint32_t)std::min(blocks, resident)),
                       dim3(kBlock), 0, s, a, a.work, a.totals);
    return hipGetLastError();
  }
  const uint32_t C = (a.L + 15u) / 16u;
  const uint32_t gpb = kBlock / C;
  const uint32_t grid = (uint32_t)std::min<uint64_t>((a.n_groups + gpb - 1) / gpb, resident);
  if (gpb <= 8u)
    return nontemporal ? launch_revive_k<true, true>(a, C, gpb, grid, s)
                       : launch_revive_k<false, true>(a, C, gpb, grid, s);
  return nontemporal ? launch_revive_k<true, false>(a, C, gpb, grid, s)
                     : launch_revive_k<false, false>(a, C, gpb, grid, s);
}

constexpr int kRaggedBlockWaves = 4, kRaggedBlockGroups = 8;  // ragged_block_kernel shape

hipError_t launch_revive_ragged(const ReviveRaggedArgs& a, hipStream_t s) {
  if (a.n_groups == 0) return hipSuccess;
  hipError_t e = launch_revive_passes(a, s);
  if (e != hipSuccess) return e;
  // the count stays on the device: as many blocks as the device holds at once
  // (asked of the runtime: with the VGPRs of this build six per CU, and a grid
  // of eight per CU left a quarter of the blocks to run after the others, at a
  // third of the device: 1.35x the dense recover with every group revived) or
  // the worst case, whichever is smaller; the blocks loop over the list steps
  static const int per_cu = [] {
    int nb = 0;
    const hipError_t q = hipOccupancyMaxActiveBlocksPerMultiprocessor(
        &nb, revive_ragged_kernel<kRaggedBlockWaves, kRaggedBlockGroups>, 64 * kRaggedBlockWaves,
        0);
    return q == hipSuccess && nb > 0 ? nb : 4;
  }();
  const uint64_t resident = (uint64_t)(a.ncu ? a.ncu : 256u) * (uint64_t)per_cu;
  const uint64_t steps = (a.n_groups + kRaggedBlockGroups - 1) / kRaggedBlockGroups;
  hipLaunchKernelGGL((revive_ragged_kernel<kRaggedBlockWaves, kRaggedBlockGroups>),
                     dim3((uint32_t)std::min(steps, resident)), dim3(64 * kRaggedBlockWaves), 0, s,
                     a, a.work, a.totals);
  return hipGetLastError();
}

// The gather's grid: its waves loop over the rows, eight workgroups per CU
// (every wave slot) or one wave per row, whichever is smaller.
static uint32_t close_gather_grid(const CloseArgs& a) {
  const uint64_t blocks = (a.n_groups + kBlock / 64 - 1) / (kBlock / 64);
  return (uint32_t)std::min<uint64_t>(blocks, (uint64_t)(a.ncu ? a.ncu : 256u) * 8u);
}

hipError_t launch_close_emit(const CloseArgs& a, hipStream_t s) {
  if (a.n_groups == 0) return hipSuccess;
  hipLaunchKernelGGL(close_gather_kernel<false>, dim3(close_gather_grid(a)), dim3(kBlock), 0, s, a,
                     nullptr, nullptr);
  return hipGetLastError();
}

// Both closing revives: the three passes for Args, then the gather over the
// work list.  The gather is one kernel for both: an entry carries its group and
// length, and what it reads besides (acc, acc_stride, slot, out, out_off) is
// CloseArgs's part of either struct.
template <typename Args>
static hipError_t launch_close_revive_as(const Args& a, hipStream_t s) {
  if (a.n_groups == 0) return hipSuccess;
  hipError_t e = launch_revive_passes(a, s);
  if (e != hipSuccess) return e;
  if (!a.out) return hipSuccess;  // the revived packets are the rows
  // the count stays on the device: the grid is sized by the worst case
  const CloseArgs& c = a;
  hipLaunchKernelGGL(close_gather_kernel<true>, dim3(close_gather_grid(c)), dim3(kBlock), 0, s, c,
                     a.work, a.totals);
  return hipGetLastError();
}

hipError_t launch_close_revive(const CloseArgs& a, hipStream_t s) {
  return launch_close_revive_as(a, s);
}

hipError_t launch_tracked_revive(const TrackedCloseArgs& a, hipStream_t s) {
  return launch_close_revive_as(a, s);
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

hipError_t launch_accumulate_ragged(const AccumulateRaggedArgs& a0, hipStream_t s) {
  if (a0.n_groups == 0) return hipSuccess;
  const uint64_t gpb = kRaggedBlockGroups;
  const uint64_t maxg = kMaxBlocks256 * gpb;
  for (uint64_t g = 0; g < a0.n_groups; g += maxg) {
    AccumulateRaggedArgs a = a0;
    a.n_groups = std::min<uint64_t>(maxg, a0.n_groups - g);
    a.grp_ptr = a0.grp_ptr + g;
    if (a0.slot) a.slot = a0.slot + g;
    else a.slot_base = (uint32_t)g;
    const uint64_t blocks = (a.n_groups + gpb - 1) / gpb;
    hipLaunchKernelGGL((accumulate_ragged_kernel<kRaggedBlockWaves, kRaggedBlockGroups>),
                       dim3((uint32_t)blocks), dim3(64 * kRaggedBlockWaves), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_ragged(const RaggedArgs& a0, bool recover, hipStream_t s, bool small_groups) {
  if (a0.n_groups == 0) return hipSuccess;
  const uint64_t gpb = kRaggedBlockGroups;
  const uint64_t maxg = kMaxBlocks256 * gpb;
  for (uint64_t g = 0; g < a0.n_groups; g += maxg) {
    RaggedArgs a = a0;
    a.n_groups = std::min<uint64_t>(maxg, a0.n_groups - g);
    a.grp_ptr = a0.grp_ptr + g;
    if (recover) {
      a.parity_len = a0.parity_len + g;
      a.missing = a0.missing + g;
      a.out_off = a0.out_off + g;
      a.parity_off = a0.parity_off + g;
    } else {
      a.parity_off = a0.parity_off + g;
      a.parity_len_out = a0.parity_len_out + g;
    }
    const uint64_t blocks = (a.n_groups + gpb - 1) / gpb;
    // (two groups per wave x 4 waves: the block kernel's 8 groups per block)
    static_assert(2 * kFlatWaves == kRaggedBlockGroups, "one grid for both kernels");
    static_assert(kPairGroups * kPairWaves == kRaggedBlockGroups && 64 * kPairWaves == kBlock,
                  "the pair kernel's block");
    if (small_groups) {
      if (recover)
        hipLaunchKernelGGL((ragged_multi_kernel<true>), dim3((uint32_t)blocks),
                           dim3(kBlock), 0, s, a);
      else
        hipLaunchKernelGGL((ragged_multi_kernel<false>), dim3((uint32_t)blocks),
                           dim3(kBlock), 0, s, a);
    } else if (recover) {
      hipLaunchKernelGGL((ragged_block_kernel<true, kRaggedBlockWaves, kRaggedBlockGroups>),
                         dim3((uint32_t)blocks), dim3(64 * kRaggedBlockWaves), 0, s, a);
    } else {
      hipLaunchKernelGGL((ragged_block_kernel<false, kRaggedBlockWaves, kRaggedBlockGroups>),
                         dim3((uint32_t)blocks), dim3(64 * kRaggedBlockWaves), 0, s, a);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_ragged_latency(const RaggedArgs& a, bool recover, hipStream_t s) {
  if (a.n_groups == 0) return hipSuccess;
  if (a.n_groups > kMaxBlocks256) return hipErrorInvalidValue;  // small batches only
  const uint64_t blocks = (a.n_groups + kFlatWaves - 1) / kFlatWaves;
  // all of a group's loads in flight at once: kWindowPB = 16 load slots per
  // lane cover up to 16 received packets (+ their second windows) in one round
  // trip
  if (recover)
    hipLaunchKernelGGL((ragged_window_kernel<true>), dim3((uint32_t)blocks),
                       dim3(kBlock), 0, s, a);
  else
    hipLaunchKernelGGL((ragged_window_kernel<false>), dim3((uint32_t)blocks),
                       dim3(kBlock), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_ragged_service(SvcShared* sh, SvcDev* dv, const SvcJob* ring, uint32_t* flags,
                                 uint64_t idle_ticks, uint32_t epoch, hipStream_t s) {
  hipLaunchKernelGGL(ragged_service_kernel, dim3(kSvcWgs), dim3(64 * kSvcWaves), 0, s, sh, dv,
                     ring, flags, idle_ticks, epoch);
  return hipGetLastError();
}

hipError_t launch_xor_into(const uint8_t* in, uint64_t n, uint8_t* out, hipStream_t s) {
  if (n == 0) return hipSuccess;
  uint64_t blocks = (n / 16u + kBlock - 1) / kBlock;
  if (blocks < 1) blocks = 1;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(xor_into_kernel, dim3((uint32_t)blocks), dim3(kBlock), 0, s, in, n, out);
  return hipGetLastError();
}

hipError_t launch_stream_probe(const uint8_t* src, uint64_t n, uint8_t* dst, bool copy,
                               hipStream_t s) {
  if (n < 16) return hipSuccess;
  const dim3 grid(8192), blk(kBlock);
  if (copy)
    hipLaunchKernelGGL(stream_probe_kernel<true>, grid, blk, 0, s, src, n & ~15ull, dst);
  else
    hipLaunchKernelGGL(stream_probe_kernel<false>, grid, blk, 0, s, src, n & ~15ull, dst);
  return hipGetLastError();
}

hipError_t launch_synth_fixed(uint8_t* rows, uint32_t k, uint32_t L, uint64_t row_stride,
                              uint64_t group_stride, uint64_t g0, uint64_t n, uint64_t seed,
                              hipStream_t s) {
  const uint64_t total_rows = n * k;
  const uint64_t chunk = kMaxBlocks256;  // rows per launch (one workgroup each)
  for (uint64_t r = 0; r < total_rows; r += chunk) {
    const uint64_t cnt = std::min<uint64_t>(chunk, total_rows - r);
    hipLaunchKernelGGL(synth_fixed_kernel, dim3((uint32_t)cnt), dim3(kBlock), 0, s, rows, k, L,
                       row_stride, group_stride, g0, r, seed);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_synth_ragged(uint8_t* bytes, const uint64_t* pkt_off, const uint16_t* pkt_len,
                               const uint32_t* grp_ptr, uint64_t g0, uint64_t n, uint64_t seed,
                               hipStream_t s) {
  const uint64_t chunk = kMaxBlocks256;  // groups per launch (one workgroup each)
  for (uint64_t g = 0; g < n; g += chunk) {
    const uint64_t cnt = std::min<uint64_t>(chunk, n - g);
    hipLaunchKernelGGL(synth_ragged_kernel, dim3((uint32_t)cnt), dim3(kBlock), 0, s, bytes,
                       pkt_off, pkt_len, grp_ptr, g0, g, seed);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace qfec
