// qfec_device.h — the device code that both kernel files use: the turn passes
// (qturn_kernels.hip) and the XOR kernels (qfec_kernels.hip).  Device-only: it
// is included by the two .hip files and by nothing a host compiler reads.
// Every function here is inlined, and into each file's kernels on that file's
// terms: the compiler specialises a helper on the arguments of the callers it
// sees in one file (wave_incl_scan where every caller's lane is tid & 63:
// DESIGN.md §4, "The turn passes in a file of their own").
#pragma once
#include "qfec_internal.h"

namespace qfec {

// The four wave helpers: the first of the workgroup primitives of the turn
// passes, under the contract stated there (qturn_kernels.hip); the ragged
// kernels and the service worker use them too.
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

// The status of a group after the revive's classify pass (qturn_kernels.hip),
// and the index of its count in `totals`, which the revive kernels read.
constexpr uint32_t kGroupComplete = 0, kGroupRevived = 1, kGroupUnrevivable = 2;

// The slot of group g of a closing revive (CloseArgs's rules: qturn_kernels.hip).
__device__ __forceinline__ uint32_t close_slot(const CloseArgs& a, uint64_t g) {
  return a.slot ? a.slot[g] : (uint32_t)g;
}

}  // namespace qfec
