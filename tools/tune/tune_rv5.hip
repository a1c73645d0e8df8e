// tune_rv5.hip — round 6: a persistent, grid-phased form
// of the product's ragged block body for configs[3] (2^20 groups, k 5-15,
// payloads 64-1350 B).
//
// Round 6's 2x2 diagnostic (profiles/round6/tune_rblock_diag_r6e.txt) found
// the one-pass block kernel's time to be its read time plus its write time:
// 1,273 us reading without stores (0.85 of 8 TB/s) + ~300 us of stores =
// 1,582 us; and the read body without its tail logic reads in 1,161 us (0.94)
// but is SLOWER with its stores in (1,696 us) -- the faster reads crowd the
// writes out.  So the lever is the two together: the tail-free read body
// (exact when payloads sit on 16-B boundaries with zero padding, the payload
// arena's layout) AND the writes moved into phases of their own.
//
// Here: P workgroups per CU, each looping over blocks of GPB groups (block b,
// b + grid, ...) with the product's block body (setup, flat windows), its
// accumulators the slots of a ring in LDS.  A finished block's parities stay
// in the ring; every BP blocks the workgroup ARRIVES at the next grid-wide
// meeting without waiting (split-phase: sub-counters + a top counter, as the
// fixed phased kernel's), and at each block boundary it tests the oldest
// meeting it arrived at: once every workgroup has arrived there, it stores
// every parity it holds.  It waits only when the ring is full.  Meetings only
// shape timing (nothing reads what another workgroup wrote); a wait longer
// than 200 us raises an abandon flag that ends all waiting.
// MODE 0: no stores (the read rate of the persistent form); 1: stores right
// after each block (persistent one-pass); 2: phased.
// Every exact variant is byte-compared with the product kernel first.
//
//   tune_rv5 [reps=10] [rounds=5] [palign=16] [slot=1536]
// build: hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/tune/tune_rv5.hip \
//          -o tools/tune/build/tune_rv5
#include "../../libquic_amd/csrc/qfec_kernels.hip"
// (its launch_*revive* functions call launch_revive_passes, defined here)
#include "../../libquic_amd/csrc/qturn_kernels.hip"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#define CK(x)                                                                              \
  do {                                                                                     \
    hipError_t e_ = (x);                                                                   \
    if (e_ != hipSuccess) {                                                                \
      std::fprintf(stderr, "%s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_)); \
      std::exit(1);                                                                        \
    }                                                                                      \
  } while (0)

using qfec::RaggedArgs;
using qfec::u32x4;

namespace rv5 {

constexpr uint64_t kTimeout = 20000;  // 100-MHz ticks: 200 us

__device__ __forceinline__ uint32_t* mw(uint32_t* ms, uint32_t i) { return ms + 64u * i; }
__device__ __forceinline__ uint32_t mload(uint32_t* w) {
  return __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// thread 0: arrive at meeting e (1, 2, ...)
__device__ __forceinline__ void arrive(uint32_t* ms, uint32_t e) {
  const uint32_t B = gridDim.x, sub = blockIdx.x & 15u, nsub = (B - sub + 15u) / 16u;
  const uint32_t old =
      __hip_atomic_fetch_add(mw(ms, 1u + sub), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (old + 1u == e * nsub)
    __hip_atomic_fetch_add(mw(ms, 0), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ bool met(uint32_t* ms, uint32_t e) {
  return mload(mw(ms, 0)) >= e * min(gridDim.x, 16u) || mload(mw(ms, 17)) != 0u;
}
// thread 0: wait for meeting e (bounded)
__device__ __forceinline__ void wait_met(uint32_t* ms, uint32_t e) {
  const uint64_t t0 = wall_clock64();
  while (!met(ms, e)) {
    if (wall_clock64() - t0 > kTimeout) {
      __hip_atomic_fetch_or(mw(ms, 17), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      break;
    }
    __builtin_amdgcn_s_sleep(1);
  }
}

template <bool RECOVER, int WAVES, int GPB, int U, bool NOTAIL, int MODE, int RSLOTS, int BP, int PADW>
__global__ __launch_bounds__(64 * WAVES) void rv5_kernel(RaggedArgs a, uint32_t* ms, uint32_t nblocks) {
  using namespace qfec;
  constexpr uint32_t NT = 64u * WAVES;
  constexpr uint32_t NBLK = NT;
  constexpr uint32_t CAPW = 64u * NBLK;
  constexpr uint32_t NRING = RSLOTS / GPB;  // blocks the ring holds
  static_assert(RSLOTS % GPB == 0 && NRING >= 1, "ring of whole blocks");
  static_assert(MODE != 2 || NRING > BP, "arrive before the ring is full");
  static_assert(RSLOTS <= 64, "held slots scanned by one wave");
  __shared__ uint32_t s_ring[RSLOTS * kAccWords];
  __shared__ u32x4 pk[NT];
  __shared__ uint64_t s_head[NBLK];
  __shared__ uint32_t s_cnt[NBLK];
  __shared__ uint32_t s_rb[GPB + 1], s_kb[GPB], s_m[GPB], s_pl[GPB], s_ob[GPB + 1];
  __shared__ uint64_t s_doff[GPB], s_poff[GPB];
  __shared__ uint32_t s_w[WAVES], s_fit, s_flag;
  __shared__ uint64_t s_sdoff[RSLOTS];
  __shared__ uint32_t s_spl[RSLOTS], s_sob[RSLOTS + 1];
  __shared__ uint32_t s_pad[PADW > 0 ? PADW : 1];
  const uint32_t tid = threadIdx.x;
  const uint32_t lane = lane_id();
  const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane(tid >> 6);
  if (PADW > 0 && tid == 0) s_pad[0] = 0u;  // (keeps the padding allocated)

  // store every parity of the ring's held blocks [hb, hb + nh) (block slots)
  auto store_held = [&](uint32_t hb, uint32_t nh) __attribute__((always_inline)) {
    const uint32_t ns = nh * GPB;
    if (wv == 0u) {
      uint32_t nw = 0;
      if (lane < ns) {
        const uint32_t s = (hb * GPB + lane) % RSLOTS;
        nw = (s_spl[s] + 15u) >> 4;
      }
      const uint32_t incl = wave_incl_scan(nw, lane);
      if (lane < ns) s_sob[lane] = incl - nw;
      if (lane == 0u) s_sob[ns] = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    }
    __syncthreads();
    const uint32_t NW = s_sob[ns];
    for (uint32_t q = tid; q < NW; q += NT) {
      uint32_t lo = 0, hi = ns;  // last i with s_sob[i] <= q
      while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (s_sob[mid] <= q) lo = mid;
        else hi = mid;
      }
      const uint32_t s = (hb * GPB + lo) % RSLOTS;
      const uint32_t t = q - s_sob[lo];
      const uint32_t plen = s_spl[s];
      uint8_t* dst = a.out + s_sdoff[s];
      const uint32_t* ac = s_ring + s * kAccWords;
      if (16u * t + 16u <= plen) {
        st16t<true>(dst + 16u * t, lds_get16(ac, t));
      } else {
        const uint32_t o = plen - 16u * t;
        st16t<true>(dst + plen - 16u, bytes16_at(lds_get16(ac, t - 1u), lds_get16(ac, t), o));
      }
    }
    __syncthreads();
  };

  uint32_t hbase = 0, nheld = 0, done = 0, arrived = 0, handled = 0;
  for (uint32_t b = blockIdx.x; b < nblocks; b += gridDim.x) {
    if constexpr (MODE == 2) {
      if (arrived > handled) {
        if (tid == 0) {
          bool ok = met(ms, handled + 1u);
          if (!ok && nheld == NRING) {
            wait_met(ms, handled + 1u);
            ok = true;
          }
          s_flag = ok ? 1u : 0u;
        }
        __syncthreads();
        if (s_flag) {
          store_held(hbase, nheld);
          hbase = (hbase + nheld) % NRING;
          nheld = 0;
          handled = arrived;
        }
      }
    }
    const uint32_t slot0 = MODE == 2 ? ((hbase + nheld) % NRING) * GPB : 0u;
    uint32_t* acc = s_ring + slot0 * kAccWords;
    const uint64_t g0 = (uint64_t)b * GPB;
    const uint32_t ng = (uint32_t)min<uint64_t>((uint64_t)GPB, a.n_groups - g0);
    s_head[tid] = 0ull;
    if (wv == 0u) {
      uint32_t k = 0, m = 0xFFFFFFFFu, pl = 0, r = 0, p0 = 0;
      uint64_t d = 0, po = 0;
      bool ok = true;
      if (lane < ng) {
        p0 = a.grp_ptr[g0 + lane];
        k = a.grp_ptr[g0 + lane + 1] - p0;
        if constexpr (RECOVER) {
          m = a.missing[g0 + lane];
          pl = a.parity_len[g0 + lane];
          d = a.out_off[g0 + lane];
          po = a.parity_off[g0 + lane];
          ok = m < k && pl >= 16u && pl <= kMaxPacket;
        } else {
          d = a.parity_off[g0 + lane];
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
      const bool all_ok = !wave_any(lane < ng && !ok);
      if (lane == 0u) {
        s_rb[GPB] = R;
        s_fit = (all_ok && R <= NT) ? 1u : 0u;
      }
    }
    __syncthreads();
    const uint32_t R = s_rb[GPB];
    if (RECOVER) {
      for (uint32_t q = tid; q < GPB * (uint32_t)kParWin; q += NT) {
        const uint32_t jq = q / (uint32_t)kParWin, t = q - jq * (uint32_t)kParWin;
        u32x4 w = {0u, 0u, 0u, 0u};
        if (jq < ng) w = parity_window_bf<true>(a.parity + s_poff[jq], s_pl[jq], t);
        lds_put16(acc + jq * kAccWords, t, w);
      }
    }
    uint32_t len = 0, offlo = 0, offhi = 0, j = 0;
    if (tid < R) {
#pragma unroll
      for (int q = 1; q < GPB; ++q) j += tid >= s_rb[q] ? 1u : 0u;
      const uint32_t i = tid - s_rb[j];
      const uint32_t p = s_kb[j] + i + (RECOVER && i >= s_m[j] ? 1u : 0u);
      len = a.pkt_len[p];
      const uint64_t o = a.pkt_off[p];
      offlo = (uint32_t)o;
      offhi = (uint32_t)(o >> 32);
      const uint32_t lim = RECOVER ? s_pl[j] : kMaxPacket;
      if (len < 16u || len > lim || (NOTAIL && (o & 15u) != 0u)) s_fit = 0u;
      if (!RECOVER) atomicMax(&s_pl[j], len);
    }
    const uint32_t n = (len + 15u) >> 4;
    uint32_t W;
    const uint32_t S = block_excl_scan<WAVES>(n, lane, wv, s_w, W);
    if (!(s_fit != 0u && W <= CAPW)) {
      // (outside this probe's form: a real kernel would run the per-group
      // body; the configs[3] batch never gets here)
      if (tid == 0) atomicOr(a.err, 0x80000000u);
      continue;
    }
    if (tid < R) {
      pk[tid] = u32x4{offlo, offhi, len | (j << 16), S};
      __hip_atomic_fetch_or(&s_head[S >> 6], 1ull << (S & 63u), __ATOMIC_RELAXED,
                            __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    if (!RECOVER) {
      for (uint32_t q = tid; q < GPB * (uint32_t)kParWin; q += NT) {
        const uint32_t jq = q / (uint32_t)kParWin, t = q - jq * (uint32_t)kParWin;
        lds_put16(acc + jq * kAccWords, t, u32x4{0u, 0u, 0u, 0u});
      }
    }
    __syncthreads();
    const uint32_t nblk = (W + 63u) >> 6;
    uint32_t tot;
    const uint32_t c = block_excl_scan<WAVES>(tid < nblk ? (uint32_t)__popcll(s_head[tid]) : 0u,
                                              lane, wv, s_w, tot);
    s_cnt[tid] = c;
    if (wv == 0u) {
      if (!RECOVER && lane < ng) a.parity_len_out[g0 + lane] = (uint16_t)s_pl[lane];
      if (MODE == 2 && lane < (uint32_t)GPB) {  // the block's slots: where their parities go
        s_sdoff[slot0 + lane] = s_doff[lane];
        s_spl[slot0 + lane] = lane < ng ? s_pl[lane] : 0u;
      }
      if (MODE == 1) {
        const uint32_t nw = lane < ng ? (s_pl[lane] + 15u) >> 4 : 0u;
        const uint32_t incl = wave_incl_scan(nw, lane);
        if (lane < (uint32_t)GPB) s_ob[lane] = incl - nw;
        if (lane == 0u) s_ob[GPB] = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
      }
    }
    __syncthreads();
    const uint64_t below = lane == 63u ? ~0ull : ((2ull << lane) - 1ull);
    const uint32_t nit = (W + NT - 1u) / NT;
    for (uint32_t it = 0; it < nit; it += U) {
      u32x4 md[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const uint32_t f = (it + (uint32_t)u) * NT + tid;
        const uint32_t bb = min(f >> 6, nblk - 1u);
        const uint64_t M = s_head[bb];
        const uint32_t pi = min(s_cnt[bb] + (uint32_t)__popcll(M & below) - 1u, R - 1u);
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
        inp[u] = NOTAIL || full || (win < ln && (at & 15u) == 0u);
        v[u] = ld16t<true>(a.bytes + (inp[u] ? at : at - win + ln - 16u));
        sh[u] = full ? 0u : min(win + 16u - ln, 15u);
        tt[u] = f < W ? (md[u].z >> 16) * kAccWords + (f - md[u].w) : 0xFFFFFFFFu;
      }
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (tt[u] != 0xFFFFFFFFu) {
          u32x4 w;
          if constexpr (NOTAIL) {
            w = v[u];  // zero padding past the payload: the whole window
          } else {
            const u32x4 ones = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
            const u32x4 mm = shr_bytes_bf(inp[u] ? ones : v[u], sh[u]);
            w = inp[u] ? (mm & v[u]) : mm;
          }
          lds_xor16<__HIP_MEMORY_SCOPE_WORKGROUP>(acc, tt[u], w);
        }
    }
    __syncthreads();
    if constexpr (MODE == 1) {
      const uint32_t NW = s_ob[GPB];
      for (uint32_t q = tid; q < NW; q += NT) {
        uint32_t jq = 0;
#pragma unroll
        for (int i = 1; i < GPB; ++i) jq += q >= s_ob[i] ? 1u : 0u;
        const uint32_t t = q - s_ob[jq];
        const uint32_t plen = s_pl[jq];
        uint8_t* dst = a.out + s_doff[jq];
        const uint32_t* ac = acc + jq * kAccWords;
        if (16u * t + 16u <= plen) {
          st16t<true>(dst + 16u * t, lds_get16(ac, t));
        } else {
          const uint32_t o = plen - 16u * t;
          st16t<true>(dst + plen - 16u, bytes16_at(lds_get16(ac, t - 1u), lds_get16(ac, t), o));
        }
      }
      __syncthreads();
    }
    if constexpr (MODE == 2) {
      ++nheld;
      ++done;
      if (done % BP == 0u) {
        ++arrived;
        if (tid == 0) arrive(ms, arrived);
      }
    }
  }
  if constexpr (MODE == 2) {
    // every workgroup arrives at every meeting of the launch, then stores
    // what it holds once the last one is met
    const uint32_t maxb = (nblocks + gridDim.x - 1u) / gridDim.x;
    const uint32_t E = (maxb + BP - 1u) / BP;
    if (tid == 0) {
      while (arrived < E) arrive(ms, ++arrived);
      wait_met(ms, E);
    }
    arrived = E;
    __syncthreads();
    if (nheld) store_held(hbase, nheld);
  }
}

}  // namespace rv5

static uint64_t sm64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

template <typename T>
static T* up(const std::vector<T>& v) {
  T* d;
  CK(hipMalloc(&d, v.size() * sizeof(T)));
  CK(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  return d;
}

struct V {
  std::string name;
  bool rec, exact;
  std::function<void(const RaggedArgs&)> run;
};

int main(int argc, char** argv) {
  setvbuf(stdout, nullptr, _IOLBF, 0);
  const uint64_t G = 1 << 20;
  const int reps = argc > 1 ? atoi(argv[1]) : 10;
  const int rounds = argc > 2 ? atoi(argv[2]) : 5;
  const uint64_t palign = argc > 3 ? (uint64_t)atoi(argv[3]) : 16u;
  const uint64_t slot = argc > 4 ? (uint64_t)atoi(argv[4]) : 1536u;
  const uint64_t seed = 0x51554944;
  int ncu = 0;
  CK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, 0));
  std::vector<uint32_t> ptr{0};
  std::vector<uint16_t> len;
  std::vector<uint64_t> off, poff(G);
  std::vector<uint8_t> miss(G);
  uint64_t bytes = 0;
  double enc_alg = 0, rec_alg = 0;
  for (uint64_t g = 0; g < G; ++g) {
    const uint32_t k = 5 + (uint32_t)(sm64(seed ^ (0x6Bull << 56) ^ g) % 11);
    miss[g] = (uint8_t)(sm64(seed ^ (0x4Dull << 56) ^ g) % k);
    uint32_t mx = 0;
    double s = 0, sm = 0;
    for (uint32_t i = 0; i < k; ++i) {
      const uint32_t ln = 64 + (uint32_t)(sm64(seed ^ (0x4Cull << 56) ^ (g * 256 + i)) % 1287);
      len.push_back((uint16_t)ln);
      off.push_back(bytes);
      bytes += (ln + palign - 1) / palign * palign;
      s += ln;
      if (i != miss[g]) sm += ln;
      mx = std::max(mx, ln);
    }
    enc_alg += s + mx;
    rec_alg += sm + 2.0 * mx;
    ptr.push_back((uint32_t)len.size());
    poff[g] = g * slot;
  }
  uint8_t* data;
  CK(hipMalloc(&data, bytes + 4096));
  CK(hipMemset(data, 0, bytes + 4096));  // zero padding past every payload (the arena's)
  uint64_t* d_off = up(off);
  uint16_t* d_len = up(len);
  uint32_t* d_ptr = up(ptr);
  uint64_t* d_poff = up(poff);
  uint8_t* d_miss = up(miss);
  CK(qfec::launch_synth_ragged(data, d_off, d_len, d_ptr, 0, G, seed, 0));
  const uint64_t OB = G * slot;
  uint8_t *par_ref, *out_ref, *buf;
  uint16_t *plen_ref, *plen_v;
  uint32_t *err, *ms;
  CK(hipMalloc(&par_ref, OB));
  CK(hipMalloc(&out_ref, OB));
  CK(hipMalloc(&buf, OB));
  CK(hipMalloc(&plen_ref, G * 2));
  CK(hipMalloc(&plen_v, G * 2));
  CK(hipMalloc(&err, 4));
  CK(hipMalloc(&ms, 64 * 4 * 20));
  CK(hipMemset(err, 0, 4));
  CK(hipMemset(par_ref, 0xA5, OB));
  CK(hipMemset(out_ref, 0xA5, OB));
  RaggedArgs e{};
  e.bytes = data;
  e.pkt_off = d_off;
  e.pkt_len = d_len;
  e.grp_ptr = d_ptr;
  e.parity_off = d_poff;
  e.parity_len_out = plen_ref;
  e.out = par_ref;
  e.n_groups = G;
  e.err = err;
  RaggedArgs r = e;
  r.parity = par_ref;
  r.parity_len = plen_ref;
  r.missing = d_miss;
  r.out_off = d_poff;
  r.parity_len_out = nullptr;
  r.out = out_ref;
  auto product = [](bool rec, int diag) {
    return [=](const RaggedArgs& a) {
      const dim3 g((uint32_t)((a.n_groups + 7) / 8)), bl(256);
      if (rec) {
        if (diag == 4) hipLaunchKernelGGL((qfec::ragged_block_kernel<true, 4, 8, 4>), g, bl, 0, 0, a);
        else hipLaunchKernelGGL((qfec::ragged_block_kernel<true, 4, 8, 0>), g, bl, 0, 0, a);
      } else {
        if (diag == 4) hipLaunchKernelGGL((qfec::ragged_block_kernel<false, 4, 8, 4>), g, bl, 0, 0, a);
        else if (diag == 5) hipLaunchKernelGGL((qfec::ragged_block_kernel<false, 4, 8, 5>), g, bl, 0, 0, a);
        else hipLaunchKernelGGL((qfec::ragged_block_kernel<false, 4, 8, 0>), g, bl, 0, 0, a);
      }
    };
  };
  product(false, 0)(e);
  product(true, 0)(r);
  CK(hipDeviceSynchronize());
  RaggedArgs ev = e, rv = r;
  ev.out = buf;
  ev.parity_len_out = plen_v;
  rv.out = buf;
  const uint32_t nblocks = (uint32_t)((G + 7) / 8);
#define RV5(REC, U, NOTAIL, MODE, RS, BP, PADW, P)                                                    \
  [=](const RaggedArgs& a) {                                                                        \
    CK(hipMemsetAsync(ms, 0, 64 * 4 * 20, 0));                                                      \
    hipLaunchKernelGGL((rv5::rv5_kernel<REC, 4, 8, U, NOTAIL, MODE, RS, BP, PADW>),                \
                       dim3((uint32_t)(P * ncu)), dim3(256), 0, 0, a, ms, nblocks);                  \
  }
  std::vector<V> vs;
  vs.push_back({"product", false, true, product(false, 0)});
  vs.push_back({"product, no tail (exact here)", false, true, product(false, 4)});
  vs.push_back({"product, no tail, no stores", false, false, product(false, 5)});
  // LDS per workgroup: ring RS x 1,472 B + ~8 KiB; PADW words more to set P per CU
  vs.push_back({"rv5 no stores P8 (ring 8)", false, false, RV5(false, 2, true, 0, 8, 1, 0, 8)});
  vs.push_back({"rv5 no stores P4", false, false, RV5(false, 2, true, 0, 8, 1, 5000, 4)});
  vs.push_back({"rv5 no stores P2 U4", false, false, RV5(false, 4, true, 0, 8, 1, 10000, 2)});
  vs.push_back({"rv5 one-pass P8", false, true, RV5(false, 2, true, 1, 8, 1, 0, 8)});
  vs.push_back({"rv5 phased P2 ring 40 BP2", false, true, RV5(false, 2, true, 2, 40, 2, 0, 2)});
  vs.push_back({"rv5 phased P2 ring 40 BP3", false, true, RV5(false, 2, true, 2, 40, 3, 0, 2)});
  vs.push_back({"rv5 phased P2 ring 40 BP4 U4", false, true, RV5(false, 4, true, 2, 40, 4, 0, 2)});
  vs.push_back({"rv5 phased P3 ring 24 BP2", false, true, RV5(false, 2, true, 2, 24, 2, 0, 3)});
  vs.push_back({"rv5 phased P4 ring 16 BP1", false, true, RV5(false, 2, true, 2, 16, 1, 0, 4)});
  vs.push_back({"rv5 phased P2 BP3, tail logic", false, true, RV5(false, 2, false, 2, 40, 3, 0, 2)});
  vs.push_back({"product recover", true, true, product(true, 0)});
  vs.push_back({"rv5 phased recover P2 BP3", true, true, RV5(true, 2, true, 2, 40, 3, 0, 2)});

  std::vector<uint8_t> h_ref(OB), h_v(OB);
  std::vector<uint16_t> hp_ref(G), hp_v(G);
  CK(hipMemcpy(hp_ref.data(), plen_ref, G * 2, hipMemcpyDeviceToHost));
  bool all_ok = true;
  for (const V& v : vs) {
    CK(hipMemset(buf, 0xA5, OB));
    CK(hipMemset(plen_v, 0, G * 2));
    CK(hipMemset(err, 0, 4));
    v.run(v.rec ? rv : ev);
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(h_ref.data(), v.rec ? out_ref : par_ref, OB, hipMemcpyDeviceToHost));
    CK(hipMemcpy(h_v.data(), buf, OB, hipMemcpyDeviceToHost));
    uint32_t e_h = 0, ab = 0;
    CK(hipMemcpy(&e_h, err, 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(&ab, ms + 64 * 17, 4, hipMemcpyDeviceToHost));
    bool ok = h_ref == h_v && e_h == 0;
    if (!v.rec) {
      CK(hipMemcpy(hp_v.data(), plen_v, G * 2, hipMemcpyDeviceToHost));
      ok = ok && hp_ref == hp_v;
    }
    std::printf("check %-32s == product: %s (err %#x, abandoned %u)%s\n", v.name.c_str(),
                ok ? "yes" : "NO", e_h, ab, v.exact ? "" : " [not exact: timing only]");
    if (v.exact) all_ok = all_ok && ok;
  }
  if (!all_ok) return 2;
  hipEvent_t t0, t1;
  CK(hipEventCreate(&t0));
  CK(hipEventCreate(&t1));
  std::vector<std::vector<float>> tms(vs.size());
  for (int rd = 0; rd < rounds; ++rd)
    for (size_t i = 0; i < vs.size(); ++i) {
      const V& v = vs[i];
      v.run(v.rec ? rv : ev);
      float tot = 0;
      for (int q = 0; q < reps; ++q) {  // one event pair per launch (the memset outside)
        CK(hipMemsetAsync(ms, 0, 64 * 4 * 20, 0));
        CK(hipEventRecord(t0, 0));
        v.run(v.rec ? rv : ev);
        CK(hipEventRecord(t1, 0));
        CK(hipEventSynchronize(t1));
        float m = 0;
        CK(hipEventElapsedTime(&m, t0, t1));
        tot += m;
      }
      tms[i].push_back(tot / reps);
    }
  std::printf("\nconfigs[3]: %llu groups, k 5-15, len 64-1350, palign %llu (zero padding), slot %llu; "
              "%d CUs; algorithmic GB: encode %.3f, recover %.3f\n",
              (unsigned long long)G, (unsigned long long)palign, (unsigned long long)slot, ncu,
              enc_alg / 1e9, rec_alg / 1e9);
  for (size_t i = 0; i < vs.size(); ++i) {
    std::vector<float> s = tms[i];
    std::sort(s.begin(), s.end());
    const double med = s[s.size() / 2] * 1e-3;
    const double gbs = (vs[i].rec ? rec_alg : enc_alg) / med / 1e9;
    std::printf("%-32s median %8.1f us  %7.1f GB/s  %.4f of 8 TB/s\n", vs[i].name.c_str(), med * 1e6,
                gbs, gbs / 8000.0);
  }
  return 0;
}
