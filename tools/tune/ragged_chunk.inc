// ragged_chunk.inc — EXPERIMENT (round 3, VERDICT r2 next-round 3): the
// ragged kernel phased by chunks, with the fixed kernel's read / write
// separation.  Not in the library: measured slower than ragged_multi_kernel
// (tools/tune/tune_rchunk.hip, profiles/round3/ragged_chunk/; DESIGN.md §4).
// Included after qfec_kernels.hip (uses its helpers, namespace qfec).
namespace qfec {
namespace {

// A looser meeting for phases of uneven work (ragged chunks): wait until
// `quorum` of the gridDim.x workgroups have arrived at meeting `epoch`
// (cumulative arrivals over the 16 sub-counters), so the slowest few do not
// hold the rest.  Same timeout / abandon path as phase_meet.
__device__ __forceinline__ void phase_meet_quorum(uint32_t* ps, uint32_t epoch, uint32_t quorum) {
  __syncthreads();
  if (threadIdx.x == 0 && ph_load(ph_word(ps, 18)) == 0u) {
    const uint32_t B = gridDim.x, sub = blockIdx.x & 15u;
    __hip_atomic_fetch_add(ph_word(ps, 1u + sub), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t target = (epoch - 1u) * B + quorum;
    const uint64_t t0 = wall_clock64();
    for (;;) {
      uint32_t n = 0;
#pragma unroll
      for (uint32_t i = 0; i < 16u; ++i) n += ph_load(ph_word(ps, 1u + i));
      if (n >= target) break;
      if (wall_clock64() - t0 > kPhTimeout) {
        if (__hip_atomic_fetch_or(ph_word(ps, 18), 1u, __ATOMIC_RELAXED,
                                  __HIP_MEMORY_SCOPE_AGENT) == 0u)
          __hip_atomic_fetch_add(ph_word(ps, 19), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        break;
      }
      if (ph_load(ph_word(ps, 18)) != 0u) break;
      __builtin_amdgcn_s_sleep(1);
    }
  }
  __syncthreads();
}

// ---------------------------------------------------------------------------
// Ragged CSR, large batches: phased by chunks (the fixed kernel's read / write
// separation, VERDICT r2 next-round 3).
// ---------------------------------------------------------------------------
// A persistent grid of one 1,024-lane workgroup per CU walks the batch in
// phases.  In phase p workgroup b owns a chunk of GP groups — steps of kRcGPS
// adjacent groups, the steps of all workgroups interleaved so that at any time
// the grid reads one contiguous window of the batch — and
//   1. builds the chunk's tables cooperatively in LDS: the groups' scalars,
//      one received packet per lane (offset, length, its group's accumulator
//      slot, its first flat window S from a workgroup scan), a start bitmask
//      over the chunk's flat 16-byte windows and per 64-window block the
//      number of packets starting before it — ONE pass of dependent loads
//      per phase instead of one per group pair (the round-2 phased attempts
//      paid it per pair and ran at 0.41-0.47 of 8 TB/s, DESIGN.md §4);
//   2. streams the chunk's flat windows (lane l of wave w, iteration i:
//      window 1024 i + 64 w + l; packet = starts before its block + popcount
//      of the block's mask below the lane), each window XORed into its
//      group's accumulator in LDS (component-major, as ragged_multi_kernel);
//   3. meets the grid, then stores every group's parity / revived row.
// A chunk the tables cannot hold (more than kRcMaxPk received packets or
// 64 x kRcMaxBlk windows), or with any invalid field or a packet below 16
// bytes, runs the exact per-group body (ragged_group) instead, so outputs and
// error bits are those of ragged_multi_kernel.
constexpr int kRcWaves = 16;
constexpr int kRcThreads = 64 * kRcWaves;
constexpr int kRcGroups = 80;   // accumulators per CU: 80 x 1,472 B = 115 KiB of LDS
constexpr int kRcGPS = 2;       // adjacent groups per step
constexpr int kRcMaxPk = 1024;  // received packets per chunk (one per lane)
constexpr int kRcMaxBlk = 1024;  // 64-window blocks per chunk

// Exclusive prefix sum over a workgroup of NW waves (x per lane); the total
// in *total.  Contains barriers: every lane of the workgroup must call it.
template <int NW>
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t x, uint32_t lane, uint32_t wv,
                                                    uint32_t* wsum, uint32_t* total) {
  const uint32_t incl = wave_incl_scan(x, lane);
  if (lane == 63u) wsum[wv] = incl;
  __syncthreads();
  uint32_t before = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < NW; ++w) {
    const uint32_t s = wsum[w];
    before += (uint32_t)w < wv ? s : 0u;
    tot += s;
  }
  __syncthreads();
  *total = tot;
  return before + incl - x;
}

template <int GP>
__device__ __forceinline__ uint64_t chunk_group(uint32_t p, uint32_t j, uint64_t B, uint32_t b) {
  constexpr uint32_t SPC = GP / kRcGPS;  // steps per chunk
  return (((uint64_t)p * SPC + j / kRcGPS) * B + b) * kRcGPS + j % kRcGPS;
}

// TIMED (tools/tune only): workgroups 0 and gridDim/2 record s_memrealtime
// at the end of each phase step into tstamp[(wg? 1 : 0) * 4 * nphase + 4p + step].
template <bool RECOVER, int U = 2, int GP = kRcGroups, bool TIMED = false, bool MEET = true>
__global__ __launch_bounds__(kRcThreads) void ragged_chunk_kernel(RaggedArgs a, uint32_t nphase,
                                                                  uint32_t* psync, uint32_t* phost,
                                                                  uint64_t* tstamp = nullptr) {
  static_assert(GP % kRcGPS == 0 && GP <= kRcThreads, "chunk shape");
  constexpr uint32_t kSlot = 4u * kParWin;  // accumulator words per group (= kAccWords)
  __shared__ uint32_t s_acc[GP * kSlot];
  __shared__ u32x4 s_pk[kRcMaxPk];  // {off lo, off hi, len | slot << 16, first window S}
  __shared__ uint64_t s_head[kRcMaxBlk];
  __shared__ uint32_t s_blk[kRcMaxBlk];
  __shared__ uint32_t s_gq[GP + 1];  // received-packet base of group slot j
  __shared__ uint32_t s_gp[GP], s_gm[GP], s_pl[GP];
  __shared__ uint64_t s_do[GP], s_po[GP];
  __shared__ uint32_t s_wsum[kRcWaves];
  __shared__ uint32_t s_flag;
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
  const uint64_t B = gridDim.x;
  const uint64_t below = lane == 63u ? ~0ull : ((2ull << lane) - 1ull);
  for (uint32_t p = 0; p < nphase; ++p) {
    // ---- 1a. the chunk's groups (lane j < GP: group slot j)
    uint32_t kr = 0;
    bool bad = false;
    if (tid < (uint32_t)GP) {
      const uint64_t g = chunk_group<GP>(p, tid, B, blockIdx.x);
      uint32_t k = 0, m = 0xFFFFFFFFu, pl = 0, P = 0;
      uint64_t dof = 0, pof = 0;
      if (g < a.n_groups) {
        P = a.grp_ptr[g];
        k = a.grp_ptr[g + 1] - P;
        if constexpr (RECOVER) {
          m = a.missing[g];
          pl = a.parity_len[g];
          dof = a.out_off[g];
          pof = a.parity_off[g];
          bad = !(k >= 1u && k <= 255u && m < k && pl >= 16u && pl <= kMaxPacket);
        } else {
          dof = a.parity_off[g];
          bad = !(k >= 1u && k <= 255u);
        }
        kr = bad ? 0u : (RECOVER ? k - 1u : k);
      }
      s_gp[tid] = P;
      s_gm[tid] = m;
      s_pl[tid] = pl;  // encode: 0 here, the max length below
      s_do[tid] = dof;
      s_po[tid] = pof;
    }
    if (tid == 0) s_flag = 0u;
    __syncthreads();
    if (bad) s_flag = 1u;
    uint32_t NQ;
    const uint32_t Q = block_excl_scan<kRcWaves>(kr, lane, wv, s_wsum, &NQ);
    if (tid < (uint32_t)GP) s_gq[tid] = Q;
    if (tid == 0) {
      s_gq[GP] = NQ;
      if (NQ > (uint32_t)kRcMaxPk) s_flag = 1u;
    }
    __syncthreads();
    // ---- 1b. one received packet per lane
    uint32_t len = 0, offlo = 0, offhi = 0, slot = 0;
    const bool fast0 = s_flag == 0u;
    if (fast0 && tid < NQ) {
      uint32_t lo = 0, hi = GP;  // s_gq[lo] <= tid < s_gq[hi]
#pragma unroll 1
      while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (s_gq[mid] <= tid) lo = mid; else hi = mid;
      }
      slot = lo;
      const uint32_t i = tid - s_gq[lo];
      const uint32_t pidx = s_gp[lo] + i + (RECOVER && i >= s_gm[lo] ? 1u : 0u);
      len = a.pkt_len[pidx];
      const uint64_t o = a.pkt_off[pidx];
      offlo = (uint32_t)o;
      offhi = (uint32_t)(o >> 32);
      const uint32_t lim = RECOVER ? s_pl[lo] : kMaxPacket;
      if (len < 16u || len > lim) s_flag = 1u;
    }
    uint32_t W;
    const uint32_t S = block_excl_scan<kRcWaves>((len + 15u) >> 4, lane, wv, s_wsum, &W);
    const uint32_t nblk = (W + 63u) >> 6;
    for (uint32_t q = tid; q < nblk && q < (uint32_t)kRcMaxBlk; q += kRcThreads) s_head[q] = 0ull;
    if (!RECOVER && tid < (uint32_t)GP) s_pl[tid] = 0u;
    if (tid == 0 && nblk > (uint32_t)kRcMaxBlk) s_flag = 1u;
    __syncthreads();
    const bool fast = s_flag == 0u;
    const bool tw = TIMED && tid == 0 && (blockIdx.x == 0 || blockIdx.x == gridDim.x / 2);
    uint64_t* ts = tstamp + (blockIdx.x == 0 ? 0u : 4u * nphase) + 4u * p;
    if (fast) {
      if (tid < NQ) {
        s_pk[tid] = u32x4{offlo, offhi, len | (slot << 16), S};
        __hip_atomic_fetch_or(&s_head[S >> 6], 1ull << (S & 63u), __ATOMIC_RELAXED,
                              __HIP_MEMORY_SCOPE_WORKGROUP);
        if constexpr (!RECOVER) atomicMax(&s_pl[slot], len);
      }
      // accumulators: the parity rows (recover) or zero (encode)
      for (uint32_t q = tid; q < (uint32_t)GP * kParWin; q += kRcThreads) {
        const uint32_t j = q / kParWin, t = q - j * kParWin;
        u32x4 v = {0u, 0u, 0u, 0u};
        if constexpr (RECOVER) {
          const uint32_t pl = s_pl[j];
          if (pl >= 16u) v = parity_window_bf<true>(a.parity + s_po[j], pl, t);
        }
        lds_put16(s_acc + j * kSlot, t, v);
      }
      __syncthreads();
      // packet starts before each 64-window block
      const uint32_t c = tid < nblk ? (uint32_t)__popcll(s_head[tid]) : 0u;
      uint32_t nst;
      const uint32_t bs = block_excl_scan<kRcWaves>(c, lane, wv, s_wsum, &nst);
      if (tid < nblk) s_blk[tid] = bs;
      __syncthreads();
      if (tw) ts[0] = wall_clock64();
      // ---- 2. the chunk's flat windows, U iterations' loads in flight
      const uint32_t nit = (nblk + kRcWaves - 1u) / kRcWaves;
      for (uint32_t it = 0; it < nit; it += U) {
        uint64_t M[U];
        uint32_t b0[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const uint32_t b = (it + u) * kRcWaves + wv;
          M[u] = b < nblk ? s_head[b] : 0ull;
          b0[u] = b < nblk ? s_blk[b] : NQ;
        }
        u32x4 md[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const uint32_t pi = min(b0[u] + (uint32_t)__popcll(M[u] & below) - 1u, NQ - 1u);
          md[u] = s_pk[pi];
        }
        u32x4 v[U];
        uint32_t tt[U], sh[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const uint32_t f = ((it + u) * kRcWaves + wv) * 64u + lane;
          const uint32_t ln = md[u].z & 0xFFFFu;
          const uint32_t win = 16u * (f - md[u].w);
          const bool full = win + 16u <= ln;
          v[u] = ld16t<true>(a.bytes + (((uint64_t)md[u].y << 32) | md[u].x) +
                             (full ? win : ln - 16u));
          sh[u] = full ? 0u : min(win + 16u - ln, 15u);
          tt[u] = f < W ? (md[u].z >> 16) * kSlot + (f - md[u].w) : 0xFFFFFFFFu;
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
          if (tt[u] != 0xFFFFFFFFu) lds_xor16(s_acc, tt[u], shr_bytes_bf(v[u], sh[u]));
      }
    } else {
      // the per-group body (exact outputs and error bits), one wave per group,
      // its scratch carved from the accumulators
      uint32_t* base = s_acc + wv * (kSlot + 2u * kParWin + 4u * 64u);
      uint32_t* par = base;
      uint64_t* head = reinterpret_cast<uint64_t*>(base + kSlot);
      u32x4* meta = reinterpret_cast<u32x4*>(base + kSlot + 2u * kParWin);
      for (uint32_t j = wv; j < (uint32_t)GP; j += kRcWaves) {
        const uint64_t g = chunk_group<GP>(p, j, B, blockIdx.x);
        if (g >= a.n_groups) continue;
        GroupPrefetch f;
        group_scalars<RECOVER>(a, g, f);
        group_vectors<RECOVER>(a, g, lane, f);
        wave_lds_order();
        ragged_group<RECOVER>(a, g, lane, f, par, head, meta);
        wave_lds_order();
      }
    }
    if (tw) ts[1] = wall_clock64();
    if constexpr (MEET) phase_meet(psync, p + 1u);
    else __syncthreads();
    if (tw) ts[2] = wall_clock64();
    // ---- 3. stores
    if (fast) {
      if (!RECOVER && tid < (uint32_t)GP) {
        const uint64_t g = chunk_group<GP>(p, tid, B, blockIdx.x);
        if (g < a.n_groups) a.parity_len_out[g] = (uint16_t)s_pl[tid];
      }
      for (uint32_t q = tid; q < (uint32_t)GP * kParWin; q += kRcThreads) {
        const uint32_t j = q / kParWin, t = q - j * kParWin;
        const uint32_t pl = s_pl[j];
        if (16u * t >= pl) continue;  // absent groups have pl = 0
        uint8_t* dst = a.out + s_do[j];
        const uint32_t* acc = s_acc + j * kSlot;
        if (16u * t + 16u <= pl) {
          st16t<true>(dst + 16u * t, lds_get16(acc, t));
        } else {
          const uint32_t o = pl - 16u * t;  // 1..15
          st16t<true>(dst + pl - 16u, bytes16_at(lds_get16(acc, t - 1u),
                                                 lds_get16(acc, t), o));
        }
      }
    }
    __syncthreads();  // the stores' LDS reads before the next chunk's tables
    if (tw) ts[3] = wall_clock64();
  }
  phase_exit(psync, phost);
}

// The same chunk-phased kernel with its table loads pipelined across phases:
// the group scalars of phase p+2 and the packet table of phase p+1 are loaded
// into registers while phase p streams, so a phase's setup is LDS work only
// (two table buffers of group scalars; the packet table, start mask and block
// counts are rebuilt in place after the stores).
struct RcGroupRegs {
  uint32_t P, k, m, pl;
  uint64_t dof, pof;
  bool present;
};

template <bool RECOVER, int GP>
__device__ __forceinline__ RcGroupRegs rc_load_groups(const RaggedArgs& a, uint32_t p,
                                                     uint32_t nphase, uint32_t tid) {
  RcGroupRegs r{0u, 0u, 0xFFFFFFFFu, 0u, 0ull, 0ull, false};
  if (tid < (uint32_t)GP && p < nphase) {
    const uint64_t g = chunk_group<GP>(p, tid, gridDim.x, blockIdx.x);
    if (g < a.n_groups) {
      r.present = true;
      r.P = a.grp_ptr[g];
      r.k = a.grp_ptr[g + 1] - r.P;
      if constexpr (RECOVER) {
        r.m = a.missing[g];
        r.pl = a.parity_len[g];
        r.dof = a.out_off[g];
        r.pof = a.parity_off[g];
      } else {
        r.dof = a.parity_off[g];
      }
    }
  }
  return r;
}

template <int GP>
struct RcTables {
  uint32_t gq[2][GP + 1], gp[2][GP], gm[2][GP], pl[2][GP];
  uint64_t dof[2][GP], pof[2][GP];
  uint32_t nq[2], flag[2];
};

template <bool RECOVER, int U = 2, int GP = kRcGroups, bool TIMED = false, int QPCT = 100>
__global__ __launch_bounds__(kRcThreads) void ragged_chunk2_kernel(RaggedArgs a, uint32_t nphase,
                                                                   uint32_t* psync, uint32_t* phost,
                                                                   uint64_t* tstamp = nullptr) {
  static_assert(GP % kRcGPS == 0 && GP <= kRcThreads, "chunk shape");
  constexpr uint32_t kSlot = 4u * kParWin;
  __shared__ uint32_t s_acc[GP * kSlot];
  __shared__ u32x4 s_pk[kRcMaxPk];
  __shared__ uint64_t s_head[kRcMaxBlk];
  __shared__ uint32_t s_blk[kRcMaxBlk];
  __shared__ RcTables<GP> T;
  __shared__ uint32_t s_wsum[kRcWaves];
  __shared__ uint32_t s_W;
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
  const uint64_t below = lane == 63u ? ~0ull : ((2ull << lane) - 1ull);

  // the group table of phase q from its registers (buffer q & 1): scalars,
  // received-packet bases (workgroup scan), the fallback flag
  auto group_table = [&](const RcGroupRegs& r, uint32_t q) {
    const uint32_t bf = q & 1u;
    bool bad = false;
    uint32_t kr = 0;
    if (r.present) {
      bad = RECOVER ? !(r.k >= 1u && r.k <= 255u && r.m < r.k && r.pl >= 16u && r.pl <= kMaxPacket)
                    : !(r.k >= 1u && r.k <= 255u);
      kr = bad ? 0u : (RECOVER ? r.k - 1u : r.k);
    }
    if (tid < (uint32_t)GP) {
      T.gp[bf][tid] = r.P;
      T.gm[bf][tid] = r.m;
      T.pl[bf][tid] = r.present ? r.pl : 0u;  // encode: the max length, set in build_tables
      T.dof[bf][tid] = r.dof;
      T.pof[bf][tid] = r.pof;
    }
    if (tid == 0) T.flag[bf] = 0u;
    __syncthreads();
    if (bad) T.flag[bf] = 1u;
    uint32_t NQ;
    const uint32_t Q = block_excl_scan<kRcWaves>(kr, lane, wv, s_wsum, &NQ);
    if (tid < (uint32_t)GP) T.gq[bf][tid] = Q;
    if (tid == 0) {
      T.gq[bf][GP] = NQ;
      T.nq[bf] = NQ;
      if (NQ > (uint32_t)kRcMaxPk) T.flag[bf] = 1u;
    }
    __syncthreads();
  };
  // the packet of lane tid in phase q's chunk, loaded into registers
  struct PkRegs {
    uint32_t len, offlo, offhi, slot;
  };
  auto load_packets = [&](uint32_t q) {
    const uint32_t bf = q & 1u;
    PkRegs r{0u, 0u, 0u, 0u};
    if (q < nphase && T.flag[bf] == 0u && tid < T.nq[bf]) {
      uint32_t lo = 0, hi = GP;
#pragma unroll 1
      while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (T.gq[bf][mid] <= tid) lo = mid; else hi = mid;
      }
      r.slot = lo;
      const uint32_t i = tid - T.gq[bf][lo];
      const uint32_t pidx = T.gp[bf][lo] + i + (RECOVER && i >= T.gm[bf][lo] ? 1u : 0u);
      r.len = a.pkt_len[pidx];
      const uint64_t o = a.pkt_off[pidx];
      r.offlo = (uint32_t)o;
      r.offhi = (uint32_t)(o >> 32);
    }
    return r;
  };
  // packet table, start mask, block counts and accumulators of phase q
  auto build_tables = [&](const PkRegs& r, uint32_t q) {
    const uint32_t bf = q & 1u;
    const uint32_t NQ = T.nq[bf];
    if (tid < NQ && T.flag[bf] == 0u) {
      const uint32_t lim = RECOVER ? T.pl[bf][r.slot] : kMaxPacket;
      if (r.len < 16u || r.len > lim) T.flag[bf] = 1u;
    }
    uint32_t W;
    const uint32_t S = block_excl_scan<kRcWaves>((r.len + 15u) >> 4, lane, wv, s_wsum, &W);
    const uint32_t nblk = (W + 63u) >> 6;
    for (uint32_t x = tid; x < nblk && x < (uint32_t)kRcMaxBlk; x += kRcThreads) s_head[x] = 0ull;
    if (!RECOVER && tid < (uint32_t)GP) T.pl[bf][tid] = 0u;
    if (tid == 0) {
      s_W = W;
      if (nblk > (uint32_t)kRcMaxBlk) T.flag[bf] = 1u;
    }
    __syncthreads();
    if (T.flag[bf] != 0u) return;
    if (tid < NQ) {
      s_pk[tid] = u32x4{r.offlo, r.offhi, r.len | (r.slot << 16), S};
      __hip_atomic_fetch_or(&s_head[S >> 6], 1ull << (S & 63u), __ATOMIC_RELAXED,
                            __HIP_MEMORY_SCOPE_WORKGROUP);
      if constexpr (!RECOVER) atomicMax(&T.pl[bf][r.slot], r.len);
    }
    // per 64-window block: the packet holding its first window (no scan:
    // each packet marks the <= 2 block starts it covers); the stream adds the
    // starts inside the block below the lane
    if (tid < NQ) {
      const uint32_t n = (r.len + 15u) >> 4;
      for (uint32_t b = (S + 63u) >> 6; 64u * b < S + n; ++b) s_blk[b] = tid;
    }
    for (uint32_t x = tid; x < (uint32_t)GP * kParWin; x += kRcThreads) {
      const uint32_t j = x / kParWin, t = x - j * kParWin;
      u32x4 v = {0u, 0u, 0u, 0u};
      if constexpr (RECOVER) {
        const uint32_t pl = T.pl[bf][j];
        if (pl >= 16u) v = parity_window_bf<true>(a.parity + T.pof[bf][j], pl, t);
      }
      lds_put16(s_acc + j * kSlot, t, v);
    }
    __syncthreads();
  };

  RcGroupRegs g0 = rc_load_groups<RECOVER, GP>(a, 0u, nphase, tid);
  group_table(g0, 0u);
  PkRegs pk = load_packets(0u);
  RcGroupRegs gn = rc_load_groups<RECOVER, GP>(a, 1u, nphase, tid);
  for (uint32_t p = 0; p < nphase; ++p) {
    const uint32_t bf = p & 1u;
    build_tables(pk, p);
    // pipeline: the next phase's group table (its scalars arrived during this
    // phase's predecessor), its packet loads and the group loads two ahead
    group_table(gn, p + 1u);
    pk = load_packets(p + 1u);
    gn = rc_load_groups<RECOVER, GP>(a, p + 2u, nphase, tid);
    const bool fast = T.flag[bf] == 0u;
    const bool tw = TIMED && tid == 0 && (blockIdx.x == 0 || blockIdx.x == gridDim.x / 2);
    uint64_t* ts = tstamp + (blockIdx.x == 0 ? 0u : 4u * nphase) + 4u * p;
    if (tw) ts[0] = wall_clock64();
    if (fast) {
      const uint32_t NQ = T.nq[bf], W = s_W, nblk = (W + 63u) >> 6;
      const uint32_t nit = (nblk + kRcWaves - 1u) / kRcWaves;
      for (uint32_t it = 0; it < nit; it += U) {
        uint64_t M[U];
        uint32_t b0[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const uint32_t b = (it + u) * kRcWaves + wv;
          M[u] = b < nblk ? s_head[b] : 0ull;
          b0[u] = b < nblk ? s_blk[b] : NQ - 1u;
        }
        u32x4 md[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const uint32_t pi = min(b0[u] + (uint32_t)__popcll(M[u] & below & ~1ull), NQ - 1u);
          md[u] = s_pk[pi];
        }
        u32x4 v[U];
        uint32_t tt[U], sh[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const uint32_t f = ((it + u) * kRcWaves + wv) * 64u + lane;
          const uint32_t ln = md[u].z & 0xFFFFu;
          const uint32_t win = 16u * (f - md[u].w);
          const bool full = win + 16u <= ln;
          v[u] = ld16t<true>(a.bytes + (((uint64_t)md[u].y << 32) | md[u].x) +
                             (full ? win : ln - 16u));
          sh[u] = full ? 0u : min(win + 16u - ln, 15u);
          tt[u] = f < W ? (md[u].z >> 16) * kSlot + (f - md[u].w) : 0xFFFFFFFFu;
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
          if (tt[u] != 0xFFFFFFFFu) lds_xor16(s_acc, tt[u], shr_bytes_bf(v[u], sh[u]));
      }
    } else {
      uint32_t* base = s_acc + wv * (kSlot + 2u * kParWin + 4u * 64u);
      uint32_t* par = base;
      uint64_t* head = reinterpret_cast<uint64_t*>(base + kSlot);
      u32x4* meta = reinterpret_cast<u32x4*>(base + kSlot + 2u * kParWin);
      for (uint32_t j = wv; j < (uint32_t)GP; j += kRcWaves) {
        const uint64_t g = chunk_group<GP>(p, j, gridDim.x, blockIdx.x);
        if (g >= a.n_groups) continue;
        GroupPrefetch f;
        group_scalars<RECOVER>(a, g, f);
        group_vectors<RECOVER>(a, g, lane, f);
        wave_lds_order();
        ragged_group<RECOVER>(a, g, lane, f, par, head, meta);
        wave_lds_order();
      }
    }
    if (tw) ts[1] = wall_clock64();
    if constexpr (QPCT >= 100) phase_meet(psync, p + 1u);
    else phase_meet_quorum(psync, p + 1u, (gridDim.x * QPCT + 99u) / 100u);
    if (tw) ts[2] = wall_clock64();
    if (fast) {
      if (!RECOVER && tid < (uint32_t)GP) {
        const uint64_t g = chunk_group<GP>(p, tid, gridDim.x, blockIdx.x);
        if (g < a.n_groups) a.parity_len_out[g] = (uint16_t)T.pl[bf][tid];
      }
      for (uint32_t x = tid; x < (uint32_t)GP * kParWin; x += kRcThreads) {
        const uint32_t j = x / kParWin, t = x - j * kParWin;
        const uint32_t pl = T.pl[bf][j];
        if (16u * t >= pl) continue;
        uint8_t* dst = a.out + T.dof[bf][j];
        const uint32_t* acc = s_acc + j * kSlot;
        if (16u * t + 16u <= pl) {
          st16t<true>(dst + 16u * t, lds_get16(acc, t));
        } else {
          const uint32_t o = pl - 16u * t;
          st16t<true>(dst + pl - 16u, bytes16_at(lds_get16(acc, t - 1u),
                                                 lds_get16(acc, t), o));
        }
      }
    }
    __syncthreads();
    if (tw) ts[3] = wall_clock64();
  }
  phase_exit(psync, phost);
}

}  // namespace
}  // namespace qfec
