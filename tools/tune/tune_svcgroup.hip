// tune_svcgroup.hip — round 5: the service's first group takes 5.6 us
// (stamps_svc5c.txt) where the bare PCIe shape of its bytes takes 2.8 us
// (tune_hostlat C, warm).  One wave runs the product's window_group (the
// service's body: tables in LDS, payloads and outputs in mapped host memory)
// on one 10 x 1350 B group, timed in the kernel with the 100-MHz wall clock:
//   first   the first call of a fresh launch (cold instruction cache)
//   again   a second call right after (warm instruction cache, warm TLB)
//   idle    a call after ~100 us of polling a host word (the service's idle
//           between flushes)
//   fence   the system-scope fence after the second call
// variants: tables in LDS (product) or in device memory; parity_len_out in
// host or device memory.  Medians of 300 launches; outputs byte-checked.
// build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -I libquic_amd/csrc tools/tune/tune_svcgroup.hip -o tools/tune/build/tune_svcgroup
#include "../../libquic_amd/csrc/qfec_kernels.hip"
// (its launch_*revive* functions call launch_revive_passes, defined here)
#include "../../libquic_amd/csrc/qturn_kernels.hip"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define CK(x)                                                                              \
  do {                                                                                     \
    hipError_t e_ = (x);                                                                   \
    if (e_ != hipSuccess) {                                                                \
      std::fprintf(stderr, "%s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_)); \
      std::exit(1);                                                                        \
    }                                                                                      \
  } while (0)

namespace {
constexpr int kP = 10;
constexpr uint32_t kL = 1350;
// table layout (bytes): off[10] u64, len[10] u16, ptr[2] u32, poff[1] u64
constexpr uint32_t kTOff = 0, kTLen = 80, kTPtr = 104, kTPoff = 112, kTBytes = 128;

__global__ __launch_bounds__(64) void svcgroup_probe(qfec::RaggedArgs a, const uint8_t* tab_src,
                                                     int lds_tables, const uint64_t* idle_word,
                                                     uint64_t* res) {
  __shared__ uint32_t s_par[4 * qfec::kParWin];
  __shared__ uint64_t s_head[qfec::kParWin];
  __shared__ qfec::u32x4 s_meta[64];
  __shared__ __attribute__((aligned(16))) uint8_t s_tab[kTBytes];
  const uint32_t lane = threadIdx.x;
  if (lane < kTBytes / 16u)
    *reinterpret_cast<qfec::u32x4*>(s_tab + 16u * lane) =
        *reinterpret_cast<const qfec::u32x4*>(tab_src + 16u * lane);
  __syncthreads();
  const uint8_t* tb = lds_tables ? s_tab : tab_src;
  a.pkt_off = reinterpret_cast<const uint64_t*>(tb + kTOff);
  a.pkt_len = reinterpret_cast<const uint16_t*>(tb + kTLen);
  a.grp_ptr = reinterpret_cast<const uint32_t*>(tb + kTPtr);
  a.parity_off = reinterpret_cast<const uint64_t*>(tb + kTPoff);
  uint64_t t[8];
  t[0] = wall_clock64();
  qfec::window_group<false, qfec::kSvcPB>(a, 0, lane, s_par, s_head, s_meta);
  t[1] = wall_clock64();
  qfec::window_group<false, qfec::kSvcPB>(a, 0, lane, s_par, s_head, s_meta);
  t[2] = wall_clock64();
  __threadfence_system();
  t[3] = wall_clock64();
  // ~100 us polling a host word (as the idle service), then once more
  const uint64_t w0 = wall_clock64();
  uint64_t x = 0;
  while (wall_clock64() - w0 < 10000u) {
    x += __hip_atomic_load(idle_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __builtin_amdgcn_s_sleep(2);
  }
  asm volatile("" ::"v"((uint32_t)x));
  t[4] = wall_clock64();
  qfec::window_group<false, qfec::kSvcPB>(a, 0, lane, s_par, s_head, s_meta);
  t[5] = wall_clock64();
  __threadfence_system();
  t[6] = wall_clock64();
  if (lane == 0)
    for (int q = 0; q < 7; ++q) res[q] = t[q];
}
}  // namespace

int main() {
  setvbuf(stdout, nullptr, _IOLBF, 0);
  const unsigned fl = hipHostMallocMapped | hipHostMallocPortable;
  uint8_t *h_pay, *h_out;
  uint16_t* h_plen;
  CK(hipHostMalloc(&h_pay, 1 << 20, fl));
  CK(hipHostMalloc(&h_out, 1 << 16, fl));
  CK(hipHostMalloc(&h_plen, 4096, fl));
  uint64_t s = 0x9E3779B97F4A7C15ull;
  for (int i = 0; i < (1 << 20); ++i) {
    s ^= s << 13; s ^= s >> 7; s ^= s << 17;
    h_pay[i] = (uint8_t)s;
  }
  std::vector<uint8_t> tab(kTBytes, 0);
  for (int r = 0; r < kP; ++r) {
    const uint64_t o = 4096 + (uint64_t)r * kL;
    std::memcpy(&tab[kTOff + 8 * r], &o, 8);
    const uint16_t l = kL;
    std::memcpy(&tab[kTLen + 2 * r], &l, 2);
  }
  const uint32_t ptr[2] = {0, kP};
  std::memcpy(&tab[kTPtr], ptr, 8);
  const uint64_t poff = 128;
  std::memcpy(&tab[kTPoff], &poff, 8);
  std::vector<uint8_t> want(kL, 0);
  for (int r = 0; r < kP; ++r)
    for (uint32_t b = 0; b < kL; ++b) want[b] ^= h_pay[4096 + r * kL + b];
  uint8_t *d_tab, *d_pay, *d_out;
  uint16_t *d_hplen, *d_dplen;
  uint64_t* d_res;
  CK(hipMalloc(&d_tab, kTBytes));
  CK(hipMemcpy(d_tab, tab.data(), kTBytes, hipMemcpyHostToDevice));
  CK(hipMalloc(&d_dplen, 4096));
  CK(hipMalloc(&d_res, 64));
  CK(hipHostGetDevicePointer(reinterpret_cast<void**>(&d_pay), h_pay, 0));
  CK(hipHostGetDevicePointer(reinterpret_cast<void**>(&d_out), h_out, 0));
  CK(hipHostGetDevicePointer(reinterpret_cast<void**>(&d_hplen), h_plen, 0));
  uint32_t* d_err;
  CK(hipMalloc(&d_err, 64));
  CK(hipMemset(d_err, 0, 64));
  struct Var {
    const char* name;
    int lds;
    bool host_plen;
  } vars[] = {{"tables in LDS, lengths to host (product)", 1, true},
              {"tables in device memory, lengths to host", 0, true},
              {"tables in LDS, lengths to device memory", 1, false}};
  const int R = 300;
  for (const Var& v : vars) {
    qfec::RaggedArgs a{};
    a.bytes = d_pay;
    a.out = d_out;
    a.parity_len_out = v.host_plen ? d_hplen : d_dplen;
    a.n_groups = 1;
    a.err = d_err;
    std::vector<double> c[5];
    bool ok = true;
    for (int r = 0; r < R + 10; ++r) {
      std::memset(h_out, 0, 4096);
      hipLaunchKernelGGL(svcgroup_probe, dim3(1), dim3(64), 0, 0, a, d_tab, v.lds,
                         reinterpret_cast<const uint64_t*>(d_pay), d_res);
      CK(hipDeviceSynchronize());
      uint64_t t[7];
      CK(hipMemcpy(t, d_res, sizeof(t), hipMemcpyDeviceToHost));
      ok = ok && std::memcmp(h_out + poff, want.data(), kL) == 0;
      if (r < 10) continue;
      c[0].push_back((t[1] - t[0]) * 0.01);
      c[1].push_back((t[2] - t[1]) * 0.01);
      c[2].push_back((t[3] - t[2]) * 0.01);
      c[3].push_back((t[5] - t[4]) * 0.01);
      c[4].push_back((t[6] - t[5]) * 0.01);
    }
    std::printf("%s: outputs %s\n", v.name, ok ? "IDENTICAL" : "DIFFER");
    const char* cn[] = {"first call", "again", "fence after again", "after 100 us idle",
                        "fence after idle call"};
    for (int q = 0; q < 5; ++q) {
      std::sort(c[q].begin(), c[q].end());
      std::printf("  %-22s median %6.2f us  p10 %6.2f  p90 %6.2f\n", cn[q], c[q][c[q].size() / 2],
                  c[q][c[q].size() / 10], c[q][c[q].size() * 9 / 10]);
    }
    if (!ok) return 2;
  }
  return 0;
}
