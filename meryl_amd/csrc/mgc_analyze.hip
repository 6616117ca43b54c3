// mgc_analyze.hip -- gfx950 kernels of include/meryl_analyze.h: composition scores of k-mers and their (histogram, score, value)
// histograms.
//
// Reference side: src/meryl-analyze/meryl-analyze.C -- histGC / histGA / histGT score one k-mer at a time in a loop over its
// bases (:176-201, :262-299, :364-401) and insert its value into a std::map per (histogram, score).  Here one thread scores one
// k-mer; a value below the dense bound is one LDS atomic per histogram into the workgroup's table, which is flushed once with
// 64-bit global adds; any other value is appended, one wave at a time, to a list of packed (histogram, score, value) entries
// that the caller sorts and run-length counts (mgc_sort.hip, mgc_scan.hip).
#include "mgc_common.hpp"
#include "mgc_analyze_dev.hpp"
#include "../../include/meryl_analyze.h"

namespace mgc {
namespace {

constexpr int AN_BLOCK = 512;
constexpr u32 AN_DENSE = MGC_ANALYZE_DENSE_VALUES;

// the run rule over the bases of one word, last base first (the sum over maximal runs does not depend on the direction).
// alphabet bit: 1 = forward alphabet; the letter inside an alphabet is the low bit of the code.  State: the open run's
// alphabet (2: none yet), its length and which of its two letters it has shown.
struct RunState { u32 cur, len, seen, f, r; };
template <int TYPE>
__device__ __forceinline__ void run_bases(u64 w, u32 nb, RunState &s) {
  for (u32 j = 0; j < nb; j++) {
    const u32 c = (u32)w & 3u;
    w >>= 2;
    const u32 a = (TYPE == MGC_ANALYZE_GA) ? (((c ^ (c >> 1)) & 1u) ^ 1u) : (c >> 1);   // -ga: A (0) and G (3); -gt: T (2) and G (3)
    const bool brk = a != s.cur;
    const u32 closed = (brk && s.seen == 3u) ? s.len : 0u;
    s.f += (s.cur == 1u) ? closed : 0u;
    s.r += (s.cur == 0u) ? closed : 0u;
    s.len = brk ? 1u : s.len + 1u;
    s.seen = (brk ? 0u : s.seen) | (1u << (c & 1u));
    s.cur = a;
  }
}
__device__ __forceinline__ void run_close(RunState &s) {
  const u32 closed = (s.seen == 3u) ? s.len : 0u;
  s.f += (s.cur == 1u) ? closed : 0u;
  s.r += (s.cur == 0u) ? closed : 0u;
}

template <typename K> struct AnKey;
template <> struct AnKey<u64> {
  static __device__ __forceinline__ u64 lo(u64 k) { return k; }
  static __device__ __forceinline__ u64 hi(u64) { return 0ull; }
};
template <> struct AnKey<K128> {
  static __device__ __forceinline__ u64 lo(K128 k) { return k.lo; }
  static __device__ __forceinline__ u64 hi(K128 k) { return k.hi; }
};

// (forward, reverse) of one k-mer of k bases; both are at most k
template <typename K, int TYPE>
__device__ __forceinline__ void analyze_score(K key, u32 k, u32 &f, u32 &r) {
  const u64 lo = AnKey<K>::lo(key), hi = AnKey<K>::hi(key);
  const u32 nlo = k < 32u ? k : 32u, nhi = k - nlo;
  if (TYPE == MGC_ANALYZE_GC) {
    // C (1) and G (3) are the codes with the low bit set
    const u64 mlo = nlo == 32u ? 0x5555555555555555ull : (0x5555555555555555ull & ((1ull << (2u * nlo)) - 1ull));
    const u64 mhi = nhi == 32u ? 0x5555555555555555ull : (0x5555555555555555ull & ((1ull << (2u * nhi)) - 1ull));
    f = (u32)__popcll(lo & mlo) + (u32)__popcll(hi & mhi);
    r = k - f;
  } else {
    RunState s = {2u, 0u, 0u, 0u, 0u};
    run_bases<TYPE>(lo, nlo, s);
    run_bases<TYPE>(hi, nhi, s);
    run_close(s);
    f = s.f; r = s.r;
  }
}

template <typename K, int TYPE>
__global__ __launch_bounds__(256)
void analyze_score_kernel(const K *__restrict__ keys, u64 n, u32 k, uint8_t *__restrict__ fscore, uint8_t *__restrict__ rscore) {
  const u64 stride = (u64)gridDim.x * blockDim.x;
  for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    u32 f, r;
    analyze_score<K, TYPE>(keys[i], k, f, r);
    fscore[i] = (uint8_t)f;
    rscore[i] = (uint8_t)r;
  }
}

// NH histograms per k-mer: -gc 1 (forward), -ga / -gt 3 (forward, reverse, max of the two)
template <typename K, int TYPE>
__global__ __launch_bounds__(AN_BLOCK)
void analyze_hist_kernel(const K *__restrict__ keys, const u32 *__restrict__ values, u64 n, u32 k, u32 dense, u32 do_dense,
                         u64 *__restrict__ g_dense, u64 *__restrict__ list, u64 list_cap, u64 *__restrict__ list_n) {
  constexpr u32 NH = (TYPE == MGC_ANALYZE_GC) ? 1u : 3u;
  extern __shared__ u32 s_t[];                            // [NH][k + 1][AN_DENSE] when the dense tier counts, nothing otherwise
  const u32 rows = k + 1u;
  const u32 table = (dense && do_dense) ? NH * rows * AN_DENSE : 0u;
  for (u32 i = threadIdx.x; i < table; i += AN_BLOCK) s_t[i] = 0u;
  __syncthreads();

  // every wave runs the same number of iterations with all its lanes, so that the ballot below sees whole waves
  const u64 stride = (u64)gridDim.x * AN_BLOCK;
  const u64 iters = (n + stride - 1) / stride;
  const u64 gid = (u64)blockIdx.x * AN_BLOCK + threadIdx.x;
  const u32 lane = lane_id();
  for (u64 it = 0; it < iters; it++) {
    const u64 i = it * stride + gid;
    const bool valid = i < n;
    u32 sc[3] = {0u, 0u, 0u};
    u32 v = 0u;
    if (valid) {
      v = values[i];
      analyze_score<K, TYPE>(keys[i], k, sc[0], sc[1]);
      sc[2] = sc[0] > sc[1] ? sc[0] : sc[1];
    }
    const bool small = v < dense;
    if (valid && small && do_dense) {
#pragma unroll
      for (u32 h = 0; h < NH; h++) atomicAdd(&s_t[(h * rows + sc[h]) * AN_DENSE + v], 1u);
    }
    const bool ov = valid && !small;
    const u64 bal = __ballot(ov);
    if (bal) {                                            // (uniform over the wave)
      u64 base = 0ull;
      if (lane == 0) base = atomicAdd(reinterpret_cast<unsigned long long *>(list_n), (unsigned long long)__popcll(bal) * NH);
      base = __shfl(base, 0);
      if (ov) {
        const u64 at = base + (u64)__popcll(bal & ((1ull << lane) - 1ull)) * NH;
#pragma unroll
        for (u32 h = 0; h < NH; h++)
          if (at + h < list_cap) list[at + h] = ((u64)h << 39) | ((u64)sc[h] << 32) | (u64)v;
      }
    }
  }
  __syncthreads();
  for (u32 i = threadIdx.x; i < table; i += AN_BLOCK) {
    const u32 c = s_t[i];
    if (c) {
      const u32 h = i / (rows * AN_DENSE), rem = i - h * rows * AN_DENSE;     // rem = score * AN_DENSE + value
      atomicAdd(reinterpret_cast<unsigned long long *>(g_dense + (u64)h * ANALYZE_SCORES * AN_DENSE + rem), (unsigned long long)c);
    }
  }
}

}  // namespace

hipError_t launch_analyze_scores(const void *d_keys, uint64_t n, uint32_t k, int type, uint8_t *d_fscore, uint8_t *d_rscore, hipStream_t st) {
  if (n == 0) return hipSuccess;
  const dim3 grid((uint32_t)std::min<uint64_t>((n + 255) / 256, 1u << 16)), block(256);
#define MGC_AN_SCORE(K_, T_) hipLaunchKernelGGL((analyze_score_kernel<K_, T_>), grid, block, 0, st, reinterpret_cast<const K_ *>(d_keys), (u64)n, k, d_fscore, d_rscore)
  if (k > 32) {
    if (type == MGC_ANALYZE_GC) MGC_AN_SCORE(K128, MGC_ANALYZE_GC); else if (type == MGC_ANALYZE_GA) MGC_AN_SCORE(K128, MGC_ANALYZE_GA); else MGC_AN_SCORE(K128, MGC_ANALYZE_GT);
  } else {
    if (type == MGC_ANALYZE_GC) MGC_AN_SCORE(u64, MGC_ANALYZE_GC); else if (type == MGC_ANALYZE_GA) MGC_AN_SCORE(u64, MGC_ANALYZE_GA); else MGC_AN_SCORE(u64, MGC_ANALYZE_GT);
  }
#undef MGC_AN_SCORE
  return hipGetLastError();
}

hipError_t launch_analyze_hist(const void *d_keys, const uint32_t *d_values, uint64_t n, uint32_t k, int type, uint32_t dense, bool do_dense,
                               uint64_t *d_dense, uint64_t *d_list, uint64_t list_cap, uint64_t *d_list_n, uint32_t n_cus, hipStream_t st) {
  if (n == 0) return hipSuccess;
  if (n > (1ull << 31) || k == 0 || k > MGC_ANALYZE_MAX_K || (dense != 0 && dense != AN_DENSE)) return hipErrorInvalidValue;
  const uint32_t nh = analyze_device_hists(type);
  const size_t lds = (dense && do_dense) ? sizeof(u32) * nh * (k + 1) * AN_DENSE : 0;       // at most 74,880 bytes
  // as many workgroups as stay resident: by their table (160 KiB of LDS per CU) and by 32 waves per CU
  uint32_t per_cu = lds ? (uint32_t)std::min<size_t>((160u << 10) / lds, 4) : 4u;
  const uint64_t want = (n + AN_BLOCK - 1) / AN_BLOCK;
  const dim3 grid((uint32_t)std::min<uint64_t>(want, (uint64_t)std::max(n_cus, 1u) * per_cu)), block(AN_BLOCK);
#define MGC_AN_HIST(K_, T_) do {                                                                                                     \
    if (lds > (48u << 10))                                                                                                           \
      MGC_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&analyze_hist_kernel<K_, T_>), hipFuncAttributeMaxDynamicSharedMemorySize, \
                                    (int)(sizeof(u32) * ANALYZE_HISTS * ANALYZE_SCORES * AN_DENSE)));                                \
    hipLaunchKernelGGL((analyze_hist_kernel<K_, T_>), grid, block, lds, st, reinterpret_cast<const K_ *>(d_keys), d_values, (u64)n, k, dense, \
                       do_dense ? 1u : 0u, reinterpret_cast<u64 *>(d_dense), reinterpret_cast<u64 *>(d_list), (u64)list_cap,         \
                       reinterpret_cast<u64 *>(d_list_n)); } while (0)
  if (k > 32) {
    if (type == MGC_ANALYZE_GC) MGC_AN_HIST(K128, MGC_ANALYZE_GC); else if (type == MGC_ANALYZE_GA) MGC_AN_HIST(K128, MGC_ANALYZE_GA); else MGC_AN_HIST(K128, MGC_ANALYZE_GT);
  } else {
    if (type == MGC_ANALYZE_GC) MGC_AN_HIST(u64, MGC_ANALYZE_GC); else if (type == MGC_ANALYZE_GA) MGC_AN_HIST(u64, MGC_ANALYZE_GA); else MGC_AN_HIST(u64, MGC_ANALYZE_GT);
  }
#undef MGC_AN_HIST
  return hipGetLastError();
}

}  // namespace mgc
