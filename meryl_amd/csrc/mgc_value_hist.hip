// mgc_value_hist.hip -- the value-histogram accumulator of include/meryl_db.h (mgc_value_hist_*): value -> number of k-mers that
// carry it, over any number of device-resident value arrays.
//
// Reference side: merylHistogram::addValue per k-mer in every compute thread, the 64 per-slice histograms summed in
// merylOpTemplate::finishAction (src/meryl2/merylOpTemplate.C:285-307).  Here one kernel pass per array:
//   dense tier   values below VH_DENSE are counted in LDS bins (uint32, one set per workgroup).  Before the LDS atomic a wave
//                looks for a value that at least VH_COMBINE_MIN = 32 of its lanes hold -- the value of its first active lane, then
//                of the first lane that differs from it -- and the leader adds the number of those lanes once; the other lanes
//                take plain LDS atomics.  A wave whose lanes all hold 1 (the normal shape of count data) issues one LDS atomic
//                from one lane, not 64 on one address, and no address is ever hit by more than 31 lanes of one instruction.
//                (Combining EVERY repeated value -- three leaders peeled in turn, whatever their share -- was measured first
//                and costs more than the conflicts it removes: both runs are in profiles/setops_bench_hist.jsonl and
//                DESIGN.md section 9.)  Each workgroup flushes its non-zero bins into the accumulator's uint64 global bins once.
//   list tier    values of VH_DENSE and above are appended to a device list as uint64 by a wave-aggregated append: one returning
//                global atomic per wave and iteration (up to 256 values), every lane writes at the leader's base plus its rank in
//                the ballots.  The list has room for every value of the pass, so it cannot overflow and nothing is retried.
// A non-empty list is sorted over 32 bits and run-length counted on the device, and its (value, occurrences) pairs are merged into a
// sorted host vector: the one list tier of mgc_hist_list.hpp.  A pass takes at most VH_CHUNK = 2^26 values, so the 32-bit run lengths
// of the rle kernels and the uint32 LDS bins cannot wrap.
//
// kernel-resource-usage (scripts/kres.py value_hist_tiers mgc_value_hist.hip): in DESIGN.md §9, "Value histograms of tree results".
#include "../../include/meryl_db.h"
#include "mgc_device.h"
#include "mgc_hist_list.hpp"
#include "mgc_session.hpp"

#include <algorithm>
#include <vector>

namespace mgc {
namespace {
typedef uint32_t u32;
typedef uint64_t u64;

constexpr u32 VH_DENSE  = 4096;              // values below it: LDS bins (16 KiB per workgroup: eight workgroups per CU)
constexpr u32 VH_BLOCK  = 256;               // threads per workgroup
constexpr u32 VH_VEC    = 4;                 // values per lane and iteration (one 16-byte load)
constexpr u32 VH_COMBINE_MIN = 32;           // lanes of a wave that must hold one value for it to be added once by their leader
constexpr u32 VH_LEADERS = 2;                // candidates tried per wave-wide step
constexpr u64 VH_CHUNK  = 1ull << 26;        // values per pass

// one wave-wide step of the dense tier: lanes with `mine` set hold v < VH_DENSE
__device__ __forceinline__ void dense_add(u32 *s_bins, u32 v, bool mine, u32 lane) {
  u64 left = __ballot(mine);
  for (u32 r = 0; r < VH_LEADERS && (u32)__popcll(left) >= VH_COMBINE_MIN; r++) {
    const u32 leader = (u32)__ffsll((unsigned long long)left) - 1u;
    const u32 lv = (u32)__builtin_amdgcn_readlane((int)v, (int)leader);       // (leader is wave-uniform: no trip through LDS)
    const u64 same = __ballot(mine && v == lv);
    if ((u32)__popcll(same) >= VH_COMBINE_MIN) {                              // (wave-uniform)
      if (lane == leader) atomicAdd(&s_bins[lv], (u32)__popcll(same));
      mine = mine && v != lv;
      break;
    }
    left &= ~same;
  }
  if (mine) atomicAdd(&s_bins[v], 1u);
}

// values[0, n): head (< 4 values up to the first 16-byte boundary), n_vec 16-byte vectors, tail (< 4 values).  The scalar ends
// are taken by the first wave of workgroup 0.  list has room for n entries; *list_n is zeroed by the caller.
__global__ __launch_bounds__(VH_BLOCK)
void value_hist_tiers_kernel(const u32 *__restrict__ values, u64 n, u32 head, u64 n_vec, u64 *__restrict__ dense /*[VH_DENSE]*/,
                             u64 *__restrict__ list, unsigned long long *__restrict__ list_n) {
  __shared__ u32 s_bins[VH_DENSE];
  for (u32 i = threadIdx.x; i < VH_DENSE; i += VH_BLOCK) s_bins[i] = 0;
  __syncthreads();
  const u32 lane = threadIdx.x & 63u;
  const u64 lt_mask = (1ull << lane) - 1ull;
  // one iteration of one wave: up to VH_VEC values per lane (cnt of them valid), one list atomic
  auto step = [&](const u32 (&v)[VH_VEC], u32 cnt) {
    u64 big[VH_VEC];
    u32 total = 0;
#pragma unroll
    for (u32 c = 0; c < VH_VEC; c++) {
      const bool valid = c < cnt;
      dense_add(s_bins, v[c], valid && v[c] < VH_DENSE, lane);
      big[c] = __ballot(valid && v[c] >= VH_DENSE);
      total += (u32)__popcll(big[c]);
    }
    if (total == 0) return;                                  // (wave-uniform)
    unsigned long long base = 0;
    if (lane == 0) base = atomicAdd(list_n, (unsigned long long)total);
    base = ((unsigned long long)(u32)__builtin_amdgcn_readlane((int)(u32)(base >> 32), 0) << 32) | (u32)__builtin_amdgcn_readlane((int)(u32)base, 0);
    u32 before = 0;
#pragma unroll
    for (u32 c = 0; c < VH_VEC; c++) {
      if (c < cnt && v[c] >= VH_DENSE) {
        const u64 at = base + before + (u32)__popcll(big[c] & lt_mask);
        if (at < n) list[at] = (u64)v[c];                    // (always true: at most n values are appended)
      }
      before += (u32)__popcll(big[c]);
    }
  };
  const uint4 *vec = reinterpret_cast<const uint4 *>(values + head);
  const u64 stride = (u64)gridDim.x * VH_BLOCK;
  // every lane of a wave makes the same number of trips: the ballots and shuffles see whole waves
  // the next trip's vector is fetched before this trip's values are counted: a wave makes its trips one after the other, and the
  // ballots of a trip are a serial chain the load's latency would otherwise be added to
  u64 first = (u64)blockIdx.x * VH_BLOCK + (threadIdx.x & ~63u);
  uint4 q = make_uint4(0, 0, 0, 0);
  bool have = first + lane < n_vec;
  if (have) q = vec[first + lane];
  for (; first < n_vec; first += stride) {
    const u32 v[VH_VEC] = {q.x, q.y, q.z, q.w};
    const u32 cnt = have ? VH_VEC : 0u;
    const u64 next = first + stride + lane;
    have = next < n_vec;
    if (have) q = vec[next];
    step(v, cnt);
  }
  if (blockIdx.x == 0 && threadIdx.x < 64) {
    const u64 tail_at = (u64)head + VH_VEC * n_vec;
    const u32 n_ends = head + (u32)(n - tail_at);            // at most 6
    u32 v[VH_VEC] = {0, 0, 0, 0};
    u32 cnt = 0;
    if (lane < n_ends) { v[0] = values[lane < head ? (u64)lane : tail_at + (lane - head)]; cnt = 1; }
    step(v, cnt);
  }
  __syncthreads();
  for (u32 i = threadIdx.x; i < VH_DENSE; i += VH_BLOCK)
    if (s_bins[i]) atomicAdd(reinterpret_cast<unsigned long long *>(dense + i), (unsigned long long)s_bins[i]);
}

hipError_t launch_value_hist_tiers(const u32 *d_values, u64 n, u64 *d_dense, u64 *d_list, u64 *d_list_n, u32 n_cus, hipStream_t st) {
  if (n == 0) return hipSuccess;
  const u64 mis = ((uintptr_t)d_values & 15u) / 4u;
  const u32 head = (u32)std::min<u64>(n, mis ? 4u - mis : 0u);
  const u64 n_vec = (n - head) / VH_VEC;
  const u64 want = (n_vec + VH_BLOCK - 1) / VH_BLOCK;
  const u32 grid = (u32)std::max<u64>(1, std::min<u64>(want, (u64)n_cus * 8u));
  hipLaunchKernelGGL(value_hist_tiers_kernel, dim3(grid), dim3(VH_BLOCK), 0, st, d_values, n, head, n_vec, d_dense, d_list,
                     reinterpret_cast<unsigned long long *>(d_list_n));
  return hipGetLastError();
}
}  // namespace

hipError_t warm_value_hist() { hipFuncAttributes a; return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&value_hist_tiers_kernel)); }
}  // namespace mgc

using mgc::set_err;

struct mgc_value_hist {
  typedef mgc::DBuf DBuf;
  int device = -1;
  uint32_t n_cus = 1;
  bool ready = false;
  DBuf d_dense;
  mgc::ListTier list{"mgc_value_hist"};     // values of VH_DENSE and above
  std::vector<mgc::HistPair> rows;          // both tiers, ascending by value (cache)
  bool rows_ok = false;
  bool failed = false;                      // an add failed part of the way: the dense bins may hold values the list lost

  ~mgc_value_hist() { if (d_dense.p) (void)hipSetDevice(device); }      // (the buffers go after this body, on that device)

#define VH_TRY(expr) do { hipError_t e__ = (expr); if (e__ != hipSuccess) {                                         \
    set_err(nullptr, "mgc_value_hist: %s -> %s", #expr, hipGetErrorString(e__));                                  \
    return (e__ == hipErrorOutOfMemory) ? MGC_ENOMEM : MGC_EHIP; } } while (0)

  int init(hipStream_t st) {                // the first touch of the device; st: where the first values are counted
    if (ready) { VH_TRY(hipSetDevice(device)); return MGC_OK; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { (void)hipGetLastError(); set_err(nullptr, "mgc_value_hist: no HIP device"); return MGC_EHIP; }
    if (device < 0) (void)hipGetDevice(&device);
    VH_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    VH_TRY(hipGetDeviceProperties(&prop, device));
    n_cus = (uint32_t)std::max(prop.multiProcessorCount, 1);
    VH_TRY(d_dense.ensure(8 * mgc::VH_DENSE));
    VH_TRY(hipMemsetAsync(d_dense.p, 0, 8 * mgc::VH_DENSE, st));      // (ordered before the first kernel, whatever kind of stream st is)
    ready = true;
    return MGC_OK;
  }

  int add_chunk(const uint32_t *d_values, uint64_t n, hipStream_t st) {
    VH_TRY(list.reserve(n));
    VH_TRY(list.reset(st));
    VH_TRY(mgc::launch_value_hist_tiers(d_values, n, d_dense.as<uint64_t>(), list.list(), list.list_n(), n_cus, st));
    uint64_t need = 0;
    VH_TRY(hipMemcpyAsync(&need, list.list_n(), 8, hipMemcpyDeviceToHost, st));
    VH_TRY(hipStreamSynchronize(st));
    if (need > n) { set_err(nullptr, "mgc_value_hist: the list holds more entries than the pass has values"); return MGC_EHIP; }
    return list.drain(need, 32, st);
  }

  int add(const uint32_t *d_values, uint64_t n, hipStream_t st) {
    rows_ok = false;
    for (uint64_t o = 0; o < n; o += mgc::VH_CHUNK) {
      const int rc = add_chunk(d_values + o, std::min<uint64_t>(mgc::VH_CHUNK, n - o), st);
      if (rc != MGC_OK) return rc;
    }
    return MGC_OK;
  }

  int build() {
    if (failed) { set_err(nullptr, "mgc_value_hist: an add failed; the accumulator can only be closed"); return MGC_ESTATE; }
    if (rows_ok) return MGC_OK;
    rows.clear();
    if (ready) {
      VH_TRY(hipSetDevice(device));
      std::vector<uint64_t> hd(mgc::VH_DENSE);
      VH_TRY(hipMemcpy(hd.data(), d_dense.p, 8 * mgc::VH_DENSE, hipMemcpyDeviceToHost));
      for (uint32_t v = 0; v < mgc::VH_DENSE; v++) if (hd[v]) rows.push_back(mgc::HistPair{v, hd[v]});
    }
    rows.insert(rows.end(), list.acc.begin(), list.acc.end());         // every list value is >= VH_DENSE: already ascending
    rows_ok = true;
    return MGC_OK;
  }
#undef VH_TRY
};

extern "C" mgc_value_hist *mgc_value_hist_open(int device) {
  mgc_value_hist *h = new mgc_value_hist();
  h->device = device;
  return h;
}

extern "C" void mgc_value_hist_close(mgc_value_hist *h) { delete h; }

extern "C" void mgc_value_hist_geometry(uint32_t *dense_limit, uint32_t *workgroup_values) {
  if (dense_limit) *dense_limit = mgc::VH_DENSE;
  if (workgroup_values) *workgroup_values = mgc::VH_BLOCK * mgc::VH_VEC;
}

extern "C" int mgc_value_hist_add(mgc_value_hist *h, const uint32_t *d_values, uint64_t n, void *stream) {
  if (!h) { set_err(nullptr, "mgc_value_hist_add: NULL accumulator"); return MGC_EINVAL; }
  if (n && !d_values) { set_err(nullptr, "mgc_value_hist_add: NULL array of %llu values", (unsigned long long)n); return MGC_EINVAL; }
  if ((uintptr_t)d_values & 3u) { set_err(nullptr, "mgc_value_hist_add: the values are not aligned to 4 bytes"); return MGC_EINVAL; }
  if (n == 0) return MGC_OK;
  if (h->failed) { set_err(nullptr, "mgc_value_hist_add: an earlier add failed; the accumulator can only be closed"); return MGC_ESTATE; }
  int rc = h->init((hipStream_t)stream);
  if (rc == MGC_OK) rc = h->add(d_values, n, (hipStream_t)stream);
  if (rc != MGC_OK) h->failed = true;
  return rc;
}

extern "C" int mgc_value_hist_len(mgc_value_hist *h, uint64_t *n_pairs) {
  if (!h || !n_pairs) { set_err(nullptr, "mgc_value_hist_len: NULL argument"); return MGC_EINVAL; }
  const int rc = h->build();
  if (rc == MGC_OK) *n_pairs = h->rows.size();
  return rc;
}

extern "C" int mgc_value_hist_get(mgc_value_hist *h, uint64_t *values, uint64_t *occurrences) {
  if (!h) { set_err(nullptr, "mgc_value_hist_get: NULL accumulator"); return MGC_EINVAL; }
  const int rc = h->build();
  if (rc != MGC_OK) return rc;
  if (!h->rows.empty() && (!values || !occurrences)) { set_err(nullptr, "mgc_value_hist_get: NULL array"); return MGC_EINVAL; }
  for (size_t i = 0; i < h->rows.size(); i++) { values[i] = h->rows[i].key; occurrences[i] = h->rows[i].n; }
  return MGC_OK;
}

extern "C" int mgc_value_hist_totals(mgc_value_hist *h, uint64_t *unique, uint64_t *distinct, uint64_t *total) {
  if (!h) { set_err(nullptr, "mgc_value_hist_totals: NULL accumulator"); return MGC_EINVAL; }
  const int rc = h->build();
  if (rc != MGC_OK) return rc;
  uint64_t u = 0, d = 0, t = 0;
  for (const mgc::HistPair &p : h->rows) { if (p.key == 1) u = p.n; d += p.n; t += p.key * p.n; }
  if (unique) *unique = u;
  if (distinct) *distinct = d;
  if (total) *total = t;
  return MGC_OK;
}
