// mgc_lookup_dev.hpp -- what the lookup translation units (mgc_lookup.hip, mgc_filter.hip) share: the table handle, the one
// lookup (lk_find) and the rolling forward / reverse-complement windows (lk_roll / lk_walk).  Not installed.
#pragma once
#include "../../include/meryl_db.h"
#include "../../include/meryl_lookup.h"
#include "mgc_common.hpp"
#include "mgc_devbuf.hpp"

#include <string>

struct mgc_lookup {
  int      device = 0;
  uint32_t k = 0, kw = 1, index_bits = 0, shift = 0;
  uint64_t n = 0, n_db = 0;
  mgc::DBuf d_keys, d_vals, d_index;               // kw x uint64[n], uint32[n], uint64[2^index_bits + 1]
};

namespace mgc {

void lk_set_error(const std::string &m);            // the text mgc_lookup_error() returns (per thread; mgc_lookup.hip)

template <typename K> struct LkOps;
template <> struct LkOps<u64> {
  typedef u64 W;                                   // arithmetic type of a rolling k-mer
  static __device__ __forceinline__ u64 bucket(u64 k, u32 shift) { return shift >= 64 ? 0ull : (k >> shift); }
  static __device__ __forceinline__ u64 key(W w) { return w; }
};
template <> struct LkOps<K128> {
  typedef u128 W;
  static __device__ __forceinline__ u64 bucket(K128 k, u32 shift) { return shift >= 128 ? 0ull : (u64)(KeyOps<K128>::v(k) >> shift); }
  static __device__ __forceinline__ K128 key(W w) { return KeyOps<K128>::mk(w); }
};

template <typename K>
__device__ __forceinline__ u32 lk_find(const K *__restrict__ keys, const u32 *__restrict__ vals, const u64 *__restrict__ index,
                                       u32 shift, K q, u64 n_index = ~0ull /* 2^index_bits: the index holds one entry more */) {
  const u64 p = LkOps<K>::bucket(q, shift);
  if (p >= n_index) return 0u;                        // a query with bits above 2k (queries are looked up as given): not a k-mer, not stored
  u64 lo = index[p];
  const u64 end = index[p + 1];
  u64 hi = end;
  while (lo < hi) {
    const u64 mid = lo + ((hi - lo) >> 1);
    if (KeyOps<K>::lt(keys[mid], q)) lo = mid + 1; else hi = mid;
  }
  return (lo < end && !KeyOps<K>::ne(keys[lo], q)) ? vals[lo] : 0u;
}

// The same search for the position index (mgc_positions.hip): the k-mer's rank in the table -- merylExactLookup::index() --
// or LK_NO_SLOT.  A sibling of lk_find and not its body: lk_find stays as it is compiled into the timed lookup kernels.
constexpr u32 LK_NO_SLOT = 0xFFFFFFFFu;             // (tables of the position index hold at most 2^32 - 2 k-mers)
template <typename K>
__device__ __forceinline__ u32 lk_find_slot(const K *__restrict__ keys, const u64 *__restrict__ index, u32 shift, K q, u64 n_index) {
  const u64 p = LkOps<K>::bucket(q, shift);
  if (p >= n_index) return LK_NO_SLOT;
  u64 lo = index[p];
  const u64 end = index[p + 1];
  u64 hi = end;
  while (lo < hi) {
    const u64 mid = lo + ((hi - lo) >> 1);
    if (KeyOps<K>::lt(keys[mid], q)) lo = mid + 1; else hi = mid;
  }
  return (lo < end && !KeyOps<K>::ne(keys[lo], q)) ? (u32)lo : LK_NO_SLOT;
}

// 2-bit code of a base (A0 C1 T2 G3, reference.rst:525), -1 for anything else
__device__ __forceinline__ int lk_code(u32 c) {
  const u32 l = c | 0x20u;
  const bool ok = (l == 'a') | (l == 'c') | (l == 'g') | (l == 't');
  return ok ? (int)((c >> 1) & 3u) : -1;
}

constexpr int LK_RUN = 16;                          // window starts per thread

// Every window start of [i0, i0 + LK_RUN): the rolling forward / reverse-complement pair of the reference's kmerIterator
// (call sites src/meryl-lookup/existence.C:69-77, dump.C:98-112), restarted at i0 -- windows that start at or after i0 depend on
// no earlier base.  visit(start, fmer, rmer, fmer == rmer)
template <typename K, typename F>
__device__ __forceinline__ void lk_roll(const uint8_t *__restrict__ bases, u64 n_bases, u32 k, u64 i0, F visit) {
  typedef typename LkOps<K>::W W;
  const W one = 1;
  const W mask = (2 * k >= sizeof(W) * 8) ? ~(W)0 : ((one << (2 * k)) - 1);
  W f = 0, r = 0;
  u32 load = 0;
  const u64 jend = (i0 + LK_RUN + k - 1 < n_bases) ? (i0 + LK_RUN + k - 1) : n_bases;
  for (u64 j = i0; j < jend; j++) {
    const int code = lk_code(bases[j]);
    if (code < 0) { load = 0; f = 0; r = 0; continue; }
    f = ((f << 2) | (W)code) & mask;
    r = (r >> 2) | ((W)(code ^ 2) << (2 * k - 2));
    if (load < k) load++;
    if (load < k) continue;
    const u64 s = j + 1 - k;                        // >= i0 because load restarted at i0
    if (s >= i0 + LK_RUN) break;
    visit(s, LkOps<K>::key(f), LkOps<K>::key(r), f == r);
  }
}

// visit(start, value_or_0) of every window start of [i0, i0 + LK_RUN) in one table
template <typename K, typename F>
__device__ __forceinline__ void lk_walk(const K *__restrict__ keys, const u32 *__restrict__ vals, const u64 *__restrict__ index,
                                        u32 shift, const uint8_t *__restrict__ bases, u64 n_bases, u32 k, u64 i0, F visit) {
  lk_roll<K>(bases, n_bases, k, i0, [&](u64 s, K f, K r, bool pal) {
    u32 v = lk_find<K>(keys, vals, index, shift, f);
    if (v == 0 && !pal) v = lk_find<K>(keys, vals, index, shift, r);   // value(fmer) > 0 || value(rmer) > 0
    visit(s, v);
  });
}

// The tables of one pass travel in the kernel-argument segment: a device-resident array of descriptors written at launch,
// read with uniform loads, no allocation or upload per call.  At most 32 tables (one presence bit each).
constexpr u32 LK_MAX_TABLES = 32;
struct LkTable { const void *keys; const u32 *vals; const u64 *index; u64 n_index; u32 shift, reserved; };
struct LkSet { LkTable t[LK_MAX_TABLES]; u32 n, k; };

__device__ __forceinline__ u32 rp_dec_len(u64 x) {
  u32 l = 1;
  for (u64 p = 10; l < 20 && x >= p; p *= 10) l++;
  return l;
}

}  // namespace mgc
