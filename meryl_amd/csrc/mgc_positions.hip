// mgc_positions.hip -- kernels of the k-mer position index and of query painting (include/meryl_positions.h), gfx950.
//
// Replaces merylExactLookup::index / loadPositions / _posStart / _posData [meryl-utility, not in tree] as position-lookup uses
// them (src/meryl-lookup/position-lookup.C:140-141, 197-203, 248-259, 272-288, 299-327).  The reference walks the position
// list of every hit and increments one counter per position; here every reference base knows its slot (ref_slot), the hits of
// a batch are summed per SLOT from the sorted (slot, query) pairs, and the per-base reports are gathers through ref_slot:
// O(hits + reference) whatever the repeats, exact, order-independent, and no atomic shared by more than two threads.
// Integer work bound by the latency of the table searches, like mgc_lookup.hip; everything else streams.
#include "mgc_lookup_dev.hpp"
#include "mgc_compact.hpp"
#include "mgc_positions_dev.hpp"

namespace mgc {

static_assert(POS_NONE == LK_NO_SLOT, "one sentinel");

// last sequence starting at or before p: the non-empty one that holds it
__device__ __forceinline__ u64 pos_seq_of(const u64 *__restrict__ ss, u64 n_seq, u64 p) {
  u64 lo = 0, hi = n_seq;
  while (hi - lo > 1) { const u64 mid = lo + ((hi - lo) >> 1); if (ss[mid] <= p) lo = mid; else hi = mid; }
  return lo;
}

// One thread = LK_RUN window starts, one workgroup = 256 * LK_RUN = 4096 of them (the tile of lookup_stream_kernel).
// position-lookup.C:197-203: only min(fmer, rmer) is looked up.  QUERY: the per-sequence sums of -hpq (:248-259) -- a thread
// adds up the hits of the sequence it is in and hands them over when the sequence changes; what the threads hold at the end
// belongs to one sequence wherever a wave lies inside one (contigs, long reads): it is summed over the wave, then over the
// waves of the workgroup that agree, before it touches memory.
template <typename K, bool QUERY>
__global__ __launch_bounds__(256)
void pos_slots_kernel(const K *__restrict__ keys, const u64 *__restrict__ index, u32 shift, u64 n_index,
                      const uint8_t *__restrict__ bases, u64 n_bases, u32 k, u32 *__restrict__ slot_out,
                      const u64 *__restrict__ seq_start, u64 n_seq, const u64 *__restrict__ pos_start,
                      u32 *__restrict__ t_cov, u32 *__restrict__ n_per) {
  const u64 i0 = ((u64)blockIdx.x * blockDim.x + threadIdx.x) * LK_RUN;
  u64 cur = ~0ull;
  u32 cov = 0, per = 0;
  if (i0 < n_bases) {
    if (slot_out)
      for (int q = 0; q < LK_RUN; q++) if (i0 + q < n_bases) slot_out[i0 + q] = LK_NO_SLOT;
    lk_roll<K>(bases, n_bases, k, i0, [&](u64 s, K f, K r, bool) {
      const K c = KeyOps<K>::lt(r, f) ? r : f;
      u32 sl = lk_find_slot<K>(keys, index, shift, c, n_index);
      if (QUERY) {
        if (cur == ~0ull || s >= seq_start[cur + 1]) {
          if (cov) { atomicAdd(t_cov + cur, cov); atomicAdd(n_per + cur, per); }
          cov = 0; per = 0;
          cur = pos_seq_of(seq_start, n_seq, s);
        }
        if (s + k > seq_start[cur + 1]) sl = LK_NO_SLOT;            // a window must lie inside its sequence
        if (sl != LK_NO_SLOT && t_cov) { cov++; per += (u32)(pos_start[(u64)sl + 1] - pos_start[sl]); }
      }
      if (slot_out && sl != LK_NO_SLOT) slot_out[s] = sl;
    });
  }
  if constexpr (QUERY) {
    if (!t_cov) return;
    __shared__ u64 s_seq[4];
    __shared__ u32 s_cov[4], s_per[4];
    const u64 have = __ballot(cov != 0);
    u64 c0 = ~0ull;
    bool one = false;                                               // the wave's open sums belong to one sequence, c0
    if (have) {
      c0 = __shfl(cur, (int)__builtin_ctzll(have));
      one = __all(cov == 0 || cur == c0);
      if (one) {
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) { cov += __shfl_down(cov, d); per += __shfl_down(per, d); }
      } else if (cov) {
        atomicAdd(t_cov + cur, cov); atomicAdd(n_per + cur, per);
      }
    }
    if (lane_id() == 0) { s_seq[wave_id()] = one ? c0 : ~0ull; s_cov[wave_id()] = one ? cov : 0u; s_per[wave_id()] = one ? per : 0u; }
    __syncthreads();
    if (threadIdx.x == 0) {                                         // waves in stream order: equal sequences are neighbours
      u64 sq = ~0ull;
      u32 a = 0, b = 0;
      for (int w = 0; w < 4; w++) {
        if (s_seq[w] != sq) {
          if (sq != ~0ull && a) { atomicAdd(t_cov + sq, a); atomicAdd(n_per + sq, b); }
          sq = s_seq[w]; a = 0; b = 0;
        }
        a += s_cov[w]; b += s_per[w];
      }
      if (sq != ~0ull && a) { atomicAdd(t_cov + sq, a); atomicAdd(n_per + sq, b); }
    }
  }
}

// ---- (slot, payload) pairs in stream order: count per tile, scan, emit (mgc_compact.hpp) ------------------------------
constexpr int PP_TILE = (int)POS_PAIR_TILE;
template <bool EMIT>
__global__ __launch_bounds__(256)
void pos_pairs_kernel(const u32 *__restrict__ slot, u64 n, const u64 *__restrict__ seq_start, u64 n_seq,
                      u64 *__restrict__ tiles /*EMIT: exclusive bases*/, u64 *__restrict__ out_k, u32 *__restrict__ out_v) {
  const u64 base = (u64)blockIdx.x * PP_TILE + (u64)threadIdx.x * 8;
  u32 sl[8];
  u32 keep = 0;
#pragma unroll
  for (int q = 0; q < 8; q++) {
    const u64 i = base + q;
    sl[q] = i < n ? slot[i] : LK_NO_SLOT;
    keep |= (u32)(sl[q] != LK_NO_SLOT) << q;
  }
  u64 o;
  if (!compact_slot<256, EMIT>(__popc(keep), tiles, &o)) return;
  if (!keep) return;
  u64 sid = 0;
  if (seq_start) sid = pos_seq_of(seq_start, n_seq, base + (u32)(__ffs(keep) - 1));
#pragma unroll
  for (int q = 0; q < 8; q++)
    if ((keep >> q) & 1u) {
      const u64 i = base + q;
      u32 payload = (u32)i;
      if (seq_start) { while (sid + 1 < n_seq && seq_start[sid + 1] <= i) sid++; payload = (u32)sid; }
      out_k[o] = sl[q]; out_v[o] = payload; o++;
    }
}

// ---- pos_start from the boundaries of the sorted pairs ---------------------------------------------------------------------
// the first pair of every slot that has one writes its index; the slots without one take the next slot's (reverse min scan)
__global__ __launch_bounds__(256)
void pos_heads_kernel(const u64 *__restrict__ keys, u64 n, u64 *__restrict__ pos_start) {
  const u64 stride = (u64)gridDim.x * blockDim.x;
  for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const u64 s = keys[i];
    if (i == 0 || keys[i - 1] != s) pos_start[s] = i;
  }
}

__global__ __launch_bounds__(256)
void pos_list_stats_kernel(const u64 *__restrict__ pos_start, u64 n_table, u64 *__restrict__ stats) {
  __shared__ u64 s_used[4], s_max[4];
  const u64 stride = (u64)gridDim.x * blockDim.x;
  u64 used = 0, longest = 0;
  for (u64 s = (u64)blockIdx.x * blockDim.x + threadIdx.x; s < n_table; s += stride) {
    const u64 len = pos_start[s + 1] - pos_start[s];
    used += len != 0;
    longest = len > longest ? len : longest;
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    used += __shfl_down(used, d);
    const u64 m = __shfl_down(longest, d);
    longest = m > longest ? m : longest;
  }
  if (lane_id() == 0) { s_used[wave_id()] = used; s_max[wave_id()] = longest; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; w++) { used += s_used[w]; longest = s_max[w] > longest ? s_max[w] : longest; }
    if (used) atomicAdd(reinterpret_cast<unsigned long long *>(stats), (unsigned long long)used);
    if (longest) atomicMax(reinterpret_cast<unsigned long long *>(stats + 1), (unsigned long long)longest);
  }
}

// ---- per-slot sums of a batch's sorted (slot, query) pairs (position-lookup.C:272-288, 299-327) --------------------------
// heads[i] = 1 where (slot, query) differs from the pair before (:308); heads[n] = 0, so that the exclusive scan leaves the
// total there
__global__ __launch_bounds__(256)
void pos_query_heads_kernel(const u64 *__restrict__ keys, const u32 *__restrict__ vals, u64 n, u64 *__restrict__ heads) {
  const u64 stride = (u64)gridDim.x * blockDim.x;
  for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i <= n; i += stride)
    heads[i] = (i < n && (i == 0 || keys[i - 1] != keys[i] || vals[i - 1] != vals[i])) ? 1ull : 0ull;
}
// A slot's pairs are one run [b, e): hits += e - b, queries += heads_before[e] - heads_before[b].  The run's first pair adds the
// negative part and its last pair the positive one (mod 2^32), so nobody walks a run and a slot sees at most two adds however
// many hits it took.
__global__ __launch_bounds__(256)
void pos_slot_sums_kernel(const u64 *__restrict__ keys, u64 n, const u64 *__restrict__ heads_before, u32 *__restrict__ hits,
                          u32 *__restrict__ queries) {
  const u64 stride = (u64)gridDim.x * blockDim.x;
  for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const u64 s = keys[i];
    const bool first = i == 0 || keys[i - 1] != s, last = i + 1 == n || keys[i + 1] != s;
    if (!first && !last) continue;
    u32 h = 0, q = 0;
    if (first) { h -= (u32)i; if (queries) q -= (u32)heads_before[i]; }
    if (last)  { h += (u32)(i + 1); if (queries) q += (u32)heads_before[i + 1]; }
    if (hits) atomicAdd(hits + s, h);
    if (queries) atomicAdd(queries + s, q);
  }
}

// ---- gathers -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256)
void pos_gather_kernel(const u32 *__restrict__ slot, u64 n, const u32 *__restrict__ per_slot, u32 *__restrict__ out) {
  const u64 stride = (u64)gridDim.x * blockDim.x;
  for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const u32 s = slot[i];
    out[i] = s == LK_NO_SLOT ? 0u : per_slot[s];
  }
}

template <typename K>
__global__ __launch_bounds__(256)
void pos_find_kernel(const K *__restrict__ keys, const u64 *__restrict__ index, u32 shift, u64 n_index, const K *__restrict__ q, u64 n,
                     const u64 *__restrict__ pos_start, u64 *__restrict__ begin, u32 *__restrict__ count) {
  const u64 stride = (u64)gridDim.x * blockDim.x;
  for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const u32 s = lk_find_slot<K>(keys, index, shift, q[i], n_index);
    const u64 b = s == LK_NO_SLOT ? 0ull : pos_start[s];
    begin[i] = b;
    count[i] = s == LK_NO_SLOT ? 0u : (u32)(pos_start[(u64)s + 1] - b);
  }
}

// ================================================================================================
//  launchers
// ================================================================================================
static inline uint32_t pos_grid(uint64_t n) { uint64_t g = (n + 255) / 256; if (g > 65536) g = 65536; return (uint32_t)(g ? g : 1); }

PosTable pos_table_of(const mgc_lookup *t) {
  PosTable p;
  p.keys = t->d_keys.p; p.index = t->d_index.as<uint64_t>(); p.n = t->n; p.n_index = 1ull << t->index_bits;
  p.k = t->k; p.key_words = t->kw; p.shift = t->shift; p.device = t->device;
  return p;
}

template <typename K>
static hipError_t pos_slots_t(const PosTable &t, const uint8_t *d_bases, uint64_t n_bases, uint32_t *d_slot, const uint64_t *d_seq_start,
                              uint64_t n_seq, const uint64_t *d_pos_start, uint32_t *d_t_cov, uint32_t *d_n_per, hipStream_t st) {
  const uint64_t threads = (n_bases + LK_RUN - 1) / LK_RUN;
  const dim3 g((uint32_t)((threads + 255) / 256));
  const K *keys = reinterpret_cast<const K *>(t.keys);
  const u64 *index = reinterpret_cast<const u64 *>(t.index);
  if (d_seq_start)
    hipLaunchKernelGGL((pos_slots_kernel<K, true>), g, dim3(256), 0, st, keys, index, t.shift, (u64)t.n_index, d_bases, (u64)n_bases, t.k, d_slot,
                       reinterpret_cast<const u64 *>(d_seq_start), (u64)n_seq, reinterpret_cast<const u64 *>(d_pos_start), d_t_cov, d_n_per);
  else
    hipLaunchKernelGGL((pos_slots_kernel<K, false>), g, dim3(256), 0, st, keys, index, t.shift, (u64)t.n_index, d_bases, (u64)n_bases, t.k, d_slot,
                       (const u64 *)nullptr, (u64)0, (const u64 *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr);
  return hipGetLastError();
}

hipError_t launch_pos_slots(const PosTable &t, const uint8_t *d_bases, uint64_t n_bases, uint32_t *d_slot, const uint64_t *d_seq_start,
                            uint64_t n_seq, const uint64_t *d_pos_start, uint32_t *d_t_cov, uint32_t *d_n_per, hipStream_t st) {
  if (n_bases == 0) return hipSuccess;
  if (n_bases >> 32 || (d_seq_start && n_seq == 0) || (d_t_cov && (!d_n_per || !d_pos_start || !d_seq_start))) return hipErrorInvalidValue;
  if (t.key_words == 2) return pos_slots_t<K128>(t, d_bases, n_bases, d_slot, d_seq_start, n_seq, d_pos_start, d_t_cov, d_n_per, st);
  return pos_slots_t<u64>(t, d_bases, n_bases, d_slot, d_seq_start, n_seq, d_pos_start, d_t_cov, d_n_per, st);
}

static inline uint64_t pp_tiles(uint64_t n) { return (n + PP_TILE - 1) / PP_TILE; }
size_t pos_pairs_workspace_bytes(uint64_t n_bases) { return compact_ws_elems(pp_tiles(n_bases)) * sizeof(u64); }

hipError_t launch_pos_pairs_count(const uint32_t *d_slot, uint64_t n_bases, void *d_ws, hipStream_t st) {
  const uint64_t t = pp_tiles(n_bases);
  const CompactWs w = compact_ws_at(d_ws, t);
  if (t == 0) return hipMemsetAsync(w.total, 0, sizeof(u64), st);
  hipLaunchKernelGGL(pos_pairs_kernel<false>, dim3((uint32_t)t), dim3(256), 0, st, d_slot, (u64)n_bases, (const u64 *)nullptr, (u64)0, w.tiles,
                     (u64 *)nullptr, (u32 *)nullptr);
  return compact_scan(w, st);
}

hipError_t launch_pos_pairs_emit(const uint32_t *d_slot, uint64_t n_bases, const uint64_t *d_seq_start, uint64_t n_seq, void *d_ws,
                                 uint64_t *d_keys, uint32_t *d_vals, hipStream_t st) {
  const uint64_t t = pp_tiles(n_bases);
  if (t == 0) return hipSuccess;
  const CompactWs w = compact_ws_at(d_ws, t);
  hipLaunchKernelGGL(pos_pairs_kernel<true>, dim3((uint32_t)t), dim3(256), 0, st, d_slot, (u64)n_bases, reinterpret_cast<const u64 *>(d_seq_start),
                     (u64)n_seq, w.tiles, reinterpret_cast<u64 *>(d_keys), d_vals);
  return hipGetLastError();
}

size_t pos_starts_scratch_elems(uint64_t n_table) { return scan_scratch_elems(n_table + 1); }

hipError_t launch_pos_starts(const uint64_t *d_sorted_keys, uint64_t n_pairs, uint64_t n_table, uint64_t *d_pos_start, uint64_t *d_scratch,
                             hipStream_t st) {
  MGC_CHECK(hipMemsetAsync(d_pos_start, 0xFF, sizeof(u64) * (n_table + 1), st));
  if (n_pairs) {
    hipLaunchKernelGGL(pos_heads_kernel, dim3(pos_grid(n_pairs)), dim3(256), 0, st, reinterpret_cast<const u64 *>(d_sorted_keys), (u64)n_pairs,
                       reinterpret_cast<u64 *>(d_pos_start));
    MGC_CHECK(hipGetLastError());
  }
  return scan_u64_min_reverse(reinterpret_cast<u64 *>(d_pos_start), n_table + 1, reinterpret_cast<u64 *>(d_scratch), (u64)n_pairs, st);
}

hipError_t launch_pos_list_stats(const uint64_t *d_pos_start, uint64_t n_table, uint64_t *d_stats, hipStream_t st) {
  if (n_table == 0) return hipSuccess;
  hipLaunchKernelGGL(pos_list_stats_kernel, dim3(pos_grid(n_table)), dim3(256), 0, st, reinterpret_cast<const u64 *>(d_pos_start), (u64)n_table,
                     reinterpret_cast<u64 *>(d_stats));
  return hipGetLastError();
}

size_t pos_sums_scratch_elems(uint64_t n_pairs) { return scan_scratch_elems(n_pairs + 1); }

hipError_t launch_pos_slot_sums(const uint64_t *d_sorted_keys, const uint32_t *d_sorted_vals, uint64_t n_pairs, uint32_t *d_hits,
                                uint32_t *d_queries, uint64_t *d_heads, uint64_t *d_scratch, hipStream_t st) {
  if (n_pairs == 0 || (!d_hits && !d_queries)) return hipSuccess;
  if (n_pairs >> 32) return hipErrorInvalidValue;
  const u64 *keys = reinterpret_cast<const u64 *>(d_sorted_keys);
  u64 *heads = reinterpret_cast<u64 *>(d_heads);
  if (d_queries) {
    hipLaunchKernelGGL(pos_query_heads_kernel, dim3(pos_grid(n_pairs + 1)), dim3(256), 0, st, keys, d_sorted_vals, (u64)n_pairs, heads);
    MGC_CHECK(hipGetLastError());
    MGC_CHECK(scan_u64_exclusive(heads, n_pairs + 1, reinterpret_cast<u64 *>(d_scratch), nullptr, st));
  }
  hipLaunchKernelGGL(pos_slot_sums_kernel, dim3(pos_grid(n_pairs)), dim3(256), 0, st, keys, (u64)n_pairs, (const u64 *)heads, d_hits, d_queries);
  return hipGetLastError();
}

hipError_t launch_pos_gather(const uint32_t *d_slot, uint64_t n_bases, const uint32_t *d_per_slot, uint32_t *d_out, hipStream_t st) {
  if (n_bases == 0) return hipSuccess;
  hipLaunchKernelGGL(pos_gather_kernel, dim3(pos_grid(n_bases)), dim3(256), 0, st, d_slot, (u64)n_bases, d_per_slot, d_out);
  return hipGetLastError();
}

hipError_t launch_pos_find(const PosTable &t, const void *d_kmers, uint64_t n, const uint64_t *d_pos_start, uint64_t *d_begin,
                           uint32_t *d_count, hipStream_t st) {
  if (n == 0) return hipSuccess;
  const u64 *index = reinterpret_cast<const u64 *>(t.index);
  if (t.key_words == 2)
    hipLaunchKernelGGL(pos_find_kernel<K128>, dim3(pos_grid(n)), dim3(256), 0, st, reinterpret_cast<const K128 *>(t.keys), index, t.shift,
                       (u64)t.n_index, reinterpret_cast<const K128 *>(d_kmers), (u64)n, reinterpret_cast<const u64 *>(d_pos_start),
                       reinterpret_cast<u64 *>(d_begin), d_count);
  else
    hipLaunchKernelGGL(pos_find_kernel<u64>, dim3(pos_grid(n)), dim3(256), 0, st, reinterpret_cast<const u64 *>(t.keys), index, t.shift,
                       (u64)t.n_index, reinterpret_cast<const u64 *>(d_kmers), (u64)n, reinterpret_cast<const u64 *>(d_pos_start),
                       reinterpret_cast<u64 *>(d_begin), d_count);
  return hipGetLastError();
}

}  // namespace mgc
