// mgc_compact.hpp -- the device half of every order-preserving compaction ("keep some of the items, in order"): count the kept
// items per tile, scan the tile counts (compact_scan, mgc_common.hpp), emit each tile at its base.  One kernel template with a
// `bool EMIT` parameter is both passes: it evaluates its predicate once and calls compact_slot, so the emit pass cannot write
// more than the count pass reserved.  merge_kernel, select_kernel and merge_many_kernel (mgc_merge.hip, mgc_merge_many.hip) have
// the same shape but keep their own three lines after the scan: through the helper their instructions came out reordered, and
// those kernels are timed.  Not installed.
#pragma once
#include "mgc_common.hpp"

namespace mgc {

// Every thread of the block calls it once, after it knows how many of its items it keeps.
//   count pass: stores the tile's total in tiles[blockIdx.x] and returns false -- the kernel returns.
//   emit pass : tiles[] holds the exclusive bases by now; *o = where this thread's first kept item goes; returns true.
// *tile_total (may be null): the kept items of the whole tile, in either pass.
template <int BLOCK, bool EMIT>
__device__ __forceinline__ bool compact_slot(u32 kept, u64 *tiles, u64 *o, u32 *tile_total = nullptr) {
  __shared__ u32 s_tmp[BLOCK / 64 + 1];
  u32 tot;
  const u32 off = block_excl_scan<BLOCK, u32>(kept, s_tmp, &tot);
  if (tile_total) *tile_total = tot;
  if constexpr (!EMIT) {
    if (threadIdx.x == 0) tiles[blockIdx.x] = tot;
    return false;
  } else {
    *o = tiles[blockIdx.x] + off;
    return true;
  }
}

}  // namespace mgc
