// mgc_stream_geom.hpp -- the geometry of hash_count_stream_kernel (mgc_finish.hip): how an n-key sub-bucket is cut into chunks, how
// many table slots it gets, and where a wave's queue of pending keys lies in LDS.  The kernel takes all of it from here once per
// sub-bucket, and so can a plain host program: tests/host/stream_geom_host.cpp walks every n of both table sizes.  No dependency
// but <cstdint>.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MGC_GEOM_FN __host__ __device__ __forceinline__
#else
#define MGC_GEOM_FN inline
#endif

namespace mgc {

// chunks of an n-key sub-bucket: 1..3 of them, evenly cut, whole rows of `block` keys, none above `ch` keys (n <= max_size < 3 * ch);
// 0: not counted by this kernel (empty, or above max_size: the streaming launch's)
MGC_GEOM_FN uint32_t stream_chunk_size(uint32_t n, uint32_t max_size, uint32_t ch, uint32_t block) {
  if (n == 0u || n > max_size) return 0u;
  uint32_t per = n;
  if (n > 2u * ch) per = ((n + 2u) * 43691u) >> 17;                  // ceil(n / 3)  (exact below 2^15)
  else if (n > ch) per = (n + 1u) >> 1;
  return (per + block - 1u) & ~(block - 1u);
}

// table slots of an n-key sub-bucket: the power of two >= 2n (D is not known, the keys bound it), 256 .. table
MGC_GEOM_FN uint32_t stream_slots_for(uint32_t n, uint32_t table) {
  if (2u * n <= 256u) return 256u;
  const uint32_t s = 1u << (32 - __builtin_clz(2u * n - 1u));
  return s < table ? s : table;
}

// the per-wave queue of keys whose first probe met another suffix: STREAM_QCAP keys per wave, wave w's segment behind wave w - 1's.
// A row of 64 lanes appends at most 64 keys, and the queue is drained before an append that would not fit, so
// stream_queue_must_drain() is the only capacity test: after a drain (fill == 0) every row fits.
constexpr uint32_t STREAM_QCAP = 128u;
MGC_GEOM_FN bool     stream_queue_must_drain(uint32_t fill, uint32_t row_keys) { return fill + row_keys > STREAM_QCAP; }
MGC_GEOM_FN uint32_t stream_queue_index(uint32_t wave, uint32_t fill, uint32_t rank_in_row) { return wave * STREAM_QCAP + fill + rank_in_row; }

}  // namespace mgc
