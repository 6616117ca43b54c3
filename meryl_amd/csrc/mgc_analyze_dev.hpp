// mgc_analyze_dev.hpp -- launch interface between the C-ABI layer of include/meryl_analyze.h (mgc_analyze.cpp) and the gfx950
// kernels of mgc_analyze.hip.  Not installed.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace mgc {

constexpr uint32_t ANALYZE_SCORES = 65;                 // rows of a histogram in device memory: scores 0..64
constexpr uint32_t ANALYZE_HISTS  = 3;                  // forward, reverse, combined (-gc accumulates the forward one only)

// histograms a report type accumulates on the device: -gc 1 (AT is GC with the score mirrored), -ga / -gt 3
inline uint32_t analyze_device_hists(int type) { return type == 0 ? 1u : 3u; }

// an overflow entry: histogram << 39 | score << 32 | value
constexpr uint32_t ANALYZE_KEY_BITS = 41;
inline uint64_t analyze_pack(uint32_t h, uint32_t score, uint32_t value) { return ((uint64_t)h << 39) | ((uint64_t)score << 32) | value; }

// d_fscore[n], d_rscore[n] <- the scores of d_keys[n] (key_words from k)
hipError_t launch_analyze_scores(const void *d_keys, uint64_t n, uint32_t k, int type, uint8_t *d_fscore, uint8_t *d_rscore, hipStream_t st);

// One pass over n <= 2^31 entries.  Values below `dense` (0, or MGC_ANALYZE_DENSE_VALUES) are added to
// d_dense[ANALYZE_HISTS][ANALYZE_SCORES][MGC_ANALYZE_DENSE_VALUES] (uint64) when do_dense is set; every other value appends one
// packed entry per histogram to d_list.  d_list_n[0] (zeroed by the caller) ends up as the number of entries the pass
// produced, whether or not they fitted list_cap: entries beyond list_cap are NOT written, and the caller repeats the pass
// with do_dense = false and a list that holds them all.
hipError_t launch_analyze_hist(const void *d_keys, const uint32_t *d_values, uint64_t n, uint32_t k, int type, uint32_t dense, bool do_dense,
                               uint64_t *d_dense, uint64_t *d_list, uint64_t list_cap, uint64_t *d_list_n, uint32_t n_cus, hipStream_t st);

}  // namespace mgc
