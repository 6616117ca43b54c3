// mgc_import_dev.hpp -- launch interface between the C-ABI layer of include/meryl_import.h (mgc_import.cpp) and the gfx950
// kernels of mgc_import.hip.  Not installed.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace mgc {

// ---- `kmer value` text -> (k-mer, value) pairs ---------------------------------------------------------------------
// what the parser keeps on the device from chunk to chunk, and what its count pass found in the current chunk
struct ImportState {
  uint64_t lines_seen, records_seen;       // chunks already committed
  uint64_t first_bad;                      // (1-based line << 3) | MGC_IMPORT_BAD_*; ~0: none
  uint32_t persistent, pad0;               // meryl-import.C:175
  uint64_t chunk_lines, chunk_records;     // the chunk the count pass saw last
  uint32_t chunk_has, chunk_val;           // it holds a `#` line / the number of its last one
  uint64_t chunk_bad;                      // (byte offset of the line << 3) | kind; ~0: none
};
size_t     import_parse_workspace_bytes(uint64_t n_text);
hipError_t launch_import_begin(ImportState *d_state, hipStream_t st);
hipError_t launch_import_parse_count(const uint8_t *d_text, uint64_t n, uint32_t k, ImportState *d_state, void *d_ws, hipStream_t st);
hipError_t launch_import_parse_emit(const uint8_t *d_text, uint64_t n, uint32_t k, int mode, ImportState *d_state, void *d_ws,
                                    void *d_keys, uint32_t *d_values, hipStream_t st);

// ---- (key, value) pairs: stable low-digit-first radix sort, 8-bit digits ---------------------------------------------
size_t     sort_pairs_workspace_bytes(uint64_t n);
hipError_t launch_sort_pairs(void *d_keys, uint32_t *d_vals, void *d_alt_keys, uint32_t *d_alt_vals, uint64_t n, uint32_t key_words,
                             uint32_t begin_bit, uint32_t end_bit, void *d_ws, int *result_in_alt, hipStream_t st);

// ---- sorted pairs -> distinct keys + wrapped uint32 sums --------------------------------------------------------------
size_t     reduce_pairs_workspace_bytes(uint64_t n);
// leaves the number of distinct keys in the first uint64 of the workspace
hipError_t launch_reduce_pairs_count(const void *d_keys, const uint32_t *d_vals, uint64_t n, uint32_t key_words, void *d_ws, hipStream_t st);
hipError_t launch_reduce_pairs_emit(const void *d_keys, const uint32_t *d_vals, uint64_t n, uint32_t key_words, void *d_ws,
                                    void *d_out_keys, uint32_t *d_out_vals, hipStream_t st);

}  // namespace mgc
