// mgc_import_dev.hpp -- launch interface between the C-ABI layer of include/meryl_import.h and include/meryl_import_labelled.h
// (mgc_import.cpp) and the gfx950 kernels of mgc_import.hip.  Not installed.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace mgc {

// ---- text -> records in input order.  The state type names the dialect: ImportState `kmer value` (meryl 1), Import2State
//      `kmer value label` (meryl 2, include/meryl_import_labelled.h) ---------------------------------------------------------
// what the parser keeps on the device from chunk to chunk, and what its count pass found in the current chunk
struct ImportState {
  uint64_t lines_seen, records_seen;       // chunks already committed
  uint64_t first_bad;                      // (1-based line << 3) | MGC_IMPORT_BAD_*; ~0: none
  uint32_t persistent, pad0;               // meryl-import.C:175
  uint64_t chunk_lines, chunk_records;     // the chunk the count pass saw last
  uint32_t chunk_has, chunk_val;           // it holds a `#` line / the number of its last one
  uint64_t chunk_bad;                      // (byte offset of the line << 3) | kind; ~0: none
};
struct Import2State {
  uint64_t lines_seen, records_seen;       // chunks already committed
  uint64_t first_bad;                      // (1-based line << 3) | MGC_IMPORT_BAD_*; ~0: none
  uint64_t persistent_label;               // meryl2-import/meryl-import.C:177
  uint32_t persistent_value, pad0;         // :176
  uint64_t chunk_lines, chunk_records;     // the chunk the count pass saw last
  uint64_t chunk_lab;                      // the number of its last `label=` line
  uint32_t chunk_vhas, chunk_val;          // it holds a `value=` line / the number of its last one
  uint32_t chunk_lhas, pad1;               // it holds a `label=` line
  uint64_t chunk_bad;                      // (byte offset of the line << 3) | kind; ~0: none
};
// State: ImportState (label_width and d_labels are not read) or Import2State; defined for these two in mgc_import.hip
template <typename State> size_t     parse_workspace_bytes(uint64_t n_text);
template <typename State> hipError_t launch_parse_begin(State *d_state, hipStream_t st);
template <typename State> hipError_t launch_parse_count(const uint8_t *d_text, uint64_t n, uint32_t k, uint32_t label_width, State *d_state,
                                                        void *d_ws, hipStream_t st);
template <typename State> hipError_t launch_parse_emit(const uint8_t *d_text, uint64_t n, uint32_t k, int mode, uint32_t label_width,
                                                       State *d_state, void *d_ws, void *d_keys, uint32_t *d_values, uint64_t *d_labels,
                                                       hipStream_t st);

// ---- (key, value) pairs: stable low-digit-first radix sort, 8-bit digits ---------------------------------------------
size_t     sort_pairs_workspace_bytes(uint64_t n);
hipError_t launch_sort_pairs(void *d_keys, uint32_t *d_vals, void *d_alt_keys, uint32_t *d_alt_vals, uint64_t n, uint32_t key_words,
                             uint32_t begin_bit, uint32_t end_bit, void *d_ws, int *result_in_alt, hipStream_t st);

// ---- triples: the pair sort over (key, record number), then a gather; the result is always in the alternates -----------------
size_t     sort_triples_workspace_bytes(uint64_t n);
hipError_t launch_sort_triples(void *d_keys, uint32_t *d_vals, uint64_t *d_labs, void *d_alt_keys, uint32_t *d_alt_vals, uint64_t *d_alt_labs,
                               uint64_t n, uint32_t key_words, uint32_t begin_bit, uint32_t end_bit, void *d_ws, int *result_in_alt,
                               hipStream_t st);

// ---- sorted pairs (d_labs NULL) or triples -> distinct keys + wrapped uint32 value sums [+ label sums modulo 2^label_width] -----
size_t     reduce_pairs_workspace_bytes(uint64_t n);
size_t     reduce_triples_workspace_bytes(uint64_t n);
// leaves the number of distinct keys in the first uint64 of the workspace
hipError_t launch_reduce_count(const void *d_keys, const uint32_t *d_vals, const uint64_t *d_labs, uint64_t n, uint32_t key_words, void *d_ws,
                               hipStream_t st);
hipError_t launch_reduce_emit(const void *d_keys, const uint32_t *d_vals, const uint64_t *d_labs, uint64_t n, uint32_t key_words,
                              uint32_t label_width, void *d_ws, void *d_out_keys, uint32_t *d_out_vals, uint64_t *d_out_labs, hipStream_t st);

}  // namespace mgc
