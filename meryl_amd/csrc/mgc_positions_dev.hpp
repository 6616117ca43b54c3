// mgc_positions_dev.hpp -- launch interface between the C-ABI layer of include/meryl_positions.h (mgc_positions.cpp) and the
// gfx950 kernels of mgc_positions.hip.  Not installed.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <string>

struct mgc_lookup;

namespace mgc {

void lk_set_error(const std::string &m);            // the text mgc_lookup_error() returns (mgc_lookup.hip)

// what the kernels need of a lookup table (mgc_lookup_dev.hpp keeps the handle itself among the .hip files)
struct PosTable { const void *keys; const uint64_t *index; uint64_t n, n_index; uint32_t k, key_words, shift; int device; };
PosTable pos_table_of(const mgc_lookup *t);

constexpr uint32_t POS_NONE = 0xFFFFFFFFu;
constexpr uint64_t POS_PAIR_TILE = 256 * 8;         // items per workgroup of the pair compaction

// ---- slots of every window of a base stream ----------------------------------------------------------------------------
// d_slot[i] (n_bases entries) = slot of the canonical k-mer of the window beginning at base i, POS_NONE where there is none.
// With d_seq_start (n_seq + 1 device entries, n_seq >= 1) the stream is a query batch: a window must lie inside its sequence,
// and with d_t_cov / d_n_per (zeroed by the caller) the hits of every sequence and their summed list lengths
// (d_pos_start[slot + 1] - d_pos_start[slot]) are added up.  d_slot may be null then (only the sums are wanted).
hipError_t launch_pos_slots(const PosTable &t, const uint8_t *d_bases, uint64_t n_bases, uint32_t *d_slot,
                            const uint64_t *d_seq_start, uint64_t n_seq, const uint64_t *d_pos_start, uint32_t *d_t_cov,
                            uint32_t *d_n_per, hipStream_t st);

// ---- (slot, payload) pairs of the windows that have a slot, in stream order ---------------------------------------------
// payload: the window's offset (d_seq_start null) or the index of its sequence.  Count, then emit: the count pass leaves the
// number of pairs in the first uint64 of the workspace.
size_t     pos_pairs_workspace_bytes(uint64_t n_bases);
hipError_t launch_pos_pairs_count(const uint32_t *d_slot, uint64_t n_bases, void *d_ws, hipStream_t st);
hipError_t launch_pos_pairs_emit(const uint32_t *d_slot, uint64_t n_bases, const uint64_t *d_seq_start, uint64_t n_seq, void *d_ws,
                                 uint64_t *d_keys, uint32_t *d_vals, hipStream_t st);

// ---- sorted pairs -> pos_start --------------------------------------------------------------------------------------------
// d_pos_start[s] (n_table + 1 entries) = first sorted pair whose slot is >= s; d_scratch: pos_starts_scratch_elems uint64
size_t     pos_starts_scratch_elems(uint64_t n_table);
hipError_t launch_pos_starts(const uint64_t *d_sorted_keys, uint64_t n_pairs, uint64_t n_table, uint64_t *d_pos_start,
                             uint64_t *d_scratch, hipStream_t st);
// d_stats[0] += slots with a non-empty list, d_stats[1] = max(d_stats[1], longest list)   (zeroed by the caller)
hipError_t launch_pos_list_stats(const uint64_t *d_pos_start, uint64_t n_table, uint64_t *d_stats, hipStream_t st);

// ---- sorted (slot, query) pairs of a batch -> per-slot sums -------------------------------------------------------------
// d_hits[slot] += pairs of the slot; d_queries[slot] += distinct (slot, query) among them (the sort is stable and the queries
// were generated ascending, so equal ones are adjacent).  Either may be null.  d_heads: n_pairs + 1 uint64 of scratch (the
// other key buffer of the sort), d_scratch: pos_sums_scratch_elems uint64.
size_t     pos_sums_scratch_elems(uint64_t n_pairs);
hipError_t launch_pos_slot_sums(const uint64_t *d_sorted_keys, const uint32_t *d_sorted_vals, uint64_t n_pairs, uint32_t *d_hits,
                                uint32_t *d_queries, uint64_t *d_heads, uint64_t *d_scratch, hipStream_t st);

// ---- gathers ------------------------------------------------------------------------------------------------------------------
// d_out[i] = d_slot[i] == POS_NONE ? 0 : d_per_slot[d_slot[i]]
hipError_t launch_pos_gather(const uint32_t *d_slot, uint64_t n_bases, const uint32_t *d_per_slot, uint32_t *d_out, hipStream_t st);
// explicit k-mers, as given: d_begin[i] / d_count[i] = begin and length of the list, 0 / 0 when absent
hipError_t launch_pos_find(const PosTable &t, const void *d_kmers, uint64_t n, const uint64_t *d_pos_start, uint64_t *d_begin,
                           uint32_t *d_count, hipStream_t st);

}  // namespace mgc
