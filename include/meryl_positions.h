/*
 * meryl_positions.h -- C ABI of the k-mer position index and of query painting: the sixth program of the reference's
 * src/main.mk, position-lookup (src/meryl-lookup/position-lookup.C), on the device.
 *
 * Replaces
 *   merylExactLookup::index(kmer) / loadPositions(sequence) / _posStart / _posData
 * [class in the absent meryl-utility].  What loadPositions stores is therefore READ OFF ITS CALL SITES,
 * src/meryl-lookup/position-lookup.C:140-141 (load, loadPositions), :197-203 (index(min(fmer, rmer)) per query window),
 * :248-259 (-hpq), :272-288 (-mpb), :299-327 (-qpb); that reading is the contract here:
 *
 *   slot      the rank of a k-mer in the lookup table (index(cmer), after the table's -min / -max filter).  The reference
 *             keeps it in a uint32 (hit_s::refPos): a table of more than 2^32 - 2 k-mers is MGC_EINVAL, and so is a
 *             reference of 2^32 bases or more.
 *   window    the kmerIterator windows of meryl_lookup.h: k consecutive ACGT bases, either case, any other byte breaks them.
 *             ONLY the canonical k-mer min(fmer, rmer) is looked up (:198): a window whose canonical k-mer is not in the
 *             table is a miss even when the other strand's k-mer is (a count-forward database) -- unlike mgc_lookup_stream.
 *   list      the position list of a slot: the begin offsets, in the reference base stream, of every reference window whose
 *             canonical k-mer has that slot, ascending; both strands feed one list.  n_pos(slot) is its length; it may be 0.
 *
 * The one deliberate divergence: the reference takes a list's length from the k-mer's VALUE (valueAtIndex, :252), which is
 * only defined when the database is the count of that very reference -- there value = n_pos and the two agree exactly.
 * Everywhere else n_pos is used.
 *
 * Coordinates: the reference's paint arrays ignore refID and fold every sequence onto one axis; here everything is an offset
 * into the reference base STREAM (the sequences one after the other, '.' after each, as every other stream of this library).
 *
 * MI355X form: ref_slot (4 B per reference base: the slot of the window beginning there), pos_start (8 B per table k-mer + 8)
 * and pos_data (4 B per placed window), all resident in HBM.  Every reference base belongs to at most one slot, so painting
 * is: per-slot sums H (hits) and Q (distinct query sequences) from the sorted (slot, query) pairs of a batch, then a GATHER
 * mers[base] = H[ref_slot[base]] -- O(hits + reference), exact, no loop over position lists and no contended atomics.
 * Errors: the codes of meryl_gpu_count.h, text via mgc_lookup_error().
 */
#ifndef MERYL_POSITIONS_H
#define MERYL_POSITIONS_H

#include <stddef.h>
#include <stdint.h>

#include "meryl_lookup.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mgc_posidx mgc_posidx;
typedef struct mgc_paint  mgc_paint;

#define MGC_POS_NONE 0xFFFFFFFFu   /* ref_slot of a base where no window begins, or whose canonical k-mer is not in the table */

typedef struct mgc_posidx_info {
  uint32_t k, reserved;
  uint64_t n_kmers;            /* k-mers of the table = slots */
  uint64_t n_ref_bases;        /* bases of the reference stream */
  uint64_t n_placed;           /* reference windows placed = entries of pos_data */
  uint64_t n_slots_used;       /* slots with a non-empty list */
  uint64_t longest_list;
  uint64_t device_bytes;       /* ref_slot + pos_start + pos_data */
} mgc_posidx_info;

/* loadPositions (:141) over a reference base stream that is already on the device.  The table must outlive the index.
 * NULL on failure.  MGC_EINVAL cases (no device is touched): no table, no bases, n_bases >= 2^32, more than 2^32 - 2 k-mers. */
mgc_posidx *mgc_posidx_build(const mgc_lookup *table, const uint8_t *d_ref_bases, uint64_t n_bases, void *stream);
void        mgc_posidx_free(mgc_posidx *idx);
int         mgc_posidx_get_info(const mgc_posidx *idx, mgc_posidx_info *info);

/* Borrowed device pointers, valid until mgc_posidx_free: ref_slot[n_ref_bases] (uint32, MGC_POS_NONE), pos_start[n_kmers + 1]
 * (uint64), pos_data[n_placed] (uint32 offsets; list of slot s = pos_data[pos_start[s], pos_start[s + 1])).  Any may be NULL. */
int mgc_posidx_arrays(const mgc_posidx *idx, const uint32_t **d_ref_slot, const uint64_t **d_pos_start, const uint32_t **d_pos_data);

/* n k-mers on the device (uint64, or {lo, hi} pairs for k > 32), looked up AS GIVEN -- not canonicalised, like
 * mgc_lookup_values: d_begin[i] = where its list begins in pos_data, d_count[i] = its length; an absent k-mer: 0, 0. */
int mgc_posidx_find(const mgc_posidx *idx, const void *d_kmers, uint64_t n, uint64_t *d_begin, uint32_t *d_count, void *stream);

#define MGC_PAINT_HITS    1u   /* -hpq (:241-266): per query sequence tCov = its windows that hit, nPer = sum of n_pos over them */
#define MGC_PAINT_MERS    2u   /* -mpb (:271-289): per reference base, the query windows that hit the k-mer beginning there */
#define MGC_PAINT_QUERIES 4u   /* -qpb (:294-328): per reference base, the distinct query SEQUENCES that hit that k-mer */

/* An accumulator over one index (which must outlive it); `what` is a mask of MGC_PAINT_*.  NULL on failure. */
mgc_paint *mgc_paint_open(const mgc_posidx *idx, uint32_t what);
void       mgc_paint_close(mgc_paint *p);

/* One batch of whole query sequences: sequence s is bases [d_seq_start[s], d_seq_start[s + 1]) (device, n_seq + 1 entries,
 * the rules of mgc_lookup_existence) and d_seq_start[n_seq] must be n_bases -- MGC_EINVAL otherwise; of the argument checks
 * this one alone reads the device (that one entry).  d_n_per / d_t_cov (n_seq uint32 each, they wrap as the reference's do)
 * receive -hpq's columns and may be NULL without MGC_PAINT_HITS.  The per-base results accumulate over the calls; they do not
 * depend on how the queries are split into calls, since a sequence never spans two.  A batch holds fewer than 2^32 bases.
 * n_seq == 0 is a no-op.  The call returns after the batch is done (it sizes its buffers from the number of hits). */
int mgc_paint_add(mgc_paint *p, const uint8_t *d_bases, uint64_t n_bases, const uint64_t *d_seq_start, uint64_t n_seq,
                  uint32_t *d_n_per, uint32_t *d_t_cov, void *stream);

/* which: MGC_PAINT_MERS or MGC_PAINT_QUERIES (opened); d_out[n_ref_bases] uint32, 0 where no window begins or it missed. */
int mgc_paint_get(const mgc_paint *p, uint32_t which, uint32_t *d_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MERYL_POSITIONS_H */
