/*
 * meryl_lookup.h -- C ABI of the exact k-mer lookup table: how meryl-lookup and Merqury
 * consume a counted database.
 *
 * Replaces, for loading and querying, the reference's
 *   merylExactLookup::estimateMemoryUsage / load(db, maxMemory, ..., minValue, maxValue)
 *   merylExactLookup::value(kmer) / exists(kmer) / nKmers()
 * [class in the absent meryl-utility; call sites src/meryl-lookup/meryl-lookup.C:36-100 (load),
 *  src/meryl-lookup/existence.C:63-82 (value(fmer) > 0 || value(rmer) > 0 per k-mer of a sequence, nKmers())].
 *
 * MI355X form: the table IS the database's own order -- the distinct k-mers ascending with their values, resident in
 * HBM, plus a direct index over their top bits (first k-mer of every 2^P-th part of the key space).  A lookup is
 * one index read and a binary search over the handful of k-mers that share the top bits: exact, no hashing, no extra
 * copy of the keys, 12 (20) B per k-mer + 8 B per index entry.  Queries come in batches that are already on the device:
 * explicit k-mers (mgc_lookup_values) or a base stream whose every window is looked up (mgc_lookup_stream,
 * mgc_lookup_existence -- the reference's -existence report; mgc_lookup_positions / mgc_lookup_report -- its -bed, -bed-runs,
 * -wig-count and -wig-depth reports, src/meryl-lookup/dump.C).
 */
#ifndef MERYL_LOOKUP_H
#define MERYL_LOOKUP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mgc_lookup mgc_lookup;

typedef struct mgc_lookup_info {
  uint32_t k, key_words, index_bits, reserved;
  uint64_t n_kmers;            /* merylExactLookup::nKmers(): k-mers kept after the value filter */
  uint64_t n_kmers_in_db;      /* before the filter */
  uint64_t device_bytes;       /* keys + values + index */
} mgc_lookup_info;

/* merylExactLookup::load (src/meryl-lookup/meryl-lookup.C:91): the k-mers of the database at `db_path` whose value v has
 * min_value <= v <= max_value (-min / -max of meryl-lookup; 0 and UINT64_MAX keep everything), decoded by `host_threads`
 * threads, uploaded and indexed on `device` (< 0: current).  NULL on failure; text via mgc_lookup_error(). */
mgc_lookup *mgc_lookup_load(const char *db_path, uint64_t min_value, uint64_t max_value, int device, int host_threads);

/* merylExactLookup::estimateMemoryUsage (src/meryl-lookup/meryl-lookup.C:62-73): what mgc_lookup_load of this database with this
 * value filter will hold on the device, WITHOUT loading it and without a device -- the number of k-mers kept comes from the
 * database's own value histogram (exact), the bytes from the table's layout (8 or 16 B per k-mer + 4 B per value + the top-bits
 * index).  0 on success; text of a failure: mgc_lookup_error(). */
int mgc_lookup_estimate(const char *db_path, uint64_t min_value, uint64_t max_value, mgc_lookup_info *info);

/* The same from a (k-mer, value) stream that is already in HBM (distinct, ascending: a count session's result, a merge):
 * no file round trip.  The arrays are copied. */
mgc_lookup *mgc_lookup_from_device(const void *d_keys, const uint32_t *d_values, uint64_t n, uint32_t k,
                                   uint64_t min_value, uint64_t max_value, int device);

void        mgc_lookup_free(mgc_lookup *t);
int         mgc_lookup_get_info(const mgc_lookup *t, mgc_lookup_info *info);
const char *mgc_lookup_error(void);

/* merylExactLookup::value() for n k-mers on the device (uint64, or {lo, hi} pairs for k > 32; looked up as given -- no
 * canonicalisation): d_values_out[i] = value, 0 if absent. */
int mgc_lookup_values(const mgc_lookup *t, const void *d_kmers, uint64_t n, uint32_t *d_values_out, void *stream);

/* Every k-mer window of a base stream (ASCII, '.' or any non-ACGT byte breaks a k-mer -- the stream mgc_push_bases
 * takes): d_values_out[i] = value of the k-mer STARTING at base i, looked up as the reference's lookups do --
 * value(fmer), or value(rmer) when the forward k-mer is absent (existence.C:73-76) -- and 0 where the k-mer is absent,
 * broken, or would run past the end.  d_values_out holds n_bases entries. */
int mgc_lookup_stream(const mgc_lookup *t, const uint8_t *d_bases, uint64_t n_bases, uint32_t *d_values_out, void *stream);

/* meryl-lookup -existence (src/meryl-lookup/existence.C:48-82): for each of the n_seq sequences -- sequence s is
 * bases[d_seq_start[s], d_seq_start[s+1]) of the stream -- the number of k-mers it holds (d_total[s]) and how many of
 * them are in the table (d_found[s]).  d_seq_start has n_seq + 1 device entries. */
int mgc_lookup_existence(const mgc_lookup *t, const uint8_t *d_bases, uint64_t n_bases, const uint64_t *d_seq_start,
                         uint64_t n_seq, uint64_t *d_total, uint64_t *d_found, void *stream);

/* ---- position reports over several tables (src/meryl-lookup/dump.C) ------------------------------------------------------
 * Windows are the reference's kmerIterator windows (k consecutive ACGT bases, either case; any other byte breaks them), f the
 * forward k-mer of a window and r its reverse complement.  Every table must have the same k; at most 32 tables. */
#define MGC_LOOKUP_MAX_TABLES 32

#define MGC_LOOKUP_PRESENCE 0   /* bit t: table t holds f or r                                      (dump.C:109-135) */
#define MGC_LOOKUP_COUNT    1   /* sum over the tables of value(f) + value(r), value(f) alone when f == r, in uint32 (it
                                   wraps mod 2^32)                                                   (dump.C:139-164) */
#define MGC_LOOKUP_DEPTH    2   /* at every BASE: the windows covering it that table 0 -- only table 0, as the code does; the
                                   help text says "any database" -- holds (f or r)                   (dump.C:175-244) */

/* Replaces processSequence (dump.C:89-245) for a whole base stream: d_out[i] (n_bases entries, device) is the `what` of the
 * window starting at base i (PRESENCE, COUNT; 0 where no window starts) or of base i (DEPTH). */
int mgc_lookup_positions(const mgc_lookup *const *tables, uint32_t n_tables, int what, const uint8_t *d_bases, uint64_t n_bases,
                         uint32_t *d_out, void *stream);

#define MGC_REPORT_BED       0  /* -bed      (dump.C:251-298): name \t p \t p+k [\t label] \n, p ascending, then table  */
#define MGC_REPORT_BED_RUNS  1  /* -bed-runs (dump.C:302-364): name \t bgn \t E+k [\t label] \n per maximal run of a table's
                                   flags, E = the first position AFTER the run (so the end is one past the last window's end:
                                   the help text's example, meryl-lookup-help.C:68-69, shows one less); E ascending, then table */
#define MGC_REPORT_WIG_COUNT 2  /* -wig-count (dump.C:368-405): variableStep chrom=name \n for every sequence, then
                                   p+1 \t count \n where the COUNT is not 0                          */
#define MGC_REPORT_WIG_DEPTH 3  /* -wig-depth: the same with the DEPTH                                */

/* Receives the report's text in order; nonzero stops the report (mgc_lookup_report returns MGC_ESTATE). */
typedef int (*mgc_lookup_write_cb)(const void *data, uint64_t n, void *user);

/* Replaces dumpExistence / outputSequence (dump.C:409-441) with its outputBED / outputBEDruns / outputWIG: the exact text of
 * `mode` for the n_seq sequences of the device base stream d_bases -- sequence s is bases [seq_start[s], seq_start[s+1]) with
 * positions counted from 0 at seq_start[s]; seq_start (host, n_seq + 1 entries) starts at 0, never decreases and ends at
 * n_bases, and every non-empty sequence ends with a byte that is not ACGT (the stream meryl-lookup builds: '.' after each).
 * names[s] is the sequence's identifier; labels[t] (n_labels of them, may be 0) is appended to table t's -bed lines.  Labels
 * are "present" when at least one is non-empty (meryl-lookup.C:27-31): without them only "found in any table" is kept
 * (dump.C:127-131).  The WIG modes take no labels.  The text goes to write_cb as consecutive pieces of at most chunk_bytes;
 * it is formatted on the device over ranges of positions, each piece copied back through pinned memory while the next one is
 * formatted.  Device memory: O(n_bases) plus two staging buffers of chunk_bytes.  MGC_EINVAL: tables of different k, more
 * than 32 tables, chunk_bytes shorter than the longest line the report can hold, a stream that breaks the rules above. */
int mgc_lookup_report(const mgc_lookup *const *tables, uint32_t n_tables, int mode, const char *const *labels, uint32_t n_labels,
                      const uint8_t *d_bases, uint64_t n_bases, const uint64_t *seq_start, const char *const *names, uint64_t n_seq,
                      uint64_t chunk_bytes, mgc_lookup_write_cb write_cb, void *user);

/* ---- read filtering: meryl-lookup -include / -exclude (src/meryl-lookup/include-exclude.C) --------------------------------------
 * Records are taken in order, record i of the first input together with record i of the second when there is one (:44-58).
 * found = the windows of the first sequence with value(fmer) > 0 || value(rmer) > 0 (:64-78) plus those of the second (:92-93);
 * with skip_first = 23 (-10x) the windows of the FIRST input that begin before base 23 are not counted (:71).  The pair is
 * written when found > 0 (INCLUDE) or found == 0 (EXCLUDE) (:124-125), each sequence to its own output, as
 *   >ident nKmers=found \n bases \n                       when the record has no qualities
 *   @ident nKmers=found \n bases \n + \n qualities \n     otherwise                                         (:107-108)
 * ident is the header up to the first blank or tab; the bases are the sequence lines joined (multi-line FASTA; \r, \n, blanks
 * and tabs dropped, every other byte kept); FASTQ is four lines per record -- anything else is MGC_EFORMAT. */
#define MGC_FILTER_INCLUDE 0
#define MGC_FILTER_EXCLUDE 1
typedef struct mgc_filter_result {
  uint64_t n_records, n_kept;      /* records (pairs) processed / written */
  uint64_t consumed[2];            /* bytes of each input's piece that belonged to those records */
  uint64_t out_bytes[2];           /* text written per output -- or needed, when an output buffer was too small */
  uint32_t format[2];              /* MGC_TEXT_FASTA / MGC_TEXT_FASTQ (meryl_gpu_count.h) per input, from its first byte; 0: empty */
} mgc_filter_result;

/* One step, device in, device out.  d_text[i] / n_text[i]: a piece of raw FASTA/FASTQ text of input i (n_inputs 1 or 2) that
 * begins at a record start.  final: the pieces end their inputs -- a last record without a line end is complete, and two inputs
 * with different numbers of records are MGC_EINVAL (the message names both counts).  Not final: the last record of a piece
 * is complete only when another record start follows it; with two inputs min(records_1, records_2) records of each are
 * processed, and res->consumed tells where the caller's next pieces begin.  The kept text goes to d_out[i] (out_cap[i] bytes).
 * When an output is too small NOTHING is written, res->out_bytes holds the sizes needed and the call returns MGC_EINVAL
 * (its "capacity" meaning); d_out may be NULL to ask for the sizes.  The text is never copied to the host. */
int mgc_lookup_filter_text(const mgc_lookup *t, int mode, uint32_t skip_first, uint32_t n_inputs, const uint8_t *const d_text[2],
                           const uint64_t n_text[2], int final, uint8_t *const d_out[2], const uint64_t out_cap[2],
                           mgc_filter_result *res, void *stream);

/* Whole files (path2, out2 NULL: one input): both are read through msr_read_text (plain, gzip, BGZF, "-") into pinned
 * buffers in pieces of about batch_bytes (0: 64 MiB), what a step did not consume is carried into the next piece, a piece
 * grows when one record is longer than it, and the kept text is handed to the callbacks in order.  Inputs with different
 * numbers of records: MGC_EINVAL naming both counts, after the common records have been written. */
int mgc_lookup_filter_files(const mgc_lookup *t, int mode, uint32_t skip_first, const char *path1, const char *path2,
                            uint64_t batch_bytes, mgc_lookup_write_cb out1, void *user1, mgc_lookup_write_cb out2, void *user2,
                            mgc_filter_result *totals);

#ifdef __cplusplus
}
#endif
#endif /* MERYL_LOOKUP_H */
