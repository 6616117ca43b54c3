/*
 * meryl_analyze.h -- C ABI of `meryl-analyze`: composition histograms over every (k-mer, value) of a database, on the device.
 *
 * Replaces the reference's src/meryl-analyze/meryl-analyze.C: histGC (:154-237), histGA (:240-337), histGT (:340-439) and
 * printHist (:139-152).  The reference walks the database on one thread (merylFileReader::nextMer), scores the 2-bit code of
 * theFMer() -- the stored k-mer as it is, nothing is reverse-complemented -- and inserts the value into one std::map per
 * (histogram, score).  Here the (k-mer, value) arrays are scored by one thread per k-mer and counted into histograms keyed
 * by (histogram, score, value): values below MGC_ANALYZE_DENSE_VALUES in per-workgroup LDS tables flushed once with 64-bit
 * adds, every other value as a packed key in an overflow list that the library's radix sort and run-length count reduce.
 * The result is exact for any value distribution: nothing is capped, nothing is dropped.
 *
 * Scores (code A0 C1 T2 G3):
 *   MGC_ANALYZE_GC  forward = bases that are C or G (:176-201), reverse = bases that are A or T = k - forward.
 *   MGC_ANALYZE_GA  every base belongs to the forward alphabet {A, G} or to the reverse alphabet {T, C}; the k-mer splits into
 *                   maximal runs that alternate between the two.  forward = summed length of the {A, G} runs that hold BOTH
 *                   letters, reverse = the same over the {T, C} runs (:262-299), combined = max(forward, reverse) (:314-320).
 *   MGC_ANALYZE_GT  the same with forward {G, T} and reverse {A, C} (:364-401, :416-422).
 *
 * Return codes, device pointers and `stream` follow include/meryl_gpu_count.h; failure text: mgc_analyze_error().
 */
#ifndef MERYL_ANALYZE_H
#define MERYL_ANALYZE_H

#include <stddef.h>
#include <stdint.h>

#include "meryl_gpu_count.h"

#ifdef __cplusplus
extern "C" {
#endif

/* report type (the -gc / -ga / -gt of meryl-analyze.C:462-469) */
#define MGC_ANALYZE_GC 0
#define MGC_ANALYZE_GA 1
#define MGC_ANALYZE_GT 2

/* which histogram of a report.  -gc: forward = GC, reverse = AT, no combined one.  -ga: GA, TC, GA_TC.  -gt: GT, AC, GT_AC. */
#define MGC_ANALYZE_FORWARD  0
#define MGC_ANALYZE_REVERSE  1
#define MGC_ANALYZE_COMBINED 2

#define MGC_ANALYZE_MAX_K 64
/* Values below this bound are counted in the dense tier (LDS tables of (k + 1) scores x this many values per histogram: at
 * k = 64 three histograms take 74,880 bytes, two workgroups per CU; at k = 21 25,344 bytes); a value at or above it goes
 * through the overflow list.  Both tiers give the same rows. */
#define MGC_ANALYZE_DENSE_VALUES 96

/* The scoring loops of :176-201 / :262-299 / :364-401 on their own: d_keys[n] (uint64, or {lo,hi} for k > 32: what a
 * count session's result and the database decoder hold) -> d_fscore[n], d_rscore[n], one byte each.
 * Asynchronous on `stream`. */
int mgc_dev_analyze_scores(const void *d_keys, uint64_t n, uint32_t k, int type, uint8_t *d_fscore, uint8_t *d_rscore, void *stream);

/* An accumulator of one report type for k-mers of one size, on one device (< 0: the current one).  Opening it does not
 * touch the device; the first mgc_analyze_add_* does. */
typedef struct mgc_analyze mgc_analyze;
int mgc_analyze_open(uint32_t k, int type, int device, mgc_analyze **a);
void mgc_analyze_close(mgc_analyze *a);

/* The while (nextMer()) loop of :171-223 / :257-322 / :359-424 over n (k-mer, value) entries in device memory: every entry
 * is one insertion into each histogram of the report.  May be called any number of times; returns once the entries are
 * counted (the arrays are not needed afterwards). */
int mgc_analyze_add_device(mgc_analyze *a, const void *d_keys, const uint32_t *d_values, uint64_t n, void *stream);

/* The same over all 64 files of the database at `path`: the raw bytes of a file are read by host threads (host_threads,
 * 0: four), uploaded and decoded on the device while the next files are read; a file framed in a way only the host decoder
 * follows is decoded by it and uploaded as arrays.  The database's k must be the accumulator's (MGC_EINVAL).  Labels are
 * ignored, and every stored entry of a multiset is one insertion. */
int mgc_analyze_add_database(mgc_analyze *a, const char *path, int host_threads);

/* Histogram `which` as rows (score, value, number of k-mers), ascending by (score, value), rows with no k-mers left out:
 * what printHist (:139-152) walks.  mgc_analyze_result fills arrays of *n_rows entries each. */
int mgc_analyze_result_rows(mgc_analyze *a, int which, uint64_t *n_rows);
int mgc_analyze_result(mgc_analyze *a, int which, uint32_t *scores, uint32_t *values, uint64_t *occurrences);

/* printHist for every histogram of the report, one line "%u\t%u\t%lu\n" per row: <prefix>.GC.hist and .AT.hist (:228-234),
 * <prefix>.GA_TC.hist, .GA.hist and .TC.hist (:328-335), <prefix>.GT_AC.hist, .GT.hist and .AC.hist (:430-437).  Every file
 * is created, also when it stays empty. */
int mgc_analyze_write(mgc_analyze *a, const char *prefix);

typedef struct mgc_analyze_info {
  uint64_t n_kmers;           /* entries added: "Processed <n> kmers in total." (:224) */
  uint64_t n_files;           /* database files read */
  uint64_t n_overflow_kmers;  /* entries whose value took the overflow list */
  uint64_t n_overflow_retries;/* launches repeated for the overflow list alone because the list had to grow */
  double   decode_ms;         /* HIP events, summed: upload + device decode of the database files */
  double   hist_ms;           /* score + histogram kernels */
  double   overflow_ms;       /* sort + run-length count of the overflow list */
  double   read_s;            /* wall clock the host threads spent reading files (overlaps the device work) */
  double   total_s;           /* wall clock inside mgc_analyze_add_* */
} mgc_analyze_info;
int mgc_analyze_get_info(const mgc_analyze *a, mgc_analyze_info *info);

const char *mgc_analyze_error(void);

#ifdef __cplusplus
}
#endif
#endif /* MERYL_ANALYZE_H */
