/*
 * meryl_import.h -- C ABI of `meryl-import`: text `kmer value` lines -> meryl database, on the device.
 *
 * Replaces the reference's src/meryl-import/meryl-import.C: the line loop (:177-219: split into words, `#<value>` lines set
 * the persistent value, addR of every base of the first word, reverse complement, canonical / forward / reverse pick) and
 * what it feeds -- 1024 merylCountArrays WITH values, countSingleKmersWithValues (src/meryl/merylCountArray.C:369-411: unpack,
 * std::sort of (suffix, value) records, sum the values of equal suffixes) and dumpCountedKmers into a wPrefix = 10 database
 * (:143, :229-247).  Here the text is parsed on the device into (k-mer, value) pairs, the pairs are sorted by k-mer, the
 * values of equal k-mers are summed (uint32, wrapping like kmvalu arithmetic, merylCountArray.C:403; a sum of 0 is stored
 * as 0), and the ascending distinct pairs go through the device encoder of include/meryl_db.h.
 *
 * Where the reference's behaviour is undefined (it depends on the absent meryl-utility or "will probably lead to a crash",
 * :104) the input is REFUSED with the 1-based number of the first offending line: a k-mer word shorter than k, a byte in it
 * that is not ACGTacgt, a value or `#` number that is not all decimal digits or exceeds 2^32 - 1.  A word longer than k
 * gives its LAST k bases (the addR loop, :196-197).  k is 6..64 (wPrefix = 10 must leave a suffix).  -multiset is not part
 * of this build.
 *
 * Return codes, device pointers and `stream` follow include/meryl_gpu_count.h; failure text: mgc_import_error().
 */
#ifndef MERYL_IMPORT_H
#define MERYL_IMPORT_H

#include <stddef.h>
#include <stdint.h>

#include "meryl_gpu_count.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MGC_IMPORT_W_PREFIX 10     /* meryl-import.C:143 */
#define MGC_IMPORT_MIN_K    6
#define MGC_IMPORT_MAX_K    64

/* what is wrong with the first offending line (mgc_import_info.bad_kind, mgc_import_parse_result.bad_kind) */
#define MGC_IMPORT_BAD_NONE   0
#define MGC_IMPORT_BAD_BASE   1    /* a byte of the k-mer word is not ACGTacgt */
#define MGC_IMPORT_BAD_SHORT  2    /* the k-mer word holds fewer than k bases */
#define MGC_IMPORT_BAD_VALUE  3    /* the value is not all decimal digits, or exceeds 2^32 - 1 */
#define MGC_IMPORT_BAD_HASH   4    /* the number of a `#` line is missing, not all decimal digits, or exceeds 2^32 - 1 */

/* ------------------------------------------------------------------------
 * Device steps on their own (tests, and callers that hold the text or the pairs in HBM already).
 * ------------------------------------------------------------------------ */

/* The line loop of meryl-import.C:177-219 over one chunk of text in device memory.  A chunk must hold whole lines (every
 * chunk but the last ends in '\n') and fewer than 2^32 bytes.  What survives from chunk to chunk -- the persistent value
 * (:175, :188-191), the lines seen so far (for error line numbers) and the first bad line -- lives in d_state
 * (mgc_dev_import_parse_state_bytes() bytes, started by mgc_dev_import_parse_begin).
 *
 * Two steps: mgc_dev_import_parse_count reads the chunk, validates every line and returns how many lines and records it
 * holds (synchronises `stream`); res->bad_kind != 0 means the input is refused and nothing more may be parsed.
 * mgc_dev_import_parse then writes the chunk's records in input order -- d_keys[n_records] (uint64, or {lo,hi} for k > 32:
 * the library's 2-bit packing, A0 C1 T2 G3, first base most significant; mode = MGC_MODE_*: min(forward, reverse
 * complement) / forward / reverse complement, :204-211) and d_values[n_records] -- and moves d_state past the chunk.
 * d_workspace (mgc_dev_import_parse_workspace_bytes(n_text)) must be the same, untouched, for both steps. */
typedef struct mgc_import_parse_result {
  uint64_t n_lines;          /* lines of this chunk, blank ones included */
  uint64_t n_records;        /* lines that hold a k-mer */
  uint64_t bad_line;         /* 1-based number, over all chunks since mgc_dev_import_parse_begin, of the first refused line */
  uint32_t bad_kind;         /* MGC_IMPORT_BAD_* */
  uint32_t persistent_value; /* the value that holds after this chunk */
} mgc_import_parse_result;
size_t mgc_dev_import_parse_state_bytes(void);
size_t mgc_dev_import_parse_workspace_bytes(uint64_t n_text);
int mgc_dev_import_parse_begin(void *d_state, void *stream);
int mgc_dev_import_parse_count(const uint8_t *d_text, uint64_t n_text, uint32_t k, void *d_state, void *d_workspace,
                               size_t workspace_bytes, mgc_import_parse_result *res, void *stream);
int mgc_dev_import_parse(const uint8_t *d_text, uint64_t n_text, uint32_t k, int mode, void *d_state, void *d_workspace,
                         size_t workspace_bytes, void *d_keys, uint32_t *d_values, void *stream);

/* The std::sort of merylCountArray.C:387: n (key, value) pairs ordered by key bits [begin_bit, end_bit), the value carried
 * along; pairs of equal keys keep their input order.  key_words 1: uint64 keys, 2: {lo,hi}.  Ping-pongs between
 * (d_keys, d_values) and (d_alt_keys, d_alt_values); *result_in_alt says where the result is.  Asynchronous on `stream`. */
size_t mgc_dev_sort_pairs_workspace_bytes(uint64_t n);
int mgc_dev_sort_pairs(void *d_keys, uint32_t *d_values, void *d_alt_keys, uint32_t *d_alt_values, uint64_t n,
                       uint32_t key_words, uint32_t begin_bit, uint32_t end_bit, void *d_workspace, size_t workspace_bytes,
                       int *result_in_alt, void *stream);

/* The summing loop of merylCountArray.C:393-408 over pairs sorted by key: _count leaves the number of distinct keys in
 * *n_distinct (one synchronisation); _emit (same inputs, the workspace _count left) writes the distinct keys ascending and
 * the sum of every key's values, uint32, wrapping.  A key's pairs may span any number of workgroups. */
size_t mgc_dev_reduce_pairs_workspace_bytes(uint64_t n);
int mgc_dev_reduce_pairs_count(const void *d_sorted_keys, const uint32_t *d_sorted_values, uint64_t n, uint32_t key_words,
                               void *d_workspace, size_t workspace_bytes, uint64_t *n_distinct, void *stream);
int mgc_dev_reduce_pairs_emit(const void *d_sorted_keys, const uint32_t *d_sorted_values, uint64_t n, uint32_t key_words,
                              void *d_workspace, size_t workspace_bytes, void *d_out_keys, uint32_t *d_out_values, void *stream);

/* ------------------------------------------------------------------------
 * Text -> database (main() of meryl-import.C:137-256).
 * ------------------------------------------------------------------------ */
typedef struct mgc_import_info {
  uint64_t n_lines;          /* lines read, blank and `#` lines included */
  uint64_t n_records;        /* "Found <n> kmers in the input." (:223) */
  uint64_t n_distinct;       /* k-mers written */
  uint64_t n_batches;
  uint64_t text_bytes;
  uint64_t bad_line;         /* refusal: 1-based number of the first offending line (0: none) */
  uint32_t bad_kind;         /* MGC_IMPORT_BAD_* */
  uint32_t reserved;
  double   upload_ms;        /* host -> device copies of the text (HIP events, summed over the batches) */
  double   parse_ms;         /* both parser passes */
  double   sort_ms;
  double   reduce_ms;
  double   read_s;           /* wall clock the reader spent filling batches (overlaps the device work) */
  double   write_s;          /* run merge + encode + file writes after the last batch */
  double   total_s;
} mgc_import_info;

/* Reads `path` ("-": standard input; plain text or gzip) in batches through pinned buffers, every batch cut at its last
 * '\n' (the tail is carried into the next); parses, sorts and reduces each batch on `device` (< 0: the current one).  One
 * batch goes straight to the database stream; more are parked as runs (mgc_runs_add) and merged once (mgc_runs_write).
 * Batch size: from the free device memory; MGC_IMPORT_BATCH (bytes of text) overrides it.
 * A refused input returns MGC_EFORMAT with info->bad_line / bad_kind set and leaves nothing at `output`.  info may be NULL. */
int mgc_import_file(const char *path, uint32_t k, int mode, const char *output, int device, int host_threads,
                    mgc_import_info *info);
/* The same for text in host memory. */
int mgc_import_text(const char *text, uint64_t n_text, uint32_t k, int mode, const char *output, int device,
                    int host_threads, mgc_import_info *info);
const char *mgc_import_error(void);

#ifdef __cplusplus
}
#endif
#endif /* MERYL_IMPORT_H */
