/*
 * meryl_import_labelled.h -- C ABI of `meryl-import -labelwidth <lw>`: text `kmer value label` lines -> labelled meryl
 * database, on the device.  The meryl 1 dialect and its entry points stay in meryl_import.h, unchanged.
 *
 * Replaces the reference's src/meryl2-import/meryl-import.C.  Its line loop (:199-233): a line is split at blanks, tabs and
 * '\r'; empty lines are skipped (:199-206); a first word that starts with `value=` sets the persistent value (:210-213), one
 * that starts with `label=` the persistent label (:215-218), words after either are ignored; any other first word is a
 * k-mer -- addR of every base, so a longer word gives its LAST k bases (:222-223) -- whose second word is its value (else
 * the persistent one, :225-228) and whose third word is its label (else the persistent one, :230-233); further words are
 * ignored; canonical / forward / reverse pick (:235-246).  A `#...` line is not part of this dialect: its first word is a
 * k-mer with a bad base.  The reference leaves pval / plab unset (:176-177); here the persistent value starts at 1 and the
 * persistent label at 0.  It feeds 64 merylCountArrays (wPrefix = 6, :158) whose countKmers sums the values of equal k-mers
 * and adds their labels, `_labels[...] += getLabel()` (src/meryl2/merylCountArray.C:381-400); the writer stores the low
 * label_width bits.  Here: value sums are uint32 and wrap, a sum of 0 is stored as 0, label sums are modulo 2^label_width.
 *
 * Numbers -- value and label words, the numbers of `value=` / `label=` lines -- are what decodeInteger reads
 * (documentation/source/reference.rst:615-617): decimal `123` or `123d`, `<hex digits>h` (digits in either case),
 * `<octal digits>o`, `<binary digits>b`.  The suffix letter is lower case, is the word's last byte and decides the base; at
 * least one digit comes before it; leading zeros are fine.  SI suffixes (`123k`, `1mi`) are refused.
 *
 * Refusals carry the 1-based number of the first offending line, as in meryl_import.h: MGC_IMPORT_BAD_BASE, _SHORT, _VALUE
 * (malformed or above 2^32 - 1), and the two kinds below.  label_width is 1..64, k is 6..64 (a 6-bit prefix must leave a
 * suffix).  Arguments are checked before anything touches the device; n = 0 is MGC_OK without a launch (the parser's _count
 * still copies the state back to report the persistent words).  -multiset is not part of this build.
 *
 * Return codes, device pointers and `stream` follow include/meryl_gpu_count.h; failure text: mgc_import_error().
 */
#ifndef MERYL_IMPORT_LABELLED_H
#define MERYL_IMPORT_LABELLED_H

#include "meryl_import.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MGC_IMPORT2_W_PREFIX 6     /* meryl2-import/meryl-import.C:158 */
#define MGC_IMPORT_MIN_LABEL_WIDTH 1
#define MGC_IMPORT_MAX_LABEL_WIDTH 64

#define MGC_IMPORT_BAD_LABEL  5    /* the label word is malformed or has a bit at or above label_width (the reference's
                                      "failed to correctly set label", :260-264, leaves the k-mer half added) */
#define MGC_IMPORT_BAD_ASSIGN 6    /* the number of a `value=` / `label=` line is missing, malformed or out of range for its kind */

/* The triple sort carries 32-bit record numbers: more records than this in one sort is MGC_EINVAL with a message. */
#define MGC_SORT_TRIPLES_MAX_N 0xFFFFFFFFull

/* ------------------------------------------------------------------------
 * Device steps on their own.
 * ------------------------------------------------------------------------ */

/* The parser of meryl_import.h for this dialect: same chunk rules (whole lines, fewer than 2^32 bytes), same two steps, same
 * workspace discipline.  d_state (mgc_dev_import2_parse_state_bytes() bytes, started by mgc_dev_import2_parse_begin) carries
 * BOTH persistent words from chunk to chunk.  _count fills *res (persistent_value: the value that holds after the chunk) and
 * *persistent_label (may be NULL) with the label that holds after it.  mgc_dev_import2_parse writes d_keys[n_records],
 * d_values[n_records] (uint32) and d_labels[n_records] (uint64) in input order and moves d_state past the chunk. */
size_t mgc_dev_import2_parse_state_bytes(void);
size_t mgc_dev_import2_parse_workspace_bytes(uint64_t n_text);
int mgc_dev_import2_parse_begin(void *d_state, void *stream);
int mgc_dev_import2_parse_count(const uint8_t *d_text, uint64_t n_text, uint32_t k, uint32_t label_width, void *d_state,
                                void *d_workspace, size_t workspace_bytes, mgc_import_parse_result *res,
                                uint64_t *persistent_label, void *stream);
int mgc_dev_import2_parse(const uint8_t *d_text, uint64_t n_text, uint32_t k, int mode, uint32_t label_width, void *d_state,
                          void *d_workspace, size_t workspace_bytes, void *d_keys, uint32_t *d_values, uint64_t *d_labels,
                          void *stream);

/* n (key, value, label) triples ordered by key bits [begin_bit, end_bit); triples of equal keys keep their input order.
 * The keys are sorted with a 32-bit record number as their payload (mgc_dev_sort_pairs), then values and labels are gathered
 * once: n may not exceed MGC_SORT_TRIPLES_MAX_N.  *result_in_alt says where ALL THREE arrays of the result are (1 whenever
 * anything was sorted; 0 for n = 0 or an empty bit range, when nothing moved).  Asynchronous on `stream`. */
size_t mgc_dev_sort_triples_workspace_bytes(uint64_t n);
int mgc_dev_sort_triples(void *d_keys, uint32_t *d_values, uint64_t *d_labels, void *d_alt_keys, uint32_t *d_alt_values,
                         uint64_t *d_alt_labels, uint64_t n, uint32_t key_words, uint32_t begin_bit, uint32_t end_bit,
                         void *d_workspace, size_t workspace_bytes, int *result_in_alt, void *stream);

/* mgc_dev_reduce_pairs_* with labels: _emit writes the distinct keys ascending, the uint32 sum of every key's values
 * (wrapping) and the sum of its labels modulo 2^label_width.  A key's triples may span any number of workgroups. */
size_t mgc_dev_reduce_triples_workspace_bytes(uint64_t n);
int mgc_dev_reduce_triples_count(const void *d_sorted_keys, const uint32_t *d_sorted_values, const uint64_t *d_sorted_labels,
                                 uint64_t n, uint32_t key_words, void *d_workspace, size_t workspace_bytes, uint64_t *n_distinct,
                                 void *stream);
int mgc_dev_reduce_triples_emit(const void *d_sorted_keys, const uint32_t *d_sorted_values, const uint64_t *d_sorted_labels,
                                uint64_t n, uint32_t key_words, uint32_t label_width, void *d_workspace, size_t workspace_bytes,
                                void *d_out_keys, uint32_t *d_out_values, uint64_t *d_out_labels, void *stream);

/* ------------------------------------------------------------------------
 * Text -> labelled database (main() of meryl2-import/meryl-import.C:152-309).
 * ------------------------------------------------------------------------ */

/* Reads `path` like mgc_import_file (batches through pinned buffers, MGC_IMPORT_BATCH).  Every batch is parsed as it arrives
 * and its triples are appended to device arrays; after the last batch there is ONE sort and ONE reduce, and the result goes
 * to a wPrefix = 6 database with label_width-bit labels.  info->n_batches: text batches.  Input whose triples and sort
 * buffers do not fit the free device memory returns MGC_ENOMEM (the message names the bytes needed); a refused line returns
 * MGC_EFORMAT with info->bad_line / bad_kind set.  Either leaves nothing at `output`.  info may be NULL. */
int mgc_import_labelled_file(const char *path, uint32_t k, int mode, uint32_t label_width, const char *output, int device,
                             int host_threads, mgc_import_info *info);
/* The same for text in host memory. */
int mgc_import_labelled_text(const char *text, uint64_t n_text, uint32_t k, int mode, uint32_t label_width, const char *output,
                             int device, int host_threads, mgc_import_info *info);

#ifdef __cplusplus
}
#endif
#endif /* MERYL_IMPORT_LABELLED_H */
