/*
 * meryl_gpu_count.h -- C ABI of the MI355X-native `meryl count` engine.
 *
 * This is the drop-in boundary for the reference's counting engine
 * (marbl/meryl, paths relative to the reference root):
 *
 *   upstream   bool merylInput::loadBases(char *seq, uint64 maxLength,
 *                                         uint64 &seqLength, bool &endOfSequence)
 *              src/meryl/merylInput.H:67-70, called from
 *              src/meryl/merylOp-countThreads.C:180-182
 *   engine     merylOperation::configureCounting()  src/meryl/merylOp-count.C:300-403
 *              merylOperation::countThreads()       src/meryl/merylOp-countThreads.C:385-474
 *   downstream merylFileWriter::initialize(wPrefix) / numberOfFiles() /
 *              firstPrefixInFile() / lastPrefixInFile()
 *              merylBlockWriter::addBlock(prefix, nKmers, suffixes, counts)
 *              call sites src/meryl/merylOp-countThreads.C:404,453-464,
 *              src/meryl/merylCountArray.C:472-475
 *
 * A maintainer replaces the body of countThreads() with: mgc_open, a loop of
 * mgc_push_bases over merylInput::loadBases, then mgc_finish whose callback
 * calls merylBlockWriter::addBlock -- see INTEGRATION.md.
 *
 * Plain C types only: pointers and sizes, no C++/torch types.  Functions
 * return MGC_OK (0) or a negative MGC_E* code instead of the reference's
 * fprintf(stderr)+exit(1); mgc_last_error() gives the text.
 *
 * Pointers named d_* are DEVICE pointers (HBM of the current HIP device);
 * `stream` is a hipStream_t passed as void* (NULL = the null stream).
 */
#ifndef MERYL_GPU_COUNT_H
#define MERYL_GPU_COUNT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MGC_OK            0
#define MGC_EINVAL       -1    /* bad argument (k, mode, NULL pointer, capacity) */
#define MGC_ENOMEM       -2    /* host or device allocation failed */
#define MGC_EHIP         -3    /* a HIP runtime call or kernel failed */
#define MGC_ESTATE       -4    /* call out of order (e.g. finish before count) */
#define MGC_EUNSUPPORTED -5    /* valid in the reference, not implemented here yet */
#define MGC_ETIMEOUT     -6    /* an in-kernel bounded spin expired (never hangs) */
#define MGC_EFORMAT      -7    /* mgc_end_text: the file is not what the device parser handles (see there) */

/* opCount / opCountForward / opCountReverse, src/meryl/merylOp.H:40-42 and
 * src/meryl/merylOp-countThreads.C:241-258 */
#define MGC_MODE_CANONICAL 0
#define MGC_MODE_FORWARD   1
#define MGC_MODE_REVERSE   2

#define MGC_NUM_FILES_BITS 6   /* 64 files: src/meryl/merylOp-count.C:185-187, documentation/source/usage.rst:18 */
#define MGC_NUM_FILES      64

/* ------------------------------------------------------------------------
 * Configuration -- replaces merylOperation::configureCounting
 * (src/meryl/merylOp-count.C:300-403).  Pure host arithmetic.
 * ---------------------------------------------------------------------- */
#define MGC_MAX_COUNT_SUFFIX 32

typedef struct mgc_count_config {
  /* in */
  uint32_t k;                     /* kmerTiny::merSize(), 1..64 */
  int32_t  mode;                  /* MGC_MODE_* */
  uint64_t n_kmers_estimate;      /* n= / guesstimateNumberOfkmersInInput (:317,449) */
  uint64_t memory_allowed;        /* memory= in bytes (merylCommandBuilder.C:299-302) */
  uint32_t threads;               /* threads= (host threads used by mgc_finish) */
  uint32_t count_suffix_length;   /* count-suffix= length (see count_suffix below); forces simple mode (:379-382) */
  uint32_t homopoly_compress;     /* `compress` (merylInput.C:261-262) */
  uint32_t page_size;             /* 0 -> 4096 (getPageSize()) */
  uint32_t sizeof_count_array;    /* 0 -> 3232 (sizeof(merylCountArray), merylCountArray.H:44,71-74) */
  /* out */
  int32_t  use_simple;            /* :368-382 */
  uint32_t w_prefix;              /* wPrefix_ */
  uint64_t n_prefix;              /* nPrefix_ */
  uint32_t w_data;                /* wData_ = 2k - wPrefix */
  uint32_t n_batches;             /* incl. the reference's post-increment quirk (:355-358) */
  uint64_t memory_used;           /* what the "Configured ... mode for %.3f GB" line prints (:398-401) */
  /* in (at the end: added after the first layout) */
  char     count_suffix[MGC_MAX_COUNT_SUFFIX + 4];   /* count-suffix=<bases> (merylCommandBuilder.C:271-272, merylOp.H:139-147):
                                      only k-mers -- the canonical / forward / reverse one that is counted -- ENDING in these
                                      bases are counted (merylOp-countSimple.C:50-58,88-93); count_suffix_length of them,
                                      NUL-terminated; needs k - length >= 3 */
  /* in: value-labelled k-mers (meryl2).  The count hands ONE constant label to the writer when it dumps a block:
   * addCountedBlock(prefix, nKmers, suffix, counts, labels = nullptr, label = _lConstant)
   * (src/meryl2/merylCountArray.C:469-471, src/meryl2/merylOp-countThreads.C:363-367,464-468; `label=#<n>` sets it,
   * src/meryl2/merylCommandBuilder-isAssign.C:124; the global `-l <bits>` fixes the width, src/meryl2/merylGlobals.C:75-77).
   * label_size = 0: unlabelled (meryl v1 behaviour). */
  uint32_t label_size;            /* bits of label per k-mer, 0..64 */
  uint32_t reserved0;
  uint64_t label_constant;
} mgc_count_config;

int mgc_configure_counting(mgc_count_config *cfg);

/* Formats the Canu-parsed line of src/meryl/merylOp-count.C:398-401 into buf. */
int mgc_format_configured_line(const mgc_count_config *cfg, char *buf, size_t buflen);

/* ------------------------------------------------------------------------
 * Device-level operators (stateless; caller owns all memory).  These are the
 * hot path: the HIP kernels that replace insertKmers (merylOp-countThreads.C:
 * 235-280), merylCountArray::add/get (merylCountArray.C:490-847) and
 * countSingleKmers (merylCountArray.C:323-365).  Keys are full k-mers
 * (prefix<<wData | suffix): uint64 for k <= 32 (key_words = 1), 16-byte
 * little-endian {lo, hi} pairs for k in 33..64 (key_words = 2) -- the same
 * 128-bit kmdata the reference uses (src/tests/merylCountArrayTest.C:27-31).
 * ---------------------------------------------------------------------- */

/* Number of partition buckets is 2^bucket_bits, bucket = key >> (2k-bucket_bits);
 * bucket_bits = 6 gives the reference's 64 files, 0 a single bucket. */
#define MGC_MAX_BUCKET_BITS 10

/* Scratch needed by mgc_dev_kmer_histogram / mgc_dev_kmer_partition. */
size_t mgc_dev_partition_workspace_bytes(uint32_t bucket_bits);

/* Pass 1: count k-mer instances per bucket.  Writes d_bucket_counts[2^bucket_bits]
 * (uint64, overwritten) and fills the workspace with the per-workgroup counts
 * pass 2 needs.  Bases are ASCII; any byte that is not ACGTacgt (e.g. the '.'
 * breakers of merylOp-countThreads.C:196,214-215, or N) breaks the k-mer. */
int mgc_dev_kmer_histogram(const uint8_t *d_bases, uint64_t n_bases, uint32_t k, int mode,
                           uint32_t bucket_bits, uint64_t *d_bucket_counts,
                           void *d_workspace, size_t workspace_bytes, void *stream);

/* Pass 2: pack every k-mer instance (2 bits/base, A0 C1 T2 G3, first base most
 * significant), pick fmer/rmer per `mode`, and scatter it into its bucket's
 * region: bucket b occupies d_keys[d_bucket_starts[b] ...).  d_bucket_starts
 * holds 2^bucket_bits uint64 offsets (in keys) chosen by the caller from the
 * pass-1 counts (any layout with enough room per bucket).  Must be called
 * with the same bases/k/mode/bucket_bits and the workspace left by pass 1.
 * Order inside a bucket is unspecified (the sort follows). */
int mgc_dev_kmer_partition(const uint8_t *d_bases, uint64_t n_bases, uint32_t k, int mode,
                           uint32_t bucket_bits, const uint64_t *d_bucket_starts,
                           void *d_keys, void *d_workspace, size_t workspace_bytes, void *stream);

/* mgc_dev_kmer_histogram + the k-mers per top FIFTEEN bits (d_fine_hist: uint64[2^15], zeroed here), one pass over the bases;
 * bucket_bits 6..8.  What a sharded count's senders run: the bucket counts feed the routing plan, the workspace rows the
 * partition, the fifteen-bit histogram -- summed over the ranks -- the owners' first grouping digit (mgc_count_buckets_into). */
int mgc_dev_kmer_histogram_fine(const uint8_t *d_bases, uint64_t n_bases, uint32_t k, int mode, uint32_t bucket_bits,
                                uint64_t *d_bucket_counts, uint64_t *d_fine_hist, void *d_workspace, size_t workspace_bytes, void *stream);

/* LSB radix sort of keys (key_words 1 or 2) on bits [begin_bit, end_bit).
 * Ping-pongs between d_keys and d_alt (both n keys); *result_in_alt tells
 * where the sorted keys ended up. */
size_t mgc_dev_sort_workspace_bytes(uint64_t n);
int mgc_dev_radix_sort(void *d_keys, void *d_alt, uint64_t n, uint32_t key_words,
                       uint32_t begin_bit, uint32_t end_bit,
                       void *d_workspace, size_t workspace_bytes,
                       int *result_in_alt, void *stream);
/* The GROUPING passes the count path uses on a file's top bits (not a sort): the keys come out grouped by bits
 * [begin_bit, end_bit), groups ascending, members in ANY order (unstable).  Defined for ranges of at most two digits
 * (18 bits) and n < 2^30; anything else takes the stable sort above.  Same arguments and workspace.  Replaces the top-bit
 * part of unpackSuffixes + std::sort (merylCountArray.C:276-289,330), which the sub-bucket count does not need ordered. */
int mgc_dev_radix_group(void *d_keys, void *d_alt, uint64_t n, uint32_t key_words,
                        uint32_t begin_bit, uint32_t end_bit,
                        void *d_workspace, size_t workspace_bytes,
                        int *result_in_alt, void *stream);

/* Run-length count of a sorted key array (countSingleKmers' two passes,
 * merylCountArray.C:334-358).  Step 1 returns the number of distinct keys
 * (synchronises the stream); step 2 writes d_unique[n_distinct] and
 * d_counts[n_distinct] (uint32, wraps mod 2^32 like merylCountArray.C:357). */
size_t mgc_dev_rle_workspace_bytes(uint64_t n);
int mgc_dev_rle_count(const void *d_sorted, uint64_t n, uint32_t key_words, void *d_workspace,
                      size_t workspace_bytes, uint64_t *n_distinct, void *stream);
int mgc_dev_rle_emit(const void *d_sorted, uint64_t n, uint32_t key_words, void *d_workspace,
                     size_t workspace_bytes, void *d_unique, uint32_t *d_counts, void *stream);

/* d_block_start[p] = index of the first distinct key with (key >> w_data) >= p,
 * for p in [0, n_prefix]; block p of the database is
 * [d_block_start[p], d_block_start[p+1]) -- the (prefix, nKmers) of addBlock. */
int mgc_dev_block_offsets(const void *d_unique, uint64_t n_distinct, uint32_t key_words, uint32_t w_data,
                          uint64_t n_prefix, uint64_t *d_block_start, void *stream);

/* Merge of two (k-mer, value) streams with distinct ascending keys -- the two-input step of the reference's k-way merge
 * (merylOperation::nextMer, src/meryl/merylOp-nextMer.C:478-641: smallest k-mer over the inputs, values of the inputs that
 * hold it combined) and of merylBlockWriter::finish() folding the batches a memory-limited count spilled.  Step 1 returns
 * the output length (synchronises the stream), step 2 writes d_keys_out / d_counts_out (that many entries), with the
 * same inputs and the workspace step 1 left.  Sums wrap mod 2^32 like the reference's kmvalu arithmetic. */
#define MGC_MERGE_UNION_SUM     0     /* opUnionSum      src/meryl/merylOp-nextMer.C:571-573 (findSumCount :43-48) */
#define MGC_MERGE_UNION_MIN     1     /* opUnionMin      :563-565 */
#define MGC_MERGE_UNION_MAX     2     /* opUnionMax      :567-569 */
#define MGC_MERGE_INTERSECT_SUM 3     /* opIntersectSum  :590-593 (k-mers in BOTH inputs) */
#define MGC_MERGE_INTERSECT_MIN 4     /* opIntersectMin  :580-583 */
#define MGC_MERGE_INTERSECT_MAX 5     /* opIntersectMax  :585-588 */
#define MGC_MERGE_INTERSECT     6     /* opIntersect     :575-578: in both, the FIRST input's value */
#define MGC_MERGE_SUBTRACT      7     /* opSubtract      :595-602 + subtractCount :51-62: in A; a - b while a > b, otherwise dropped */
#define MGC_MERGE_DIFFERENCE    8     /* opDifference    :604-607: in A and not in B */
#define MGC_MERGE_SYMMETRIC_DIFFERENCE 9  /* opSymmetricDifference :609-612: in exactly one input */
#define MGC_MERGE_UNION        10     /* opUnion         :559-561: value = number of inputs holding the k-mer (mgc_db_merge only) */
size_t mgc_dev_merge_workspace_bytes(uint64_t na, uint64_t nb);
int mgc_dev_merge_count(const void *d_keys_a, uint64_t na, const void *d_keys_b, uint64_t nb, uint32_t key_words, int op,
                        void *d_workspace, size_t workspace_bytes, uint64_t *n_out, void *stream);
int mgc_dev_merge_emit(const void *d_keys_a, const uint32_t *d_counts_a, uint64_t na,
                       const void *d_keys_b, const uint32_t *d_counts_b, uint64_t nb, uint32_t key_words, int op,
                       void *d_workspace, size_t workspace_bytes, void *d_keys_out, uint32_t *d_counts_out, void *stream);
/* step 1 with the values at hand: MGC_MERGE_SUBTRACT needs them to know what is written (mgc_dev_merge_count refuses it) */
int mgc_dev_merge_count_values(const void *d_keys_a, const uint32_t *d_counts_a, uint64_t na, const void *d_keys_b,
                               const uint32_t *d_counts_b, uint64_t nb, uint32_t key_words, int op, void *d_workspace,
                               size_t workspace_bytes, uint64_t *n_out, void *stream);

/* Merge of 2..MGC_MERGE_MANY_MAX streams at once -- the reference's k-way step itself (merylOperation::nextMer,
 * src/meryl/merylOp-nextMer.C:478-523: the smallest k-mer over the inputs and _actLen / _actCount[] / _actIndex[], the inputs
 * that hold it in input order; :559-612 with findMin/Max/SumCount and subtractCount :23-62 combine them).  Every
 * MGC_MERGE_* operation, MGC_MERGE_UNION included.  d_keys / d_values / n: HOST arrays of n_inputs device pointers and
 * lengths (distinct ascending keys each, a length below 2^32).  The result equals the left fold of the two-input merge over
 * the same inputs element by element (a sum that wraps to 0 is kept).  Two steps like the two-input merge; the count step
 * takes the values, since MGC_MERGE_SUBTRACT needs them.  n_inputs outside 2..32 or an operation outside 0..10: MGC_EINVAL.
 * mgc_dev_merge_many_tile: the merged positions one workgroup handles (tile borders fall on whole groups of equal k-mers, at
 * most n_inputs - 1 positions earlier). */
#define MGC_MERGE_MANY_MAX 32
uint32_t mgc_dev_merge_many_tile(uint32_t key_words);
size_t mgc_dev_merge_many_workspace_bytes(const uint64_t *n, uint32_t n_inputs, uint32_t key_words);
int mgc_dev_merge_many_count(const void *const *d_keys, const uint32_t *const *d_values, const uint64_t *n, uint32_t n_inputs,
                             uint32_t key_words, int op, void *d_workspace, size_t workspace_bytes, uint64_t *n_out, void *stream);
int mgc_dev_merge_many_emit(const void *const *d_keys, const uint32_t *const *d_values, const uint64_t *n, uint32_t n_inputs,
                            uint32_t key_words, int op, void *d_workspace, size_t workspace_bytes, void *d_keys_out,
                            uint32_t *d_values_out, void *stream);

/* One (k-mer, value) stream through a single-input operation of src/meryl/merylOp-nextMer.C:490-557: the value filters
 * (the value passes or the k-mer is dropped) and the arithmetic operations (with the reference's overflow / underflow /
 * divide-by-zero results; a k-mer whose new value is 0 is dropped, :470-474).  Two steps like the merge. */
#define MGC_VALUE_LESS_THAN     0     /* opLessThan     :490-492  value <  constant */
#define MGC_VALUE_GREATER_THAN  1     /* opGreaterThan  :494-496 */
#define MGC_VALUE_AT_LEAST      2     /* opAtLeast      :498-500 */
#define MGC_VALUE_AT_MOST       3     /* opAtMost       :502-504 */
#define MGC_VALUE_EQUAL_TO      4     /* opEqualTo      :506-508 */
#define MGC_VALUE_NOT_EQUAL_TO  5     /* opNotEqualTo   :510-512 */
#define MGC_VALUE_INCREASE      6     /* opIncrease     :514-519 */
#define MGC_VALUE_DECREASE      7     /* opDecrease     :521-526 */
#define MGC_VALUE_MULTIPLY      8     /* opMultiply     :528-533 */
#define MGC_VALUE_DIVIDE        9     /* opDivide       :535-540 */
#define MGC_VALUE_DIVIDE_ROUND 10     /* opDivideRound  :541-550 */
#define MGC_VALUE_MODULO       11     /* opModulo       :552-557 */
size_t mgc_dev_select_workspace_bytes(uint64_t n);
int mgc_dev_select_count(const void *d_keys, const uint32_t *d_values, uint64_t n, uint32_t key_words, int value_op, uint64_t constant,
                         void *d_workspace, size_t workspace_bytes, uint64_t *n_out, void *stream);
int mgc_dev_select_emit(const void *d_keys, const uint32_t *d_values, uint64_t n, uint32_t key_words, int value_op, uint64_t constant,
                        void *d_workspace, size_t workspace_bytes, void *d_keys_out, uint32_t *d_values_out, void *stream);

/* ---- labels through the merge and value operations (meryl2) ----------------------------------------------------------
 * A k-mer may carry a label of up to 64 bits beside its value (kmlabl).  When an operation writes a k-mer it computes the
 * label from the labels L[j] and values V[j] of its ACTIVE inputs (the inputs that hold the k-mer, in input order: _acta[],
 * _actLen) and the operation's label constant c -- merylOpCompute::findOutputLabel, src/meryl2/merylOpCompute.C:286-395.
 * Labels never decide which k-mers are written.  Between operations a label is a full 64-bit value; it is cut to the
 * database's label_size bits only where it is stored or printed.
 *   SET         c                                                                             (:295-297)
 *   FIRST       L[0]: the first ACTIVE input, which need not be input 0                        (:304-307)
 *   MIN         (l, v) = (c, 2^32-1); for each j: V[j] < v (strict) takes (L[j], V[j]); l      (:309-320; an input whose
 *               value is 2^32-1 never wins, as there)
 *   MAX         numeric maximum of c and every L[j]                                            (:322-326)
 *   AND OR XOR  c combined with every L[j]                                                     (:329-345)
 *   DIFFERENCE  L[0] & ~c & ~L[1] & ...                                                        (:347-352)
 *   LIGHTEST    starts with c; L[j] replaces it when its popcount is strictly smaller          (:354-359)
 *   HEAVIEST    the same with strictly larger                                                  (:361-366)
 *   INVERT      ~L[0]; one active input only: value operations and one-input merges           (:368-371)
 *   SELECTED    the label of the input whose VALUE the operation selected: under *-min the first active input with the
 *               smallest value, under *-max the first with the largest, FIRST under every other operation.  The
 *               reference's own labelSelected is a placeholder that takes _acta[0] under a `#warning wrong` (:299-302);
 *               this follows its stated meaning instead.
 *   DEFAULT     what the operation's alias sets (src/meryl2/merylCommandBuilder-processText.C:384-499): union, union-sum
 *               -> OR; intersect, intersect-sum -> AND; union-min/-max, intersect-min/-max -> SELECTED; subtract ->
 *               DIFFERENCE; difference, symmetric-difference and every value operation -> FIRST.
 * The reference's shift-* and rotate-* label words are not offered: its code for them shifts the wrong way and its rotate
 * is a shift (`#warning wrong`, :373-393).
 * The constant is always taken as given; mgc_label_default_constant(op) is the one the reference uses when the command
 * names none (merylCommandBuilder-isAssign.C:124-156): all ones for AND, XOR and LIGHTEST, 0 otherwise. */
#define MGC_LABEL_DEFAULT     0
#define MGC_LABEL_SET         1
#define MGC_LABEL_FIRST       2
#define MGC_LABEL_MIN         3
#define MGC_LABEL_MAX         4
#define MGC_LABEL_AND         5
#define MGC_LABEL_OR          6
#define MGC_LABEL_XOR         7
#define MGC_LABEL_DIFFERENCE  8
#define MGC_LABEL_LIGHTEST    9
#define MGC_LABEL_HEAVIEST   10
#define MGC_LABEL_INVERT     11
#define MGC_LABEL_SELECTED   12
uint64_t mgc_label_default_constant(int label_op);
/* Step 2 of the merges above with labels: d_labels[i] (HOST array of device pointers) holds input i's labels, NULL = all 0
 * (an unlabelled input costs no buffer); d_labels_out receives one label per written k-mer.  The count step is
 * mgc_dev_merge_many_count over the same inputs, whose workspace this takes (labels do not change what is written).
 * n_inputs = 1 is accepted here (the count step refuses it): every k-mer of the one input is written, so the output has
 * n[0] entries, and this call runs the count pass itself.  MGC_LABEL_INVERT with two or more inputs, an unknown label
 * operation: MGC_EINVAL. */
int mgc_dev_merge_many_emit_labelled(const void *const *d_keys, const uint32_t *const *d_values, const uint64_t *const *d_labels,
                                     const uint64_t *n, uint32_t n_inputs, uint32_t key_words, int op, int label_op,
                                     uint64_t label_constant, void *d_workspace, size_t workspace_bytes, void *d_keys_out,
                                     uint32_t *d_values_out, uint64_t *d_labels_out, void *stream);
/* Step 2 of the value operations with labels: the label operation over the one active input (d_labels NULL = all 0);
 * the count step is mgc_dev_select_count. */
int mgc_dev_select_emit_labelled(const void *d_keys, const uint32_t *d_values, const uint64_t *d_labels, uint64_t n,
                                 uint32_t key_words, int value_op, uint64_t constant, int label_op, uint64_t label_constant,
                                 void *d_workspace, size_t workspace_bytes, void *d_keys_out, uint32_t *d_values_out,
                                 uint64_t *d_labels_out, void *stream);
/* ---- selectors (meryl2) -------------------------------------------------------------------------------------------------
 * After an operation has assigned the value and the label of a k-mer, a SELECTOR decides whether it is written: a sum of
 * products of tests (src/meryl2/merylSelector.{H,C}, merylCommandBuilder-isSelect.C, merylOp-nextMer.C:58-192).  A program
 * is an array of at most MGC_SELECT_MAX_TERMS terms; a term with ends_product set closes its product (the word `or`
 * followed it); the k-mer is kept when every term of some product holds; an empty program keeps everything.  A selector
 * only removes k-mers: the operation's own rule (in all inputs, value not zero, ...) still applies.
 * A side of a VALUE or LABEL term: index -1 = the constant, 0 = the output k-mer (after the operation's value and label
 * rules), n = input n (1-based, command-line order).  merylSelector::isTrue (merylSelector.C:72-156):
 *   VALUE  32-bit compare (a constant is cut to 32 bits).  A referenced input that does not hold the k-mer makes the term
 *          FALSE, also under `not` (the reference returns before it applies _t, :89,:95).
 *   LABEL  the same over 64-bit labels (:101-118).
 *   BASES  the number of the letters of base_mask in the k-mer (MGC_SEL_BASE_*; merylSelector.H:123-145 -- the letter is
 *          XORed to A, the two bits of a base are squashed and the set bits counted, over the 2k bits that hold bases) against
 *          a constant: one side has index 0, the other -1.
 *   INPUT  bit (number of inputs holding the k-mer) of count_mask is set AND every input of required_mask (bit i = input
 *          i + 1) holds it (:141-150).
 * negate (`not`) inverts BASES and INPUT terms, and VALUE / LABEL terms except in the absent-input case. */
#define MGC_SELECT_MAX_TERMS 16
#define MGC_SEL_VALUE 1
#define MGC_SEL_LABEL 2
#define MGC_SEL_BASES 3
#define MGC_SEL_INPUT 4
#define MGC_REL_EQ  1            /* merylSelectorRelation, merylSelector.H */
#define MGC_REL_NEQ 2
#define MGC_REL_LEQ 3
#define MGC_REL_GEQ 4
#define MGC_REL_LT  5
#define MGC_REL_GT  6
#define MGC_SEL_BASE_A 1u        /* base_mask: bit = the 2-bit code of the letter (A 0, C 1, T 2, G 3) */
#define MGC_SEL_BASE_C 2u
#define MGC_SEL_BASE_T 4u
#define MGC_SEL_BASE_G 8u
typedef struct mgc_select_term {
  uint8_t  quantity;             /* MGC_SEL_* */
  uint8_t  relation;             /* MGC_REL_* (unused by INPUT) */
  uint8_t  negate;
  uint8_t  ends_product;
  uint8_t  base_mask;            /* BASES */
  uint8_t  reserved[3];
  int32_t  lhs_index, rhs_index; /* -1 constant, 0 output k-mer, n input n */
  uint64_t lhs_constant, rhs_constant;
  uint64_t count_mask;           /* INPUT: bit c = "held by exactly c inputs" passes (c = 0..32) */
  uint32_t required_mask;        /* INPUT: inputs that must hold the k-mer */
  uint32_t reserved2;
} mgc_select_term;               /* 48 bytes */
/* THE parser of selector words (the CLI and Python both call it): words[0..n_words) are the words that follow a set or
 * value operation of n_inputs inputs --
 *   value:[lhs]REL rhs   label:[lhs]REL rhs     REL: == = eq != <> ne <= le >= ge < lt > gt; a side: @n, #c or an integer
 *                                               (decimal, 0x.., 0b..); a missing lhs is the output k-mer (decodeSelector)
 *   bases:<letters of acgt>:REL n
 *   input:w[:w...]       separator : or , ; w: n  n-m  all  any  n-all  first  @n  @a-@b
 *   not   and (ignored)   or
 * `n-all` means "in at least n inputs", as the reference documents it (merylSelector.H:236, isSelect.C:377); its code
 * (merylSelector.C:243-246) marks inputs n..N as required instead.  distinct= / word-frequency= / threshold= inside a selector
 * are refused.  Writes at most cap terms and their number; MGC_EINVAL with text in mgc_last_error(NULL) for a word it cannot
 * decode and for everything mgc_select_check refuses. */
int mgc_select_parse(const char *const *words, uint32_t n_words, uint32_t n_inputs, mgc_select_term *terms, uint32_t cap,
                     uint32_t *n_terms);
/* What every entry point that takes a program checks before any launch (MGC_EINVAL, text in mgc_last_error(NULL)): more than
 * MGC_SELECT_MAX_TERMS terms; an unknown quantity or relation; an index below -1 or above n_inputs; both sides of a term the
 * same source; a BASES term that names an input, without letters, or without exactly one k-mer side; an INPUT term that
 * allows a count above n_inputs or requires an input above it. */
int mgc_select_check(const mgc_select_term *terms, uint32_t n_terms, uint32_t n_inputs);
/* The two steps of mgc_dev_merge_many_* with a program ANDed onto the operation's rule.  n_inputs = 1 is accepted.  k: the
 * k-mer size (BASES terms; 1..32 for key_words 1, 1..64 for 2).  d_labels (HOST array of device pointers, entries or the
 * array itself may be NULL = all zeros) and label_op / label_constant (MGC_LABEL_*) feed LABEL terms and d_labels_out (NULL:
 * no labels written).  The count step reads the values when a VALUE or LABEL term or the operation needs them and the labels
 * when a LABEL term is present, and decides exactly what the emit step writes. */
int mgc_dev_merge_many_count_selected(const void *const *d_keys, const uint32_t *const *d_values, const uint64_t *const *d_labels,
                                      const uint64_t *n, uint32_t n_inputs, uint32_t key_words, uint32_t k, int op, int label_op,
                                      uint64_t label_constant, const mgc_select_term *terms, uint32_t n_terms, void *d_workspace,
                                      size_t workspace_bytes, uint64_t *n_out, void *stream);
int mgc_dev_merge_many_emit_selected(const void *const *d_keys, const uint32_t *const *d_values, const uint64_t *const *d_labels,
                                     const uint64_t *n, uint32_t n_inputs, uint32_t key_words, uint32_t k, int op, int label_op,
                                     uint64_t label_constant, const mgc_select_term *terms, uint32_t n_terms, void *d_workspace,
                                     size_t workspace_bytes, void *d_keys_out, uint32_t *d_values_out, uint64_t *d_labels_out,
                                     void *stream);
/* The same for the value operations: "output value" is the value after the operation, @1 the input's value, and INPUT terms
 * see one active input. */
int mgc_dev_select_count_selected(const void *d_keys, const uint32_t *d_values, const uint64_t *d_labels, uint64_t n, uint32_t key_words,
                                  uint32_t k, int value_op, uint64_t constant, int label_op, uint64_t label_constant,
                                  const mgc_select_term *terms, uint32_t n_terms, void *d_workspace, size_t workspace_bytes,
                                  uint64_t *n_out, void *stream);
int mgc_dev_select_emit_selected(const void *d_keys, const uint32_t *d_values, const uint64_t *d_labels, uint64_t n, uint32_t key_words,
                                 uint32_t k, int value_op, uint64_t constant, int label_op, uint64_t label_constant,
                                 const mgc_select_term *terms, uint32_t n_terms, void *d_workspace, size_t workspace_bytes,
                                 void *d_keys_out, uint32_t *d_values_out, uint64_t *d_labels_out, void *stream);

/* ---- value assignment (meryl2) ---------------------------------------------------------------------------------------------
 * value=<word>[#c] after a set or value-filter operation names how the VALUE of a written k-mer comes from the values V[j] of its
 * ACTIVE inputs (the inputs that hold the k-mer, in input order) and the constant c, cut to 32 bits --
 * merylOpCompute::findOutputValue, src/meryl2/merylOpCompute.C:136-282; all arithmetic is on 32-bit kmvalu.  With an assignment
 * the operation supplies only the presence rule (merylCommandBuilder-processText.C:384-442): union* any input, intersect* all
 * inputs, subtract the first input holds it, difference the first input and only it, symmetric-difference exactly one input.  A
 * k-mer whose assigned value is 0 is not written (src/meryl2/merylOp-nextMer.C:119).  A selector's "output value" is the assigned
 * value; labels still see the inputs' values.
 *   NONE      the operation's own rule, exactly as without an assignment                      (valueNOP :142-143)
 *   SET       c                                                                              (:145-147)
 *   FIRST     V[0]: the first ACTIVE input                                                   (:154-157)
 *   SELECTED  V[0].  The reference's valueSelected is a placeholder that takes _acta[0] under a `#warning wrong` (:149-152);
 *             its stated meaning -- the value of the input the assignment selects -- is the first active input's here too, so
 *             SELECTED and FIRST coincide.
 *   MIN MAX   the smallest / largest of c and every V[j]                                     (:159-169)
 *   ADD       c + V[0] + ..., SATURATING at 2^32-1 (:171-178) -- unlike MGC_MERGE_UNION_SUM, which keeps wrapping
 *   SUB       V[0] - V[1] - ... - c; a step that would reach 0 or less gives 0               (:180-194)
 *   MUL       c * V[0] * ..., saturating at 2^32-1 (:196-203).  A running value of 0 stays 0: the reference divides
 *             kmvalumax by it (:199), which is undefined there.
 *   DIV       V[0] / V[1] / ... / c, truncating; a zero divisor gives 0                      (:206-220)
 *   DIVZ      per divisor d (V[1], ..., then c): d == 0 gives 0; running < d gives 1 (also when running is 0, as there);
 *             otherwise round(running / (double)d), computed as (2 * running + d) / (2 * d) in 64-bit integers, which is the
 *             same number for all 32-bit operands                                            (:227-245)
 *   MOD       q = V[0], r = 0; per divisor d (V[1], ..., then c): d > 0: r += q mod d, q = q / d; d == 0: r += q, q = 0;
 *             the value is r, accumulated mod 2^32                                           (:248-275)
 *   COUNT     the number of active inputs                                                    (:278-280)
 * mgc_value_default_constant(assign): the constant the reference uses when the command names none
 * (merylCommandBuilder-isAssign.C:78-91): 2^32-1 for MIN, 1 for MUL, DIV and DIVZ, 0 otherwise.  The reference's float constants
 * for mul / div are not offered. */
#define MGC_ASSIGN_NONE      0
#define MGC_ASSIGN_SET       1
#define MGC_ASSIGN_FIRST     2
#define MGC_ASSIGN_SELECTED  3
#define MGC_ASSIGN_MIN       4
#define MGC_ASSIGN_MAX       5
#define MGC_ASSIGN_ADD       6
#define MGC_ASSIGN_SUB       7
#define MGC_ASSIGN_MUL       8
#define MGC_ASSIGN_DIV       9
#define MGC_ASSIGN_DIVZ     10
#define MGC_ASSIGN_MOD      11
#define MGC_ASSIGN_COUNT    12
uint64_t mgc_value_default_constant(int assign);
/* THE parser of what follows `value=` (the CLI and Python both call it): `word`, `word#c` or `#c` with the words first selected
 * min max add sum sub dif mul div divzero mod rem count (isAssignValue, merylCommandBuilder-isAssign.C:44-103) and c an
 * integer as the selector parser takes them (decimal, 0x.., 0b..).  Without #c the constant is the word's default.  MGC_EINVAL
 * with text in mgc_last_error(NULL): an unknown word, a constant above 2^32-1 or that is no integer, and a constant on count,
 * first or selected (the reference knows no `count#`, `first#` or `selected#`). */
int mgc_value_assign_parse(const char *text, int *assign, uint64_t *constant);
/* The two steps of mgc_dev_merge_many_*_selected with a value assignment: value_assign = MGC_ASSIGN_*, value_constant cut to 32
 * bits.  n_inputs = 1 is accepted and the program may be empty.  The count step reads the values unless the rule is SET or COUNT
 * (and no term asks), and decides exactly what the emit step writes.  MGC_LABEL_SELECTED follows the assignment (MIN, MAX,
 * otherwise FIRST).  MGC_ASSIGN_NONE gives exactly the _selected result; an unknown code: MGC_EINVAL with text. */
int mgc_dev_merge_many_count_assigned(const void *const *d_keys, const uint32_t *const *d_values, const uint64_t *const *d_labels,
                                      const uint64_t *n, uint32_t n_inputs, uint32_t key_words, uint32_t k, int op, int value_assign,
                                      uint64_t value_constant, int label_op, uint64_t label_constant, const mgc_select_term *terms,
                                      uint32_t n_terms, void *d_workspace, size_t workspace_bytes, uint64_t *n_out, void *stream);
int mgc_dev_merge_many_emit_assigned(const void *const *d_keys, const uint32_t *const *d_values, const uint64_t *const *d_labels,
                                     const uint64_t *n, uint32_t n_inputs, uint32_t key_words, uint32_t k, int op, int value_assign,
                                     uint64_t value_constant, int label_op, uint64_t label_constant, const mgc_select_term *terms,
                                     uint32_t n_terms, void *d_workspace, size_t workspace_bytes, void *d_keys_out,
                                     uint32_t *d_values_out, uint64_t *d_labels_out, void *stream);

/* What the library's owning device buffers hold in this process right now: bytes and buffers (either may be NULL).  The
 * session arena, the run store's parked runs and pinned memory are not counted.  For tests and leak hunts: it is exact and
 * process-local, where hipMemGetInfo is device-wide.  Always MGC_OK. */
int mgc_dev_buffers_live(uint64_t *bytes, uint64_t *buffers);

/* Database blocks decoded on the device (mgc_decode.hip): d_file = the bytes of one data file followed by 16 bytes of slack,
 * d_blocks = the mdb_raw_block array of include/meryl_db.h (mdb_reader_raw_file gives both, validated against the file
 * size), suffix_size / label_size as the database's mdb_info has them.  d_keys / d_values / d_labels receive the k-mers of
 * block b from index blocks[b].out_offset on; d_labels may be NULL (labels skipped) and is filled with zeros when
 * label_size is 0, as the host reader does.  MGC_EINVAL with a message when a block is corrupt. */
int mgc_dev_decode_blocks(const void *d_file, const void *d_blocks, uint64_t n_blocks, uint32_t suffix_size, uint32_t label_size,
                          uint32_t key_words, void *d_keys, uint32_t *d_values, uint64_t *d_labels, void *stream);

/* Homopolymer compression of a base stream (the `compress` word: merylInput.C:
 * 237-240,261-268 calls homopolyCompress() on every chunk loadBases returns,
 * carrying the last byte across chunks of a sequence).  Drops every byte equal,
 * ignoring case, to the byte before it; d_out needs n bytes; *n_out = new length.
 * The session applies this itself when cfg.homopoly_compress is set. */
size_t mgc_dev_homopoly_workspace_bytes(uint64_t n);
int mgc_dev_homopoly_compress(const uint8_t *d_in, uint64_t n, uint8_t *d_out, uint64_t *n_out,
                              void *d_workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------
 * Session -- replaces merylOperation::countThreads
 * (src/meryl/merylOp-countThreads.C:385-474).
 * ---------------------------------------------------------------------- */
typedef struct mgc_session mgc_session;

/* cfg must have been through mgc_configure_counting (w_prefix decides the
 * block structure, countThreads.C:404).  device < 0 keeps the current device. */
mgc_session *mgc_open(const mgc_count_config *cfg, int device);
void         mgc_close(mgc_session *s);
const char  *mgc_last_error(const mgc_session *s);   /* s may be NULL: last open/config error */

/* Same contract as merylInput::loadBases's output (merylInput.H:67-70): a run
 * of bases of the current sequence; end_of_sequence != 0 appends the '.'
 * breaker the reference's loader appends (merylOp-countThreads.C:214-215).
 * Bases are copied; the caller may reuse the buffer on return. */
int mgc_push_bases(mgc_session *s, const char *bases, size_t len, int end_of_sequence);

/* Out-of-core input (the analogue of writeBatch's memory-full spill, merylOp-countThreads.C:323-379, and of
 * merylBlockWriter::finish() merging the iterations, :461-464): bases pushed from the host travel through two pinned
 * buffers (asynchronous uploads) into a staging buffer in HBM; when the staged bases -- pushed or parsed from text --
 * reach what one pass can hold, everything up to the last sequence boundary is counted as one BATCH by a worker thread
 * while the caller keeps pushing into a second staging buffer.  A batch's (k-mer, count) result is parked as a sorted
 * RUN -- in HBM while the result budget lasts, in pinned host DRAM otherwise (include/meryl_db.h, mgc_runs_*) -- and the
 * runs are merged ONCE, when the count ends:
 *   - every run still in HBM and their merge fits: one device-resident result, every result call works as after a
 *     single pass;
 *   - otherwise the result is OUT OF CORE (mgc_result_out_of_core() == 1; mgc_get_result_info reports n_distinct = 0
 *     until it has been delivered): mgc_write_database and mgc_finish / mgc_finish_labelled merge the runs chunk by
 *     chunk into the consumer, the calls that hand out the whole result (mgc_copy_result*, mgc_get_result_device)
 *     return MGC_ESTATE.  The result may be larger than HBM; host DRAM bounds it.
 * By default the batch size is derived from the free HBM at the first input (mgc_set_batch_bases overrides it: bases per
 * batch) and the runs may keep 60 % of the HBM that is free when the first batch has been counted
 * (mgc_set_result_budget: bytes; 0 restores the default). */
int mgc_set_batch_bases(mgc_session *s, uint64_t bases_per_batch);
/* Optional, right after mgc_open: about how many bases will be pushed.  The count's largest buffer is then allocated by a
 * helper thread while the caller reads and uploads its input (a first large hipMalloc is slow, and nothing needs the
 * memory before mgc_count).  Ignored when the input is expected to take batches; a wrong estimate only costs time. */
int mgc_prepare(mgc_session *s, uint64_t expected_bases);
int mgc_set_result_budget(mgc_session *s, uint64_t device_bytes);
int mgc_result_out_of_core(const mgc_session *s);

/* Sequence-file TEXT instead of bases: the raw bytes of a FASTA or FASTQ file (after any decompression), in
 * chunks of any size and alignment.  The library stages them through pinned buffers, uploads them and parses
 * them ON THE DEVICE into the same base stream mgc_push_bases builds ('.' between sequences; headers, qualities
 * and line ends dropped) -- the device-side replacement of dnaSeqFile::loadBases behind
 * merylInput::loadBases (src/meryl/merylInput.C:245-271) and of the loader's chunk assembly
 * (src/meryl/merylOp-countThreads.C:138-231).  FASTA may be multi-line; FASTQ must be strict four-line records:
 * every '@' and '+' line start is checked on the device and mgc_end_text returns MGC_EFORMAT if the structure
 * does not hold -- the file's output is then already rolled back and the caller feeds the file through
 * mgc_push_bases instead (include/meryl_seq.h reads multi-line FASTQ).  Text input is batched like pushed bases
 * (a batch may be cut inside a file: if such a file is refused AFTER part of it was counted, mgc_end_text returns
 * MGC_EINVAL instead of MGC_EFORMAT -- nothing can be rolled back then); it may be mixed with mgc_push_bases.
 *
 * SAM text (MGC_TEXT_SAM; also what `samtools view -h` makes of a CRAM): the SEQ column is extracted on the device.  A LINE START is a
 * byte that begins the file or follows '\n'.
 *   line start '\n'   an empty line: emits nothing.
 *   line start '@'    a header line: emits nothing through its '\n', whatever it holds (tabs, any length).
 *   line start '\r'   the file is REFUSED (the host reader skips such bytes before it decides a line's kind; the device does not).
 *   anything else     an alignment line.  A byte's column is the number of '\t' before it in the line.  The bytes of column 9 that are
 *                     not '\t' '\n' '\r' '*' are emitted as they are, nothing else of the line is (columns 10 and up -- QUAL, aux
 *                     fields, any number of tabs -- are ignored), and the line's '\n' emits one '.'.  A '\n' with fewer than 9 tabs
 *                     before it in the line REFUSES the file, as the host reader does ("fewer than 10 columns").
 * A last alignment line without '\n' emits its column-9 bytes if it reaches that column, and nothing (no error) if it does not;
 * mgc_end_text adds its usual single '.'.  No FLAG filtering, no reverse-complementing: SEQ as stored, as the BAM route and the host
 * reader give it.  Refusal works as for FASTQ: mgc_end_text reads the device's error word, rolls the file's output back and returns
 * MGC_EFORMAT (MGC_EINVAL after part of the file was counted); mgc_last_error names the reason.  For every accepted file the stream
 * equals msr_load_stream's for the same bytes (SEQ + '.' per record) plus the end-of-file breaker.  SAM is never sniffed (format 0
 * tells FASTA from FASTQ only: a leading '@' means FASTQ); it is asked for by name wherever a format is taken. */
#define MGC_TEXT_FASTA 1
#define MGC_TEXT_FASTQ 2
#define MGC_TEXT_SAM   3
int mgc_reserve_text(mgc_session *s, uint64_t text_bytes);       /* optional: expected total, avoids regrowth */
int mgc_begin_text(mgc_session *s, int format);
int mgc_push_text(mgc_session *s, const char *text, size_t len);
int mgc_end_text(mgc_session *s);
/* One whole UNCOMPRESSED FASTA/FASTQ file (format 0 = tell from the first record): begin + push + end in one call, the
 * file read by `reader_threads` threads (0 = default) straight into pinned upload buffers.  Return codes as mgc_end_text. */
int mgc_push_text_file(mgc_session *s, const char *path, int format, int reader_threads);
/* A byte window [begin, end) of such a file -- begin at a record start (mgc_text_record_start), end = where the next reader
 * begins (or anything >= the file size): the ranks of a node count read disjoint windows of the input, each through its
 * own device's link.  mgc_text_record_start: the first record start at or after `offset` (FASTA: a line starting with
 * '>'; FASTQ: a line starting with '@' whose next-but-one line starts with '+'; SAM: any line start); the file size when there is none;
 * format 0 = sniff.  Host I/O only, no device. */
int mgc_push_text_file_range(mgc_session *s, const char *path, int format, int reader_threads, uint64_t begin, uint64_t end);
int mgc_text_record_start(const char *path, int format, uint64_t offset, uint64_t *start);
/* One whole BGZF file of FASTA/FASTQ text (bgzip: independent gzip members of <= 64 KiB with their compressed size in a 'BC' extra
 * field, SAMv1 4.1): mapped, its blocks inflated by `threads` threads (0 = default) straight into the pinned upload buffers, uploaded
 * and parsed in order.  The reference reads every compressed input through ONE decoder (its second loader thread,
 * src/meryl/merylOp-countThreads.C:162-168).  MGC_EFORMAT: not BGZF / a corrupt block / neither FASTA nor strict FASTQ (nothing of
 * the file stays in the session unless part of it was already counted as a batch).  mgc_is_bgzf_file: 1 when the file starts with a
 * BGZF block (host I/O only). */
int mgc_push_text_bgzf_file(mgc_session *s, const char *path, int format, int threads);
int mgc_is_bgzf_file(const char *path);

/* A whole FASTA / FASTQ file in PLAIN gzip (one deflate stream per member, any number of members; not BGZF), which has no index of
 * independent blocks: `threads` workers (0: 16) start inflating at guessed deflate block boundaries, one per span of MGC_GZIP_SPAN
 * compressed bytes (default 4 MiB), straight into the pinned upload ring, and write MARKERS where a back-reference reaches into the
 * 32 KiB before their start.  The device, which receives the pieces in stream order, replaces the markers from the text it already
 * holds and computes every member's CRC-32 over the resolved text; CRC32 and ISIZE are compared with the trailers.  A worker's output
 * is taken only when the piece before it ended exactly at its start, so the text is exact whatever was guessed: a file of fixed blocks
 * only, or one where every guess is wrong, inflates serially.  MGC_GZIP_TEXT_CAP: bytes of text per piece (default and most 32 MiB).
 * Bytes after the last member that do not start a gzip member are ignored, as zlib's gzread ignores them.
 * Return codes and rollback as mgc_push_text_bgzf_file: MGC_EFORMAT -- not gzip, a damaged or truncated stream, a CRC32 / ISIZE
 * mismatch, neither FASTA nor strict FASTQ -- leaves nothing of the file in the session; MGC_EINVAL when part of the file was already
 * counted as a batch, or when the file cannot be opened.  mgc_last_error names the file and the compressed offset.
 * info (may be NULL): members read; chunks = spans + cuts; confirmed: spans whose worker's output was taken; discarded: spans whose
 * worker started from a false candidate; text_bytes; symbol_bytes: 16-bit symbols uploaded beside the text; cuts: pieces that continue a
 * worker's output because it did not fit one slot.  mgc_is_gzip_file: 1 when the file starts with a gzip member that is not BGZF. */
typedef struct {
  uint64_t members, chunks, confirmed, discarded;
  uint64_t text_bytes, symbol_bytes, cuts;
} mgc_gzip_info;
int mgc_push_text_gzip_file(mgc_session *s, const char *path, int format, int threads, mgc_gzip_info *info);
int mgc_is_gzip_file(const char *path);

/* The parse alone, device to device, for tests and benchmarks: one whole file of text_bytes at d_text (any alignment) -> its base
 * stream at d_out (room for text_bytes), without mgc_end_text's final '.', on `stream`.  d_workspace: 256-byte aligned,
 * mgc_dev_text_parse_workspace_bytes(text_bytes) bytes; afterwards its first 8 bytes hold the stream's length (uint64) and the
 * uint32 at byte 24 is the error word (not 0: mgc_end_text would refuse the file). */
uint64_t mgc_dev_text_parse_workspace_bytes(uint64_t text_bytes);
int mgc_dev_text_parse(const uint8_t *d_text, uint64_t text_bytes, int format, void *d_workspace, uint8_t *d_out, void *stream);

/* The device side of the above, on buffers of the caller's (any alignment; `stream`: a hipStream_t, NULL: the default stream).
 * mgc_dev_gzip_resolve: d_text[i] = d_symbols[i] < 256 ? d_symbols[i] : d_window_in[d_symbols[i] - 0x8000] for i < n_symbols
 * (<= text_bytes), in place; a symbol in 0x100..0x7FFF ORs 1 into *d_error, a marker below 32768 - window_valid ORs 2, both write 0.
 * d_window_out (NULL: none; never d_window_in): the last 32 KiB of (d_window_in ++ d_text[0 .. text_bytes)), read after the patch.
 * d_window_in may be NULL when window_valid is 0.  mgc_dev_crc32_pieces: d_crc[i] = CRC-32 of d_text[d_begin[i] .. + d_len[i]),
 * d_len[i] <= 4096; zlib's crc32_combine joins them. */
int mgc_dev_gzip_resolve(uint8_t *d_text, uint64_t text_bytes, const uint16_t *d_symbols, uint64_t n_symbols,
                         const uint8_t *d_window_in, uint32_t window_valid, uint8_t *d_window_out, uint32_t *d_error, void *stream);
int mgc_dev_crc32_pieces(const uint8_t *d_text, const uint64_t *d_begin, const uint32_t *d_len, uint64_t n_pieces, uint32_t *d_crc,
                         void *stream);

/* BAM records instead of text: the INFLATED bytes of a BAM file (SAMv1 4.2: magic, header text, reference names, then records
 * of block_size + 32 fixed bytes + read name + CIGAR + SEQ packed two bases per byte + qualities + aux), in pieces of any
 * size.  The host only walks the records -- header fields and the 36 fixed bytes of every record, resumable across pieces --
 * and checks every length the device will rely on; the bytes are uploaded as they are and a kernel expands the SEQ fields
 * into the base stream through the nt16 alphabet "=ACMGRSVTWYHKDBN" (SAMv1 4.2), high nibble first: every record's SEQ as
 * stored, no FLAG filtering, one '.' after every record (a record without SEQ gives just the '.'), as the host reader of
 * include/meryl_seq.h does.  begin / push / end mirror the text triple and share its one "open file": while a BAM is open,
 * mgc_push_bases, mgc_begin_text, mgc_count and mgc_staged_bases return MGC_ESTATE.  A damaged stream (bad magic, a negative
 * l_text / n_ref / l_name / l_seq, block_size < 32, fields longer than the record; at mgc_end_bam: a stream that ends inside
 * the header or a record) is MGC_EFORMAT from the call that sees it: the file is closed and taken back out of the stream,
 * mgc_last_error names the fault and the stream offset.  BAM input is batched like pushed bases (a batch may be cut inside a
 * file, at a '.'): damage found AFTER part of the file was counted is MGC_EINVAL -- nothing can be rolled back then. */
int mgc_begin_bam(mgc_session *s);
int mgc_push_bam(mgc_session *s, const void *bam_bytes, size_t len);   /* inflated BAM bytes, any chunking */
int mgc_end_bam(mgc_session *s);
/* One whole BGZF BAM file (what samtools, SMRT Link and dorado write): mapped, its blocks inflated (CRC checked) by `threads`
 * threads (0 = default) straight into the pinned upload buffers, walked, uploaded and decoded in file order.  MGC_EFORMAT: not
 * BGZF / a corrupt block / a damaged BAM stream (nothing of the file stays in the session unless part of it was already counted
 * as a batch: MGC_EINVAL then); mgc_last_error names the file.  MGC_EINVAL: the file cannot be opened. */
int mgc_push_bam_file(mgc_session *s, const char *path, int threads);
/* The decode alone, device to device, for tests and benchmarks: piece_bytes (< 4 GiB) of inflated BAM at d_piece and n_segments
 * segments of 16 bytes {uint32 src_off; uint32 n_bases | '.' follows << 31; uint64 out_off} that tile [0, out_bytes) in ascending
 * order -> out_bytes at d_out (any alignment), on `stream`.  Offsets that point outside the piece read as 0, never outside. */
int mgc_dev_bam_decode(const uint8_t *d_piece, uint64_t piece_bytes, const void *d_segments, uint64_t n_segments, uint64_t out_bytes,
                       uint8_t *d_out, void *stream);

/* Bases already resident in HBM (breakers included).  The buffer is borrowed
 * until mgc_count returns.  May be called once per session. */
int mgc_push_bases_device(mgc_session *s, const uint8_t *d_bases, uint64_t n_bases);

/* The base stream staged so far -- everything pushed (host bases, parsed text, files), breakers included, resident
 * on the session's device -- without counting it: for callers that route the bases themselves (the `gpus=` option
 * of the CLI hands slices of it to mgc_count_node).  The view is valid until the next push, mgc_count or
 * mgc_close.  MGC_ESTATE once a batch has been counted out of core (the early bases are gone by then). */
int mgc_staged_bases(mgc_session *s, const uint8_t **d_bases, uint64_t *n_bases);

/* Runs histogram -> partition -> per-file radix sort -> run-length count ->
 * block offsets over everything pushed.  Results stay in HBM. */
int mgc_count(mgc_session *s);

/* Owner side of a sharded (multi-GPU) count: the k-mers are already extracted (canonical 2-bit encoding, uint64 for
 * k <= 32, {lo,hi} for k > 32) and laid out FILE-MAJOR in device memory -- file f (the top six bits of the k-mer,
 * merylOp-countThreads.C:255-262 prefix routing restricted to the 64 output files) occupies file_counts[f] consecutive
 * keys, files ascending; files this rank does not own have count 0.  Runs everything mgc_count runs after the
 * partition (grouping passes, LDS finish, blocks) IN PLACE on d_keys; results are read like after mgc_count.
 * The caller must have completed all writes to d_keys (synchronise the producing stream) before the call. */
int mgc_count_partitioned(mgc_session *s, void *d_keys, const uint64_t *file_counts /*[64]*/, void *reserved);

/* The same with a finer granularity: 2^bucket_bits buckets (6..10 bits: the top bucket_bits bits of the k-mer, i.e. every
 * file cut into 2^(bucket_bits-6) ranges), bucket-major, bucket_counts[2^bucket_bits].  A node of N GPUs routes
 * 64*N buckets so that an owner-side bucket is as large as a single-GPU file (a whole file would be N times larger
 * and need a third grouping pass). */
int mgc_count_buckets(mgc_session *s, void *d_keys, uint32_t bucket_bits, const uint64_t *bucket_counts);
/* ... and the packed result -- distinct k-mers ascending, their counts -- written STRAIGHT into the caller's device buffers when
 * it fits (capacity in k-mers; *n_distinct tells): the waves of a sharded count are counted into one pre-sized result instead of
 * being copied out of the session and concatenated (the reference's threads hand their blocks to ONE writer the same way,
 * merylOp-countThreads.C:452-459).  *n_distinct > capacity: nothing was written there, the result is in the session (read it with
 * mgc_copy_result_device) -- the caller grows its buffer.  The session's result views point into the caller's buffers until the
 * next count. */
int mgc_count_buckets_into(mgc_session *s, void *d_keys, uint32_t bucket_bits, const uint64_t *bucket_counts,
                           void *d_out_keys, uint32_t *d_out_counts, uint64_t capacity, uint64_t *n_distinct,
                           const uint64_t *d_fine_hist /* optional (device, uint64[2^15]): k-mers per top FIFTEEN bits over ALL ranks'
                           reads of this batch (mgc_dev_kmer_histogram_fine, summed) -- with bucket_bits <= 8 the owner's grouping passes
                           take their first digit's histogram from it instead of reading the keys for one */);

typedef struct mgc_result_info {
  uint64_t n_bases;
  uint64_t n_instances;           /* k-mer instances (sum of counts) */
  uint64_t n_distinct;
  uint32_t w_prefix, w_data;
  uint64_t n_prefix;
  uint64_t file_instances[MGC_NUM_FILES];   /* instances per file = the 6-bit histogram */
} mgc_result_info;
int mgc_get_result_info(const mgc_session *s, mgc_result_info *info);

/* Device-to-device copy of the result (distinct k-mers ascending, their counts) into caller-owned device buffers of
 * n_distinct keys / counts; completes before returning.  Either pointer may be NULL. */
int mgc_copy_result_device(mgc_session *s, void *d_keys_out, uint32_t *d_counts_out);

/* Device views of the result (valid until mgc_close / the next mgc_count). */
int mgc_get_result_device(const mgc_session *s, const void **d_unique, const uint32_t **d_counts,
                          const uint64_t **d_block_start, uint32_t *key_words);

/* Copies the result to host arrays sized from mgc_get_result_info
 * (keys_lo/keys_hi/counts: n_distinct; block_start: n_prefix+1).  Any pointer
 * may be NULL; keys_hi is zero-filled for k <= 32. */
int mgc_copy_result(const mgc_session *s, uint64_t *keys_lo, uint64_t *keys_hi, uint32_t *counts,
                    uint64_t *block_start);

/* Delivery in the reference's addBlock convention (merylCountArray.C:472-475;
 * merylOp-countThreads.C:452-459): for every file ff, for every prefix of the
 * file in ascending order -- empty blocks included -- cb(ctx, prefix, nKmers,
 * suffix_lo, suffix_hi, counts).  Suffixes are the low w_data bits of the
 * k-mer split in two uint64 halves (suffix_hi is NULL while k <= 32); the
 * callee must not keep the pointers (caller-owned, as in the reference).
 * Files are delivered from up to `host_threads` threads concurrently, one
 * file per thread, exactly like the reference's `omp parallel for` over files. */
typedef int (*mgc_block_cb)(void *ctx, uint64_t prefix, uint64_t n_kmers,
                            const uint64_t *suffix_lo, const uint64_t *suffix_hi,
                            const uint32_t *counts);
int mgc_finish(mgc_session *s, mgc_block_cb cb, void *ctx, int host_threads);

/* The same in meryl2's addCountedBlock convention (src/meryl2/merylCountArray.C:469-471): `labels` is NULL and
 * `label` is the session's constant label (cfg.label_constant) for every k-mer of the block. */
typedef int (*mgc_block_cb2)(void *ctx, uint64_t prefix, uint64_t n_kmers,
                             const uint64_t *suffix_lo, const uint64_t *suffix_hi,
                             const uint32_t *counts, const uint64_t *labels, uint64_t label);
int mgc_finish_labelled(mgc_session *s, mgc_block_cb2 cb, void *ctx, int host_threads);

/* Per-stage device timings of the last mgc_count (HIP events on the session's
 * stream).  Enable before mgc_count. */
#define MGC_STAGE_HISTOGRAM 0
#define MGC_STAGE_PARTITION 1
#define MGC_STAGE_SORT      2
#define MGC_STAGE_RLE       3
#define MGC_STAGE_BLOCKS    4
#define MGC_NUM_STAGES      5
typedef struct mgc_profile {
  double   stage_ms[MGC_NUM_STAGES];
  uint32_t stage_launches[MGC_NUM_STAGES];
  double   sort_pass_ms_total;     /* sum over the radix scatter-pass kernels only */
  uint32_t sort_pass_launches;
  uint64_t sort_pass_keys;         /* keys moved by those launches (sum of n per launch) */
  double   total_ms;
  double   merge_ms;               /* out-of-core: device merges of batch results into the running result (all batches) */
  uint32_t n_batches;              /* batches the input was counted in (1 = single pass) */
  uint32_t narrow_digit_widths;    /* bit b set: a narrowed file's first grouping pass took a digit of b bits (8: the 256-counter kernel, 9: the 512-counter one) */
  /* the same pass launches split by position: [0] a file's first pass, [1] its later passes -- with their ALGORITHMIC
   * bytes (key bytes read + written; narrowed files: 8 + 4 in the first pass, 4 + 4 in the second) */
  double   pass_ms[2];
  uint64_t pass_bytes[2];
  uint64_t pass_keys[2];
  uint32_t pass_launches[2];
  /* the sub-bucket count kernels (hash_count* / bitmap_count / lds_sort_count: one launch per file, on two alternating
   * streams): sum of the launches' own durations (HIP events on the stream each is launched on), their ALGORITHMIC bytes
   * (the keys read: 4 B narrowed, 8 / 16 B otherwise; the distinct suffixes + counts written) and keys */
  double   finish_ms;
  uint64_t finish_bytes, finish_keys;
  uint32_t finish_launches;
  uint32_t wide_msd_files;         /* files whose WHOLE keys took the high-digit-first grouping passes (mgc_device.h, launch_group_wide) */
  /* round 6: which plans the files took */
  uint32_t stream_files;           /* files on the distinct-sized count (hash_count_stream_kernel) and its coarser sub-buckets */
  uint32_t k96_files;              /* files that lay as 12-byte K96 records (k = 33..51) */
  uint32_t k96_widened_files;      /* ... of which widened back to 16-byte keys (an oversized sub-bucket nothing streams) */
  uint32_t hpc_mixed_files;        /* `compress` buckets grouped by a dense-rank high digit + the plain eight bits of four bases (3^9 sub-buckets) */
  uint64_t stream_retries;         /* sub-buckets with more distinct suffixes than that kernel's table holds (counted by its retry launch) */
  double   probe_ratio;            /* distinct / instances of the probe file that chose between the plans (0: no probe ran) */
  /* what the rest of the count stage lasts (offsets of the sub-buckets in the packed result + the packing kernels of all files), on
   * the session stream behind the count kernels: stage_ms[MGC_STAGE_RLE] - pack_ms = the wall clock of the count kernels themselves.
   * With early packing (early_pack_files below) that is only the part of the packing the count kernels do not hide */
  double   pack_ms;
  uint64_t hist_bytes;             /* ALGORITHMIC bytes of the histogram kernel (the bases read + the packed base stream it stores, 6 bytes per
                                    * 16 bases, where the count has one: not with MGC_PACKED_BASES=0) ... */
  uint64_t partition_bytes;        /* ... and of the partition (the packed base stream read -- without one, the bases -- + the k-mers written in
                                    * the layout the files take: 5 / 8 / 12 / 16 B) */
  /* kernel launches of the first / the second grouping pass: pass_launches[] counts one per FILE and pass whether or not files shared a
   * launch; a batched launch over m files (mgc_device.h, GroupBatch) adds m there and 1 here */
  uint32_t pass_kernel_launches[2];
  /* early packing (files packed on a third stream while later files are still counted; MGC_PACK_OVERLAP=0: off): files packed by
   * the chain on that stream (not deferred; WHEN their launches ran against the count kernels a kernel trace shows, not this number),
   * and files the device deferred to the serial path behind the last count kernel (a retry list, a result without room).  Both 0:
   * the count took the serial path for every file.  pack_ms is only the part of the packing the count kernels did not hide: from
   * the end of the last count kernel to the end of the last packing launch */
  uint32_t early_pack_files, early_pack_deferred;
  int32_t  probe_file;             /* the file that was counted first to choose the others' plan (probe_ratio); -1: no probe ran */
  uint32_t wide_digit_widths;      /* whole-key files on the high-digit-first passes (wide_msd_files), ORed over them: bit b set: a HIGH digit of b
                                    * bits (the plan's pass_bits[1]); bit 16 + b: a LOW digit of b bits (pass_bits[0]).  `compress`: the ten-bit
                                    * field of a dense-rank digit counts as 10 */
  /* gigantic sub-buckets (above 65536 keys: cut into slices, the slices' pairs merged; the dense ones counted by 64 ranges of the suffix
   * space), summed over the files of the count -- which path ran, counted on the device:
   *   huge_cut, huge_slices   sub-buckets cut and the slices planned for them (MGC_HUGE_SLICES=0: both stay 0, and so does huge_dense)
   *   huge_dense              cut sub-buckets a slice marked dense (more distinct suffixes than 1/8 of the slice's keys)
   *   huge_repasses[m]        passes that overflowed their table and were run again over a narrower suffix range: [0] an oversized
   *                           sub-bucket that is not cut, [1] a slice, [2] the merge of a sub-bucket's pairs, [3] a range of a dense one
   *   huge_empty_ranges       ranges of dense sub-buckets that held no suffix (equal splitters: a heavy k-mer) */
  uint32_t huge_cut, huge_slices, huge_dense;
  uint32_t huge_repasses[4];
  uint32_t huge_empty_ranges;
} mgc_profile;
int mgc_set_profiling(mgc_session *s, int enable);
int mgc_get_profile(const mgc_session *s, mgc_profile *p);

/* ------------------------------------------------------------------------
 * Bench/test utility: deterministic synthetic reads generated in HBM
 * (byte-identical to oracle/oracle_count.c orc_synth_reads).
 * ---------------------------------------------------------------------- */
int mgc_dev_synth_reads(uint64_t seed, uint64_t genome_len, uint64_t first_read, uint64_t n_reads,
                        uint32_t read_len, uint32_t sub_rate_ppm, uint32_t n_rate_ppm,
                        uint8_t *d_out, void *stream);
/* ... with repeat families in the genome: repeat_ppm of its `repeat_unit`-base blocks show one of
 * `repeat_families` template sequences, family 0 by far the most frequent (byte-identical to orc_synth_reads_ex). */
int mgc_dev_synth_reads_ex(uint64_t seed, uint64_t genome_len, uint64_t first_read, uint64_t n_reads,
                           uint32_t read_len, uint32_t sub_rate_ppm, uint32_t n_rate_ppm,
                           uint32_t repeat_ppm, uint32_t repeat_unit, uint32_t repeat_families,
                           uint8_t *d_out, void *stream);

/* Library/ABI version: major<<16 | minor. */
uint32_t mgc_version(void);

#ifdef __cplusplus
}
#endif
#endif /* MERYL_GPU_COUNT_H */
