/*
 * meryl_db.h -- C ABI of the meryl database writer/reader (the downstream
 * side of the count path).
 *
 * Replaces, for the count path only, the reference's
 *   merylFileWriter(name) / ::initialize(wPrefix) / ::getBlockWriter()
 *   merylBlockWriter::addBlock(prefix, nKmers, suffixes, counts) / finish()
 * whose call sites are src/meryl/merylOp.C:262,
 * src/meryl/merylOp-countThreads.C:48,404,453-464 and
 * src/meryl/merylCountArray.C:472-475.  Those classes live in the absent
 * submodule marbl/meryl-utility (utility/src/kmers-v1/kmers-writer*.C), so
 * the BYTE LAYOUT written here is a restatement of that library's published
 * v1 format from its documented shape (documentation/source/usage.rst:13-45,
 * reference.rst:73-77) and is marked PARITY UNPINNED: no reference-written
 * database exists in the tree to diff against.  Every layout assumption is
 * listed in DESIGN.md ("database encoding").  What IS pinned: 64 data files +
 * 64 index files + one master `merylIndex`; prefixSize / suffixSize /
 * numFilesBits=6 / numBlocksBits=prefixSize-6; block header fields
 * prefix nKmers kCode uBits bBits k1 cCode c1 c2 with uBits+bBits=suffixSize.
 */
#ifndef MERYL_DB_H
#define MERYL_DB_H

#include <stddef.h>
#include <stdint.h>

#include "meryl_gpu_count.h"   /* MGC_MERGE_* */

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mdb_writer mdb_writer;
typedef struct mdb_reader mdb_reader;
struct mgc_session;

/* Creates directory `path` (merylFileWriter ctor, merylOp.C:262) and fixes the
 * geometry (merylFileWriter::initialize(wPrefix), countThreads.C:404). */
mdb_writer *mdb_writer_open(const char *path, uint32_t k, uint32_t w_prefix);

/* The same with two extensions:
 *  label_size  bits of label stored per k-mer (0..64; 0 = none: the bytes written are then exactly the unlabelled ones).
 *              meryl2 sets it with the global `-l <bits>` (src/meryl2/merylGlobals.C:75-77) and its count hands ONE constant
 *              label to the writer at dump time: addCountedBlock(prefix, nKmers, suffix, counts, labels=nullptr, label)
 *              (src/meryl2/merylCountArray.C:469-471, src/meryl2/merylOp-countThreads.C:363-367,464-468).
 *  part / n_parts  a database written by several writers, one per rank of a sharded (multi-GPU) count: writer `part`
 *              receives the blocks of a contiguous prefix range (ranges ascend with `part`; a range may begin or end in
 *              the middle of a file).  It writes `0xBBBBBB.merylData.part<part>` files and a side file; once every part
 *              is closed, ONE caller runs mdb_merge_parts, which stitches the data files (rename when a file has one
 *              contributor, append otherwise), and writes the 64 per-file indexes and the master index.  The resulting
 *              directory is byte-identical to what a single writer fed the same blocks produces.  n_parts = 1, part = 0
 *              is the plain writer. */
mdb_writer *mdb_writer_open_ex(const char *path, uint32_t k, uint32_t w_prefix, uint32_t label_size,
                               uint32_t part, uint32_t n_parts);
int mdb_merge_parts(const char *path, uint32_t n_parts);

/* merylBlockWriter::addBlock.  May be called concurrently from several threads
 * as long as each FILE (prefix >> (w_prefix-6)) is fed by one thread with
 * ascending prefixes -- the reference's convention (countThreads.C:452-459).
 * suffix_hi may be NULL when 2k - w_prefix <= 64.  Arrays are not retained. */
int mdb_writer_add_block(mdb_writer *w, uint64_t prefix, uint64_t n_kmers,
                         const uint64_t *suffix_lo, const uint64_t *suffix_hi, const uint32_t *counts);

/* merylBlockWriter::addCountedBlock of meryl2 (src/meryl2/merylCountArray.C:469-471): per-k-mer labels, or -- labels ==
 * NULL -- the one constant `label` for every k-mer of the block.  Only the low label_size bits are stored. */
int mdb_writer_add_block_labelled(mdb_writer *w, uint64_t prefix, uint64_t n_kmers,
                                  const uint64_t *suffix_lo, const uint64_t *suffix_hi, const uint32_t *counts,
                                  const uint64_t *labels, uint64_t label);

/* Blocks that are already encoded (the device encoder behind mgc_write_database): `nbytes` bytes of data file ff holding
 * the blocks `entries` list (prefixes ascending and after everything file ff has received so far; entries[i].position
 * is the block's offset inside `bytes`); bytes before the first entry -- or all of them when n_entries is 0 -- continue
 * the block the previous call ended in (a block larger than the caller's copy buffer arrives in pieces).  Same threading rule as mdb_writer_add_block (one thread per file).  The value
 * histogram of such blocks is handed over separately, once or in pieces: (value, occurrences) pairs. */
typedef struct mdb_index_entry { uint64_t prefix, position, n_kmers; } mdb_index_entry;
int mdb_writer_add_encoded(mdb_writer *w, uint32_t ff, const void *bytes, uint64_t nbytes,
                           const mdb_index_entry *entries, uint64_t n_entries);
/* The same in two steps, so that many threads can write ONE file at once: reserve (same ordering rule as above, no data)
 * registers the index entries and returns the file offset the nbytes belong at; mdb_writer_write_at then puts them
 * there with pwrite -- thread-safe, in any order, from any thread. */
int mdb_writer_reserve_encoded(mdb_writer *w, uint32_t ff, uint64_t nbytes, const mdb_index_entry *entries,
                               uint64_t n_entries, uint64_t *file_offset);
int mdb_writer_write_at(mdb_writer *w, uint32_t ff, uint64_t file_offset, const void *bytes, uint64_t nbytes);
int mdb_writer_add_histogram(mdb_writer *w, const uint64_t *values, const uint64_t *occurrences, uint64_t n_pairs);

/* merylBlockWriter::finish() + ~merylFileWriter(): per-file indexes, master
 * index with the value histogram.  Frees the writer.  0 on success. */
int mdb_writer_close(mdb_writer *w);
/* Frees a writer without writing the indexes (error paths: nothing that looks like a finished database is left behind). */
void mdb_writer_discard(mdb_writer *w);

const char *mdb_last_error(void);

typedef struct mdb_info {
  uint32_t k;
  uint32_t prefix_size, suffix_size, num_files_bits, num_blocks_bits, flags;
  uint64_t num_unique, num_distinct, num_total;   /* histogram header */
  uint64_t hist_len;                              /* number of (value, occurrences) pairs */
  uint32_t label_size;                            /* bits of label per k-mer (flags bits 8..15) */
  uint32_t reserved;
} mdb_info;

mdb_reader *mdb_reader_open(const char *path);
int  mdb_reader_info(const mdb_reader *r, mdb_info *info);
/* histogram pairs, each array hist_len long */
int  mdb_reader_histogram(const mdb_reader *r, uint64_t *values, uint64_t *occurrences);
/* All k-mers of file ff (0..63) in stored order as full k-mers (prefix<<suffixSize|suffix).
 * Arrays are malloc'd; release with mdb_free.  keys_hi is NULL-filled (zeros) for k <= 32. */
int  mdb_reader_read_file(mdb_reader *r, uint32_t ff, uint64_t **keys_lo, uint64_t **keys_hi,
                          uint32_t **counts, uint64_t *n_kmers);
/* ... and their labels (zeros when the database stores none); labels may be NULL. */
int  mdb_reader_read_file_ex(mdb_reader *r, uint32_t ff, uint64_t **keys_lo, uint64_t **keys_hi,
                             uint32_t **counts, uint64_t **labels, uint64_t *n_kmers);
/* The per-file index (1 << num_blocks_bits entries) and the header of the block at a data-file position: what
 * `meryl dumpFile` prints (src/meryl/meryl.C:41-45; shape documentation/source/usage.rst:24-45). */
typedef struct mdb_block_header {
  uint64_t prefix, n_kmers;
  uint32_t k_code, unary_bits, binary_bits, c_code;
  uint64_t k1, c1, c2;
} mdb_block_header;
int  mdb_reader_file_index(mdb_reader *r, uint32_t ff, mdb_index_entry *entries);
int  mdb_reader_block_header(mdb_reader *r, uint32_t ff, uint64_t position, mdb_block_header *h);
/* One block decoded the way dumpFile lists it: for k-mer i the unary prefix delta, the accumulated top part, the two
 * halves of the binary remainder and the value; arrays of n_kmers entries, malloc'd (mdb_free). */
int  mdb_reader_read_block_raw(mdb_reader *r, uint32_t ff, uint64_t position, mdb_block_header *h,
                               uint64_t **prefix_delta, uint64_t **top, uint64_t **rem_hi, uint64_t **rem_lo,
                               uint32_t **values);
/* For a decoder that does not run on the host (meryl_amd/csrc/mgc_decode.hip): the raw bytes of data file ff (malloc'd, *size
 * bytes followed by 16 zero bytes) and, for every block of its index that holds k-mers, where its stuffedBits object lies
 * and how long it is -- every object's framing validated against the file size, out_offset = k-mers of the blocks before it.
 * MGC_EUNSUPPORTED when an object is framed in a way only the host decoder follows (mdb_reader_read_file_ex reads it). */
typedef struct mdb_raw_block { uint64_t object_offset, n_bits, n_sub_blocks, n_kmers, prefix, out_offset; } mdb_raw_block;
int  mdb_reader_raw_file(mdb_reader *r, uint32_t ff, unsigned char **bytes, uint64_t *size, mdb_raw_block **blocks,
                         uint64_t *n_blocks, uint64_t *n_kmers);
void mdb_reader_close(mdb_reader *r);
void mdb_free(void *p);

/* ------------------------------------------------------------------------
 * Device-resident (k-mer, count) streams -> database files, encoded ON THE DEVICE
 * (meryl_amd/csrc/mgc_encode.hip) -- the MI355X replacement of the 64 host threads that run
 * countKmers + dumpCountedKmers -> merylBlockWriter::addBlock per file
 * (src/meryl/merylOp-countThreads.C:452-459, src/meryl/merylCountArray.C:472-475): the host only copies finished
 * file bytes out of HBM through pinned buffers and writes them.
 *
 * A stream is one writer (or one part of a sharded database, see mdb_writer_open_ex) fed with ascending,
 * non-overlapping prefix ranges.  mgc_db_stream_write queues one range: d_keys/d_counts are DEVICE pointers to the
 * n distinct k-mers (uint64, or {lo,hi} pairs for k > 32; ascending) whose prefixes lie in [prefix_begin, prefix_end)
 * and their counts; every prefix of the range gets its block, empty ones included.  The call returns once the range
 * is planned; encoding, the device-to-host copies and the file writes run on the stream's own threads, so the
 * caller can go on counting (a sharded count writes the buckets of wave i while wave i+1 is exchanged and counted).
 * The buffers must stay valid and unchanged until mgc_db_stream_sync or mgc_db_stream_close returns.
 * Errors are sticky: the first one is returned by every later call; mgc_db_stream_error gives the text. */
typedef struct mgc_db_stream mgc_db_stream;
typedef struct mgc_db_write_profile {
  double   plan_ms;        /* block offsets + sizes + histogram kernels, planning */
  double   encode_ms;      /* device encode kernels (HIP events) */
  double   copy_write_s;   /* wall clock of device-to-host copies + file writes (overlapped with each other) */
  double   total_s;        /* open -> close */
  uint64_t data_bytes;     /* bytes of .merylData written */
  uint64_t n_kmers, n_blocks;
} mgc_db_write_profile;
mgc_db_stream *mgc_db_stream_open(const char *path, uint32_t k, uint32_t w_prefix, uint32_t label_size, uint64_t label,
                                  uint32_t part, uint32_t n_parts, int host_threads, int device);
int  mgc_db_stream_write(mgc_db_stream *d, const void *d_keys, const uint32_t *d_counts, uint64_t n,
                         uint64_t prefix_begin, uint64_t prefix_end);
/* The same with one label per k-mer (d_labels: n device uint64; NULL = the stream's constant label, i.e. exactly
 * mgc_db_stream_write): the low label_size bits (mgc_db_stream_open) of every label are stored, as
 * mdb_writer_add_block_labelled stores them. */
int  mgc_db_stream_write_labelled(mgc_db_stream *d, const void *d_keys, const uint32_t *d_counts, const uint64_t *d_labels,
                                  uint64_t n, uint64_t prefix_begin, uint64_t prefix_end);
int  mgc_db_stream_sync(mgc_db_stream *d);
/* Waits for everything queued, closes the writer (a part: its side file; the plain writer: indexes + master index)
 * and frees the stream.  prof may be NULL. */
int  mgc_db_stream_close(mgc_db_stream *d, mgc_db_write_profile *prof);
const char *mgc_db_stream_error(const mgc_db_stream *d);      /* d may be NULL: last open error of this thread */

/* mgc_db_stream_queued: ranges queued so far (the number of the last one).  mgc_db_stream_wait_buffers: ranges 1 .. upto
 * have been encoded and copied out of their device buffers, which may be reused; the file writes of the copied pieces may
 * still be running. */
uint64_t mgc_db_stream_queued(mgc_db_stream *d);
uint64_t mgc_db_stream_done(mgc_db_stream *d);      /* ranges 1 .. this have left their device buffers */
int  mgc_db_stream_wait_buffers(mgc_db_stream *d, uint64_t upto);

/* ------------------------------------------------------------------------
 * Sorted runs of partial results -- the spill of an out-of-core count.
 *
 * What it replaces: merylOperation::countThreads writes every bucket of a full memory as an ITERATION of the output
 * files (writeBatch, src/meryl/merylOp-countThreads.C:285-380, finishBatch :362) and merylBlockWriter::finish() merges
 * the iterations of every file at the end (:461-464; the merge itself is in the absent meryl-utility): the size of a count
 * is bounded by disk, not by memory.  Here a batch's (k-mer, count) result is a RUN: ascending distinct k-mers with their
 * counts.  A run stays in HBM while the store's device budget lasts and is parked in pinned host DRAM otherwise (one
 * asynchronous device-to-host copy behind the next batch's count).  At the end the runs are merged ONCE: the k-mer space is
 * walked in slices (top min(w_prefix, 14) bits), consecutive slices are gathered into chunks that fit the device, every
 * run's piece of the chunk is uploaded (host runs) or used in place (device runs), the pieces are merged pairwise on the
 * device (counts of equal k-mers add, uint32 wrap like the reference's value arithmetic) and the merged chunk goes to
 * the database stream -- uploads of chunk i+1 overlap the encode + write of chunk i.  Nothing is rewritten per batch.
 * The sharded / node counts park one run per (batch, wave) on the owner and merge the owner's prefix range the same way.
 *
 * device_budget_bytes: bytes of runs that may stay in HBM (0: every run goes to the host; ~0: no limit).
 * chunk_bytes: device memory the final merge may use for its buffers (0: a quarter of the free HBM, at most 24 GiB).
 * Environment (tests): MGC_OOC_BUDGET, MGC_OOC_CHUNK override both.  Failure text: mgc_runs_error(). */
typedef struct mgc_runs mgc_runs;
typedef struct mgc_runs_profile {
  uint32_t n_runs, n_host_runs;
  uint64_t n_entries;          /* (k-mer, count) pairs over all runs */
  uint64_t device_bytes, host_bytes;
  uint64_t n_merged;           /* distinct k-mers delivered by mgc_runs_write so far */
  uint32_t n_chunks;
  double   spill_s;            /* wall clock of the device-to-host copies (incl. pinning the host memory) */
  double   upload_s, merge_ms, deliver_s;
  uint64_t peak_hbm_bytes;     /* device memory in use (all of the process) at its highest sampled point */
} mgc_runs_profile;
mgc_runs *mgc_runs_open(uint32_t k, uint32_t w_prefix, int device, uint64_t device_budget_bytes, uint64_t chunk_bytes);
/* copies the n ascending distinct k-mers at d_keys (uint64, or {lo,hi} for k > 32) and their counts into a new run;
 * `stream`: where they were produced.  Returns when the source may be overwritten. */
int  mgc_runs_add(mgc_runs *r, const void *d_keys, const uint32_t *d_counts, uint64_t n, void *stream);
/* merges all runs over prefixes [prefix_begin, prefix_end) into d (ranges ascending, see mgc_db_stream_write) */
int  mgc_runs_write(mgc_runs *r, mgc_db_stream *d, uint64_t prefix_begin, uint64_t prefix_end);
int  mgc_runs_get_profile(const mgc_runs *r, mgc_runs_profile *p);
const char *mgc_runs_error(const mgc_runs *r);                 /* r may be NULL: last open error of this thread */
void mgc_runs_close(mgc_runs *r);
/* the run store of a session that counted in batches (zeros when it counted in one pass) */
int  mgc_get_runs_profile(const struct mgc_session *s, mgc_runs_profile *p);

/* Count result of a session -> database directory, through a device stream (results that live in HBM, or -- out of
 * core -- in the session's runs; host_threads file-writer threads).  prof may be NULL. */
int mgc_write_database(struct mgc_session *s, const char *path, int host_threads);
int mgc_write_database_profiled(struct mgc_session *s, const char *path, int host_threads, mgc_db_write_profile *prof);

/* `union-sum` and friends over whole databases (op = MGC_MERGE_* of include/meryl_gpu_count.h): the reference streams the
 * 64 file slices of its inputs through merylOperation::nextMer (src/meryl/merylOp-nextMer.C:418-683, slices
 * src/meryl/meryl.C:250-263); here every slice is decoded by host threads, merged two inputs at a time on the device,
 * encoded on the device and written to `output` (geometry of the first input).  All inputs must hold the same k.
 * Text of a failure: mgc_db_stream_error(NULL). */
int mgc_db_merge(const char *const *inputs, uint32_t n_inputs, int op, const char *output, int device, int host_threads);
/* The single-input operations over a whole database (value_op = MGC_VALUE_*: less-than ... not-equal-to against `constant`,
 * increase ... modulo by it; src/meryl/merylOp-nextMer.C:490-557): k-mers whose new value is 0 are not written. */
int mgc_db_filter(const char *input, int value_op, uint64_t constant, const char *output, int device, int host_threads);

/* A whole tree of merge and value operations over databases, evaluated file slice by file slice with every intermediate
 * result kept in HBM -- what the reference does when operations are nested on one command line (the inputs of a
 * merylOperation are other operations, src/meryl/merylOp-nextMer.C:418-683; only operations given `output` write,
 * :227).  nodes[]: a leaf names its database in `path`; an inner node holds a MGC_MERGE_* (merge) or MGC_VALUE_* + constant
 * (value) operation over children[first_child .. first_child + n_children), and writes a database to `path` unless it is
 * NULL -- the slice goes on to the parent either way.  Per file slice 0..63: every leaf's slice is loaded once, the nodes
 * are evaluated bottom-up (a merge of 3..MGC_MERGE_MANY_MAX inputs in one pass pair, mgc_dev_merge_many_*; more inputs, or
 * every merge under MGC_MERGE_MANY=0 in the environment, by the left fold of mgc_db_merge), and the root's slice is handed to
 * `cb` (may be NULL) as host arrays, from the calling thread, files ascending.  An output has the prefix size of its
 * leftmost leaf, no labels, and the files a staged run through mgc_db_merge / mgc_db_filter writes for that node, byte for
 * byte.  Checked before any device call and before any output directory exists (MGC_EINVAL, text: mgc_db_stream_error(NULL)):
 * indices in range, every node reached at most once, a leaf without children, a value node with exactly one, a merge node
 * with at least one; every leaf opens, holds the same k and neither labels nor a multiset; no output named twice or also
 * a leaf. */
#define MGC_NODE_DATABASE 0
#define MGC_NODE_MERGE    1
#define MGC_NODE_VALUE    2
typedef struct mgc_eval_node {
  int32_t     kind;                /* MGC_NODE_* */
  int32_t     op;                  /* MGC_MERGE_* / MGC_VALUE_* (ignored for a leaf) */
  uint64_t    constant;            /* value operations */
  const char *path;                /* leaf: the database; inner node: its output, or NULL */
  uint32_t    first_child, n_children;   /* range of children[] */
} mgc_eval_node;
/* hi_or_null: NULL for k <= 32; values: uint32 per k-mer; the arrays are valid during the call only */
typedef void (*mgc_eval_slice_cb)(void *ctx, uint32_t file, const uint64_t *lo, const uint64_t *hi_or_null,
                                  const uint32_t *values, uint64_t n);
int mgc_db_eval(const mgc_eval_node *nodes, uint32_t n_nodes, const uint32_t *children, uint32_t n_children, uint32_t root,
                mgc_eval_slice_cb cb, void *ctx, int device, int host_threads);

/* The same over databases that may store LABELS (meryl2's `-l <bits>`): every node also names how the label of a written
 * k-mer comes from the labels of the inputs that hold it -- label_op = MGC_LABEL_* (include/meryl_gpu_count.h, from
 * merylOpCompute::findOutputLabel, src/meryl2/merylOpCompute.C:286-395) and label_constant, taken as given
 * (mgc_label_default_constant names the reference's default).  Leaves are decoded with their labels (zeros where a
 * database stores none), labels travel between nodes as full 64-bit values, and an output stores their low `label_size`
 * bits; label_size = 0 means the largest label_size among the leaves.  When that is 0 too the outputs are byte-identical
 * to mgc_db_eval's.  `cb` also receives the root's labels (uncut).
 * Everything mgc_db_eval checks is checked here in the same way, before any device call and before any output directory
 * exists (a multiset leaf is still refused; a labelled leaf is what this entry point is for), and also: an unknown label
 * operation; MGC_LABEL_INVERT on a node with two or more inputs; a merge node with more than MGC_MERGE_MANY_MAX inputs --
 * the left fold that mgc_db_eval falls back on cannot express DIFFERENCE, MIN or LIGHTEST over all inputs at once.  Every
 * merge node goes through mgc_dev_merge_many_* here (a one-input merge included); MGC_MERGE_MANY=0 in the environment has
 * no effect on this entry point. */
typedef struct mgc_eval_node_labelled {
  int32_t     kind;                /* MGC_NODE_* */
  int32_t     op;                  /* MGC_MERGE_* / MGC_VALUE_* (ignored for a leaf) */
  uint64_t    constant;            /* value operations */
  const char *path;                /* leaf: the database; inner node: its output, or NULL */
  uint32_t    first_child, n_children;   /* range of children[] */
  int32_t     label_op;            /* MGC_LABEL_* (ignored for a leaf) */
  int32_t     reserved;
  uint64_t    label_constant;
} mgc_eval_node_labelled;
typedef void (*mgc_eval_slice_labelled_cb)(void *ctx, uint32_t file, const uint64_t *lo, const uint64_t *hi_or_null,
                                           const uint32_t *values, const uint64_t *labels, uint64_t n);
int mgc_db_eval_labelled(const mgc_eval_node_labelled *nodes, uint32_t n_nodes, const uint32_t *children, uint32_t n_children,
                         uint32_t root, uint32_t label_size, mgc_eval_slice_labelled_cb cb, void *ctx, int device, int host_threads);

/* The same with SELECTORS (meryl2; include/meryl_gpu_count.h: mgc_select_term, mgc_select_parse): a node may also name a program,
 * terms[first_term .. first_term + n_terms) of one terms array, that is ANDed onto the node's own rule for what is written.
 * A node with a program always goes through mgc_dev_merge_many_*_selected (a merge of one input included) or
 * mgc_dev_select_*_selected; a node without one takes exactly the route it takes today -- mgc_db_eval's when labels do not
 * travel (the left fold and MGC_MERGE_MANY=0 included), mgc_db_eval_labelled's when they do.  Labels travel when with_labels
 * or label_size is non-zero, or when any node's program holds a LABEL term; otherwise leaves that store labels are refused
 * as mgc_db_eval refuses them and `cb` receives zeros for labels.  With labels travelling and no program anywhere the outputs
 * are mgc_db_eval_labelled's, byte for byte.
 * Checked with everything the other two entry points check, before any device call and before any output directory exists
 * (MGC_EINVAL with text): a program on a database node; a range outside terms[]; more than MGC_SELECT_MAX_TERMS terms; a
 * merge node with a program and more than MGC_MERGE_MANY_MAX inputs; and per term what mgc_select_check refuses for the
 * node's input count -- an index above it, a count above it, both sides the same source, a BASES term that names an input. */
typedef struct mgc_eval_node_selected {
  int32_t     kind;                /* MGC_NODE_* */
  int32_t     op;                  /* MGC_MERGE_* / MGC_VALUE_* (ignored for a leaf) */
  uint64_t    constant;            /* value operations */
  const char *path;                /* leaf: the database; inner node: its output, or NULL */
  uint32_t    first_child, n_children;   /* range of children[] */
  int32_t     label_op;            /* MGC_LABEL_* (ignored for a leaf) */
  int32_t     reserved;
  uint64_t    label_constant;
  uint32_t    first_term, n_terms; /* range of terms[]; n_terms = 0: no selector */
} mgc_eval_node_selected;
int mgc_db_eval_selected(const mgc_eval_node_selected *nodes, uint32_t n_nodes, const uint32_t *children, uint32_t n_children,
                         uint32_t root, const mgc_select_term *terms, uint32_t n_terms, int with_labels, uint32_t label_size,
                         mgc_eval_slice_labelled_cb cb, void *ctx, int device, int host_threads);

/* The same with VALUE ASSIGNMENT (meryl2's value=<word>[#c]; include/meryl_gpu_count.h: MGC_ASSIGN_*, mgc_value_assign_parse): a
 * node may also name how the value of a written k-mer comes from the values of the inputs that hold it.  A node with an
 * assignment keeps only the presence rule of its operation, writes no k-mer whose assigned value is 0, and shows the assigned
 * value to its selector program; on a value FILTER node (MGC_VALUE_LESS_THAN .. MGC_VALUE_NOT_EQUAL_TO) the filter tests the
 * assigned value.  MGC_LABEL_SELECTED on such a node follows the assignment (MIN, MAX, otherwise FIRST).  Such a node always goes
 * through mgc_dev_merge_many_*_assigned (one input included); a node with MGC_ASSIGN_NONE takes exactly the route it takes in
 * mgc_db_eval_selected, and a tree with no assignment anywhere gives that entry point's outputs byte for byte.  The stored
 * histogram of an output describes the assigned values.  The other parameters are mgc_db_eval_selected's.
 * Checked with everything mgc_db_eval_selected checks, before any device call and before any output directory exists
 * (MGC_EINVAL with text): an unknown assign code; an assignment on a database node or on an arithmetic value node
 * (MGC_VALUE_INCREASE .. MGC_VALUE_MODULO -- the operation word is one); a merge node with an assignment and more than
 * MGC_MERGE_MANY_MAX inputs. */
typedef struct mgc_eval_node_assigned {
  int32_t     kind;                /* MGC_NODE_* */
  int32_t     op;                  /* MGC_MERGE_* / MGC_VALUE_* (ignored for a leaf) */
  uint64_t    constant;            /* value operations */
  const char *path;                /* leaf: the database; inner node: its output, or NULL */
  uint32_t    first_child, n_children;   /* range of children[] */
  int32_t     label_op;            /* MGC_LABEL_* (ignored for a leaf) */
  int32_t     reserved;
  uint64_t    label_constant;
  uint32_t    first_term, n_terms; /* range of terms[]; n_terms = 0: no selector */
  int32_t     value_assign;        /* MGC_ASSIGN_*; MGC_ASSIGN_NONE: the operation's own value rule */
  int32_t     reserved2;
  uint64_t    value_constant;      /* cut to 32 bits; taken as given (mgc_value_default_constant names the reference's default) */
} mgc_eval_node_assigned;
int mgc_db_eval_assigned(const mgc_eval_node_assigned *nodes, uint32_t n_nodes, const uint32_t *children, uint32_t n_children,
                         uint32_t root, const mgc_select_term *terms, uint32_t n_terms, int with_labels, uint32_t label_size,
                         mgc_eval_slice_labelled_cb cb, void *ctx, int device, int host_threads);

/* ------------------------------------------------------------------------
 * The value histogram of device-resident values (meryl_amd/csrc/mgc_value_hist.hip): value -> number of k-mers that carry it,
 * what merylHistogram collects per compute thread and `output:histogram` / `output:statistics` report for any action of
 * meryl2 (src/meryl2/merylOpTemplate.C:168-209,285-307).  An accumulator is opened, fed any number of arrays and read:
 * values below a dense limit are counted in LDS bins and flushed into uint64 device bins; the others go onto a device list
 * with room for every value of the call (no overflow, no second pass), which is sorted and run-length counted ON THE DEVICE --
 * only (value, occurrences) pairs cross to the host, so the traffic follows the DISTINCT large values, never the k-mers.
 * The result is exact for any uint32 values (0 and 2^32-1 included).
 * mgc_value_hist_open never fails for want of a device: the device (-1: the current one) is first touched by the first
 * non-empty add.  add: d_values is DEVICE memory, 4-byte aligned; `stream` is where the values were produced; the call
 * returns once they are counted (the array may be reused).  get: ascending by value, arrays of mgc_value_hist_len entries.
 * totals: unique = occurrences of value 1, distinct = sum of occurrences, total = sum(value * occurrences) in uint64 --
 * the three numbers of the master index's histogram header; any of the three may be NULL.
 * geometry: the dense limit and the values one workgroup takes per iteration (tests aim at both).
 * One accumulator is used by one thread at a time.  An add that fails may have counted part of its values: the accumulator is
 * unusable from then on -- every later add, len, get and totals returns MGC_ESTATE -- and can only be closed.
 * Failure text: mgc_db_stream_error(NULL). */
typedef struct mgc_value_hist mgc_value_hist;
mgc_value_hist *mgc_value_hist_open(int device);
int  mgc_value_hist_add(mgc_value_hist *h, const uint32_t *d_values, uint64_t n, void *stream);
int  mgc_value_hist_len(mgc_value_hist *h, uint64_t *n_pairs);
int  mgc_value_hist_get(mgc_value_hist *h, uint64_t *values, uint64_t *occurrences);
int  mgc_value_hist_totals(mgc_value_hist *h, uint64_t *unique, uint64_t *distinct, uint64_t *total);
void mgc_value_hist_close(mgc_value_hist *h);
void mgc_value_hist_geometry(uint32_t *dense_limit, uint32_t *workgroup_values);

/* mgc_db_eval_assigned with REPORTS: want_hist[v] != 0 asks for the value histogram of node v's result over all 64 slices --
 * an inner node's, the root's, or a leaf's (from its decoded values; it equals the one its master index stores).  After every
 * slice the flagged nodes' values are added to their accumulators on the device.  On success hists[v] is an accumulator to
 * read and close (mgc_value_hist_*) for every flagged node and NULL for the others; on failure every entry is NULL.
 * want_hist == NULL, or no node flagged: exactly mgc_db_eval_assigned -- the same routes, the same outputs byte for byte
 * (hists, if given, is filled with NULLs).  Checked with everything mgc_db_eval_assigned checks, before any device call and
 * before any output directory exists (MGC_EINVAL with text): a node flagged and hists NULL; want_hist set on a node the
 * root does not reach. */
int mgc_db_eval_reported(const mgc_eval_node_assigned *nodes, uint32_t n_nodes, const uint32_t *children, uint32_t n_children,
                         uint32_t root, const mgc_select_term *terms, uint32_t n_terms, int with_labels, uint32_t label_size,
                         mgc_eval_slice_labelled_cb cb, void *ctx, int device, int host_threads,
                         const uint8_t *want_hist /*[n_nodes]*/, mgc_value_hist **hists /*[n_nodes], out*/);

/* mgc_db_eval_reported with LISTS: want_list[v] != 0 asks for the text of node v's result -- the lines of include/meryl_list.h
 * (printKmer, src/meryl2/merylOp-nextMer.C:24-50: what `output:list=<file>` and `output:show` write for any action,
 * src/meryl2/merylCommandBuilder-processText.C:149-150,358-359, merylOpTemplate.C:76-163), with the label column when the
 * evaluation's outputs carry labels (label_size, or the largest label size among the leaves, above 0).  After node v's slice is
 * ready its k-mers are formatted on the device and list_cb(list_user, v, file, text, n_bytes) receives the text of slice `file` in
 * pieces of whole lines (n_bytes > 0; valid during the call): from the calling thread, in evaluation order, files ascending,
 * pieces in order; an empty slice makes no call.  A nonzero return stops the evaluation (MGC_ESTATE).  One pair of staging
 * buffers serves all flagged nodes; a piece holds at most 16 MiB (MGC_LIST_CHUNK, bytes, overrides it for tests; never less than
 * one line).  Leaves may be flagged -- a tree whose root is a leaf lists a database.
 * want_list == NULL, or no node flagged: exactly mgc_db_eval_reported -- the same routes, the same outputs byte for byte.
 * Checked with everything mgc_db_eval_reported checks, before any device call and before any output directory exists
 * (MGC_EINVAL with text): a node flagged and list_cb NULL; want_list set on a node the root does not reach. */
typedef int (*mgc_eval_list_cb)(void *user, uint32_t node, uint32_t file, const void *text, uint64_t n_bytes);
int mgc_db_eval_listed(const mgc_eval_node_assigned *nodes, uint32_t n_nodes, const uint32_t *children, uint32_t n_children,
                       uint32_t root, const mgc_select_term *terms, uint32_t n_terms, int with_labels, uint32_t label_size,
                       mgc_eval_slice_labelled_cb cb, void *ctx, int device, int host_threads,
                       const uint8_t *want_hist /*[n_nodes]*/, mgc_value_hist **hists /*[n_nodes], out*/,
                       const uint8_t *want_list /*[n_nodes]*/, mgc_eval_list_cb list_cb, void *list_user);

/* The `statistics` report of a histogram as text (src/meryl/merylOp-histogram.C:65-93): the four header lines, the column
 * titles and one row per pair.  Host only.  Returns the length of the text (without the final NUL); up to buf_size - 1
 * characters of it and a NUL are written to buf (buf may be NULL with buf_size 0: the length alone). */
size_t mdb_format_statistics(uint32_t k, const uint64_t *values, const uint64_t *occurrences, uint64_t n_pairs,
                             uint64_t num_unique, uint64_t num_distinct, uint64_t num_total, char *buf, size_t buf_size);

/* ONE count spread over the GPUs of a node, from one process (meryl_amd/csrc/mgc_node.cpp): rank r's reads are the
 * n_bases[r] bytes at d_bases[r] on device devices[r] (the base stream mgc_push_bases takes; with cfg->homopoly_compress
 * every rank's stream must hold whole sequences).  Every rank extracts the k-mers of its reads, the k-mers travel over
 * xGMI (peer copies, in waves that overlap with counting) to the rank that owns their range of the k-mer space, the
 * owners count and write disjoint prefix ranges, and the parts are stitched: the directory at db_path is
 * byte-identical to what one device gives for the concatenated input.  The reference has no counterpart -- its
 * node-scale recipe is "count pieces, then union-sum" (src/meryl/merylOp-count.C:251-268); this is what replaces it.
 * devices == NULL: rank r uses device r modulo the visible devices; several ranks MAY share a device (that is how a
 * one-GPU box tests the whole plan).  cfg must have been through mgc_configure_counting for the TOTAL input;
 * count-suffix is not supported here.  Failure text: mgc_last_error(NULL).
 * (The one-process-per-GPU form over RCCL is meryl_amd/count.py:count_sharded.) */
typedef struct mgc_node_profile {
  uint32_t n_ranks, bucket_bits;
  uint64_t n_bases, n_instances, n_distinct, data_bytes;
  double   partition_s;        /* slowest rank: histogram + partition of its reads */
  double   exchange_count_s;   /* slowest rank: pulls + grouping + finish + handing blocks to the writer */
  double   close_s;            /* slowest rank: waiting for its part's files */
  double   merge_parts_s, total_s;
  uint32_t n_batches, n_host_runs; /* batches every rank's reads were counted in; parked waves that went to host DRAM */
  uint64_t host_run_bytes;
  double   merge_runs_s;           /* slowest rank: merging its parked waves into its part (batches > 1) */
  uint64_t peak_hbm_bytes;         /* highest sampled device memory in use on any rank's device (batches > 1) */
} mgc_node_profile;
int mgc_count_node(const mgc_count_config *cfg, uint32_t n_ranks, const int *devices,
                   const uint8_t *const *d_bases, const uint64_t *n_bases,
                   const char *db_path, int host_threads, mgc_node_profile *prof);
/* The same with BATCHES (the node form of writeBatch's spill, merylOp-countThreads.C:323-379): no rank ever holds the
 * k-mers of more than batch_bases of its bases at once.  The routing plan comes from one histogram of ALL reads; then,
 * batch by batch, every rank partitions the next slice of its base stream (slices overlap by k-1 bases), the owners pull
 * and count their waves and park every counted wave as a run (include: mgc_runs_*; HBM first, pinned host DRAM beyond
 * the budget); after the last batch every owner merges its runs once into its part of the database.  batch_bases = 0:
 * derived from the free HBM (one batch when everything fits -- then this IS mgc_count_node, waves streamed to the writer
 * as they are counted). */
int mgc_count_node_batched(const mgc_count_config *cfg, uint32_t n_ranks, const int *devices,
                           const uint8_t *const *d_bases, const uint64_t *n_bases, uint64_t batch_bases,
                           const char *db_path, int host_threads, mgc_node_profile *prof);

/* The routing plan of mgc_count_node on its own (host arithmetic only, no device needed): *bucket_bits = the top bits of the k-mer
 * that route it for n_ranks ranks whose largest input is max_rank_bases (6 + ceil(log2 n_ranks), more for very large inputs, at
 * most 10 and at most w_prefix); with bucket_totals[2^*bucket_bits] (k-mers per bucket over all ranks) also cuts[n_ranks + 1]: rank r
 * owns buckets [cuts[r], cuts[r+1]) -- contiguous, every rank at least one, balanced by k-mers.  MGC_EINVAL when the ranks
 * outnumber the routable ranges. */
int mgc_node_plan(uint32_t n_ranks, uint32_t k, uint64_t max_rank_bases, uint32_t w_prefix, uint32_t *bucket_bits,
                  const uint64_t *bucket_totals, uint32_t *cuts);

/* The same for input that went through ONE session (pushed bases, parsed text, files -- the CLI's `gpus=N`): the staged
 * stream (mgc_staged_bases) is cut into n_ranks slices overlapping by k-1 bases -- no k-mer lost or doubled wherever the
 * cut falls; `compress` is applied before cutting -- the slices move to their devices and mgc_count_node runs.  The
 * session itself counts nothing and can only be closed afterwards.  Failure text: mgc_last_error(s). */
int mgc_count_node_staged(struct mgc_session *s, uint32_t n_ranks, const int *devices, const char *db_path,
                          int host_threads, mgc_node_profile *prof);

#ifdef __cplusplus
}
#endif
#endif /* MERYL_DB_H */
