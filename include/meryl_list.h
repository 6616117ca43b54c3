/*
 * meryl_list.h -- C ABI of the k-mer text lists: `k-mer <TAB> value [<TAB> label] <NL>` lines formatted on the device.
 *
 * Replaces the reference's printKmer (src/meryl2/merylOp-nextMer.C:24-50; v1 src/meryl/merylOp-nextMer.C:673-676), which builds
 * one line per k-mer on a compute thread and fputs() it under a lock, and the per-action lists that call it: `output:list=<file>`
 * and `output:show` of meryl2 (src/meryl2/merylCommandBuilder-processText.C:149-150,358-359, merylOpTemplate.C:76-163).  A line
 * holds, in order: the k letters of the k-mer, most significant base first, codes 0 1 2 3 as A C T G; a TAB; the value in decimal;
 * when label_size > 0 a TAB and the low label_size bits of the label in binary, most significant first; a newline.  Only the
 * length of the decimal varies from line to line.  printACGT (recanonicalizeACGTorder) is not offered.
 *
 * Here the lines of a device-resident (k-mer, value, label) stream are formatted by two kernels (meryl_amd/csrc/mgc_list.hip):
 * a length pass gives the bytes of every tile of k-mers, the library's scan turns them into tile offsets, and the format pass
 * builds every tile's text in LDS and stores it in whole 16-byte words.  The text leaves the device in pieces of whole lines
 * through two staging buffers, so that a piece is copied and handed to the callback while the next one is formatted.
 *
 * Return codes, device pointers and `stream` follow include/meryl_gpu_count.h; failure text: mgc_db_stream_error(NULL)
 * (include/meryl_db.h).  The evaluator's entry point that lists the result of any node of an operation tree is
 * mgc_db_eval_listed (include/meryl_db.h).
 */
#ifndef MERYL_LIST_H
#define MERYL_LIST_H

#include <stddef.h>
#include <stdint.h>

#include "meryl_gpu_count.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Receives a piece of text: whole lines, n > 0 bytes, valid during the call only.  A nonzero return stops the listing, which
 * then returns MGC_ESTATE. */
typedef int (*mgc_list_write_cb)(const void *text, uint64_t n, void *user);

/* A bound on the longest line of a list: k + 1 + 10 + 1 + label_size + 1 bytes, at most 141 -- k letters, TAB, ten digits, TAB,
 * the label's bits, NL.  Exact with a label; a list without labels has no second TAB, so its longest line is one byte shorter.
 * Host only. */
uint32_t mgc_list_max_line(uint32_t k, uint32_t label_size);

/* The k-mers of one tile of the kernels: a multiple of 64 that depends on (k, label_size) only (tests aim at its edges).
 * Host only; 0 for a k outside 1..64 or a label_size above 64. */
uint32_t mgc_list_tile_kmers(uint32_t k, uint32_t label_size);

/* The name of the list file of one slice: `name` with its FIRST run of '#' replaced by `file` in decimal, zero-padded to
 * max(run length, 2) digits -- what src/meryl2/merylOpTemplate.C:76-87 documents ("replacing the ##'s with digits"; at least two
 * digits: merylCommandBuilder-spawnThreads.C:62; that function itself overwrites its own buffer pointer, :50-74, and is not
 * followed).  Any '#' at all means one file per slice (nHash == 0 is the single-file test, merylOpTemplate.C:130).
 * Returns the length of the new name, which is written to buf with a final NUL; 0 when name holds no '#' (single-file mode), or
 * when buf_size cannot take the name and its NUL (nothing is written then).  Host only. */
size_t mgc_list_slice_name(const char *name, uint32_t file, char *buf, size_t buf_size);

/* The text of n k-mers in DEVICE memory, in the evaluator's layouts: d_keys holds one uint64 per k-mer for k <= 32 and interleaved
 * (lo, hi) pairs of uint64 for k > 32 (16-byte aligned); d_values uint32; d_labels uint64, or NULL for zeros.  The kernels run on
 * `stream`, after whatever produced the arrays there; the call returns once every piece has been handed to cb, in order, from the calling
 * thread.  Every piece holds whole lines and at most chunk_bytes bytes; two device and two pinned staging buffers of
 * min(chunk_bytes, the bytes of the whole text) are allocated for the call.
 * MGC_EINVAL: k outside 1..64, label_size above 64, chunk_bytes below mgc_list_max_line(k, label_size) -- the bound, so without labels
 * a chunk_bytes of exactly the longest line that can occur, one byte below it, is refused too -- cb NULL, an array NULL with n > 0.  n == 0 is success without a callback.  MGC_ESTATE: cb returned nonzero (no further call is made). */
int mgc_list_kmers(const void *d_keys, const uint32_t *d_values, const uint64_t *d_labels_or_null, uint64_t n,
                   uint32_t k, uint32_t label_size, uint64_t chunk_bytes, mgc_list_write_cb cb, void *user, void *stream);

/* The two passes on their own, device to device (what mgc_list_kmers runs per piece; scripts/list_bench.py times them): lengths
 * runs the length pass and the scan of the tile totals into d_ws (mgc_dev_list_workspace_bytes, DEVICE memory, 8-byte aligned)
 * and, when n_bytes is given, waits for `stream` and returns the bytes of the whole text; format then writes the whole text to
 * d_text (DEVICE memory, 16-byte aligned, at least that many bytes) from the same arrays and the same d_ws, asynchronously on
 * `stream`. */
size_t mgc_dev_list_workspace_bytes(uint64_t n, uint32_t k, uint32_t label_size);
int mgc_dev_list_lengths(const uint32_t *d_values, uint64_t n, uint32_t k, uint32_t label_size, void *d_ws, size_t ws_bytes,
                         uint64_t *n_bytes, void *stream);
int mgc_dev_list_format(const void *d_keys, const uint32_t *d_values, const uint64_t *d_labels_or_null, uint64_t n, uint32_t k,
                        uint32_t label_size, void *d_ws, size_t ws_bytes, void *d_text, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* MERYL_LIST_H */
