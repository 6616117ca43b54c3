// mgc_api.cpp -- C-ABI layer (include/meryl_gpu_count.h) over the gfx950 kernels.
//
// Host-side mirror of the reference's counting engine:
//   mgc_configure_counting  <-> merylOperation::configureCounting  src/meryl/merylOp-count.C:300-403
//   mgc_open/push/count/finish <-> merylOperation::countThreads     src/meryl/merylOp-countThreads.C:385-474
// Here: configuration, the bare mgc_dev_* operators, open / close, count and the result calls.  What is pushed into a session between
// open and count is staged by mgc_input.cpp (settle_input hands the staged stream over; count_staged_batch is what its batches run).
// There is NO CPU fallback in here: every compute entry point launches HIP
// kernels and fails with MGC_EHIP if the device or the code object is missing.
#include "../../include/meryl_gpu_count.h"
#include "mgc_device.h"
#include "mgc_session.hpp"
#include "mgc_runs.hpp"
#include "mgc_selector.hpp"
#include "mgc_value.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

namespace mgc {
std::string &thread_last_error() {
  thread_local std::string e;
  return e;
}

// Every MGC_* switch of the count path, from the environment (mgc_device.h: once per session / per bare-operator call)
Switches read_switches() {
  Switches sw;
  auto off = [](const char *n) { const char *e = getenv(n); return e && e[0] == '0'; };
  auto on1 = [](const char *n) { const char *e = getenv(n); return e && e[0] == '1'; };
  auto num = [](const char *n, uint64_t d) { const char *e = getenv(n); return (e && *e) ? strtoull(e, nullptr, 10) : d; };
  sw.fine_hist = !off("MGC_FINE_HIST"); sw.hpc_msd = !off("MGC_HPC_MSD"); sw.hpc_digits = !off("MGC_HPC_DIGITS");
  sw.const_k = !off("MGC_KMER_CONST_K"); sw.packed_bases = !off("MGC_PACKED_BASES"); sw.narrow = !off("MGC_NARROW"); sw.wide_msd = !off("MGC_WIDE_MSD");
  sw.group_pipe = !off("MGC_GROUP_PIPE"); sw.soa5 = !off("MGC_SOA5"); sw.k96 = !off("MGC_K96"); sw.finish = !off("MGC_FINISH");
  sw.nolist = on1("MGC_FINISH_NOLIST");
  sw.finish_trace = getenv("MGC_FINISH_TRACE") != nullptr; sw.group_dbg = getenv("MGC_GROUP_DBG") != nullptr; sw.hash_dbg = getenv("MGC_HASH_DBG") != nullptr;
  { const char *e = getenv("MGC_HASH_MULTI"); sw.hash_multi = (e && *e) ? atoi(e) : -1; }
  { const char *e = getenv("MGC_HASH_STREAM"); sw.hash_stream = (e && *e) ? atoi(e) : -1; }
  sw.min_top = (uint32_t)num("MGC_FINISH_MIN_TOP", 0);
  sw.finish_target = num("MGC_FINISH_TARGET", 0);
  sw.stream_max = num("MGC_STREAM_MAX", (uint64_t)1 << 22);
  sw.bucket_bases = num("MGC_BUCKET_BASES", 0);
  sw.huge_streams = (uint32_t)num("MGC_HUGE_STREAMS", 4);
  sw.huge_slices = !off("MGC_HUGE_SLICES");
  sw.pass_stagger = (uint32_t)num("MGC_PASS_STAGGER", 0);
  sw.group_batch_bytes = num("MGC_GROUP_BATCH_BYTES", sw.group_batch_bytes);
  sw.group_batch_files = (uint32_t)num("MGC_GROUP_BATCH_FILES", 0);
  sw.pack_overlap = !off("MGC_PACK_OVERLAP");
  { const char *e = getenv("MGC_PACK_MARGIN"); if (e && *e) sw.pack_margin = strtoll(e, nullptr, 10); }
  sw.pack_ratio = (uint32_t)num("MGC_PACK_RATIO", 0);
  return sw;
}
}  // namespace mgc
using mgc::set_err;

namespace {

// ---------------------------------------------------------------------------
// configureCounting restated (src/meryl/merylOp-count.C:118-403).  This is the
// product's own copy; oracle/oracle_count.c holds an independent restatement
// used by the tests to cross-check it.
// ---------------------------------------------------------------------------

uint64_t number_of_bits64(uint64_t v) {      // countNumberOfBits64 [meryl-utility]
  uint64_t b = 0;
  while (v) { b++; v >>= 1; }
  return b;
}

// findExpectedSimpleSize, merylOp-count.C:118-165; lowBits_t is uint16 (merylOp-countSimple.C:41-48)
uint64_t expected_simple_size(uint32_t k, uint64_t n_est, uint32_t suffix_len) {
  if (2 * k - 2 * suffix_len > 42) return UINT64_MAX;                            // :142
  const uint64_t low_bits  = 16;
  const uint64_t n_entries = (uint64_t)1 << (2 * k - 2 * suffix_len);            // :124
  const uint64_t exp_max   = (uint64_t)(0.004 * (double)n_est);                  // :126
  const uint64_t exp_bits  = number_of_bits64(exp_max) + 1;                      // :127
  const uint64_t extra     = (exp_bits < low_bits) ? 0 : (exp_bits - low_bits);  // :128
  return (n_entries * low_bits + n_entries * extra) / 8;                         // :130-132
}

// findBestPrefixSize, merylOp-count.C:173-227
void best_prefix_size(const mgc_count_config &c, uint64_t n_est, uint64_t mem_allowed, uint32_t *best,
                      uint64_t *mem_used) {
  const uint32_t k = c.k;
  const uint32_t seg_bits = c.page_size * 8, seg_bytes = c.page_size;            // pagesPerSegment()==1
  *best = 0;
  *mem_used = UINT64_MAX;
  for (uint32_t wp = 1; wp < 2 * k - 1; wp++) {                                  // :197
    const uint64_t n_prefix = (uint64_t)1 << wp;
    const uint64_t kpp = n_est / n_prefix + 1;                                   // :199
    const uint64_t kps = seg_bits / (2 * k - wp);                                // :200
    const uint64_t spp = kpp / kps + 1;                                          // :201
    if (wp + number_of_bits64(spp) + number_of_bits64(seg_bytes) >= 64) break;   // :203
    const uint64_t struct_mem = (uint64_t)c.sizeof_count_array * n_prefix + 8 * n_prefix * spp;   // :206-207
    const uint64_t data_min   = n_prefix * seg_bytes;                            // :208
    const uint64_t total      = struct_mem + n_prefix * spp * seg_bytes;         // :209-210
    if (struct_mem + data_min > mem_allowed) break;                              // :216
    if ((wp > 9) && (total + (uint64_t)16 * wp * 1024 * 1024 < *mem_used)) {     // :219
      *mem_used = total;
      *best = wp;
    }
    if (total > (uint64_t)16 * *mem_used) break;                                 // :224 (uint64 wrap kept)
  }
}

}  // namespace

extern "C" uint32_t mgc_version(void) { return (0u << 16) | 3u; }

extern "C" int mgc_configure_counting(mgc_count_config *c) {
  if (!c) return MGC_EINVAL;
  if (c->k == 0 || c->k > 64) {                                                  // :311-312 (fatal there)
    set_err(nullptr, "ERROR: Kmer size not supplied with modifier k=<kmer-size>.");
    return MGC_EINVAL;
  }
  if (c->mode < 0 || c->mode > 2) return MGC_EINVAL;
  if (c->page_size == 0) c->page_size = 4096;
  if (c->sizeof_count_array == 0) c->sizeof_count_array = 3232;

  c->use_simple = 0; c->w_prefix = 0; c->n_prefix = 0; c->w_data = 0; c->n_batches = 1; c->memory_used = 0;

  const uint64_t mem_simple = expected_simple_size(c->k, c->n_kmers_estimate, c->count_suffix_length);   // :340
  uint64_t mem_complex = UINT64_MAX;
  uint32_t best = 0, n_batches = 1;

  if (c->k > 5) {                                                                // :353
    for (n_batches = 1; mem_complex > c->memory_allowed; n_batches++) {          // :354-355
      best_prefix_size(*c, c->n_kmers_estimate / n_batches, c->memory_allowed, &best, &mem_complex);
      if (n_batches > (1u << 20)) {
        set_err(nullptr, "configureCounting: no prefix size fits in %lu bytes", (unsigned long)c->memory_allowed);
        return MGC_EINVAL;
      }
    }
    c->w_prefix = best;                                                          // findBestValues :273-276
    c->n_prefix = (uint64_t)1 << best;
    c->w_data   = 2 * c->k - best;
  }
  if ((mem_simple < mem_complex) && (mem_simple < c->memory_allowed)) {          // :368-372
    c->use_simple = 1; c->memory_used = mem_simple;
  } else {
    c->use_simple = 0; c->memory_used = mem_complex;
  }
  if (c->count_suffix_length > 0) { c->use_simple = 1; c->memory_used = mem_simple; }   // :379-382
  c->n_batches = n_batches;
  return MGC_OK;
}

extern "C" int mgc_format_configured_line(const mgc_count_config *c, char *buf, size_t buflen) {
  if (!c || !buf) return MGC_EINVAL;
  const uint64_t m = (c->memory_used < c->memory_allowed) ? c->memory_used : c->memory_allowed;
  snprintf(buf, buflen, "Configured %s mode for %.3f GB memory per batch, and up to %u batch%s.",   // :398-401
           c->use_simple ? "simple" : "complex", m / 1024.0 / 1024.0 / 1024.0, c->n_batches,
           (c->n_batches == 1) ? "" : "es");
  return MGC_OK;
}

// ---------------------------------------------------------------------------
// Stateless device operators
// ---------------------------------------------------------------------------
namespace {
int hip_rc(hipError_t e, const char *what) {
  if (e == hipSuccess) return MGC_OK;
  set_err(nullptr, "%s: %s", what, hipGetErrorString(e));
  return (e == hipErrorOutOfMemory) ? MGC_ENOMEM : MGC_EHIP;
}
bool key_args_ok(uint32_t k, int mode, uint32_t bucket_bits) {
  if (k == 0 || k > 64) { set_err(nullptr, "k=%u out of range (1..64)", k); return false; }
  if (mode < 0 || mode > 2) { set_err(nullptr, "bad mode %d", mode); return false; }
  if (bucket_bits > MGC_MAX_BUCKET_BITS || bucket_bits > 2 * k) { set_err(nullptr, "bad bucket_bits %u", bucket_bits); return false; }
  return true;
}
}  // namespace

extern "C" size_t mgc_dev_partition_workspace_bytes(uint32_t bucket_bits) {
  return mgc::kp_workspace_bytes(bucket_bits);
}

extern "C" int mgc_dev_kmer_histogram(const uint8_t *d_bases, uint64_t n_bases, uint32_t k, int mode,
                                      uint32_t bucket_bits, uint64_t *d_bucket_counts, void *d_ws, size_t ws_bytes,
                                      void *stream) {
  if (!key_args_ok(k, mode, bucket_bits)) return MGC_EINVAL;
  if ((!d_bases && n_bases) || !d_bucket_counts || !d_ws || ws_bytes < mgc::kp_workspace_bytes(bucket_bits)) return MGC_EINVAL;
  return hip_rc(mgc::launch_kmer_histogram(d_bases, n_bases, k, mode, bucket_bits, d_bucket_counts, d_ws,
                                           (hipStream_t)stream), "kmer_histogram");
}

extern "C" int mgc_dev_kmer_partition(const uint8_t *d_bases, uint64_t n_bases, uint32_t k, int mode,
                                      uint32_t bucket_bits, const uint64_t *d_bucket_starts, void *d_keys,
                                      void *d_ws, size_t ws_bytes, void *stream) {
  if (!key_args_ok(k, mode, bucket_bits)) return MGC_EINVAL;
  if ((!d_bases && n_bases) || !d_bucket_starts || !d_ws || ws_bytes < mgc::kp_workspace_bytes(bucket_bits)) return MGC_EINVAL;
  return hip_rc(mgc::launch_kmer_partition(d_bases, n_bases, k, mode, bucket_bits, d_bucket_starts, d_keys, d_ws,
                                           (hipStream_t)stream), "kmer_partition");
}

// the histogram of a sharded count's senders: k-mers per bucket (2^bucket_bits, 6..8) for the routing plan + the per-workgroup rows
// mgc_dev_kmer_partition takes its cursors from + k-mers per top FIFTEEN bits (d_fine_hist[2^15]) for the owners' first grouping digit
extern "C" int mgc_dev_kmer_histogram_fine(const uint8_t *d_bases, uint64_t n_bases, uint32_t k, int mode, uint32_t bucket_bits,
                                           uint64_t *d_bucket_counts, uint64_t *d_fine_hist, void *d_ws, size_t ws_bytes, void *stream) {
  if (!key_args_ok(k, mode, bucket_bits) || !mgc::kmer_histogram_fine_bits_ok(k, bucket_bits)) return MGC_EINVAL;
  if ((!d_bases && n_bases) || !d_bucket_counts || !d_fine_hist || !d_ws || ws_bytes < mgc::kp_workspace_bytes(bucket_bits)) return MGC_EINVAL;
  const mgc::Switches sw = mgc::read_switches();
  return hip_rc(mgc::launch_kmer_histogram_fine(d_bases, n_bases, k, mode, d_bucket_counts, d_fine_hist, d_ws, (hipStream_t)stream,
                                                sw.const_k, bucket_bits), "kmer_histogram_fine");
}

extern "C" size_t mgc_dev_sort_workspace_bytes(uint64_t n) { return mgc::sort_workspace_bytes(n) + 256; }

static int dev_radix_passes(void *d_keys, void *d_alt, uint64_t n, uint32_t key_words, uint32_t begin_bit, uint32_t end_bit, void *d_ws,
                           size_t ws_bytes, int *result_in_alt, void *stream, bool group);

extern "C" int mgc_dev_radix_sort(void *d_keys, void *d_alt, uint64_t n, uint32_t key_words, uint32_t begin_bit,
                                  uint32_t end_bit, void *d_ws, size_t ws_bytes, int *result_in_alt, void *stream) {
  return dev_radix_passes(d_keys, d_alt, n, key_words, begin_bit, end_bit, d_ws, ws_bytes, result_in_alt, stream, false);
}
// the grouping passes of the count path as a bare operator (its own entry point: an environment switch inside mgc_dev_radix_sort
// used to change that operator's contract -- ADVICE r5)
extern "C" int mgc_dev_radix_group(void *d_keys, void *d_alt, uint64_t n, uint32_t key_words, uint32_t begin_bit,
                                   uint32_t end_bit, void *d_ws, size_t ws_bytes, int *result_in_alt, void *stream) {
  return dev_radix_passes(d_keys, d_alt, n, key_words, begin_bit, end_bit, d_ws, ws_bytes, result_in_alt, stream, true);
}

static int dev_radix_passes(void *d_keys, void *d_alt, uint64_t n, uint32_t key_words, uint32_t begin_bit, uint32_t end_bit, void *d_ws,
                           size_t ws_bytes, int *result_in_alt, void *stream, bool group) {
  if (!result_in_alt || begin_bit > end_bit || (key_words != 1 && key_words != 2) || end_bit > 64 * key_words) return MGC_EINVAL;
  *result_in_alt = 0;
  if (n == 0 || begin_bit == end_bit) return MGC_OK;
  if (!d_keys || !d_alt || !d_ws || ws_bytes < mgc::sort_workspace_bytes(n) + 256) return MGC_EINVAL;
  mgc::SortPlan plan;
  mgc::make_sort_plan(begin_bit, end_bit, &plan);
  if (group) plan.mode = 3;
  // the last 256 bytes of the workspace hold the look-back error word
  uint32_t *d_err = reinterpret_cast<uint32_t *>(reinterpret_cast<unsigned char *>(d_ws) + mgc::sort_workspace_bytes(n));
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(d_err, 0, 4, st);
  if (e != hipSuccess) return hip_rc(e, "radix_sort memset");
  e = mgc::launch_radix_sort(d_keys, d_alt, n, key_words, plan, d_ws, ws_bytes - 256, d_err, result_in_alt, st, nullptr);
  if (e != hipSuccess) return hip_rc(e, "radix_sort");
  uint32_t h_err = 0;
  e = hipMemcpyAsync(&h_err, d_err, 4, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return hip_rc(e, "radix_sort sync");
  if (h_err) { set_err(nullptr, "radix sort look-back timed out"); return MGC_ETIMEOUT; }
  return MGC_OK;
}

extern "C" size_t mgc_dev_rle_workspace_bytes(uint64_t n) { return mgc::rle_workspace_bytes(n); }

extern "C" int mgc_dev_rle_count(const void *d_sorted, uint64_t n, uint32_t key_words, void *d_ws, size_t ws_bytes,
                                 uint64_t *n_distinct, void *stream) {
  if (!n_distinct || !d_ws || ws_bytes < mgc::rle_workspace_bytes(n) || (!d_sorted && n) ||
      (key_words != 1 && key_words != 2)) return MGC_EINVAL;
  hipError_t e = mgc::launch_rle_count(d_sorted, n, key_words, d_ws, (hipStream_t)stream);
  if (e != hipSuccess) return hip_rc(e, "rle_count");
  return hip_rc(mgc::rle_read_total(d_ws, n_distinct, (hipStream_t)stream), "rle_count sync");
}

extern "C" int mgc_dev_rle_emit(const void *d_sorted, uint64_t n, uint32_t key_words, void *d_ws, size_t ws_bytes,
                                void *d_unique, uint32_t *d_counts, void *stream) {
  if (!d_ws || ws_bytes < mgc::rle_workspace_bytes(n) || (n && (!d_sorted || !d_unique || !d_counts)) ||
      (key_words != 1 && key_words != 2)) return MGC_EINVAL;
  return hip_rc(mgc::launch_rle_emit(d_sorted, n, key_words, d_ws, d_unique, d_counts, (hipStream_t)stream), "rle_emit");
}

extern "C" int mgc_dev_block_offsets(const void *d_unique, uint64_t n_distinct, uint32_t key_words, uint32_t w_data,
                                     uint64_t n_prefix, uint64_t *d_block_start, void *stream) {
  if (!d_block_start || (key_words != 1 && key_words != 2) || w_data >= 64 * key_words || (n_distinct && !d_unique))
    return MGC_EINVAL;
  return hip_rc(mgc::launch_block_offsets(d_unique, n_distinct, key_words, w_data, n_prefix, d_block_start,
                                          (hipStream_t)stream), "block_offsets");
}

extern "C" size_t mgc_dev_merge_workspace_bytes(uint64_t na, uint64_t nb) { return mgc::merge_workspace_bytes(na, nb); }

extern "C" int mgc_dev_merge_count(const void *dA, uint64_t na, const void *dB, uint64_t nb, uint32_t key_words, int op, void *d_ws,
                                   size_t ws_bytes, uint64_t *n_out, void *stream) {
  if (!n_out || !d_ws || ws_bytes < mgc::merge_workspace_bytes(na, nb) || (na && !dA) || (nb && !dB) ||
      (key_words != 1 && key_words != 2) || op < 0 || op > MGC_MERGE_SYMMETRIC_DIFFERENCE || op == MGC_MERGE_SUBTRACT) return MGC_EINVAL;
  hipError_t e = mgc::launch_merge_count(dA, na, dB, nb, key_words, op, d_ws, (hipStream_t)stream);
  if (e != hipSuccess) return hip_rc(e, "merge_count");
  return hip_rc(mgc::merge_read_total(d_ws, n_out, (hipStream_t)stream), "merge_count sync");
}

extern "C" int mgc_dev_merge_count_values(const void *dA, const uint32_t *cA, uint64_t na, const void *dB, const uint32_t *cB, uint64_t nb,
                                          uint32_t key_words, int op, void *d_ws, size_t ws_bytes, uint64_t *n_out, void *stream) {
  if (!n_out || !d_ws || ws_bytes < mgc::merge_workspace_bytes(na, nb) || (na && (!dA || !cA)) || (nb && (!dB || !cB)) ||
      (key_words != 1 && key_words != 2) || op < 0 || op > MGC_MERGE_SYMMETRIC_DIFFERENCE) return MGC_EINVAL;
  hipError_t e = mgc::launch_merge_count(dA, na, dB, nb, key_words, op, d_ws, (hipStream_t)stream, cA, cB);
  if (e != hipSuccess) return hip_rc(e, "merge_count");
  return hip_rc(mgc::merge_read_total(d_ws, n_out, (hipStream_t)stream), "merge_count sync");
}

extern "C" size_t mgc_dev_select_workspace_bytes(uint64_t n) { return mgc::select_workspace_bytes(n); }

extern "C" int mgc_dev_select_count(const void *d_keys, const uint32_t *d_values, uint64_t n, uint32_t key_words, int value_op, uint64_t constant,
                                    void *d_ws, size_t ws_bytes, uint64_t *n_out, void *stream) {
  if (!n_out || !d_ws || ws_bytes < mgc::select_workspace_bytes(n) || (n && (!d_keys || !d_values)) || (key_words != 1 && key_words != 2) ||
      value_op < 0 || value_op > MGC_VALUE_MODULO) return MGC_EINVAL;
  hipError_t e = mgc::launch_select(false, mgc::SelectInput{d_keys, d_values, nullptr, nullptr, n, key_words}, value_op, constant, mgc::PassRule(), d_ws, nullptr, nullptr,
                                    (hipStream_t)stream);
  if (e != hipSuccess) return hip_rc(e, "select_count");
  return hip_rc(mgc::merge_read_total(d_ws, n_out, (hipStream_t)stream), "select_count sync");
}

extern "C" int mgc_dev_select_emit(const void *d_keys, const uint32_t *d_values, uint64_t n, uint32_t key_words, int value_op, uint64_t constant,
                                   void *d_ws, size_t ws_bytes, void *d_keys_out, uint32_t *d_values_out, void *stream) {
  if (!d_ws || ws_bytes < mgc::select_workspace_bytes(n) || (n && (!d_keys || !d_values)) || (key_words != 1 && key_words != 2) ||
      value_op < 0 || value_op > MGC_VALUE_MODULO) return MGC_EINVAL;
  return hip_rc(mgc::launch_select(true, mgc::SelectInput{d_keys, d_values, nullptr, nullptr, n, key_words}, value_op, constant, mgc::PassRule(), d_ws, d_keys_out,
                                   d_values_out, (hipStream_t)stream), "select_emit");
}

extern "C" int mgc_dev_merge_emit(const void *dA, const uint32_t *cA, uint64_t na, const void *dB, const uint32_t *cB, uint64_t nb,
                                  uint32_t key_words, int op, void *d_ws, size_t ws_bytes, void *d_keys_out, uint32_t *d_counts_out,
                                  void *stream) {
  if (!d_ws || ws_bytes < mgc::merge_workspace_bytes(na, nb) || (na && (!dA || !cA)) || (nb && (!dB || !cB)) ||
      (key_words != 1 && key_words != 2) || op < 0 || op > MGC_MERGE_SYMMETRIC_DIFFERENCE) return MGC_EINVAL;
  return hip_rc(mgc::launch_merge_emit(dA, cA, na, dB, cB, nb, key_words, op, d_ws, d_keys_out, d_counts_out, (hipStream_t)stream),
                "merge_emit");
}

extern "C" uint32_t mgc_dev_merge_many_tile(uint32_t key_words) { return mgc::merge_many_tile(key_words); }

static bool merge_many_args_ok(const void *const *d_keys, const uint32_t *const *d_values, const uint64_t *n, uint32_t n_inputs,
                               uint32_t key_words, int op, uint32_t min_inputs = 2) {
  if (!d_keys || !d_values || !n || n_inputs < min_inputs || n_inputs > MGC_MERGE_MANY_MAX || (key_words != 1 && key_words != 2) ||
      op < MGC_MERGE_UNION_SUM || op > MGC_MERGE_UNION) return false;
  for (uint32_t i = 0; i < n_inputs; i++)
    if ((n[i] && (!d_keys[i] || !d_values[i])) || (n[i] >> 32)) return false;
  return true;
}

extern "C" size_t mgc_dev_merge_many_workspace_bytes(const uint64_t *n, uint32_t n_inputs, uint32_t key_words) {
  if (!n || n_inputs > MGC_MERGE_MANY_MAX) return 0;
  return mgc::merge_many_workspace_bytes(n, n_inputs, key_words);
}

extern "C" int mgc_dev_merge_many_count(const void *const *d_keys, const uint32_t *const *d_values, const uint64_t *n, uint32_t n_inputs,
                                        uint32_t key_words, int op, void *d_ws, size_t ws_bytes, uint64_t *n_out, void *stream) {
  if (!n_out || !d_ws || !merge_many_args_ok(d_keys, d_values, n, n_inputs, key_words, op) ||
      ws_bytes < mgc::merge_many_workspace_bytes(n, n_inputs, key_words)) return MGC_EINVAL;
  hipError_t e = mgc::launch_merge_many(false, mgc::MergeManyInputs{d_keys, d_values, nullptr, n, n_inputs, key_words}, op, mgc::PassRule(), d_ws, nullptr, nullptr,
                                        (hipStream_t)stream);
  if (e != hipSuccess) return hip_rc(e, "merge_many_count");
  return hip_rc(mgc::merge_read_total(d_ws, n_out, (hipStream_t)stream), "merge_many_count sync");
}

extern "C" int mgc_dev_merge_many_emit(const void *const *d_keys, const uint32_t *const *d_values, const uint64_t *n, uint32_t n_inputs,
                                       uint32_t key_words, int op, void *d_ws, size_t ws_bytes, void *d_keys_out, uint32_t *d_values_out,
                                       void *stream) {
  if (!d_ws || !merge_many_args_ok(d_keys, d_values, n, n_inputs, key_words, op) ||
      ws_bytes < mgc::merge_many_workspace_bytes(n, n_inputs, key_words)) return MGC_EINVAL;
  return hip_rc(mgc::launch_merge_many(true, mgc::MergeManyInputs{d_keys, d_values, nullptr, n, n_inputs, key_words}, op, mgc::PassRule(), d_ws, d_keys_out,
                                       d_values_out, (hipStream_t)stream), "merge_many_emit");
}

// ---- labels (include/meryl_gpu_count.h: MGC_LABEL_*) --------------------------------------------------------------------------
extern "C" uint64_t mgc_label_default_constant(int label_op) {      // src/meryl2/merylCommandBuilder-isAssign.C:124-156
  return (label_op == MGC_LABEL_AND || label_op == MGC_LABEL_XOR || label_op == MGC_LABEL_LIGHTEST) ? ~0ull : 0ull;
}

extern "C" int mgc_dev_merge_many_emit_labelled(const void *const *d_keys, const uint32_t *const *d_values, const uint64_t *const *d_labels,
                                                const uint64_t *n, uint32_t n_inputs, uint32_t key_words, int op, int label_op,
                                                uint64_t label_constant, void *d_ws, size_t ws_bytes, void *d_keys_out,
                                                uint32_t *d_values_out, uint64_t *d_labels_out, void *stream) {
  const bool ok = merge_many_args_ok(d_keys, d_values, n, n_inputs, key_words, op, 1);
  const int lop = mgc::label_kernel_op(true, op, label_op);
  if (!d_ws || !ok || ws_bytes < mgc::merge_many_workspace_bytes(n, n_inputs, key_words)) return MGC_EINVAL;
  if (lop < 0) { set_err(nullptr, "mgc_dev_merge_many_emit_labelled: unknown label operation %d", label_op); return MGC_EINVAL; }
  if (lop == MGC_LABEL_INVERT && n_inputs > 1) {
    set_err(nullptr, "mgc_dev_merge_many_emit_labelled: label=invert takes one input (merylOpCompute.C:368-371)");
    return MGC_EINVAL;
  }
  const mgc::MergeManyInputs in{d_keys, d_values, d_labels, n, n_inputs, key_words};
  mgc::PassRule rule;
  rule.lop = lop; rule.lc = label_constant; rule.out_labs = d_labels_out;
  if (n_inputs == 1) {                                               // the count step refuses one input: its pass runs here
    hipError_t e = mgc::launch_merge_many(false, in, op, rule, d_ws, nullptr, nullptr, (hipStream_t)stream);
    if (e != hipSuccess) return hip_rc(e, "merge_many_count (one input)");
  }
  return hip_rc(mgc::launch_merge_many(true, in, op, rule, d_ws, d_keys_out, d_values_out, (hipStream_t)stream), "merge_many_emit_labelled");
}

extern "C" int mgc_dev_select_emit_labelled(const void *d_keys, const uint32_t *d_values, const uint64_t *d_labels, uint64_t n,
                                            uint32_t key_words, int value_op, uint64_t constant, int label_op, uint64_t label_constant,
                                            void *d_ws, size_t ws_bytes, void *d_keys_out, uint32_t *d_values_out, uint64_t *d_labels_out,
                                            void *stream) {
  if (!d_ws || ws_bytes < mgc::select_workspace_bytes(n) || (n && (!d_keys || !d_values)) ||
      (key_words != 1 && key_words != 2) || value_op < 0 || value_op > MGC_VALUE_MODULO) return MGC_EINVAL;
  const int lop = mgc::label_kernel_op(false, value_op, label_op);
  if (lop < 0) { set_err(nullptr, "mgc_dev_select_emit_labelled: unknown label operation %d", label_op); return MGC_EINVAL; }
  mgc::PassRule rule;
  rule.lop = lop; rule.lc = label_constant; rule.out_labs = d_labels_out;
  return hip_rc(mgc::launch_select(true, mgc::SelectInput{d_keys, d_values, nullptr, d_labels, n, key_words}, value_op, constant, rule, d_ws, d_keys_out,
                                   d_values_out, (hipStream_t)stream), "select_emit_labelled");
}

// ---- selectors (include/meryl_gpu_count.h: mgc_select_term; the evaluator, the checks and the parser are mgc_selector.hpp) ------
extern "C" int mgc_select_parse(const char *const *words, uint32_t n_words, uint32_t n_inputs, mgc_select_term *terms, uint32_t cap,
                                uint32_t *n_terms) {
  if ((n_words && !words) || !n_terms || (cap && !terms) || n_inputs == 0) { set_err(nullptr, "mgc_select_parse: bad arguments"); return MGC_EINVAL; }
  const std::string m = mgc::select_parse(words, n_words, n_inputs, terms, cap, n_terms);
  if (!m.empty()) { set_err(nullptr, "%s", m.c_str()); return MGC_EINVAL; }
  return MGC_OK;
}

extern "C" int mgc_select_check(const mgc_select_term *terms, uint32_t n_terms, uint32_t n_inputs) {
  const std::string m = mgc::select_check(terms, n_terms, n_inputs);
  if (!m.empty()) { set_err(nullptr, "selector: %s", m.c_str()); return MGC_EINVAL; }
  return MGC_OK;
}

// the arguments every *_selected entry point shares, checked before any launch; *lop: the kernel's label code
static int selected_args(const char *who, bool is_merge, int op, uint32_t n_inputs, uint32_t key_words, uint32_t k, int label_op,
                         const mgc_select_term *terms, uint32_t n_terms, int *lop) {
  if (k < 1 || k > 32 * key_words) { set_err(nullptr, "%s: k = %u does not fit %u key word(s)", who, k, key_words); return MGC_EINVAL; }
  *lop = mgc::label_kernel_op(is_merge, op, label_op);
  if (*lop < 0) { set_err(nullptr, "%s: unknown label operation %d", who, label_op); return MGC_EINVAL; }
  if (*lop == MGC_LABEL_INVERT && n_inputs > 1) { set_err(nullptr, "%s: label=invert takes one input (merylOpCompute.C:368-371)", who); return MGC_EINVAL; }
  const std::string m = mgc::select_check(terms, n_terms, n_inputs);
  if (!m.empty()) { set_err(nullptr, "%s: selector: %s", who, m.c_str()); return MGC_EINVAL; }
  return MGC_OK;
}

// the rule of a *_selected / *_assigned launch: the label code, the program (possibly empty), the assignment's kernel code
static mgc::PassRule selected_rule(int lop, uint64_t label_constant, const mgc_select_term *terms, uint32_t n_terms, uint32_t k, uint64_t *d_labels_out,
                                   int vop = 0, uint64_t value_constant = 0) {
  mgc::PassRule r;
  r.lop = lop; r.lc = label_constant; r.select = true; r.terms = terms; r.n_terms = n_terms; r.k = k;
  r.vop = vop; r.vc = value_constant; r.out_labs = d_labels_out;
  return r;
}

extern "C" int mgc_dev_merge_many_count_selected(const void *const *d_keys, const uint32_t *const *d_values, const uint64_t *const *d_labels,
                                                 const uint64_t *n, uint32_t n_inputs, uint32_t key_words, uint32_t k, int op, int label_op,
                                                 uint64_t label_constant, const mgc_select_term *terms, uint32_t n_terms, void *d_ws,
                                                 size_t ws_bytes, uint64_t *n_out, void *stream) {
  if (!n_out || !d_ws || !merge_many_args_ok(d_keys, d_values, n, n_inputs, key_words, op, 1) ||
      ws_bytes < mgc::merge_many_workspace_bytes(n, n_inputs, key_words)) return MGC_EINVAL;
  int lop = 0;
  const int rc = selected_args("mgc_dev_merge_many_count_selected", true, op, n_inputs, key_words, k, label_op, terms, n_terms, &lop);
  if (rc != MGC_OK) return rc;
  hipError_t e = mgc::launch_merge_many(false, mgc::MergeManyInputs{d_keys, d_values, d_labels, n, n_inputs, key_words}, op,
                                        selected_rule(lop, label_constant, terms, n_terms, k, nullptr), d_ws, nullptr, nullptr, (hipStream_t)stream);
  if (e != hipSuccess) return hip_rc(e, "merge_many_count_selected");
  return hip_rc(mgc::merge_read_total(d_ws, n_out, (hipStream_t)stream), "merge_many_count_selected sync");
}

extern "C" int mgc_dev_merge_many_emit_selected(const void *const *d_keys, const uint32_t *const *d_values, const uint64_t *const *d_labels,
                                                const uint64_t *n, uint32_t n_inputs, uint32_t key_words, uint32_t k, int op, int label_op,
                                                uint64_t label_constant, const mgc_select_term *terms, uint32_t n_terms, void *d_ws,
                                                size_t ws_bytes, void *d_keys_out, uint32_t *d_values_out, uint64_t *d_labels_out, void *stream) {
  if (!d_ws || !merge_many_args_ok(d_keys, d_values, n, n_inputs, key_words, op, 1) ||
      ws_bytes < mgc::merge_many_workspace_bytes(n, n_inputs, key_words)) return MGC_EINVAL;
  int lop = 0;
  const int rc = selected_args("mgc_dev_merge_many_emit_selected", true, op, n_inputs, key_words, k, label_op, terms, n_terms, &lop);
  if (rc != MGC_OK) return rc;
  return hip_rc(mgc::launch_merge_many(true, mgc::MergeManyInputs{d_keys, d_values, d_labels, n, n_inputs, key_words}, op,
                                       selected_rule(lop, label_constant, terms, n_terms, k, d_labels_out), d_ws, d_keys_out, d_values_out,
                                       (hipStream_t)stream), "merge_many_emit_selected");
}

// ---- value assignment (include/meryl_gpu_count.h: MGC_ASSIGN_*; the rule and the parser are mgc_value.hpp) ----------------------
extern "C" uint64_t mgc_value_default_constant(int assign) { return mgc::value_default_constant(assign); }

extern "C" int mgc_value_assign_parse(const char *text, int *assign, uint64_t *constant) {
  if (!text || !assign || !constant) { set_err(nullptr, "mgc_value_assign_parse: bad arguments"); return MGC_EINVAL; }
  const std::string m = mgc::value_assign_parse(text, assign, constant);
  if (!m.empty()) { set_err(nullptr, "%s", m.c_str()); return MGC_EINVAL; }
  return MGC_OK;
}

// selected_args with an assignment: *vop the kernel's value code, *lop resolved by the assignment where it is SELECTED
static int assigned_args(const char *who, int op, uint32_t n_inputs, uint32_t key_words, uint32_t k, int value_assign, int label_op,
                         const mgc_select_term *terms, uint32_t n_terms, int *vop, int *lop) {
  *vop = mgc::value_kernel_op(value_assign);
  if (*vop < 0) { set_err(nullptr, "%s: unknown value assignment %d", who, value_assign); return MGC_EINVAL; }
  const int rc = selected_args(who, true, op, n_inputs, key_words, k, label_op, terms, n_terms, lop);
  if (rc != MGC_OK) return rc;
  *lop = mgc::label_kernel_op_assigned(true, op, label_op, value_assign);
  return MGC_OK;
}

extern "C" int mgc_dev_merge_many_count_assigned(const void *const *d_keys, const uint32_t *const *d_values, const uint64_t *const *d_labels,
                                                 const uint64_t *n, uint32_t n_inputs, uint32_t key_words, uint32_t k, int op, int value_assign,
                                                 uint64_t value_constant, int label_op, uint64_t label_constant, const mgc_select_term *terms,
                                                 uint32_t n_terms, void *d_ws, size_t ws_bytes, uint64_t *n_out, void *stream) {
  if (!n_out || !d_ws || !merge_many_args_ok(d_keys, d_values, n, n_inputs, key_words, op, 1) ||
      ws_bytes < mgc::merge_many_workspace_bytes(n, n_inputs, key_words)) return MGC_EINVAL;
  int vop = 0, lop = 0;
  const int rc = assigned_args("mgc_dev_merge_many_count_assigned", op, n_inputs, key_words, k, value_assign, label_op, terms, n_terms, &vop, &lop);
  if (rc != MGC_OK) return rc;
  hipError_t e = mgc::launch_merge_many(false, mgc::MergeManyInputs{d_keys, d_values, d_labels, n, n_inputs, key_words}, op,
                                        selected_rule(lop, label_constant, terms, n_terms, k, nullptr, vop, value_constant), d_ws, nullptr, nullptr,
                                        (hipStream_t)stream);
  if (e != hipSuccess) return hip_rc(e, "merge_many_count_assigned");
  return hip_rc(mgc::merge_read_total(d_ws, n_out, (hipStream_t)stream), "merge_many_count_assigned sync");
}

extern "C" int mgc_dev_merge_many_emit_assigned(const void *const *d_keys, const uint32_t *const *d_values, const uint64_t *const *d_labels,
                                                const uint64_t *n, uint32_t n_inputs, uint32_t key_words, uint32_t k, int op, int value_assign,
                                                uint64_t value_constant, int label_op, uint64_t label_constant, const mgc_select_term *terms,
                                                uint32_t n_terms, void *d_ws, size_t ws_bytes, void *d_keys_out, uint32_t *d_values_out,
                                                uint64_t *d_labels_out, void *stream) {
  if (!d_ws || !merge_many_args_ok(d_keys, d_values, n, n_inputs, key_words, op, 1) ||
      ws_bytes < mgc::merge_many_workspace_bytes(n, n_inputs, key_words)) return MGC_EINVAL;
  int vop = 0, lop = 0;
  const int rc = assigned_args("mgc_dev_merge_many_emit_assigned", op, n_inputs, key_words, k, value_assign, label_op, terms, n_terms, &vop, &lop);
  if (rc != MGC_OK) return rc;
  return hip_rc(mgc::launch_merge_many(true, mgc::MergeManyInputs{d_keys, d_values, d_labels, n, n_inputs, key_words}, op,
                                       selected_rule(lop, label_constant, terms, n_terms, k, d_labels_out, vop, value_constant), d_ws, d_keys_out,
                                       d_values_out, (hipStream_t)stream), "merge_many_emit_assigned");
}

extern "C" int mgc_dev_select_count_selected(const void *d_keys, const uint32_t *d_values, const uint64_t *d_labels, uint64_t n, uint32_t key_words,
                                             uint32_t k, int value_op, uint64_t constant, int label_op, uint64_t label_constant,
                                             const mgc_select_term *terms, uint32_t n_terms, void *d_ws, size_t ws_bytes, uint64_t *n_out,
                                             void *stream) {
  if (!n_out || !d_ws || ws_bytes < mgc::select_workspace_bytes(n) || (n && (!d_keys || !d_values)) || (key_words != 1 && key_words != 2) ||
      value_op < 0 || value_op > MGC_VALUE_MODULO) return MGC_EINVAL;
  int lop = 0;
  const int rc = selected_args("mgc_dev_select_count_selected", false, value_op, 1, key_words, k, label_op, terms, n_terms, &lop);
  if (rc != MGC_OK) return rc;
  hipError_t e = mgc::launch_select(false, mgc::SelectInput{d_keys, d_values, nullptr, d_labels, n, key_words}, value_op, constant,
                                    selected_rule(lop, label_constant, terms, n_terms, k, nullptr), d_ws, nullptr, nullptr, (hipStream_t)stream);
  if (e != hipSuccess) return hip_rc(e, "select_count_selected");
  return hip_rc(mgc::merge_read_total(d_ws, n_out, (hipStream_t)stream), "select_count_selected sync");
}

extern "C" int mgc_dev_select_emit_selected(const void *d_keys, const uint32_t *d_values, const uint64_t *d_labels, uint64_t n, uint32_t key_words,
                                            uint32_t k, int value_op, uint64_t constant, int label_op, uint64_t label_constant,
                                            const mgc_select_term *terms, uint32_t n_terms, void *d_ws, size_t ws_bytes, void *d_keys_out,
                                            uint32_t *d_values_out, uint64_t *d_labels_out, void *stream) {
  if (!d_ws || ws_bytes < mgc::select_workspace_bytes(n) || (n && (!d_keys || !d_values)) || (key_words != 1 && key_words != 2) ||
      value_op < 0 || value_op > MGC_VALUE_MODULO) return MGC_EINVAL;
  int lop = 0;
  const int rc = selected_args("mgc_dev_select_emit_selected", false, value_op, 1, key_words, k, label_op, terms, n_terms, &lop);
  if (rc != MGC_OK) return rc;
  return hip_rc(mgc::launch_select(true, mgc::SelectInput{d_keys, d_values, nullptr, d_labels, n, key_words}, value_op, constant,
                                   selected_rule(lop, label_constant, terms, n_terms, k, d_labels_out), d_ws, d_keys_out, d_values_out,
                                   (hipStream_t)stream), "select_emit_selected");
}

extern "C" int mgc_dev_buffers_live(uint64_t *bytes, uint64_t *buffers) {
  if (bytes) *bytes = mgc::dbuf_live().bytes.load(std::memory_order_relaxed);
  if (buffers) *buffers = mgc::dbuf_live().buffers.load(std::memory_order_relaxed);
  return MGC_OK;
}

extern "C" int mgc_dev_decode_blocks(const void *d_file, const void *d_blocks, uint64_t n_blocks, uint32_t suffix_size, uint32_t label_size,
                                     uint32_t key_words, void *d_keys, uint32_t *d_values, uint64_t *d_labels, void *stream) {
  if ((key_words != 1 && key_words != 2) || label_size > 64 || suffix_size > 64 * key_words ||
      (n_blocks && (!d_file || !d_blocks || !d_keys || !d_values))) return MGC_EINVAL;
  if (n_blocks == 0) return MGC_OK;
  hipStream_t st = (hipStream_t)stream;
  mgc::DBuf d_err;
  uint32_t h_err = 0;
  hipError_t e = d_err.ensure(256);
  if (e == hipSuccess) e = hipMemsetAsync(d_err.p, 0, 4, st);
  if (e == hipSuccess) e = mgc::launch_decode_blocks(d_file, d_blocks, n_blocks, suffix_size, label_size, key_words, d_keys, d_values, d_err.as<uint32_t>(), st, d_labels);
  if (e == hipSuccess) e = hipMemcpyAsync(&h_err, d_err.p, 4, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return hip_rc(e, "decode_blocks");
  if (h_err) { set_err(nullptr, "mgc_dev_decode_blocks: corrupt block (device decoder, code %u)", h_err); return MGC_EINVAL; }
  return MGC_OK;
}

extern "C" size_t mgc_dev_homopoly_workspace_bytes(uint64_t n) { return mgc::hpc_workspace_bytes(n); }

extern "C" int mgc_dev_homopoly_compress(const uint8_t *d_in, uint64_t n, uint8_t *d_out, uint64_t *n_out, void *d_ws,
                                         size_t ws_bytes, void *stream) {
  if (!n_out || !d_ws || ws_bytes < mgc::hpc_workspace_bytes(n) || (n && (!d_in || !d_out))) return MGC_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = mgc::launch_homopoly_compress(d_in, n, d_out, d_ws, st);
  if (e == hipSuccess) e = hipMemcpyAsync(n_out, d_ws, sizeof(uint64_t), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  return hip_rc(e, "homopoly_compress");
}

extern "C" int mgc_dev_synth_reads(uint64_t seed, uint64_t genome_len, uint64_t first_read, uint64_t n_reads,
                                   uint32_t read_len, uint32_t sub_rate_ppm, uint32_t n_rate_ppm, uint8_t *d_out,
                                   void *stream) {
  return mgc_dev_synth_reads_ex(seed, genome_len, first_read, n_reads, read_len, sub_rate_ppm, n_rate_ppm, 0, 1, 1, d_out, stream);
}

extern "C" int mgc_dev_synth_reads_ex(uint64_t seed, uint64_t genome_len, uint64_t first_read, uint64_t n_reads,
                                      uint32_t read_len, uint32_t sub_rate_ppm, uint32_t n_rate_ppm,
                                      uint32_t repeat_ppm, uint32_t repeat_unit, uint32_t repeat_families,
                                      uint8_t *d_out, void *stream) {
  if (!d_out || read_len == 0 || genome_len < read_len) return MGC_EINVAL;
  return hip_rc(mgc::launch_synth_reads(seed, genome_len, first_read, n_reads, read_len, sub_rate_ppm, n_rate_ppm,
                                        repeat_ppm, repeat_unit, repeat_families, d_out, (hipStream_t)stream), "synth_reads");
}

extern "C" int mgc_dev_bam_decode(const uint8_t *d_piece, uint64_t piece_bytes, const void *d_segments, uint64_t n_segments, uint64_t out_bytes,
                                  uint8_t *d_out, void *stream) {
  if ((!d_piece && piece_bytes) || (!d_segments && n_segments) || (!d_out && out_bytes)) return MGC_EINVAL;
  if (piece_bytes > 0xffffffffull) { set_err(nullptr, "mgc_dev_bam_decode: a piece holds less than 4 GiB"); return MGC_EINVAL; }
  HIP_TRY((mgc_session *)nullptr, mgc::launch_bam_decode(d_piece, piece_bytes, d_segments, n_segments, out_bytes, d_out, static_cast<hipStream_t>(stream)));
  return MGC_OK;
}

extern "C" uint64_t mgc_dev_text_parse_workspace_bytes(uint64_t text_bytes) { return 256 + mgc::text_parse_workspace_bytes(text_bytes); }

extern "C" int mgc_dev_text_parse(const uint8_t *d_text, uint64_t text_bytes, int format, void *d_workspace, uint8_t *d_out, void *stream) {
  if ((!d_text && text_bytes) || !d_workspace || !d_out || (reinterpret_cast<uintptr_t>(d_workspace) & 255u) ||
      (format != MGC_TEXT_FASTA && format != MGC_TEXT_FASTQ && format != MGC_TEXT_SAM)) return MGC_EINVAL;
  static_assert(sizeof(uint64_t) * 2 + sizeof(uint32_t) * 4 <= 256, "the parse state lies in the workspace's first 256 bytes");
  if (mgc::text_parse_state_bytes() > 256) return MGC_EINVAL;
  hipStream_t st = static_cast<hipStream_t>(stream);
  HIP_TRY((mgc_session *)nullptr, mgc::launch_text_file_op(d_workspace, d_out, 3, st));
  HIP_TRY((mgc_session *)nullptr, mgc::launch_text_parse(d_text, text_bytes, format, d_workspace, static_cast<uint8_t *>(d_workspace) + 256, d_out, st));
  return MGC_OK;
}

extern "C" int mgc_dev_gzip_resolve(uint8_t *d_text, uint64_t text_bytes, const uint16_t *d_symbols, uint64_t n_symbols, const uint8_t *d_window_in,
                                    uint32_t window_valid, uint8_t *d_window_out, uint32_t *d_error, void *stream) {
  if ((!d_text && text_bytes) || (!d_symbols && n_symbols) || (n_symbols && !d_error) || n_symbols > text_bytes || window_valid > mgc::GZ_WINDOW ||
      (!d_window_in && window_valid) || (d_window_out && d_window_out == d_window_in)) {
    set_err(nullptr, "mgc_dev_gzip_resolve: n_symbols <= text_bytes, window_valid <= 32768 (0 without a window), two different windows");
    return MGC_EINVAL;
  }
  HIP_TRY((mgc_session *)nullptr, mgc::launch_gzip_resolve(d_text, text_bytes, d_symbols, n_symbols, d_window_in, window_valid, d_window_out, d_error,
                                                           static_cast<hipStream_t>(stream)));
  return MGC_OK;
}

extern "C" int mgc_dev_crc32_pieces(const uint8_t *d_text, const uint64_t *d_begin, const uint32_t *d_len, uint64_t n_pieces, uint32_t *d_crc, void *stream) {
  if (n_pieces && (!d_text || !d_begin || !d_len || !d_crc)) return MGC_EINVAL;
  HIP_TRY((mgc_session *)nullptr, mgc::launch_gzip_crc32(d_text, d_begin, d_len, n_pieces, d_crc, static_cast<hipStream_t>(stream)));
  return MGC_OK;
}

// ---------------------------------------------------------------------------
// Session
// ---------------------------------------------------------------------------
extern "C" const char *mgc_last_error(const mgc_session *s) {
  return s ? s->err.c_str() : mgc::thread_last_error().c_str();
}

// The block geometry a count really uses: the configuration's, or -- in simple mode -- countSimple's.
bool mgc::effective_geometry(mgc_count_config *c) {
  const uint32_t sfx_len = c->count_suffix_length;
  if (c->use_simple) {
    // The reference switches to countSimple (merylOp-count.C:368-372): a direct-index counter
    // whose RESULT is the same sorted (k-mer, count) stream but whose database geometry is
    //   psbits = 2k - 6, wSuffix = min(20, psbits), wPrefix = 6 + psbits - wSuffix
    // (merylOp-countSimple.C:172-175).  The sort-based engine produces that stream for any
    // k, so simple mode only changes the block geometry.
    if (2 * c->k < MGC_NUM_FILES_BITS + 2 * sfx_len) { set_err(nullptr, "mgc_open: k=%u too small for a 64-file database", c->k); return false; }
    // A k-mer is [file][blockPrefix][suffix][count-suffix] (:140): the count-suffix bases take no part in the split, and
    // travel at the end of every block suffix (:231-233)
    const uint32_t psbits = 2 * c->k - 2 * sfx_len - MGC_NUM_FILES_BITS;
    const uint32_t w_suffix = (psbits > 20) ? 20 : psbits;
    c->w_prefix = MGC_NUM_FILES_BITS + psbits - w_suffix;
    c->n_prefix = (uint64_t)1 << c->w_prefix;
    c->w_data   = w_suffix + 2 * sfx_len;
  }
  return true;
}

extern "C" mgc_session *mgc_open(const mgc_count_config *cfg, int device) {
  if (!cfg) { set_err(nullptr, "mgc_open: NULL config"); return nullptr; }
  mgc_count_config eff = *cfg;
  if (cfg->label_size > 64) { set_err(nullptr, "mgc_open: label_size %u (at most 64 bits)", cfg->label_size); return nullptr; }
  uint64_t sfx_mask = 0, sfx_test = 0;
  const uint32_t sfx_len = cfg->count_suffix_length;
  if (sfx_len) {
    // count-suffix=<bases>: merylOp.H:139-147 packs the string like a k-mer (2-bit codes, last base lowest);
    // merylOp-countSimple.C:50-58 builds the mask, :88-93 tests the k-mer that is counted against it
    if (sfx_len > MGC_MAX_COUNT_SUFFIX || strnlen(cfg->count_suffix, sizeof(cfg->count_suffix)) != sfx_len) {
      set_err(nullptr, "mgc_open: count_suffix must hold count_suffix_length (1..%d) bases", MGC_MAX_COUNT_SUFFIX);
      return nullptr;
    }
    if (cfg->k < sfx_len + 3) { set_err(nullptr, "mgc_open: count-suffix of %u bases needs k >= %u", sfx_len, sfx_len + 3); return nullptr; }
    if (2 * cfg->k - 2 * sfx_len > 42) {            // findExpectedSimpleSize, merylOp-count.C:142-145: "Not possible."
      set_err(nullptr, "mgc_open: count-suffix forces simple mode, which takes at most 21 free bases (k - suffix length = %u)", cfg->k - sfx_len);
      return nullptr;
    }
    for (uint32_t i = 0; i < sfx_len; i++) {
      const char ch = cfg->count_suffix[i];
      const bool ok = ch == 'A' || ch == 'C' || ch == 'G' || ch == 'T' || ch == 'a' || ch == 'c' || ch == 'g' || ch == 't';
      if (!ok) { set_err(nullptr, "mgc_open: count-suffix '%s' holds something that is not ACGT", cfg->count_suffix); return nullptr; }
      sfx_test = (sfx_test << 2) | (uint64_t)(((unsigned char)ch >> 1) & 3);        // A0 C1 T2 G3
    }
    sfx_mask = (sfx_len == 32) ? ~0ull : (((uint64_t)1 << (2 * sfx_len)) - 1);
    eff.use_simple = 1;                                                               // merylOp-count.C:379-382
  }
  if (!mgc::effective_geometry(&eff)) return nullptr;
  cfg = &eff;
  if (cfg->k == 0 || cfg->k > 64 || cfg->w_prefix < MGC_NUM_FILES_BITS || cfg->w_prefix > 2 * cfg->k ||
      cfg->w_data != 2 * cfg->k - cfg->w_prefix) {
    set_err(nullptr, "mgc_open: config has not been through mgc_configure_counting (k=%u wPrefix=%u wData=%u)",
            cfg->k, cfg->w_prefix, cfg->w_data);
    return nullptr;
  }

  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev == 0) {
    set_err(nullptr, "mgc_open: no HIP device (%s)", hipGetErrorString(e));
    return nullptr;
  }
  mgc_session *s = new mgc_session();
  s->cfg = *cfg;
  s->sfx_mask = sfx_mask;
  s->sfx_test = sfx_test;
  s->key_words = (cfg->k > 32) ? 2u : 1u;
  if (device >= 0) {
    e = hipSetDevice(device);
    if (e != hipSuccess) { set_err(nullptr, "hipSetDevice(%d): %s", device, hipGetErrorString(e)); delete s; return nullptr; }
    s->device = device;
  } else {
    (void)hipGetDevice(&s->device);
  }
  e = hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&s->st_in, hipStreamNonBlocking);
  if (e != hipSuccess) { set_err(nullptr, "hipStreamCreate: %s", hipGetErrorString(e)); delete s; return nullptr; }
  if (hipStreamCreateWithFlags(&s->stream2, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreateWithFlags(&s->ev_fork, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&s->ev_join, hipEventDisableTiming) != hipSuccess) {
    set_err(nullptr, "hipStreamCreate / hipEventCreate failed"); mgc_close(s); return nullptr;
  }
  memset(&s->prof, 0, sizeof(s->prof));
  memset(s->file_instances, 0, sizeof(s->file_instances));
  memset(s->total_file_instances, 0, sizeof(s->total_file_instances));
  s->sw = mgc::read_switches();                              // the environment is read here, once per session
  return s;
}

extern "C" void mgc_close(mgc_session *s) {
  if (!s) return;
  if (s->worker_active) { s->worker.join(); s->worker_active = false; }
  s->join_prepare();
  (void)hipSetDevice(s->device);
  if (s->st_in) (void)hipStreamSynchronize(s->st_in);
  s->free_result();
  s->free_garbage();
  s->free_arena();
  delete s->runs;
  s->runs = nullptr;
  for (int i = 0; i < 2; i++) {
    if (s->pin[i]) (void)hipHostFree(s->pin[i]);
    if (s->pin_ev[i]) (void)hipEventDestroy(s->pin_ev[i]);
  }
  if (s->st_in) (void)hipStreamDestroy(s->st_in);
  if (s->ev_fork) (void)hipEventDestroy(s->ev_fork);
  if (s->h_stats) (void)hipHostFree(s->h_stats);
  if (s->ev_join) (void)hipEventDestroy(s->ev_join);
  if (s->stream2) (void)hipStreamDestroy(s->stream2);
  for (hipEvent_t e : s->pack_ev) (void)hipEventDestroy(e);
  if (s->ev_pack_done) (void)hipEventDestroy(s->ev_pack_done);
  for (int i = 0; i < mgc_session::HUGE_EXTRA; i++) if (s->stream_h[i]) (void)hipStreamDestroy(s->stream_h[i]);
  if (s->stream) (void)hipStreamDestroy(s->stream);
  delete s;                                                  // (the input ring frees its own: mgc_input.hpp)
}

extern "C" int mgc_set_profiling(mgc_session *s, int enable) {
  if (!s) return MGC_EINVAL;
  s->profiling = enable != 0;
  return MGC_OK;
}

extern "C" int mgc_get_profile(const mgc_session *s, mgc_profile *p) {
  if (!s || !p) return MGC_EINVAL;
  *p = s->prof;
  return MGC_OK;
}

static int copy_device_result(mgc_session *s, uint64_t *keys_lo, uint64_t *keys_hi, uint32_t *counts, uint64_t *block_start) {
  const uint64_t nd = s->n_distinct;
  if (nd && (keys_lo || keys_hi)) {
    if (s->key_words == 1) {
      if (keys_lo) HIP_TRY(s, hipMemcpy(keys_lo, s->d_unique, sizeof(uint64_t) * nd, hipMemcpyDeviceToHost));
      if (keys_hi) memset(keys_hi, 0, sizeof(uint64_t) * nd);
    } else {
      std::vector<uint64_t> tmp(2 * nd);                   // {lo,hi} pairs
      HIP_TRY(s, hipMemcpy(tmp.data(), s->d_unique, sizeof(uint64_t) * 2 * nd, hipMemcpyDeviceToHost));
      for (uint64_t i = 0; i < nd; i++) {
        if (keys_lo) keys_lo[i] = tmp[2 * i];
        if (keys_hi) keys_hi[i] = tmp[2 * i + 1];
      }
    }
  }
  if (counts && nd) HIP_TRY(s, hipMemcpy(counts, s->d_counts, sizeof(uint32_t) * nd, hipMemcpyDeviceToHost));
  if (block_start)  HIP_TRY(s, hipMemcpy(block_start, s->d_block_start, sizeof(uint64_t) * (s->cfg.n_prefix + 1), hipMemcpyDeviceToHost));
  return MGC_OK;
}

// The (k-mer, count) result count_device just left in the arena is parked as a RUN (mgc_runs.cpp): in HBM while the
// store's device budget lasts, in pinned host DRAM otherwise.  Nothing is merged here -- the runs are merged once, when
// the count ends (the analogue of writeBatch's iterations and merylBlockWriter::finish() merging them,
// merylOp-countThreads.C:323-379,461-464).
static int park_batch_result(mgc_session *s) {
  if (!s->runs) {
    // Runs may take what the count itself leaves free: the arena (grow-only, sized by the batches) and the staging buffers are
    // allocated by now, and the final merge frees the arena before it allocates anything.
    uint64_t budget = s->result_budget;
    if (budget == 0) {
      size_t free_b = 0, total_b = 0;
      budget = (hipMemGetInfo(&free_b, &total_b) == hipSuccess) ? (uint64_t)((double)free_b * 0.6) : 0;
    }
    s->runs = new mgc_runs(s->cfg.k, s->cfg.w_prefix, s->device, budget, 0);
  }
  const int rc = s->runs->add(s->d_unique, s->d_counts, s->n_distinct, s->stream);
  if (rc != MGC_OK) s->err = s->runs->err;
  s->have_r = true;
  s->free_result();
  return rc;
}

// one batch: stage[which][0, n) -> count -> park.  Runs on the worker thread while the caller stages the next batch.
int mgc::count_staged_batch(mgc_session *s, int which, uint64_t n) {
  s->d_bases = mgc::stage_ptr(s, which);
  s->n_bases = n;
  int rc = mgc::count_device(s);
  if (rc != MGC_OK) return rc;
  s->total_bases += n;
  s->total_instances += s->n_instances;
  for (int f = 0; f < MGC_NUM_FILES; f++) s->total_file_instances[f] += s->file_instances[f];
  s->n_batches++;
  return park_batch_result(s);
}

// All batches are counted.  If every run is still in HBM and their merge fits beside them, the runs collapse into ONE
// device-resident result -- then the session looks like a single pass's (every result call works).  Otherwise the result
// is OUT OF CORE: it exists only as the runs, and is delivered by streaming (mgc_write_database, mgc_finish*), which merge
// chunk by chunk; the calls that hand out the whole result refuse (MGC_ESTATE).
static int finalize_from_runs(mgc_session *s) {
  hipStream_t st = s->stream;
  s->n_instances = s->total_instances;
  s->n_bases = s->total_bases;
  memcpy(s->file_instances, s->total_file_instances, sizeof(s->file_instances));
  HIP_TRY(s, hipStreamSynchronize(s->st_in));
  s->free_arena();                                            // the count's buffers: the merge gets their room
  s->state_ready = false;
  mgc_runs *r = s->runs;
  const size_t esz = sizeof(uint64_t) * s->key_words + sizeof(uint32_t);
  size_t free_b = 0, total_b = 0;
  (void)hipMemGetInfo(&free_b, &total_b);
  const bool fits = r->all_on_device() && (uint64_t)free_b > r->entries() * esz + (64ull << 20);
  s->prof.n_batches = s->n_batches;
  if (fits) {
    const void *k = nullptr; const uint32_t *c = nullptr; uint64_t n = 0;
    int rc = r->collapse(&k, &c, &n);
    if (rc == MGC_ENOMEM) {                                   // (hipMemGetInfo is an estimate: fragmentation) the store is consistent: out of core
      s->ooc = true;
      s->n_distinct = 0;
      s->merge_ms = r->prof.merge_ms;
      s->prof.merge_ms = s->merge_ms;
      return MGC_OK;
    }
    if (rc != MGC_OK) { s->err = r->err; return rc; }
    s->n_distinct = n;
    s->d_unique = const_cast<void *>(k);
    s->d_counts = const_cast<uint32_t *>(c);
    HIP_TRY(s, s->ensure(mgc_session::B_BLOCKS, sizeof(uint64_t) * (s->cfg.n_prefix + 1)));
    s->d_block_start = reinterpret_cast<uint64_t *>(s->buf[mgc_session::B_BLOCKS].p);
    HIP_TRY(s, mgc::launch_block_offsets(s->d_unique, s->n_distinct, s->key_words, s->cfg.w_data, s->cfg.n_prefix, s->d_block_start, st));
    HIP_TRY(s, hipStreamSynchronize(st));
  } else {
    s->ooc = true;
    s->n_distinct = 0;                                        // known once the runs have been merged (delivery)
  }
  s->merge_ms = r->prof.merge_ms;
  s->prof.merge_ms = s->merge_ms;
  return MGC_OK;
}

extern "C" int mgc_count(mgc_session *s) {
  if (!s) return MGC_EINVAL;
  if (s->borrowed) {                                         // the caller's device buffer: every call counts it again
    const int rc = mgc::count_device(s);
    if (rc == MGC_OK) s->counted = true;
    return rc;
  }
  if (s->counted) return MGC_OK;                             // nothing can have been pushed since: the result stands
  if (s->text_open) { set_err(&s->err, "mgc_count: a text file is still open (mgc_end_text)"); return MGC_ESTATE; }
  int rc = mgc::settle_input(s);
  if (rc != MGC_OK) return rc;
  if (!s->have_r) {                                          // everything fits in one pass
    s->d_bases = mgc::stage_ptr(s, s->fill);
    s->n_bases = s->fill_len;
    rc = mgc::count_device(s);
    s->prof.n_batches = 1;
  } else {
    if (s->fill_len) rc = mgc::count_staged_batch(s, s->fill, s->fill_len);
    if (rc == MGC_OK) rc = finalize_from_runs(s);
  }
  if (rc == MGC_OK) s->counted = true;
  s->free_garbage();
  if (getenv("MGC_IO_TRACE") && s->input_seen)
    fprintf(stderr, "[io] host pushes: memcpy into pinned %.3f s, flush (grow + async upload + wait for the other chunk) %.3f s, batch cuts %.3f s "
                    "(of which waiting for the worker %.3f s), staging-buffer growth %.3f s; %u batches, device merges %.1f ms; "
                    "arena hipMalloc/hipFree %.3f s for %.1f GB\n",
            s->tr_memcpy, s->tr_flush, s->tr_cut, s->tr_join, s->tr_grow, s->n_batches, s->merge_ms, s->tr_alloc, s->tr_alloc_bytes / 1e9);
  return rc;
}

extern "C" int mgc_staged_bases(mgc_session *s, const uint8_t **d_bases, uint64_t *n_bases) {
  if (!s || !d_bases || !n_bases) return MGC_EINVAL;
  if (s->borrowed) { *d_bases = s->d_bases; *n_bases = s->n_bases; return MGC_OK; }
  if (s->text_open) { set_err(&s->err, "mgc_staged_bases: a text file is still open (mgc_end_text)"); return MGC_ESTATE; }
  if (s->counted || s->have_r || s->n_batches) { set_err(&s->err, "mgc_staged_bases: part of the input has already been counted"); return MGC_ESTATE; }
  const int rc = mgc::settle_input(s);
  if (rc != MGC_OK) return rc;
  HIP_TRY(s, hipStreamSynchronize(s->st_in));
  *d_bases = mgc::stage_ptr(s, s->fill);
  *n_bases = s->fill_len;
  return MGC_OK;
}

static int count_buckets(mgc_session *s, const mgc::CountInput &in) {
  if (!s || !in.counts || in.bucket_bits < MGC_NUM_FILES_BITS || in.bucket_bits > MGC_MAX_BUCKET_BITS || in.bucket_bits > 2 * s->cfg.k)
    return MGC_EINVAL;
  uint64_t n = 0;
  for (uint32_t b = 0; b < (1u << in.bucket_bits); b++) n += in.counts[b];
  if (n && !in.keys) return MGC_EINVAL;
  if (s->input_seen || s->borrowed) {
    set_err(&s->err, "mgc_count_buckets: the session already holds pushed bases");
    return MGC_ESTATE;
  }
  const int rc = mgc::count_device(s, in);
  if (rc == MGC_OK) s->counted = true;
  return rc;
}

extern "C" int mgc_count_buckets(mgc_session *s, void *d_keys, uint32_t bucket_bits, const uint64_t *bucket_counts) {
  mgc::CountInput in;
  in.keys = d_keys; in.counts = bucket_counts; in.bucket_bits = bucket_bits;
  return count_buckets(s, in);
}

// ... with the packed result written straight to the caller's buffers when it fits (capacity in k-mers): the waves of a sharded
// count land in ONE pre-sized result instead of being copied out of the session and concatenated.  *n_distinct > capacity: the
// result stayed in the session (mgc_copy_result_device / mgc_get_result_device as usual).
extern "C" int mgc_count_buckets_into(mgc_session *s, void *d_keys, uint32_t bucket_bits, const uint64_t *bucket_counts,
                                      void *d_out_keys, uint32_t *d_out_counts, uint64_t capacity, uint64_t *n_distinct,
                                      const uint64_t *d_fine_hist) {
  if (!s || !n_distinct || (capacity && (!d_out_keys || !d_out_counts))) return MGC_EINVAL;
  mgc::CountInput in;
  in.keys = d_keys; in.counts = bucket_counts; in.bucket_bits = bucket_bits; in.fine = d_fine_hist;
  in.out_keys = d_out_keys; in.out_counts = d_out_counts; in.out_cap = capacity;
  const int rc = count_buckets(s, in);
  if (rc == MGC_OK) *n_distinct = s->n_distinct;
  return rc;
}

extern "C" int mgc_count_partitioned(mgc_session *s, void *d_keys, const uint64_t *file_counts, void *reserved) {
  (void)reserved;
  return mgc_count_buckets(s, d_keys, MGC_NUM_FILES_BITS, file_counts);
}

extern "C" int mgc_get_result_info(const mgc_session *s, mgc_result_info *info) {
  if (!s || !info) return MGC_EINVAL;
  if (!s->counted) return MGC_ESTATE;
  info->n_bases = s->n_bases;
  info->n_instances = s->n_instances;
  info->n_distinct = s->n_distinct;
  info->w_prefix = s->cfg.w_prefix;
  info->w_data = s->cfg.w_data;
  info->n_prefix = s->cfg.n_prefix;
  memcpy(info->file_instances, s->file_instances, sizeof(info->file_instances));
  return MGC_OK;
}

static int refuse_ooc(mgc_session *s, const char *what) {
  set_err(&s->err, "%s: the result is out of core (larger than the device holds): stream it with mgc_write_database / mgc_finish", what);
  return MGC_ESTATE;
}

extern "C" int mgc_result_out_of_core(const mgc_session *s) { return (s && s->counted && s->ooc) ? 1 : 0; }

extern "C" int mgc_set_result_budget(mgc_session *s, uint64_t device_bytes) {
  if (!s) return MGC_EINVAL;
  s->result_budget = device_bytes;
  return MGC_OK;
}

extern "C" int mgc_get_runs_profile(const mgc_session *s, mgc_runs_profile *p) {
  if (!s || !p) return MGC_EINVAL;
  memset(p, 0, sizeof(*p));
  if (s->runs) *p = s->runs->prof;
  return MGC_OK;
}

extern "C" int mgc_copy_result_device(mgc_session *s, void *d_keys_out, uint32_t *d_counts_out) {
  if (!s) return MGC_EINVAL;
  if (!s->counted) return MGC_ESTATE;
  if (s->ooc) return refuse_ooc(s, "mgc_copy_result_device");
  const size_t kbytes = sizeof(uint64_t) * s->key_words;
  if (s->n_distinct) {
    if (d_keys_out) HIP_TRY(s, hipMemcpyAsync(d_keys_out, s->d_unique, kbytes * s->n_distinct, hipMemcpyDeviceToDevice, s->stream));
    if (d_counts_out) HIP_TRY(s, hipMemcpyAsync(d_counts_out, s->d_counts, sizeof(uint32_t) * s->n_distinct, hipMemcpyDeviceToDevice, s->stream));
  }
  HIP_TRY(s, hipStreamSynchronize(s->stream));
  return MGC_OK;
}

extern "C" int mgc_get_result_device(const mgc_session *s, const void **d_unique, const uint32_t **d_counts,
                                     const uint64_t **d_block_start, uint32_t *key_words) {
  if (!s) return MGC_EINVAL;
  if (!s->counted) return MGC_ESTATE;
  if (s->ooc) return refuse_ooc(const_cast<mgc_session *>(s), "mgc_get_result_device");
  if (d_unique) *d_unique = s->d_unique;
  if (d_counts) *d_counts = s->d_counts;
  if (d_block_start) *d_block_start = s->d_block_start;
  if (key_words) *key_words = s->key_words;
  return MGC_OK;
}

extern "C" int mgc_copy_result(const mgc_session *cs, uint64_t *keys_lo, uint64_t *keys_hi, uint32_t *counts,
                               uint64_t *block_start) {
  mgc_session *s = const_cast<mgc_session *>(cs);
  if (!s) return MGC_EINVAL;
  if (!s->counted) return MGC_ESTATE;
  if (s->ooc) return refuse_ooc(s, "mgc_copy_result");
  HIP_TRY(s, hipSetDevice(s->device));
  return copy_device_result(s, keys_lo, keys_hi, counts, block_start);
}
