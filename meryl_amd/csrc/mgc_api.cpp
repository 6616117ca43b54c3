// mgc_api.cpp -- C-ABI layer (include/meryl_gpu_count.h) over the gfx950 kernels.
//
// Host-side mirror of the reference's counting engine:
//   mgc_configure_counting  <-> merylOperation::configureCounting  src/meryl/merylOp-count.C:300-403
//   mgc_open/push/count/finish <-> merylOperation::countThreads     src/meryl/merylOp-countThreads.C:385-474
// There is NO CPU fallback in here: every compute entry point launches HIP
// kernels and fails with MGC_EHIP if the device or the code object is missing.
#include "../../include/meryl_gpu_count.h"
#include "mgc_device.h"
#include "mgc_session.hpp"
#include "mgc_gzip_par.hpp"
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
    if (s->text_pinned[i]) (void)hipHostFree(s->text_pinned[i]);
    if (s->text_ev[i]) (void)hipEventDestroy(s->text_ev[i]);
    if (s->up_ev[i]) (void)hipEventDestroy(s->up_ev[i]);
    if (s->pin[i]) (void)hipHostFree(s->pin[i]);
    if (s->pin_ev[i]) (void)hipEventDestroy(s->pin_ev[i]);
    if (s->bam_seg_pinned[i]) (void)hipHostFree(s->bam_seg_pinned[i]);
    if (s->gz_sym_pinned[i]) (void)hipHostFree(s->gz_sym_pinned[i]);
    if (s->gz_tab_pinned[i]) (void)hipHostFree(s->gz_tab_pinned[i]);
  }
  for (char *&p : s->text_ring) if (p) { (void)hipHostFree(p); p = nullptr; }
  if (s->st_up) { (void)hipStreamSynchronize(s->st_up); (void)hipStreamDestroy(s->st_up); }
  if (s->st_in) (void)hipStreamDestroy(s->st_in);
  if (s->ev_fork) (void)hipEventDestroy(s->ev_fork);
  if (s->h_stats) (void)hipHostFree(s->h_stats);
  if (s->ev_join) (void)hipEventDestroy(s->ev_join);
  if (s->stream2) (void)hipStreamDestroy(s->stream2);
  for (hipEvent_t e : s->pack_ev) (void)hipEventDestroy(e);
  if (s->ev_pack_done) (void)hipEventDestroy(s->ev_pack_done);
  for (int i = 0; i < mgc_session::HUGE_EXTRA; i++) if (s->stream_h[i]) (void)hipStreamDestroy(s->stream_h[i]);
  if (s->stream) (void)hipStreamDestroy(s->stream);
  delete s;
}

// ---------------------------------------------------------------------------------------------------------------
//  Input staging (see mgc_session.hpp): one device-resident base stream per batch, double buffered
// ---------------------------------------------------------------------------------------------------------------
struct HostParseState { uint64_t out_len, file_start_len; uint32_t state, prev_nl, error, pad; };

static int count_staged_batch(mgc_session *s, int which, uint64_t n);      // count stage[which][0, n) and merge it into R

// The count's largest buffer (the k-mer instances, 8 / 16 B per base at most) is allocated NOW, by a helper thread, while the
// caller reads and uploads its input: a first large hipMalloc is the slowest single thing a freshly started process does
// (0.3 s for 100 GB on a quiet device, seconds when another process has just released that much), and until the count starts
// nobody needs the memory.  Only when the whole input is expected to fit one pass; a wrong estimate costs a re-allocation,
// never a wrong result.
extern "C" int mgc_prepare(mgc_session *s, uint64_t expected_bases) {
  if (!s) return MGC_EINVAL;
  if (s->borrowed || s->counted || s->prep_active || expected_bases == 0) return MGC_OK;
  HIP_TRY(s, hipSetDevice(s->device));
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return MGC_OK;
  const uint64_t per_base = 2 + 14ull * s->key_words;
  if (s->batch_limit && expected_bases > s->batch_limit) return MGC_OK;
  if ((double)expected_bases * (double)per_base > 0.8 * (double)free_b) return MGC_OK;       // batches: their arena is sized by the first one
  const size_t bytes = sizeof(uint64_t) * s->key_words * expected_bases;
  s->prep_active = true;
  s->prep_thread = std::thread([s, bytes] {
    (void)hipSetDevice(s->device);
    if (s->ensure(mgc_session::B_X, bytes) != hipSuccess) (void)hipGetLastError();           // the count will say so itself
    // ... and the code objects of the count and of the database encoder: loaded lazily at the first launch, i.e. inside a fresh
    // process's first count otherwise (0.36 s of count for a 0.12 s step, profiles/r04o)
    (void)mgc::warm_kmer(); (void)mgc::warm_scan(); (void)mgc::warm_sort(); (void)mgc::warm_finish(); (void)mgc::warm_encode(); (void)mgc::warm_value_hist();
    (void)hipGetLastError();
  });
  return MGC_OK;
}

extern "C" int mgc_set_batch_bases(mgc_session *s, uint64_t bases_per_batch) {
  if (!s) return MGC_EINVAL;
  s->batch_limit = bases_per_batch;
  return MGC_OK;
}

static inline int stage_id(int which) { return which ? mgc_session::B_STAGE1 : mgc_session::B_STAGE0; }
static inline uint8_t *stage_ptr(mgc_session *s, int which) { return reinterpret_cast<uint8_t *>(s->buf[stage_id(which)].p); }

// first input of a session: streams, parse state, the batch size
static int input_setup(mgc_session *s) {
  if (s->borrowed || s->counted) { set_err(&s->err, "input after device input / count"); return MGC_ESTATE; }
  HIP_TRY(s, hipSetDevice(s->device));
  if (s->state_ready) return MGC_OK;
  if (s->batch_limit == 0) {
    // One pass holds, per base: the staged base, 0.87 k-mer instances of 8 (16) B in X, 4 B of count scratch each, the
    // distinct k-mers with their counts (about a seventh of the instances at 30x), the ping-pong buffer of the largest
    // file -- measured 13 B per base at k=21 (130 GB for 10 Gbp: DESIGN.md section 2), 16 (30) B with slack.  A fifth of
    // the HBM stays free for the running result of earlier batches and its merge target.
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b) {
      const uint64_t per_base = 2 + 14ull * s->key_words;
      s->batch_limit = (uint64_t)((double)free_b * 0.80 / (double)per_base);
    }
    if (s->batch_limit < (1u << 20)) s->batch_limit = 1u << 20;
  }
  HIP_TRY(s, s->ensure(mgc_session::B_TEXT_STATE, mgc::text_parse_state_bytes() + 64));
  HIP_TRY(s, s->ensure_preserve(stage_id(s->fill), 1u << 20, 0, s->st_in));
  HIP_TRY(s, mgc::launch_text_file_op(s->buf[mgc_session::B_TEXT_STATE].p, stage_ptr(s, s->fill), 3, s->st_in));
  s->state_ready = true;
  return MGC_OK;
}

// the device knows the exact length of the staged stream; bring the host's copy up to date (synchronises st_in)
static int resolve_length(mgc_session *s, HostParseState *out = nullptr) {
  HostParseState h;
  HIP_TRY(s, hipMemcpyAsync(&h, s->buf[mgc_session::B_TEXT_STATE].p, sizeof(h), hipMemcpyDeviceToHost, s->st_in));
  HIP_TRY(s, hipStreamSynchronize(s->st_in));
  s->fill_len = h.out_len;
  s->len_inexact = false;
  if (out) *out = h;
  return MGC_OK;
}

static int join_worker(mgc_session *s) {
  if (s->worker_active) {
    const double t0 = mgc::now_s();
    s->worker.join();
    s->tr_join += mgc::now_s() - t0;
    s->worker_active = false;
    if (s->worker_rc != MGC_OK) return s->worker_rc;
  }
  return s->worker_rc;
}

// host-pushed bases collected in the current pinned chunk -> stage[fill] (asynchronous; the other chunk takes over)
static int flush_pinned(mgc_session *s) {
  if (s->pin_len == 0) return MGC_OK;
  if (s->len_inexact) { const int rc = resolve_length(s); if (rc != MGC_OK) return rc; }
  const int c = s->pin_cur;
  HIP_TRY(s, s->ensure_preserve(stage_id(s->fill), s->fill_len + s->pin_len + 4096, s->fill_len, s->st_in));
  HIP_TRY(s, hipMemcpyAsync(stage_ptr(s, s->fill) + s->fill_len, s->pin[c], s->pin_len, hipMemcpyHostToDevice, s->st_in));
  s->fill_len += s->pin_len;
  HIP_TRY(s, mgc::launch_text_set_len(s->buf[mgc_session::B_TEXT_STATE].p, s->fill_len, 0, s->st_in));
  HIP_TRY(s, hipEventRecord(s->pin_ev[c], s->st_in));
  s->pin_used[c] = true;
  s->pin_len = 0;
  s->pin_cur = c ^ 1;
  if (s->pin_used[s->pin_cur]) HIP_TRY(s, hipEventSynchronize(s->pin_ev[s->pin_cur]));     // that chunk's upload has read it
  return MGC_OK;
}

// The staged stream has reached the batch size: everything up to the last sequence boundary becomes a batch, counted by
// the worker thread while the caller goes on filling the other staging buffer (k-mers never span a breaker, so no
// carry is needed, and `compress` stays a per-sequence operation).
static int cut_batch(mgc_session *s) {
  int rc = flush_pinned(s);
  if (rc != MGC_OK) return rc;
  HostParseState h;
  rc = resolve_length(s, &h);
  if (rc != MGC_OK) return rc;
  if (s->text_open && h.error) return MGC_OK;              // the open file is about to be refused and rolled back: not now
  if (s->fill_len < s->batch_limit) return MGC_OK;         // the bound was pessimistic
  if (s->fill_len < s->no_cut_below) return MGC_OK;        // no sequence boundary was found last time: look again once the stream has doubled
  uint64_t *d_last = reinterpret_cast<uint64_t *>(reinterpret_cast<unsigned char *>(s->buf[mgc_session::B_TEXT_STATE].p) +
                                                  ((mgc::text_parse_state_bytes() + 7) / 8) * 8);
  uint64_t cut = 0;
  HIP_TRY(s, mgc::launch_last_breaker(stage_ptr(s, s->fill), s->fill_len, d_last, s->st_in));
  HIP_TRY(s, hipMemcpyAsync(&cut, d_last, sizeof(cut), hipMemcpyDeviceToHost, s->st_in));
  HIP_TRY(s, hipStreamSynchronize(s->st_in));
  uint64_t overlap = 0;
  if (cut == 0) {
    // One sequence longer than a batch (this used to return and re-scan the whole staged stream on every later
    // push -- O(n^2) -- while staging grew without bound).  The reference spills inside a sequence too; here the batch is cut
    // at the end of what is staged and the last k-1 bases are staged AGAIN in front of the next batch: a window that starts
    // in them is incomplete in this batch and complete in the next, so no k-mer is lost or counted twice (the rule the
    // node count cuts its slices by).  `compress` needs whole sequences: such a stream waits until it has doubled.
    if (s->cfg.homopoly_compress || s->text_open || s->fill_len < 4ull * s->cfg.k) {
      s->no_cut_below = s->fill_len * 2;
      return MGC_OK;
    }
    cut = s->fill_len;
    overlap = s->cfg.k - 1;
  }
  rc = join_worker(s);                                      // the previous batch is done: its staging buffer is free, R is stable
  if (rc != MGC_OK) return rc;
  const uint64_t tail = s->fill_len - cut + overlap;
  cut -= overlap;                                           // the tail starts k-1 bases before the cut ...
  const int other = s->fill ^ 1;
  HIP_TRY(s, s->ensure_preserve(stage_id(other), tail + (1u << 20), 0, s->st_in));
  if (tail) HIP_TRY(s, hipMemcpyAsync(stage_ptr(s, other), stage_ptr(s, s->fill) + cut, tail, hipMemcpyDeviceToDevice, s->st_in));
  HIP_TRY(s, mgc::launch_text_set_len(s->buf[mgc_session::B_TEXT_STATE].p, tail, s->text_open ? 1 : 0, s->st_in));
  HIP_TRY(s, hipStreamSynchronize(s->st_in));
  if (s->text_open) s->text_cut_in_file = true;
  const int which = s->fill;
  s->fill = other;
  s->fill_len = tail;
  s->no_cut_below = 0;
  cut += overlap;                                           // ... and the batch still ends at the cut
  s->worker_rc = MGC_OK;
  s->worker_active = true;
  s->worker = std::thread([s, which, cut] { s->worker_rc = count_staged_batch(s, which, cut); });
  return MGC_OK;
}

extern "C" int mgc_push_bases(mgc_session *s, const char *bases, size_t len, int end_of_sequence) {
  if (!s || (!bases && len)) return MGC_EINVAL;
  int rc = input_setup(s);
  if (rc != MGC_OK) return rc;
  if (s->text_open) { set_err(&s->err, "mgc_push_bases while a text file is open (mgc_end_text first)"); return MGC_ESTATE; }
  s->input_seen = true;
  for (int i = 0; i < 2; i++) {
    if (!s->pin[i]) HIP_TRY(s, hipHostMalloc(reinterpret_cast<void **>(&s->pin[i]), mgc_session::PIN_CHUNK, hipHostMallocDefault));
    if (!s->pin_ev[i]) HIP_TRY(s, hipEventCreateWithFlags(&s->pin_ev[i], hipEventDisableTiming));
  }
  const char breaker = '.';                                  // merylOp-countThreads.C:214-215
  for (int part = 0; part < 2; part++) {
    const char *src = part ? &breaker : bases;
    size_t left = part ? (end_of_sequence ? 1 : 0) : len;
    while (left) {
      const size_t take = std::min(left, mgc_session::PIN_CHUNK - s->pin_len);
      const double t0 = mgc::now_s();
      memcpy(s->pin[s->pin_cur] + s->pin_len, src, take);
      const double t1 = mgc::now_s();
      s->tr_memcpy += t1 - t0;
      s->pin_len += take; src += take; left -= take;
      if (s->pin_len == mgc_session::PIN_CHUNK) { rc = flush_pinned(s); if (rc != MGC_OK) return rc; }
      const double t2 = mgc::now_s();
      s->tr_flush += t2 - t1;
      if (s->fill_len + s->pin_len >= s->batch_limit) { rc = cut_batch(s); if (rc != MGC_OK) return rc; s->tr_cut += mgc::now_s() - t2; }
    }
  }
  return MGC_OK;
}

// ---- text input, parsed on the device (include/meryl_gpu_count.h) ------------------------------
static int text_setup(mgc_session *s) {
  int rc = input_setup(s);
  if (rc != MGC_OK) return rc;
  if (!s->text_pinned[0]) {
    HIP_TRY(s, s->ensure(mgc_session::B_TEXT_IN0, mgc_session::TEXT_CHUNK));
    HIP_TRY(s, s->ensure(mgc_session::B_TEXT_IN1, mgc_session::TEXT_CHUNK));
    HIP_TRY(s, s->ensure(mgc_session::B_TEXT_WS, mgc::text_parse_workspace_bytes(mgc_session::TEXT_CHUNK)));
    if (!s->st_up) HIP_TRY(s, hipStreamCreateWithFlags(&s->st_up, hipStreamNonBlocking));
    for (int i = 0; i < 2; i++) {
      if (!s->text_pinned[i]) HIP_TRY(s, hipHostMalloc(reinterpret_cast<void **>(&s->text_pinned[i]), mgc_session::TEXT_CHUNK, hipHostMallocDefault));
      if (!s->text_ev[i]) HIP_TRY(s, hipEventCreateWithFlags(&s->text_ev[i], hipEventDisableTiming));
      if (!s->up_ev[i]) HIP_TRY(s, hipEventCreateWithFlags(&s->up_ev[i], hipEventDisableTiming));
    }
  }
  return MGC_OK;
}

extern "C" int mgc_reserve_text(mgc_session *s, uint64_t text_bytes) {
  if (!s) return MGC_EINVAL;
  int rc = text_setup(s);
  if (rc != MGC_OK) return rc;
  // no more than a batch (plus what a chunk can add before the cut is noticed) is ever staged at once
  const uint64_t want = std::min<uint64_t>(text_bytes, s->batch_limit + 2 * mgc_session::TEXT_CHUNK) + 4096;
  HIP_TRY(s, s->ensure_preserve(stage_id(s->fill), want, s->fill_len, s->st_in));
  return MGC_OK;
}

extern "C" int mgc_begin_text(mgc_session *s, int format) {
  if (!s || (format != MGC_TEXT_FASTA && format != MGC_TEXT_FASTQ)) return MGC_EINVAL;
  if (s->text_open) { set_err(&s->err, "mgc_begin_text: the previous file was not ended"); return MGC_ESTATE; }
  int rc = text_setup(s);
  if (rc != MGC_OK) return rc;
  rc = flush_pinned(s);                                     // host-pushed bases come first in the stream
  if (rc != MGC_OK) return rc;
  HIP_TRY(s, mgc::launch_text_file_op(s->buf[mgc_session::B_TEXT_STATE].p, stage_ptr(s, s->fill), 0, s->st_in));
  s->text_format = format;
  s->text_open = true;
  s->text_cut_in_file = false;
  s->input_seen = true;
  return MGC_OK;
}

// one piece (<= TEXT_CHUNK bytes, in pinned memory) -> device input buffer b -> parse kernels; returns once they are queued
int mgc::text_submit(mgc_session *s, const char *pinned_src, size_t piece) {
  const uint32_t b = s->text_next & 1u;
  if (s->text_ev_used[b]) HIP_TRY(s, hipEventSynchronize(s->text_ev[b]));       // device buffer b (and its previous source) are free again
  HIP_TRY(s, s->ensure_preserve(stage_id(s->fill), s->fill_len + piece + 4096, s->fill_len, s->st_in));
  uint8_t *d_in = reinterpret_cast<uint8_t *>(s->buf[b ? mgc_session::B_TEXT_IN1 : mgc_session::B_TEXT_IN0].p);
  // the copy runs on its own stream, so that chunk c travels while chunk c-1 is parsed (one stream did them in turn: 0.56 ms
  // of copy + 0.4 ms of parse per 32 MiB, 0.6 s of the 20 GB file -> database run; profiles/r03m_e2e_io.txt)
  HIP_TRY(s, hipMemcpyAsync(d_in, pinned_src, piece, hipMemcpyHostToDevice, s->st_up));
  HIP_TRY(s, hipEventRecord(s->up_ev[b], s->st_up));
  HIP_TRY(s, hipStreamWaitEvent(s->st_in, s->up_ev[b], 0));
  HIP_TRY(s, mgc::launch_text_parse(d_in, piece, s->text_format == MGC_TEXT_FASTQ, s->buf[mgc_session::B_TEXT_STATE].p,
                                    s->buf[mgc_session::B_TEXT_WS].p, stage_ptr(s, s->fill), s->st_in));
  HIP_TRY(s, hipEventRecord(s->text_ev[b], s->st_in));
  s->text_ev_used[b] = true;
  s->text_next++;
  s->fill_len += piece;                                     // an upper bound: headers, qualities and line ends are dropped
  s->len_inexact = true;
  if (s->fill_len >= s->batch_limit) return cut_batch(s);
  return MGC_OK;
}

extern "C" int mgc_push_text(mgc_session *s, const char *text, size_t len) {
  if (!s || (!text && len)) return MGC_EINVAL;
  if (!s->text_open || s->text_format == mgc_session::TEXT_BAM) { set_err(&s->err, "mgc_push_text without mgc_begin_text"); return MGC_ESTATE; }
  HIP_TRY(s, hipSetDevice(s->device));
  while (len) {
    const size_t piece = len < mgc_session::TEXT_CHUNK ? len : mgc_session::TEXT_CHUNK;
    const uint32_t b = s->text_next & 1u;
    if (s->text_ev_used[b]) HIP_TRY(s, hipEventSynchronize(s->text_ev[b]));     // pinned + device buffer b are free again
    memcpy(s->text_pinned[b], text, piece);
    const int rc = mgc::text_submit(s, s->text_pinned[b], piece);
    if (rc != MGC_OK) return rc;
    text += piece;
    len -= piece;
  }
  return MGC_OK;
}

// the last two text uploads still read from their pinned sources: wait for them
void mgc::text_drain(mgc_session *s) {
  for (int b = 0; b < 2; b++) if (s->text_ev_used[b]) (void)hipEventSynchronize(s->text_ev[b]);
}

// Closes the open file and takes what it has put into the stream back out.  MGC_EINVAL, and the stream as it is, when part
// of the file went into a batch that is already counted: that cannot be taken back.
int mgc::text_rollback(mgc_session *s) {
  s->text_open = false;
  if (s->text_cut_in_file) return MGC_EINVAL;
  HIP_TRY(s, mgc::launch_text_file_op(s->buf[mgc_session::B_TEXT_STATE].p, stage_ptr(s, s->fill), 2, s->st_in));
  return resolve_length(s);
}

extern "C" int mgc_end_text(mgc_session *s) {
  if (!s) return MGC_EINVAL;
  if (!s->text_open || s->text_format == mgc_session::TEXT_BAM) { set_err(&s->err, "mgc_end_text without mgc_begin_text"); return MGC_ESTATE; }
  HIP_TRY(s, hipSetDevice(s->device));
  s->text_open = false;
  HIP_TRY(s, s->ensure_preserve(stage_id(s->fill), s->fill_len + 4096, s->fill_len, s->st_in));
  HIP_TRY(s, mgc::launch_text_file_op(s->buf[mgc_session::B_TEXT_STATE].p, stage_ptr(s, s->fill), 1, s->st_in));
  HostParseState h;
  int rc = resolve_length(s, &h);
  if (rc != MGC_OK) return rc;
  if (h.error) {
    rc = mgc::text_rollback(s);
    if (rc == MGC_EINVAL)
      set_err(&s->err, "the file stops being strict four-line FASTQ after part of it was counted (input larger than one batch): "
                       "convert it, or feed it through mgc_push_bases from the start");
    if (rc != MGC_OK) return rc;
    set_err(&s->err, "the file is not strict four-line FASTQ: feed it through mgc_push_bases (meryl_seq.h reader)");
    return MGC_EFORMAT;
  }
  if (s->fill_len >= s->batch_limit) return cut_batch(s);
  return MGC_OK;
}

// ---- BAM input, decoded on the device (include/meryl_gpu_count.h) ------------------------------
// The open BAM file shares the text file's state (text_open, the cut inside a file, the rollback point in the device's parse
// state); its lengths are exact on the host, so fill_len stays exact while it is open.
extern "C" int mgc_begin_bam(mgc_session *s) {
  if (!s) return MGC_EINVAL;
  if (s->text_open) { set_err(&s->err, "mgc_begin_bam: the previous file was not ended"); return MGC_ESTATE; }
  int rc = text_setup(s);
  if (rc != MGC_OK) return rc;
  rc = flush_pinned(s);                                     // host-pushed bases come first in the stream
  if (rc != MGC_OK) return rc;
  if (s->len_inexact) { rc = resolve_length(s); if (rc != MGC_OK) return rc; }
  HIP_TRY(s, mgc::launch_text_file_op(s->buf[mgc_session::B_TEXT_STATE].p, stage_ptr(s, s->fill), 0, s->st_in));
  s->bam_walker.reset();
  s->tr_bam_walk = 0;
  s->text_format = mgc_session::TEXT_BAM;
  s->text_open = true;
  s->text_cut_in_file = false;
  s->input_seen = true;
  return MGC_OK;
}

int mgc::bam_submit(mgc_session *s, const char *pinned_src, size_t piece) {
  const double t0 = mgc::now_s();
  s->bam_segs.clear();
  uint64_t out_bytes = 0;
  const bool ok = s->bam_walker.walk(reinterpret_cast<const unsigned char *>(pinned_src), piece, &s->bam_segs, &out_bytes);
  s->tr_bam_walk += mgc::now_s() - t0;
  if (!ok) return mgc::BAM_REFUSED;
  const size_t nseg = s->bam_segs.size();
  if (nseg == 0) {
    // Header bytes, names, qualities, aux -- a piece that lies wholly inside a long record's tail: nothing for the device.  The
    // whole-file reader's ring gives a slot back two pieces after its submit BECAUSE a submit waits for the piece two before it
    // (mgc_chunk_ring.hpp); a piece that queues nothing would break that count, so it waits for both pieces in flight instead.
    mgc::text_drain(s);
    return MGC_OK;
  }
  const uint32_t b = s->text_next & 1u;
  if (s->text_ev_used[b]) HIP_TRY(s, hipEventSynchronize(s->text_ev[b]));       // device buffers b (and their previous sources) are free again
  HIP_TRY(s, s->ensure_preserve(stage_id(s->fill), s->fill_len + out_bytes + 4096, s->fill_len, s->st_in));
  if (s->bam_seg_cap[b] < nseg) {                           // grow-only, with room to spare: records of one file are alike
    if (s->bam_seg_pinned[b]) { (void)hipHostFree(s->bam_seg_pinned[b]); s->bam_seg_pinned[b] = nullptr; s->bam_seg_cap[b] = 0; }
    const size_t want = nseg + nseg / 2 + 4096;
    HIP_TRY(s, hipHostMalloc(reinterpret_cast<void **>(&s->bam_seg_pinned[b]), want * sizeof(mgc::BamSegment), hipHostMallocDefault));
    s->bam_seg_cap[b] = want;
  }
  const int seg_buf = b ? mgc_session::B_BAM_SEG1 : mgc_session::B_BAM_SEG0;
  HIP_TRY(s, s->ensure(seg_buf, s->bam_seg_cap[b] * sizeof(mgc::BamSegment)));
  memcpy(s->bam_seg_pinned[b], s->bam_segs.data(), nseg * sizeof(mgc::BamSegment));
  uint8_t *d_in = reinterpret_cast<uint8_t *>(s->buf[b ? mgc_session::B_TEXT_IN1 : mgc_session::B_TEXT_IN0].p);
  HIP_TRY(s, hipMemcpyAsync(d_in, pinned_src, piece, hipMemcpyHostToDevice, s->st_up));
  HIP_TRY(s, hipMemcpyAsync(s->buf[seg_buf].p, s->bam_seg_pinned[b], nseg * sizeof(mgc::BamSegment), hipMemcpyHostToDevice, s->st_up));
  HIP_TRY(s, hipEventRecord(s->up_ev[b], s->st_up));
  HIP_TRY(s, hipStreamWaitEvent(s->st_in, s->up_ev[b], 0));
  HIP_TRY(s, mgc::launch_bam_decode(d_in, piece, s->buf[seg_buf].p, nseg, out_bytes, stage_ptr(s, s->fill) + s->fill_len, s->st_in));
  s->fill_len += out_bytes;                                 // exact
  HIP_TRY(s, mgc::launch_text_set_len(s->buf[mgc_session::B_TEXT_STATE].p, s->fill_len, 0, s->st_in));
  HIP_TRY(s, hipEventRecord(s->text_ev[b], s->st_in));
  s->text_ev_used[b] = true;
  s->text_next++;
  if (s->fill_len >= s->batch_limit) return cut_batch(s);
  return MGC_OK;
}

int mgc::bam_refuse(mgc_session *s, const char *what) {
  const std::string why = s->bam_walker.error();
  const int rc = mgc::text_rollback(s);
  if (rc == MGC_EINVAL) set_err(&s->err, "'%s': %s, after part of the file was counted (input larger than one batch)", what, why.c_str());
  if (rc != MGC_OK) return rc;
  set_err(&s->err, "'%s': %s", what, why.c_str());
  return MGC_EFORMAT;
}

extern "C" int mgc_push_bam(mgc_session *s, const void *bam_bytes, size_t len) {
  if (!s || (!bam_bytes && len)) return MGC_EINVAL;
  if (!s->text_open || s->text_format != mgc_session::TEXT_BAM) { set_err(&s->err, "mgc_push_bam without mgc_begin_bam"); return MGC_ESTATE; }
  HIP_TRY(s, hipSetDevice(s->device));
  const char *src = static_cast<const char *>(bam_bytes);
  while (len) {
    const size_t piece = len < mgc_session::TEXT_CHUNK ? len : mgc_session::TEXT_CHUNK;
    const uint32_t b = s->text_next & 1u;
    if (s->text_ev_used[b]) HIP_TRY(s, hipEventSynchronize(s->text_ev[b]));     // pinned + device buffer b are free again
    memcpy(s->text_pinned[b], src, piece);
    const int rc = mgc::bam_submit(s, s->text_pinned[b], piece);
    if (rc == mgc::BAM_REFUSED) return mgc::bam_refuse(s, "mgc_push_bam");
    if (rc != MGC_OK) return rc;
    src += piece;
    len -= piece;
  }
  return MGC_OK;
}

int mgc::bam_end(mgc_session *s, const char *what) {
  if (!s->text_open || s->text_format != mgc_session::TEXT_BAM) { set_err(&s->err, "mgc_end_bam without mgc_begin_bam"); return MGC_ESTATE; }
  HIP_TRY(s, hipSetDevice(s->device));
  if (!s->bam_walker.finish()) return mgc::bam_refuse(s, what);
  s->text_open = false;
  if (s->fill_len >= s->batch_limit) return cut_batch(s);
  return MGC_OK;
}

extern "C" int mgc_end_bam(mgc_session *s) { return s ? mgc::bam_end(s, "mgc_end_bam") : MGC_EINVAL; }

extern "C" int mgc_dev_bam_decode(const uint8_t *d_piece, uint64_t piece_bytes, const void *d_segments, uint64_t n_segments, uint64_t out_bytes,
                                  uint8_t *d_out, void *stream) {
  if ((!d_piece && piece_bytes) || (!d_segments && n_segments) || (!d_out && out_bytes)) return MGC_EINVAL;
  if (piece_bytes > 0xffffffffull) { set_err(nullptr, "mgc_dev_bam_decode: a piece holds less than 4 GiB"); return MGC_EINVAL; }
  HIP_TRY((mgc_session *)nullptr, mgc::launch_bam_decode(d_piece, piece_bytes, d_segments, n_segments, out_bytes, d_out, static_cast<hipStream_t>(stream)));
  return MGC_OK;
}

// ---- gzip input, inflated by several host threads, resolved on the device (mgc_gzip_par.hpp, mgc_gzip.hip) ----------------------
// The open gzip file IS an open text file (mgc_begin_text): its pieces go through the same device input buffers, upload stream and
// parse kernels as text_submit's.  Before the parse kernels read a piece, its unresolved prefix is patched from the window the device
// keeps of the text before it; the CRC-32 of the resolved text comes back two pieces later (or at gzip_finish) and is held against the
// members' trailers then.
static uint32_t *gz_error_word(mgc_session *s) { return reinterpret_cast<uint32_t *>(static_cast<uint8_t *>(s->buf[mgc_session::B_GZ_WIN].p) + 2 * mgc::GZ_WINDOW); }

int mgc::gzip_begin(mgc_session *s) {
  HIP_TRY(s, s->ensure(mgc_session::B_GZ_WIN, 2 * mgc::GZ_WINDOW + 256));
  HIP_TRY(s, hipMemsetAsync(s->buf[mgc_session::B_GZ_WIN].p, 0, 2 * mgc::GZ_WINDOW + 256, s->st_in));
  s->gz_win = 0;
  s->tr_gz_copy = s->tr_gz_collect = s->tr_gz_wait = 0;
  s->gz_crc = 0; s->gz_member_len = 0; s->gz_members = 0;
  s->gz_verdict.clear();
  for (int b = 0; b < 2; b++) { s->gz_pending[b].clear(); s->gz_ends[b].clear(); }
  return MGC_OK;
}

// crc32_combine(crc1, crc2, 4096) without zlib's work: zlib squares a 32 x 32 GF(2) matrix some fifteen times per call (tens of
// microseconds in zlib 1.2), and a 32 MiB piece brings 8192 values.  Nearly every CRC piece is exactly 4096 bytes, so the operator
// "append 4096 zero bytes" is built once -- the one-zero-bit operator squared fifteen times -- and applied in at most 32 steps.
static uint32_t gf2_times(const uint32_t *mat, uint32_t vec) {
  uint32_t sum = 0;
  for (; vec; vec >>= 1, mat++) if (vec & 1u) sum ^= *mat;
  return sum;
}
static uint32_t crc32_combine_4096(uint32_t crc1, uint32_t crc2) {
  static const struct Op {
    uint32_t m[32];
    Op() {
      uint32_t a[32], b[32];
      a[0] = 0xedb88320u;                                    // one zero bit
      for (int n = 1; n < 32; n++) a[n] = 1u << (n - 1);
      for (int sq = 0; sq < 15; sq++) {                      // 2^15 bits = 4096 bytes
        for (int n = 0; n < 32; n++) b[n] = gf2_times(a, a[n]);
        memcpy(a, b, sizeof(a));
      }
      memcpy(m, a, sizeof(m));
    }
  } op;
  return gf2_times(op.m, crc1) ^ crc2;
}

// the CRC values of the piece that went through buffer b have arrived (its text_ev was waited for): fold them into the member's
static void gz_collect(mgc_session *s, uint32_t b) {
  std::vector<mgc_session::GzCrcPiece> &pend = s->gz_pending[b];
  if (pend.empty()) return;
  const double t0 = mgc::now_s();
  const size_t cap = s->gz_tab_cap[b];
  const uint32_t *crc = reinterpret_cast<const uint32_t *>(s->gz_tab_pinned[b] + 12 * cap);
  const uint32_t dev_err = crc[cap];
  if (dev_err && s->gz_verdict.empty()) {
    char msg[200];
    snprintf(msg, sizeof(msg), "%s (in the piece that starts at compressed offset %llu)",
             (dev_err & 2u) ? "a back-reference reaches before the start of its gzip member" : "the inflaters produced an invalid symbol",
             (unsigned long long)s->gz_piece_off[b]);
    s->gz_verdict = msg;
  }
  for (size_t i = 0; i < pend.size(); i++) {
    s->gz_crc = pend[i].len == 4096 ? crc32_combine_4096(s->gz_crc, crc[i]) : (uint32_t)crc32_combine(s->gz_crc, crc[i], (z_off_t)pend[i].len);
    s->gz_member_len += pend[i].len;
    if (pend[i].end < 0) continue;
    const mgc_session::GzEnd &e = s->gz_ends[b][(size_t)pend[i].end];
    if (s->gz_verdict.empty() && (s->gz_crc != e.crc || (uint32_t)s->gz_member_len != e.isize)) {
      char msg[200];
      if (s->gz_crc != e.crc) snprintf(msg, sizeof(msg), "CRC32 mismatch (member %llu, trailer at compressed offset %llu: %08x, text %08x)",
                                       (unsigned long long)s->gz_members, (unsigned long long)e.comp_off, e.crc, s->gz_crc);
      else snprintf(msg, sizeof(msg), "ISIZE mismatch (member %llu, trailer at compressed offset %llu: %u, text %llu bytes)",
                    (unsigned long long)s->gz_members, (unsigned long long)e.comp_off, e.isize, (unsigned long long)s->gz_member_len);
      s->gz_verdict = msg;
    }
    s->gz_crc = 0; s->gz_member_len = 0; s->gz_members++;
  }
  pend.clear();
  s->gz_ends[b].clear();
  s->tr_gz_collect += mgc::now_s() - t0;
}

int mgc::gzip_finish(mgc_session *s) {
  const double t0 = mgc::now_s();
  mgc::text_drain(s);
  s->tr_gz_wait += mgc::now_s() - t0;
  const uint32_t older = s->text_next & 1u;
  gz_collect(s, older);
  gz_collect(s, older ^ 1u);
  return s->gz_verdict.empty() ? MGC_OK : mgc::GZIP_REFUSED;
}

int mgc::gzip_submit(mgc_session *s, const char *pinned_text, size_t piece, const uint16_t *symbols, size_t n_symbols, uint32_t window_valid,
                     const mgc::GzMemberEnd *ends, size_t n_ends, uint64_t comp_off) {
  if (piece == 0) {
    // Nothing for the device (an empty member, the end of the file).  A submit that queues nothing would break the count by which the
    // pump hands slots back (see bam_submit): it waits for both pieces in flight, and the trailers are checked here.
    if (mgc::gzip_finish(s) != MGC_OK) return mgc::GZIP_REFUSED;
    for (size_t i = 0; i < n_ends; i++) {
      if (s->gz_verdict.empty() && (s->gz_crc != ends[i].crc || (uint32_t)s->gz_member_len != ends[i].isize)) {
        char msg[160];
        snprintf(msg, sizeof(msg), "CRC32 / ISIZE mismatch (member %llu, trailer at compressed offset %llu)", (unsigned long long)s->gz_members,
                 (unsigned long long)ends[i].comp_off);
        s->gz_verdict = msg;
      }
      s->gz_crc = 0; s->gz_member_len = 0; s->gz_members++;
    }
    return s->gz_verdict.empty() ? MGC_OK : mgc::GZIP_REFUSED;
  }
  if (piece > mgc_session::TEXT_CHUNK || n_symbols > piece || window_valid > mgc::GZ_WINDOW) { set_err(&s->err, "gzip_submit: a piece out of bounds"); return MGC_EINVAL; }
  const uint32_t b = s->text_next & 1u;
  const double w0 = mgc::now_s();
  if (s->text_ev_used[b]) HIP_TRY(s, hipEventSynchronize(s->text_ev[b]));       // device buffers b (and their previous sources) are free again
  s->tr_gz_wait += mgc::now_s() - w0;
  gz_collect(s, b);
  if (!s->gz_verdict.empty()) return mgc::GZIP_REFUSED;
  s->gz_piece_off[b] = comp_off;
  HIP_TRY(s, s->ensure_preserve(stage_id(s->fill), s->fill_len + piece + 4096, s->fill_len, s->st_in));
  // the CRC table: pieces of at most 4 KiB that never cross a member's end
  std::vector<mgc_session::GzCrcPiece> &pend = s->gz_pending[b];
  const size_t want_tab = piece / 4096 + 2 * n_ends + 2;
  if (s->gz_tab_cap[b] < want_tab) {
    if (s->gz_tab_pinned[b]) { (void)hipHostFree(s->gz_tab_pinned[b]); s->gz_tab_pinned[b] = nullptr; s->gz_tab_cap[b] = 0; }
    const size_t cap = want_tab + want_tab / 2 + 1024;
    HIP_TRY(s, hipHostMalloc(reinterpret_cast<void **>(&s->gz_tab_pinned[b]), cap * 16 + 16, hipHostMallocDefault));
    s->gz_tab_cap[b] = cap;
  }
  const size_t cap = s->gz_tab_cap[b];
  const int tab_buf = b ? mgc_session::B_GZ_TAB1 : mgc_session::B_GZ_TAB0, sym_buf = b ? mgc_session::B_GZ_SYM1 : mgc_session::B_GZ_SYM0;
  HIP_TRY(s, s->ensure(tab_buf, cap * 16 + 16));
  uint64_t *h_begin = reinterpret_cast<uint64_t *>(s->gz_tab_pinned[b]);
  uint32_t *h_len = reinterpret_cast<uint32_t *>(s->gz_tab_pinned[b] + 8 * cap);
  size_t n_tab = 0;
  uint64_t at = 0;
  for (size_t e = 0; e <= n_ends; e++) {
    const uint64_t stop = e < n_ends ? ends[e].text_off : piece;
    if (stop < at || stop > piece) { set_err(&s->err, "gzip_submit: member ends out of order"); return MGC_EINVAL; }
    do {                                                                         // (a member end with no text before it: one piece of 0 bytes)
      const uint32_t l = (uint32_t)std::min<uint64_t>(4096, stop - at);
      if (e == n_ends && l == 0) break;
      h_begin[n_tab] = at; h_len[n_tab] = l;
      at += l;
      pend.push_back({l, (e < n_ends && at == stop) ? (int32_t)s->gz_ends[b].size() : -1});
      n_tab++;
    } while (at < stop);
    if (e < n_ends) s->gz_ends[b].push_back({ends[e].crc, ends[e].isize, ends[e].comp_off});
  }
  if (n_symbols * 2 > s->gz_sym_cap[b]) {
    if (s->gz_sym_pinned[b]) { (void)hipHostFree(s->gz_sym_pinned[b]); s->gz_sym_pinned[b] = nullptr; s->gz_sym_cap[b] = 0; }
    const size_t want = std::min<size_t>(2 * mgc_session::TEXT_CHUNK, n_symbols * 3 + (1u << 20));
    HIP_TRY(s, hipHostMalloc(reinterpret_cast<void **>(&s->gz_sym_pinned[b]), want, hipHostMallocDefault));
    s->gz_sym_cap[b] = want;
  }
  HIP_TRY(s, s->ensure(sym_buf, std::max<size_t>(s->gz_sym_cap[b], 256)));
  const double c0 = mgc::now_s();
  if (n_symbols) memcpy(s->gz_sym_pinned[b], symbols, n_symbols * 2);
  s->tr_gz_copy += mgc::now_s() - c0;
  uint8_t *d_in = reinterpret_cast<uint8_t *>(s->buf[b ? mgc_session::B_TEXT_IN1 : mgc_session::B_TEXT_IN0].p);
  uint8_t *d_tab = static_cast<uint8_t *>(s->buf[tab_buf].p);
  uint8_t *d_win = static_cast<uint8_t *>(s->buf[mgc_session::B_GZ_WIN].p);
  HIP_TRY(s, hipMemcpyAsync(d_in, pinned_text, piece, hipMemcpyHostToDevice, s->st_up));
  if (n_symbols) HIP_TRY(s, hipMemcpyAsync(s->buf[sym_buf].p, s->gz_sym_pinned[b], n_symbols * 2, hipMemcpyHostToDevice, s->st_up));
  HIP_TRY(s, hipMemcpyAsync(d_tab, h_begin, n_tab * 8, hipMemcpyHostToDevice, s->st_up));
  HIP_TRY(s, hipMemcpyAsync(d_tab + 8 * cap, h_len, n_tab * 4, hipMemcpyHostToDevice, s->st_up));
  HIP_TRY(s, hipEventRecord(s->up_ev[b], s->st_up));
  HIP_TRY(s, hipStreamWaitEvent(s->st_in, s->up_ev[b], 0));
  HIP_TRY(s, mgc::launch_gzip_resolve(d_in, piece, static_cast<const uint16_t *>(s->buf[sym_buf].p), n_symbols, d_win + (size_t)s->gz_win * mgc::GZ_WINDOW,
                                      window_valid, d_win + (size_t)(s->gz_win ^ 1) * mgc::GZ_WINDOW, gz_error_word(s), s->st_in));
  s->gz_win ^= 1;
  HIP_TRY(s, mgc::launch_gzip_crc32(d_in, reinterpret_cast<const uint64_t *>(d_tab), reinterpret_cast<const uint32_t *>(d_tab + 8 * cap), n_tab,
                                    reinterpret_cast<uint32_t *>(d_tab + 12 * cap), s->st_in));
  HIP_TRY(s, hipMemcpyAsync(s->gz_tab_pinned[b] + 12 * cap, d_tab + 12 * cap, n_tab * 4, hipMemcpyDeviceToHost, s->st_in));
  HIP_TRY(s, hipMemcpyAsync(s->gz_tab_pinned[b] + 16 * cap, gz_error_word(s), 4, hipMemcpyDeviceToHost, s->st_in));
  HIP_TRY(s, mgc::launch_text_parse(d_in, piece, s->text_format == MGC_TEXT_FASTQ, s->buf[mgc_session::B_TEXT_STATE].p,
                                    s->buf[mgc_session::B_TEXT_WS].p, stage_ptr(s, s->fill), s->st_in));
  HIP_TRY(s, hipEventRecord(s->text_ev[b], s->st_in));
  s->text_ev_used[b] = true;
  s->text_next++;
  s->fill_len += piece;                                     // an upper bound, as in text_submit
  s->len_inexact = true;
  if (s->fill_len >= s->batch_limit) return cut_batch(s);
  return MGC_OK;
}

int mgc::gzip_refuse(mgc_session *s, const char *what, const char *why) {
  const std::string w = why;                                // (why may point into the session's own strings)
  mgc::text_drain(s);
  for (int b = 0; b < 2; b++) { s->gz_pending[b].clear(); s->gz_ends[b].clear(); }
  const int rc = mgc::text_rollback(s);
  if (rc == MGC_EINVAL) set_err(&s->err, "'%s': %s, after part of the file was counted (input larger than one batch)", what, w.c_str());
  if (rc != MGC_OK) return rc;
  set_err(&s->err, "'%s': %s", what, w.c_str());
  return MGC_EFORMAT;
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

extern "C" int mgc_push_bases_device(mgc_session *s, const uint8_t *d_bases, uint64_t n_bases) {
  if (!s || (!d_bases && n_bases)) return MGC_EINVAL;
  if (s->borrowed || s->input_seen || s->counted) { set_err(&s->err, "device input must be the only input"); return MGC_ESTATE; }
  s->d_bases = d_bases;
  s->n_bases = n_bases;
  s->borrowed = true;
  return MGC_OK;
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
static int count_staged_batch(mgc_session *s, int which, uint64_t n) {
  s->d_bases = stage_ptr(s, which);
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
  int rc = MGC_OK;
  if (!s->state_ready) { rc = input_setup(s); if (rc != MGC_OK) return rc; }     // nothing was pushed: an empty stream
  rc = flush_pinned(s);
  if (rc == MGC_OK) rc = resolve_length(s);
  const int wrc = join_worker(s);
  if (rc == MGC_OK) rc = wrc;
  if (rc != MGC_OK) return rc;
  if (!s->have_r) {                                          // everything fits in one pass
    s->d_bases = stage_ptr(s, s->fill);
    s->n_bases = s->fill_len;
    rc = mgc::count_device(s);
    s->prof.n_batches = 1;
  } else {
    if (s->fill_len) rc = count_staged_batch(s, s->fill, s->fill_len);
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
  int rc = MGC_OK;
  if (!s->state_ready) { rc = input_setup(s); if (rc != MGC_OK) return rc; }
  rc = flush_pinned(s);
  if (rc == MGC_OK) rc = resolve_length(s);
  const int wrc = join_worker(s);
  if (rc == MGC_OK) rc = wrc;
  if (rc != MGC_OK) return rc;
  HIP_TRY(s, hipStreamSynchronize(s->st_in));
  *d_bases = stage_ptr(s, s->fill);
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
