// mgc_device.h -- internal launch interface between the host layer (mgc_api / mgc_count / mgc_stream / mgc_eval / mgc_dbfile / mgc_runs / mgc_node .cpp;
// their owning device buffer is mgc_devbuf.hpp's)
// and the gfx950 kernels (mgc_kmer / mgc_sort / mgc_scan / mgc_finish / mgc_misc / mgc_parse / mgc_encode / mgc_decode / mgc_merge
// .hip; mgc_lookup / mgc_filter / mgc_import .hip have headers of their own).  Not installed.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "mgc_label.hpp"
#include "../../include/meryl_gpu_count.h"

namespace mgc {

// ---- switches ----------------------------------------------------------------
// Every MGC_* environment switch of the count path (tests and A/B measurements; the defaults are the shipped plan), read ONCE:
// mgc_open reads them into the session (mgc_session::sw), the bare mgc_dev_* operators per call -- nothing below reads the
// environment on its own.
struct Switches {
  bool fine_hist = true;        // MGC_FINE_HIST=0: no fifteen-bit file histogram (every file's digit histogram by a read of its keys)
  bool hpc_msd = true;          // MGC_HPC_MSD=0: `compress`, low digit first everywhere
  bool hpc_digits = true;       // MGC_HPC_DIGITS=0: `compress` with plain bit digits
  bool const_k = true;          // MGC_KMER_CONST_K=0: the front-end kernels with run-time k only
  bool packed_bases = true;     // MGC_PACKED_BASES=0: the partition decodes the ASCII bases again (no packed base stream)
  bool narrow = true;           // MGC_NARROW=0: no 32-bit words after the first grouping pass
  bool wide_msd = true;         // MGC_WIDE_MSD=0: whole keys low digit first off a histogram read
  bool soa5 = true;             // MGC_SOA5=0: no 5-byte layout (k = 20..23)
  bool group_pipe = true;       // MGC_GROUP_PIPE=0: the narrowed grouping passes fetch the next tile inside the look-back phase (round 5's form)
  bool k96 = true;              // MGC_K96=0: no 12-byte records (k = 33..51)
  bool finish = true;           // MGC_FINISH=0: stable sort of all bits + run-length kernels
  bool nolist = false;          // MGC_FINISH_NOLIST=1: the dense-grid instantiations of the count kernels whatever the grid holds
  bool finish_trace = false;    // MGC_FINISH_TRACE: what happens to oversized sub-buckets, on stderr
  bool group_dbg = false;       // MGC_GROUP_DBG: per-phase cycle sums of the grouping passes (instrumented instantiations)
  uint32_t pass_stagger = 0;    // MGC_PASS_STAGGER: groups the 5-byte first pass's workgroups start in (0 / 1: together -- the default: the
                                // staggered start hands the first tiles out statically, which is only safe while ALL workgroups of the launch are
                                // resident, i.e. while nothing else holds CUs of the device; mgc_sort.hip, STAGGER)
  bool hash_dbg = false;        // MGC_HASH_DBG: per-phase cycle sums of the count kernels
  int  hash_multi = -1;         // MGC_HASH_MULTI: sub-buckets per iteration of hash_count_multi_kernel (-1: by the file's average; 0: off)
  int  hash_stream = -1;        // MGC_HASH_STREAM: the distinct-sized count (hash_count_stream_kernel) and its coarser file plan (-1: where the probe
                                // file's distinct / instances ratio allows it; 0: off; 1: on every file whose suffix fits, whatever the ratio)
                                // 2: like -1, but only on narrowed files -- not on whole 8-byte k-mers (k = 24..32: the 64-bit-entry instantiation))
  uint32_t min_top = 0;         // MGC_FINISH_MIN_TOP: at least that many grouping bits per file (tests reach the large-input plans)
  uint64_t finish_target = 0;   // MGC_FINISH_TARGET: k-mers per sub-bucket the plan aims at (0: the kernels' default)
  uint64_t stream_max = (uint64_t)1 << 22;   // MGC_STREAM_MAX: sub-buckets up to this many keys are streamed without asking the probe
  bool     huge_slices = true;  // MGC_HUGE_SLICES=0: a gigantic sub-bucket (above 65536 keys) is streamed by ONE workgroup (round 5)
  uint32_t huge_streams = 4;    // MGC_HUGE_STREAMS: streams the streaming kernels of oversized sub-buckets are spread over (1..4)
  uint64_t bucket_bases = 0;    // MGC_BUCKET_BASES: bases per partition bucket above which the partition gets finer (0: default)
  uint64_t group_batch_bytes = (uint64_t)1 << 40;   // MGC_GROUP_BATCH_BYTES: bytes of the pass buffer Y the narrowed files of ONE batched grouping
                                // launch may fill with their 4-byte words (mgc_group_batch.hpp; below two files' words: one launch per file and pass).
                                // The default holds every file (35 GB at 10 Gbp; measured against 8 GiB and one file: profiles/group_batch_ab.txt);
                                // where the arena cannot grow to it the count halves it, down to single files
  uint32_t group_batch_files = 0;   // MGC_GROUP_BATCH_FILES: at most that many files per batched launch (0: as many as the budget holds; tests)
  bool     pack_overlap = true; // MGC_PACK_OVERLAP=0: every file is packed behind the last count kernel (no early packing, mgc_pack_plan.hpp)
  int64_t  pack_margin = 64;    // MGC_PACK_MARGIN: thousandths added to the estimate of the distinct k-mers the result is sized by before the
                                // total is known (mgc_pack_plan.hpp, PACK_MARGIN_PERMILLE; tests: negative, the estimate falls short)
  uint32_t pack_ratio = 0;      // MGC_PACK_RATIO: thousandths; stands in for the probe file's distinct / instances ratio in that estimate where a
                                // count has no probe file (tests: inputs too small for one; 0: no estimate without a probe)
};
Switches read_switches();        // (mgc_api.cpp)



// ---- k-mer extraction / partition (mgc_kmer.hip) -----------------------
constexpr int      KP_BLOCK       = 256;                 // threads per workgroup
constexpr int      KP_ITEMS       = 16;                  // window starts per thread
constexpr int      KP_TILE        = KP_BLOCK * KP_ITEMS; // 4096 starts per tile
constexpr int      KP_MAX_BUCKETS = 1024;

// Persistent grid size used by both passes (they must agree).
uint32_t kp_grid_size(uint64_t n_bases, uint32_t bucket_bits);   // rows of the per-workgroup histogram (virtual workgroups)
size_t   kp_workspace_bytes(uint32_t bucket_bits);
// The packed base stream of a count (mgc_kmer.hip, PackedBases): d_packed[kp_packed_bytes(n_bases)], about 0.375 bytes per base.
// A histogram launch that gets it stores the 2-bit codes and invalid-base masks of the whole input there, and the partition
// launch of the SAME d_bases / n_bases that gets it reads them instead of the ASCII bases.  nullptr (the bare operators): ASCII.
size_t   kp_packed_bytes(uint64_t n_bases);

// sfx_mask / sfx_test: count-suffix= filter, a k-mer is kept iff (its low word & sfx_mask) == sfx_test (0, 0: keep all)
// the same + the k-mers per (file, next nine bits) into d_fine_hist[2^15] (the first digit of the narrowed grouping passes)
bool       kmer_histogram_fine_ok(uint32_t k, uint32_t bucket_bits, uint64_t sfx_mask, const Switches &sw);
// `compress`: the same histogram over dense ranks -- k-mers per (bucket, dense-rank digit of the five bases below the bucket's),
// d_fine_hist[kmer_histogram_hpc_entries(bucket_bits)], bucket_bits 6 or 8 (mgc_kmer.hip)
bool       kmer_histogram_hpc_ok(uint32_t k, uint32_t bucket_bits, uint64_t sfx_mask, const Switches &sw);
uint32_t   kmer_histogram_hpc_entries(uint32_t bucket_bits);
hipError_t launch_kmer_histogram_hpc(const uint8_t *d_bases, uint64_t n_bases, uint32_t k, int mode, uint32_t bucket_bits,
                                     uint64_t *d_bucket_counts, uint64_t *d_fine_hist, void *d_ws, hipStream_t st, bool const_k = true /*Switches::const_k*/,
                                     void *d_packed = nullptr);
hipError_t launch_kmer_histogram_fine(const uint8_t *d_bases, uint64_t n_bases, uint32_t k, int mode, uint64_t *d_bucket_counts,
                                      uint64_t *d_fine_hist, void *d_ws, hipStream_t st, bool const_k = true /*Switches::const_k*/,
                                      uint32_t bucket_bits = 6 /*6..8: d_bucket_counts[2^bucket_bits] and the per-workgroup rows the partition
                                      takes its cursors from go by that many top bits (a sharded count's senders); d_fine_hist stays 2^15*/,
                                      void *d_packed = nullptr);
bool       kmer_histogram_fine_bits_ok(uint32_t k, uint32_t bucket_bits);
hipError_t launch_kmer_histogram(const uint8_t *d_bases, uint64_t n_bases, uint32_t k, int mode,
                                 uint32_t bucket_bits, uint64_t *d_bucket_counts, void *d_ws, hipStream_t st,
                                 uint64_t sfx_mask = 0, uint64_t sfx_test = 0, void *d_packed = nullptr);
// keys are uint64 for k <= 32, 16-byte little-endian {lo,hi} for k in 33..64 (key_words 1 / 2)
hipError_t launch_kmer_partition(const uint8_t *d_bases, uint64_t n_bases, uint32_t k, int mode,
                                 uint32_t bucket_bits, const uint64_t *d_bucket_starts, void *d_keys,
                                 void *d_ws, hipStream_t st, uint64_t sfx_mask = 0, uint64_t sfx_test = 0,
                                 const uint64_t *d_soa_counts = nullptr /*64 buckets, 8-byte keys, <= 40 bits below the file: a file's region =
                                 u32[count] low words + u8[count] bits 32..39 (5 bytes per k-mer; GroupKeys::SOA5)*/,
                                 bool const_k = true /*Switches::const_k*/, void *d_packed = nullptr);

// ---- radix sort ------------------------------------------------------------
struct SortPlan {
  uint32_t radix_bits;      // digit width (9)
  uint32_t block;           // threads per workgroup (1024)
  uint32_t kpt;             // keys per thread (16; 16-byte keys: 8)
  uint32_t tile;            // block*kpt
  uint32_t mode;            // 0 = stable sort (decoupled look-back), 3 = grouping passes (not a sort: see radix_group_kernel; at most two digits)
  uint32_t hpc;             // 1: digits are DENSE RANKS of five homopolymer-free bases (make_hpc_group_plan), not bit fields; 2: only the high digit is
  uint32_t num_passes;
  uint32_t pass_shift[16];
  uint32_t pass_bits[16];
};

// Chooses digit widths for bits [begin_bit, end_bit); mode 0 (the caller sets 3 for grouping passes).
void   make_sort_plan(uint32_t begin_bit, uint32_t end_bit, SortPlan *plan);
// Grouping plan for homopolymer-compressed k-mers (`compress`): no base equals the one before it, so five bases after a
// known base take 3^5 = 243 of their 1024 bit patterns.  A digit is the dense, ORDER-PRESERVING rank of five bases given
// the base before them (10 key bits -> 0..242): `passes` (1 or 2) digits cover the 10*passes key bits above `low_bit`
// (which must be a whole number of bases above bit 0, with one more base above the top digit).  Grouping by these
// digits orders the keys exactly as grouping by the bits would, over 3^(5*passes) occupied sub-buckets instead of a
// 4^(5*passes) grid that is 94 % empty -- two digits do what took three stable passes.
void   make_hpc_group_plan(uint32_t low_bit, uint32_t passes, SortPlan *plan);
// ... and the two-digit form whose LOW digit is the plain eight bits of four bases (81 of 256 patterns): 18 key bits above `low_bit`,
// 3^9 = 19683 occupied sub-buckets of a 2^18 grid (SortPlan::hpc == 2)
void   make_hpc_mixed_plan(uint32_t low_bit, SortPlan *plan);
size_t sort_workspace_bytes(uint64_t n);

// Sorts n keys; returns where the result is via *result_in_alt.  d_error is a
// device uint32 the kernels set on a look-back timeout (checked by the caller).
hipError_t launch_radix_sort(void *d_keys, void *d_alt, uint64_t n, uint32_t key_words, const SortPlan &plan,
                             void *d_ws, size_t ws_bytes, uint32_t *d_error, int *result_in_alt,
                             hipStream_t st, hipEvent_t *pass_events /* 2 per pass or null */);
size_t     sort_header_bytes();
// ---- the two grouping passes of one file, boundaries included (mgc_sort.hip; which kernel a pass runs: mgc_group_route.hpp) ----
enum class GroupKeys : uint32_t {
  U64,                          // 8-byte keys
  SOA5,                         // the 5-byte layout of launch_kmer_partition(d_soa_counts): u32[n] low words, then u8[n] bits 32..39 (narrowed files only)
  K128,                         // 16-byte keys
  K96,                          // 12-byte K96 records (launch_kmer_partition(d_soa_counts) at k = 33..51; whole-key files only)
};
// One file's grouping launch: what launch_group_narrow and launch_group_wide take.
//
// launch_group_narrow -- two grouping passes with NARROWED keys: uint64 keys whose bits above the first digit fit 32 bits leave the
// first pass as uint32 words without that digit (its value is where the key lies), the second pass and the finish move half the
// bytes, and the sub-bucket boundaries fall out of the second pass's look-back granules.  keys: uint64[n] (or the 5-byte layout)
// in, uint32[n] out (over its first half); alt: room for n uint32; d_sub_starts: 2^(pass_bits[0] + pass_bits[1]) + 1 entries.
// The high-digit-first form (files of a session with the fifteen-bit file histogram): launch_narrow_prepare fills one
// header per file (nb <= 64, sort_header_bytes() apart) from d_fine; every file then gets its header (prepared) and a scratch area
// of narrow_scratch_bytes(n) that the caller has zeroed.  See mgc_sort.hip: nobody reads the
// keys for a digit histogram, and the sub-buckets come out in the order tr_index(., tr_a, tr_b) describes.
// prepared / scratch == nullptr: low digit first off one histogram read, scratch in ws, sub-buckets in key order.
//
// launch_group_wide -- the same high-digit-first form for WHOLE keys (8-byte keys that leave more than 32 bits below their first
// digit: k = 27..32 at the 10 Gbp scale; every 16-byte key): the high digit's histogram comes from the fifteen-bit file histogram
// (launch_narrow_prepare), the first pass counts the low digit as it goes, the boundaries fall out of the second pass's
// look-back granules -- neither the 8/16 B per k-mer digit-histogram read nor the boundary search over the grouped keys
// happens.  keys: n keys in, the grouped keys out (same place); alt: room for n keys; scratch: wide_scratch_bytes(n,
// key_words), zeroed by the caller; sub-buckets in tr_index(., tr_a, tr_b) order.
// `compress`: the plan's digits are dense ranks (make_hpc_group_plan, two digits); the headers then come from
// launch_hpc_prepare (the histogram of launch_kmer_histogram_hpc; `on`: one bit per bucket, nb <= 256)
struct GroupFile {
  void *keys = nullptr, *alt = nullptr;
  uint64_t n = 0;
  const SortPlan *plan = nullptr;
  GroupKeys layout = GroupKeys::U64;
  uint32_t soa_hi_mask = 0;                   // SOA5: the mask of the u8 array's payload bits (bits 32.. of the k-mer below the file)
  uint32_t *d_error = nullptr;                // the count's look-back time-out flag
  uint64_t *d_sub_starts = nullptr;           // out: the sub-bucket boundaries, in PHYSICAL order
  hipStream_t st = nullptr;
  hipEvent_t *pass_events = nullptr;          // 4 or null
  void *prepared = nullptr, *scratch = nullptr;   // high digit first: this file's header and its look-back scratch
  void *ws = nullptr; size_t ws_bytes = 0;    // narrowed files: the shared sort workspace (sort_workspace_bytes(n)), used low digit first
  bool pipe = false;                          // Switches::group_pipe: the fetch a whole tile ahead (the 5-byte first pass)
  uint32_t stagger = 0;                       // Switches::pass_stagger: the 5-byte first pass's workgroups start in that many groups, a tile's time shared between them
  bool dbg = false;                           // narrowed files, high digit first: the instrumented instantiations, their cycle sums on stderr
  uint32_t tr_a = 0, tr_b = 0;                // out: sub-bucket p holds the k-mers whose top bits are tr_index(p, tr_a, tr_b) (tr_a = 0: p itself)
};
bool       sort_plan_narrows(const SortPlan &plan, uint64_t n, uint32_t key_words, bool on = true /*Switches::narrow*/);
size_t     narrow_scratch_bytes(uint64_t n);
hipError_t launch_narrow_prepare(const uint64_t *d_fine, uint32_t nb, const unsigned char *bits_a, const unsigned char *on, void *d_hdrs,
                                 hipStream_t st);
hipError_t launch_group_narrow(GroupFile &f);
// launch_group_narrow_batch -- the same two passes for SEVERAL narrowed files with ONE launch per pass (and one per helper step): the
// tiles of all files in one ticket sequence, so that the tail of one file's tiles runs beside the head of the next file's.  Only the
// judged form (mgc_group_route.hpp, group_batch_form: high digit first off the 5-byte layout, fetched a tile ahead) and only files
// whose plans have the same digits; every file as launch_group_narrow takes it, each with an `alt` of its own (n uint32).
// d_table / h_table: group_batch_table_bytes(nfiles) on the device and on the host -- the host copy has to live until the stream has
// passed the launch; d_ctl: four zeroed 32-bit words on the device (the passes' tickets, the helper step's arrival counter).
struct GroupBatch {
  GroupFile *files = nullptr; uint32_t nfiles = 0;
  void *d_table = nullptr, *h_table = nullptr;
  uint32_t *d_ctl = nullptr;
  uint32_t *d_error = nullptr;
  hipStream_t st = nullptr;
  hipEvent_t *pass_events = nullptr;          // 4 or null: around each pass's launch
};
size_t     group_batch_table_bytes(uint32_t nfiles);
hipError_t launch_group_narrow_batch(GroupBatch &b);
bool       sort_plan_wide_msd(const SortPlan &plan, uint64_t n, bool on = true /*Switches::wide_msd*/);
hipError_t launch_hpc_prepare(const uint64_t *d_fine_hpc, uint32_t bucket_bits, const uint64_t on[4], void *d_hdrs, hipStream_t st);
size_t     wide_scratch_bytes(uint64_t n, uint32_t key_words);
hipError_t launch_group_wide(GroupFile &f);

// ---- run-length count ------------------------------------------------------
size_t     rle_workspace_bytes(uint64_t n);
hipError_t launch_rle_count(const void *d_sorted, uint64_t n, uint32_t key_words, void *d_ws, hipStream_t st);
// after launch_rle_count + stream sync: number of distinct keys sits at ws[0]
hipError_t rle_read_total(const void *d_ws, uint64_t *n_distinct, hipStream_t st);
// d_out_base (device, optional): offset added to every output slot
hipError_t launch_rle_emit(const void *d_sorted, uint64_t n, uint32_t key_words, void *d_ws, void *d_unique,
                           uint32_t *d_counts, hipStream_t st, const uint64_t *d_out_base = nullptr);

// ---- sub-bucket finish (LDS sort of the low bits + fused run-length count) ---------------
uint64_t   finish_capacity_for(uint32_t key_words);     // largest sub-bucket the LDS kernels accept
uint64_t   finish_target_for(uint32_t key_words, const Switches &sw);       // average sub-bucket size to aim for
// The distinct-sized count (hash_count_stream_kernel, round 6): narrowed files whose suffix fits its packed entry take sub-buckets of
// up to finish_stream_capacity() keys (twice the others' average); its table holds finish_stream_distinct() distinct suffixes, a
// sub-bucket with more goes on the retry list (launch_finish_retry).
// Whole 8-byte k-mers on the high-digit-first passes (k = 24..32, `compress`; narrow = false) take the same kernel with 64-bit entries
// (suffixes of up to 52 bits); their retry list goes through the streaming kernel of the oversized sub-buckets.
bool       finish_stream_ok(uint32_t key_words, uint32_t low_bits, bool narrow = true);
uint64_t   finish_stream_capacity();
uint64_t   finish_stream_target(const Switches &sw);
uint64_t   finish_stream_distinct();
hipError_t launch_subbucket_bounds(const void *d_keys, uint64_t n, uint32_t key_words, uint32_t low, uint32_t top_bits,
                                   uint64_t *d_starts /*[2^top+1]*/, uint64_t *d_max /*atomicMax target*/,
                                   uint32_t *d_large_list /*[2^top]: sub-buckets above the small-kernel capacity*/,
                                   uint64_t *d_large_count /*zeroed by the caller*/,
                                   uint32_t *d_nonempty_list /*[2^top]*/, uint64_t *d_nonempty_count /*zeroed by the caller*/,
                                   hipStream_t st);
hipError_t launch_subbucket_max(const uint64_t *d_starts, uint32_t key_words, uint32_t low, uint32_t top_bits, uint64_t *d_max,
                                uint32_t *d_large_list, uint64_t *d_large_count, uint32_t *d_nonempty_list, uint64_t *d_nonempty_count,
                                hipStream_t st, uint64_t small_cap = 0 /*0: the capacity of the kernels (key_words, low) selects*/);
                                // the list half of launch_subbucket_bounds (boundaries already known)
// which files the hash-count kernels take (the others: the LDS sort); their sub-buckets above finish_capacity_for() can be streamed
// through the hash-count tables (the distinct suffixes fit)
bool       finish_uses_hash(uint32_t key_words, uint32_t low_bits);
// what a file's keys are when its sub-buckets are counted
enum class FinishKeys : uint32_t {
  WHOLE8,                       // whole 8-byte k-mers
  NARROW32,                     // uint32 narrowed keys (launch_group_narrow); the distinct SUFFIXES go back in place
  K96,                          // 12-byte K96 records (k = 33..51); oversized sub-buckets only with `stream`
  WHOLE16,                      // whole 16-byte k-mers
};
// One file's count launch: what launch_finish_probe / launch_finish_file / launch_finish_retry share.
// Path counters of the gigantic sub-buckets (mgc_finish.hip, HugeSliced::stats): FIN_HUGE_STATS words of the count's flag block, from
// word FIN_HUGE_STATS_AT on -- [0] sub-buckets cut, [1] slices planned, [2] sub-buckets marked dense, [3 + MODE] passes of MODE 0 / 1 / 2 / 3
// that overflowed their table and were run again over a narrower range, [7] empty ranges of MODE 3.  Zeroed with the flags when a
// count begins, added to on the device, read back by the count only when it is profiled.
constexpr uint32_t FIN_HUGE_STATS_AT = 16, FIN_HUGE_STATS = 8;
struct FinishFile {
  void *keys = nullptr;                      // the file's segment; distinct keys are written in place
  void *alt = nullptr;                        // room for the file's keys (the streaming kernels' second buffer)
  FinishKeys layout = FinishKeys::WHOLE8;
  const uint64_t *starts = nullptr;           // [ng + 1] sub-bucket boundaries
  uint64_t ng = 0;
  uint32_t low_bits = 0;                      // bits below the sub-bucket (the suffix)
  uint32_t tr_a = 0, tr_b = 0;                // launch_group_narrow's / launch_group_wide's (whole keys: hash paths only)
  uint64_t n_keys = 0;                        // keys of the file, if known: the narrowed hash-count takes several sub-buckets per iteration by their average
  uint64_t max_sub = 0;                       // the file's largest sub-bucket, if known: small files take smaller tables
  uint32_t *cnt_tmp = nullptr;
  uint64_t *group_distinct = nullptr;
  const uint32_t *large_list = nullptr;       // the oversized list: sub-buckets above the small-kernel capacity
  uint64_t n_large = 0;
  bool stream = false;                        // large list -> streaming hash-count (otherwise the LDS sort's 8192-key instantiation)
  const uint32_t *nonempty_list = nullptr;    // the hash kernels visit only these; group_distinct must be zero for the others
  const uint64_t *nonempty_count = nullptr;
  uint32_t *retry_list = nullptr;             // [ng] + a zeroed counter: with both, dense narrowed files take hash_count_multi_kernel
  uint64_t *retry_count = nullptr;
  uint64_t stream_cap = 0;                    // nonzero (dense files, finish_stream_ok): hash_count_stream_kernel counts the sub-buckets of up
                                              // to that many keys; the ones with too many distinct suffixes go on retry_list
  // finish_huge_workspace_bytes(huge_ws_keys >= n_keys), one per stream the streaming kernels run on: with it a GIGANTIC sub-bucket --
  // above 65536 keys -- is counted in slices by many workgroups instead of one
  void *huge_ws = nullptr; size_t huge_ws_bytes = 0; uint64_t huge_ws_keys = 0;
  uint32_t *d_error = nullptr;                // the count's look-back / chain time-out flag; d_error[FIN_HUGE_STATS_AT ...]: the path counters below
  hipStream_t st = nullptr;                  // where the persistent kernels are launched
  hipStream_t st_huge = nullptr;              // where the streaming kernel of the oversized list is launched (st, or a stream forked from it)
  int  hash_multi = -1;                       // Switches::hash_multi
  bool hash_dbg = false;                      // Switches::hash_dbg
};
// would every listed sub-bucket above stream_max keys fit the streaming tables?  *d_file_fail is set to 1 if not
hipError_t launch_finish_probe(const FinishFile &f, uint64_t stream_max /*Switches::stream_max*/, uint32_t *d_file_fail);
hipError_t launch_finish_file(const FinishFile &f);
// the sub-buckets hash_count_stream_kernel put on the retry list (their number is on the device: the caller brings it back first)
hipError_t launch_finish_retry(const FinishFile &f, uint64_t n_retry);
size_t     finish_huge_workspace_bytes(uint64_t n_keys);
// what the last sliced count left in a workspace (diagnostics): sub-buckets cut, their slices, the cut ones counted by ranges
struct HugeTrace { uint32_t cut, slices, dense; };
hipError_t finish_huge_trace(const void *d_ws, uint64_t ws_keys, HugeTrace *out);
size_t     finish_scan_scratch_bytes(uint64_t ng_total);
hipError_t launch_finish_scan(uint64_t *d_group /*[ng_total+1]*/, uint64_t ng_total, void *d_scratch, hipStream_t st);
hipError_t launch_compact_groups(const void *d_keys, uint32_t key_words, const uint32_t *d_cnt_tmp, const uint64_t *d_starts,
                                 const uint64_t *d_offs, uint64_t ng, void *d_out_keys, uint32_t *d_out_counts, hipStream_t st,
                                 uint32_t tr_a = 0, uint32_t tr_b = 0 /*launch_group_wide's: d_offs goes by tr_index(sub-bucket)*/,
                                 const uint32_t *d_nonempty_list = nullptr, uint64_t n_nonempty = 0 /*visit only these (host count)*/,
                                 const uint64_t *d_gate = nullptr, uint64_t gate_above = 0 /*early packing: the launch does nothing unless
                                 *d_gate > gate_above (launch_pack_gate_scan's state[0]); nullptr: no gate*/);
// narrowed files: k-mer = base | sub-bucket << low_bits | suffix
hipError_t launch_compact_groups_narrow(const void *d_keys32, const uint32_t *d_cnt_tmp, const uint64_t *d_starts, const uint64_t *d_offs,
                                        uint64_t ng, uint64_t base, uint32_t low_bits, void *d_out_keys, uint32_t *d_out_counts, hipStream_t st,
                                        uint32_t tr_a, uint32_t tr_b, const uint32_t *d_nonempty_list = nullptr, uint64_t n_nonempty = 0,
                                        const uint64_t *d_gate = nullptr, uint64_t gate_above = 0);
// K96 records (k = 33..51: the bits below the file, 12 bytes) -> whole 16-byte k-mers; base_lo / base_hi: the file's bits in their place
hipError_t launch_compact_groups_k96(const void *d_keys96, const uint32_t *d_cnt_tmp, const uint64_t *d_starts, const uint64_t *d_offs,
                                     uint64_t ng, uint64_t base_lo, uint64_t base_hi, void *d_out_keys, uint32_t *d_out_counts, hipStream_t st,
                                     uint32_t tr_a, uint32_t tr_b, const uint32_t *d_nonempty_list = nullptr, uint64_t n_nonempty = 0,
                                     const uint64_t *d_gate = nullptr, uint64_t gate_above = 0);
// Early packing: the files of a count are packed in index order on another stream while later files are still counted.
// d_state[pack_state_bytes(m, the longest slice) / 8] for a chain of m files: [0] the first deferred file (pack_state_none(): none), [1]
// the k-mers the result has room for, [3 + i] the distinct k-mers before file i.  launch_pack_gate_scan, file i of m: unless the gate defers it (an earlier
// file deferred; *d_retry_count != 0 -- nullptr: not asked; no room for its k-mers), its slice d_slice[n] of group_distinct becomes
// the exclusive offsets the scan of ALL files would leave there, [3 + i + 1] is written and, with d_total, *d_total as well.
// force: no gate (the serial path from the first deferred file on).
size_t     pack_state_bytes(uint32_t n_files, uint64_t max_slice);
uint64_t   pack_state_none();
hipError_t launch_pack_state_init(uint64_t *d_state, uint64_t capacity, hipStream_t st);
hipError_t launch_pack_gate_scan(uint64_t *d_slice, uint64_t n, uint64_t *d_state, uint32_t n_files, uint32_t i, const uint64_t *d_retry_count,
                                 uint64_t *d_total, bool force, hipStream_t st);
hipError_t launch_widen_k96(const void *d_keys96, uint64_t n, uint64_t base_lo, uint64_t base_hi, void *d_out128, hipStream_t st);
hipError_t launch_widen_groups(const void *d_keys32, const uint64_t *d_starts, uint64_t ng, uint64_t base, uint32_t low_bits, void *d_out64,
                               hipStream_t st, uint32_t tr_a, uint32_t tr_b);      // tr_a != 0: the result is NOT in key order
hipError_t launch_store_u64(uint64_t *d_dst, const uint64_t *d_src, hipStream_t st);
hipError_t launch_sum_u64(const uint64_t *d_in, uint64_t n, uint64_t *d_out, hipStream_t st);    // *d_out <- sum of d_in[0, n)

hipError_t launch_block_offsets(const void *d_unique, uint64_t n_distinct, uint32_t key_words, uint32_t w_data,
                                uint64_t n_prefix, uint64_t *d_block_start, hipStream_t st);

// ---- database blocks encoded on the device (mgc_encode.hip; layout: mdb_layout.h) -------------------------------
// rel_start[i] = first key >= (prefix_begin + i) << w_data for i in [0, n_blocks] (n_prefix_total = 2^wPrefix)
hipError_t launch_block_offsets_range(const void *d_keys, uint64_t n, uint32_t key_words, uint32_t w_data, uint64_t prefix_begin,
                                      uint64_t n_blocks, uint64_t n_prefix_total, uint64_t *d_rel_start, hipStream_t st);
hipError_t launch_encode_sizes(const void *d_keys, uint32_t key_words, const uint64_t *d_bs, uint64_t n_blocks, uint32_t suffix_size,
                               uint32_t label_size, uint64_t *d_blk_bytes, uint64_t *d_blk_vbase, uint32_t *d_blk_bb, hipStream_t st);
hipError_t launch_encode_chunk(const void *d_keys, const uint32_t *d_counts, uint32_t key_words, const uint64_t *d_bs,
                               const uint64_t *d_blk_pos, const uint64_t *d_blk_vbase, const uint32_t *d_blk_bb,
                               uint64_t b0, uint64_t b1, uint64_t n_kmers_chunk, uint64_t prefix_of_block0,
                               uint32_t suffix_size, uint32_t label_size, uint64_t label, void *d_img, hipStream_t st,
                               const uint64_t *d_labels = nullptr /*per k-mer, beside d_counts; null: the constant `label`*/);

// ---- database blocks decoded on the device (mgc_decode.hip): d_file = the data file's bytes (+ 16 bytes of slack),
// d_blocks = mdb_raw_block[n_blocks] (include/meryl_db.h, mdb_reader_raw_file); one thread per block; *d_err != 0: a corrupt block
hipError_t launch_decode_blocks(const void *d_file, const void *d_blocks, uint64_t n_blocks, uint32_t suffix_size, uint32_t label_size,
                                uint32_t key_words, void *d_keys, uint32_t *d_counts, uint32_t *d_err, hipStream_t st,
                                uint64_t *d_labels = nullptr /*the labels beside d_counts (zeros when label_size is 0); null: skipped*/);

// ---- merge of two sorted distinct (k-mer, value) streams (mgc_merge.hip) ----------------------------------------
// op: 0 union-sum, 1 union-min, 2 union-max, 3 intersect-sum, 4 intersect-min, 5 intersect-max
size_t     merge_workspace_bytes(uint64_t na, uint64_t nb);
//     6 intersect (first input's value), 7 subtract, 8 difference, 9 symmetric-difference (mgc_merge.hip)
// cA / cB: the values -- needed by the count pass only when what is written depends on them (op 7)
hipError_t launch_merge_count(const void *dA, uint64_t na, const void *dB, uint64_t nb, uint32_t key_words, int op, void *d_ws,
                              hipStream_t st, const uint32_t *cA = nullptr, const uint32_t *cB = nullptr);
hipError_t merge_read_total(const void *d_ws, uint64_t *n_out, hipStream_t st);       // synchronises the stream
hipError_t launch_merge_emit(const void *dA, const uint32_t *cA, uint64_t na, const void *dB, const uint32_t *cB, uint64_t nb,
                             uint32_t key_words, int op, void *d_ws, void *d_out_keys, uint32_t *d_out_counts, hipStream_t st);
// ---- one description of what a count / emit pass pair does beyond its operation (mgc_merge_many.hip, mgc_merge.hip) ----------
// The same rule goes to both passes (out_labs may be set in between, once the output length is known); the launcher picks the
// kernel instantiation from it (pass_inst, mgc_route.hpp) so that the count pass decides exactly what the emit pass writes.
struct PassRule {
  int       lop = 0;                       // label operation, a kernel code (label_kernel_op, mgc_label.hpp): read with a program or out_labs
  uint64_t  lc = 0;                        //   and its constant
  bool      select = false;                // a selector program (mgc_selector.hpp), possibly empty, is ANDed onto the operation's rule
  const ::mgc_select_term *terms = nullptr;  // checked by the caller (select_check)
  uint32_t  n_terms = 0, k = 0;            //   k: the k-mer size (BASES terms)
  int       vop = 0;                       // merge_many: value assignment, a kernel code (value_kernel_op, mgc_value.hpp; 0: VOP_NONE, the
  uint64_t  vc = 0;                        //   operation's own value); its constant.  An assignment implies `select`.
  int       fop = -1;                      // merge_many, with an assignment: the value filter of a filter node tested on the assigned
  uint64_t  fc = 0;                        //   value (fop < 0: none); its threshold
  uint64_t *out_labs = nullptr;            // emit: where the labels of the written k-mers go (null: none are written)
};
// ---- merge of 1..32 sorted distinct (k-mer, value) streams in one pass pair (mgc_merge_many.hip) ----------------
// op as above, and 10 union (the value is the number of inputs holding the k-mer); keys / vals / labs / n: host arrays of device
// pointers and lengths (labs, or an entry of it, null: all zeros); without a rule equal to the left fold of the two-input merge over
// the same inputs, element by element.  count (emit false) -> merge_read_total -> emit, like the two-input merge.
struct MergeManyInputs { const void *const *keys; const uint32_t *const *vals; const uint64_t *const *labs; const uint64_t *n; uint32_t count, key_words; };
uint32_t   merge_many_tile(uint32_t key_words);
size_t     merge_many_workspace_bytes(const uint64_t *n, uint32_t n_inputs, uint32_t key_words);
hipError_t launch_merge_many(bool emit, const MergeManyInputs &in, int op, const PassRule &rule, void *d_ws, void *d_out_keys,
                             uint32_t *d_out_vals, hipStream_t st);
// one stream through a value transform (fop 0..5 filters against `constant`: less-than, greater-than, at-least, at-most, equal-to,
// not-equal-to; 6..11 arithmetic: increase, decrease, multiply, divide, divide-round, modulo; 12: keep where flags[i] == 1, without
// a program or labels only), k-mers whose new value is 0 dropped; the same two passes.  labs null: all zeros.
struct SelectInput { const void *keys; const uint32_t *vals; const uint32_t *flags; const uint64_t *labs; uint64_t n; uint32_t key_words; };
size_t     select_workspace_bytes(uint64_t n);
hipError_t launch_select(bool emit, const SelectInput &in, int fop, uint64_t constant, const PassRule &rule, void *d_ws, void *d_out_keys,
                         uint32_t *d_out_vals, hipStream_t st);
hipError_t launch_fill_u32(uint32_t *d, uint64_t n, uint32_t v, hipStream_t st);
// *d_out <- 1 + index of the last '.' in bases[0, n), 0 if none
hipError_t launch_last_breaker(const uint8_t *d_bases, uint64_t n, uint64_t *d_out, hipStream_t st);

// ---- homopolymer compression -------------------------------------------------
size_t     hpc_workspace_bytes(uint64_t n);
// compressed length lands in the first uint64 of the workspace
hipError_t launch_homopoly_compress(const uint8_t *d_in, uint64_t n, uint8_t *d_out, void *d_ws, hipStream_t st);

// ---- FASTA / FASTQ / SAM text -> base stream (mgc_parse.hip) ----------------------------------
size_t     text_parse_state_bytes();
size_t     text_parse_workspace_bytes(uint64_t n);            // for one chunk of n text bytes
// appends the bases of one text chunk to d_out at the running length kept in d_state; format: MGC_TEXT_FASTA / _FASTQ / _SAM
hipError_t launch_text_parse(const uint8_t *d_text, uint64_t n, int format, void *d_state, void *d_ws, uint8_t *d_out, hipStream_t st);
// ---- BAM records -> base stream (mgc_bam.hip) ----
// One piece of an inflated BAM stream (piece_bytes at d_piece) and the segments the host walker made of it (n_segments of 16
// bytes, mgc::BamSegment of mgc_bam_walk.hpp, tiling [0, out_total)): writes out_total bytes at d_out (any alignment) -- the SEQ
// fields through the nt16 alphabet, '.' after the flagged segments.  The running length of the stream is the caller's business.
hipError_t launch_bam_decode(const uint8_t *d_piece, uint64_t piece_bytes, const void *d_segments, uint64_t n_segments, uint64_t out_total,
                             uint8_t *d_out, hipStream_t st);
// ---- the parallel gzip reader's second pass (mgc_gzip.hip) ----
// One piece of a gzip stream's text in HBM (text_bytes at d_text, any alignment) whose first n_symbols bytes are still unresolved:
// d_symbols holds them as 16-bit symbols (mgc_gzip_par.hpp), 0x8000 + o standing for byte o of the 32 KiB window before the piece
// (d_window_in; only its last window_valid bytes belong to the piece's gzip member).  Patches d_text in place; a symbol that is
// neither a byte nor a marker inside the valid window ORs 1 / 2 into *d_error and becomes 0.  d_window_out (another buffer, or
// null): the window after the piece.  n_symbols == 0 and d_window_in == null (with window_valid 0) are fine.
hipError_t launch_gzip_resolve(uint8_t *d_text, uint64_t text_bytes, const uint16_t *d_symbols, uint64_t n_symbols, const uint8_t *d_window_in,
                               uint32_t window_valid, uint8_t *d_window_out, uint32_t *d_error, hipStream_t st);
// d_crc[i] = CRC-32 of d_text[d_begin[i] .. + d_len[i]), d_len[i] <= 4096 (more is not read)
hipError_t launch_gzip_crc32(const uint8_t *d_text, const uint64_t *d_begin, const uint32_t *d_len, uint64_t n_pieces, uint32_t *d_crc, hipStream_t st);
// what: 0 begin file, 1 end file (breaker), 2 roll the current file back, 3 reset
hipError_t launch_text_file_op(void *d_state, uint8_t *d_out, int what, hipStream_t st);
// the stream now holds new_len bytes (bases appended by a plain copy, or the tail kept after a batch was cut off);
// rebase_file: the open file's rollback point moves to 0 (what it wrote before the cut is gone)
hipError_t launch_text_set_len(void *d_state, uint64_t new_len, int rebase_file, hipStream_t st);

hipError_t launch_synth_reads(uint64_t seed, uint64_t genome_len, uint64_t first_read, uint64_t n_reads,
                              uint32_t read_len, uint32_t sub_rate_ppm, uint32_t n_rate_ppm,
                              uint32_t repeat_ppm, uint32_t repeat_unit, uint32_t repeat_families,
                              uint8_t *d_out, hipStream_t st);

// code objects load lazily at the first launch of a kernel of their translation unit: these touch one kernel each
hipError_t warm_kmer(); hipError_t warm_sort(); hipError_t warm_finish(); hipError_t warm_encode(); hipError_t warm_scan(); hipError_t warm_value_hist();
}  // namespace mgc
