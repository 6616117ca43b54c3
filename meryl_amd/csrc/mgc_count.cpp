// mgc_count.cpp -- count_device: from the bases resident in HBM (or the keys a sharded count's senders grouped by bucket) to the
// packed (k-mer, count) result in the session's arena.  CountPlan makes every host-side decision about the buckets ("files") and
// calls nothing on the device; Count runs the stages in the order the device sees them.
#include "mgc_session.hpp"
#include "mgc_group_batch.hpp"
#include "mgc_group_route.hpp"
#include "mgc_pack_plan.hpp"

#include <algorithm>
#include <vector>

#define TRY(expr) do { const int rc__ = (expr); if (rc__ != MGC_OK) return rc__; } while (0)

namespace {
using S = mgc_session;

struct StageTimer {
  bool on;
  hipStream_t st;
  hipEvent_t ev[MGC_NUM_STAGES][2];
  bool used[MGC_NUM_STAGES];
  StageTimer(bool enable, hipStream_t s) : on(enable), st(s) {
    for (int i = 0; i < MGC_NUM_STAGES; i++) {
      used[i] = false;
      if (on) { (void)hipEventCreate(&ev[i][0]); (void)hipEventCreate(&ev[i][1]); }
    }
  }
  ~StageTimer() {
    if (on) for (int i = 0; i < MGC_NUM_STAGES; i++) { (void)hipEventDestroy(ev[i][0]); (void)hipEventDestroy(ev[i][1]); }
  }
  void begin(int i) { if (on) { (void)hipEventRecord(ev[i][0], st); used[i] = true; } }
  void end(int i)   { if (on) (void)hipEventRecord(ev[i][1], st); }
};

// How a file is grouped by its top bits before the count kernels.
enum class Group : uint8_t {
  NONE,     // a file of one sub-bucket (or none): nothing to group
  SORT,     // stable LSB passes (mgc::launch_radix_sort); also what a narrowed file is once it has been widened back
  NARROW,   // the k-mers travel as 32-bit words from the first grouping pass on (mgc::launch_group_narrow)
  WIDE,     // the whole keys take the high-digit-first passes (mgc::launch_group_wide)
};

struct FilePlan {
  uint64_t size = 0, start = 0;       // k-mers, and the first one's index in X
  uint32_t top = 0;                   // grouping bits: 2^top sub-buckets
  uint32_t top_str = 0;               // the candidate coarser plan of the distinct-sized count: its grouping bits (0: none)
  mgc::SortPlan sp{};
  Group kind = Group::NONE;
  bool hpc = false;                   // `compress`: the grouping digits are dense ranks (make_hpc_group_plan)
  bool hpc_stream = false;            // ... a two-digit bucket above the index-claimed tables' reach
  bool hpc_cand = false;              // ... the distinct-sized count is a candidate the probe file decides on
  bool hpc_mixed = false;             // ... and with it 3^9 sub-buckets (make_hpc_mixed_plan)
  bool stream = false;                // counted by the distinct-sized kernel (hash_count_stream_kernel)
  bool k96 = false;                   // lies as 12-byte K96 records
  bool msd_ok = true;                 // the histogram of its high digit is at hand
  uint32_t tr_a = 0, tr_b = 0;        // in which order its sub-buckets lie (mgc::tr_index)
  uint64_t gbase = 0, sbase = 0, slots = 0;       // its sub-bucket tables: laid out for the finer of its two plans, `slots` of them
  size_t nws_off = 0;                 // its look-back scratch of the high-digit-first passes
  uint32_t *cnt = nullptr;            // where the counts of its distinct k-mers wait for the packing step
  uint64_t maxsub = 0, nlarge = 0, nzcount = 0;   // its statistics: largest sub-bucket, oversized ones, non-empty ones
  bool fallback = false;              // finished by the stable sort of all bits and the run-length kernels
  uint32_t passes = 0; bool narrowed = false, k96_passes = false;   // (profile) grouping passes that ran, and on what
  int batch_lead = -1;                // its passes ran in a batched launch: the batch's first file, which holds the launch's events (-1: launches of its own)
  uint64_t ngf() const { return size ? (uint64_t)1 << top : 0; }
};

// Buckets: the 64 files, or finer top-bit ranges of the k-mer.  The session's own partition uses the files while a file stays within
// what two grouping digits cover (1152 << 18 = 302 M k-mers); larger inputs are partitioned one or more bits finer -- the 64 files are
// ranges of buckets either way.
// `compress`: two dense-rank digits cover 3^10 sub-buckets, i.e. buckets of up to 68 M k-mers, and the digits are whole bases, so the
// buckets get finer two bits at a time.  (`compress` buckets are uneven -- a canonical k-mer starts with A or C twice as often as with G
// or T, and 36 of the 64 / 108 of the 256 bucket prefixes repeat no base -- so the largest bucket of a 10 Gbp input at 256 buckets holds
// ~100 M k-mers: above the 68 M of the index-claimed tables.  Round 6: such a bucket keeps its two dense-rank digits and is counted by
// the distinct-sized kernel, sub-buckets of up to 2304 k-mers on average, instead of falling back to the stable sort: hpc_stream.)
uint32_t plan_bucket_bits(const mgc_count_config &c, const mgc::Switches &sw, uint64_t n_bases) {
  const uint64_t per_bucket = sw.bucket_bases ? sw.bucket_bases              // tests force finer buckets on small inputs
                                              : (c.homopoly_compress ? 60000000ull : 180000000ull);
  const uint32_t step = c.homopoly_compress ? 2u : 1u;
  uint32_t bits = MGC_NUM_FILES_BITS;
  while (bits + step <= MGC_MAX_BUCKET_BITS && bits + step <= 2 * c.k && (n_bases >> bits) > per_bucket) bits += step;
  return bits;
}

// The plan of every file: host decisions only, from the configuration, the bucket histogram, which digit histogram is at hand and
// the switches.
struct CountPlan {
  const mgc_count_config &c;
  const mgc::Switches &sw;
  mgc_profile &prof;
  uint32_t kw, bucket_bits, nb, rem_bits, fine_bits;
  bool fine = false;                  // the fifteen-bit histogram is at hand (a bucket's first digit: fine_bits bits of it)
  bool fine_hpc = false;              // `compress`: its dense-rank form
  uint64_t max_bucket = 0, ng_total = 0, ns_total = 0;
  uint64_t target = 0, cap = 0, starget = 0;
  bool stream_on = false, hpc_ok = false, hpc_stream_ok = false, hpc_mixed_ok = false;
  std::vector<FilePlan> files;

  CountPlan(const mgc_count_config &c_, const mgc::Switches &sw_, mgc_profile &prof_, uint32_t kw_, uint32_t bucket_bits_)
      : c(c_), sw(sw_), prof(prof_), kw(kw_), bucket_bits(bucket_bits_), nb(1u << bucket_bits_), rem_bits(2 * c_.k - bucket_bits_),
        fine_bits(15u - bucket_bits_), files(nb) {}

  mgc::SortPlan group_plan(uint32_t low) const {          // grouping passes on bits [low, rem_bits)
    mgc::SortPlan p;
    mgc::make_sort_plan(low, rem_bits, &p);
    if (p.mode == 0) p.mode = 3;
    return p;
  }
  // msd_ok: a plan whose high digit is wider than what the fifteen-bit histogram knows gives bits to the low one; a low digit that
  // would pass nine bits keeps the low digit first
  void fit_split(FilePlan &x) const {
    mgc::SortPlan &fp = x.sp;
    if (!fine || fp.num_passes != 2 || fp.hpc || fp.pass_bits[1] <= fine_bits) return;
    const uint32_t t = fp.pass_bits[0] + fp.pass_bits[1];
    if (t - fine_bits > 9) { x.msd_ok = false; return; }
    fp.pass_bits[1] = fine_bits; fp.pass_bits[0] = t - fine_bits;
    fp.pass_shift[1] = fp.pass_shift[0] + fp.pass_bits[0];
  }

  void init() {
    target = mgc::finish_target_for(kw, sw); cap = mgc::finish_capacity_for(kw);
    stream_on = sw.hash_stream != 0 && kw == 1 && !c.homopoly_compress;
    starget = mgc::finish_stream_target(sw);
    // `compress`: the grouping digits are dense ranks of five homopolymer-free bases (make_hpc_group_plan): 10 key bits hold 243
    // patterns, 20 bits 59049.  Needs the remaining bits to be whole bases (the 64 files, or an even number of bucket bits) and the
    // bucket to fit 59049 sub-buckets; otherwise the generic bit digits (MGC_HPC_DIGITS=0: always).
    hpc_ok = sw.hpc_digits && c.homopoly_compress && (rem_bits % 2 == 0) && bucket_bits >= 2;
    // hpc_stream (round 6): a two-digit `compress` bucket whose sub-buckets average more than the index-claimed tables take counts its
    // whole 8-byte k-mers with the distinct-sized kernel (64-bit entries): everything the high-digit-first passes of such a bucket need
    // is known here (the dense-rank histogram is at hand, the suffix has 32..52 bits), so the plan is final at once
    hpc_stream_ok = hpc_ok && sw.hash_stream != 0 && sw.hash_stream != 2 && kw == 1 && fine_hpc && nb <= 256 && sw.wide_msd &&
                    rem_bits >= 20 + 32 && mgc::finish_stream_ok(kw, rem_bits - 20, false);
    hpc_mixed_ok = hpc_stream_ok && rem_bits >= 18 + 32 && mgc::finish_stream_ok(kw, rem_bits - 18, false) && mgc::finish_uses_hash(kw, rem_bits - 18);
  }

  // t top bits so that a sub-bucket holds ~target k-mers; the distinct-sized count's candidate (top_str)
  uint32_t plan_top(FilePlan &x) const {
    uint32_t t = 0;
    if (hpc_ok && x.size > target) {                                   // sub-buckets average `target` k-mers or fewer
      if (x.size <= 243ull * target && rem_bits >= 10) t = 10;
      else if (x.size <= 59049ull * target && rem_bits >= 20) t = 20;
      else if (hpc_stream_ok && x.size <= 59049ull * starget && x.size < (1ull << 30)) { t = 20; x.hpc_stream = true; }
      if (t == 20 && sw.hash_stream == 1 && hpc_stream_ok && x.size < (1ull << 30)) x.hpc_stream = true;   // (tests, A/B: every two-digit bucket)
      if (t) x.hpc = true;                                             // else (tiny k, gigantic bucket): generic path
    }
    if (!x.hpc) {
      while (t < rem_bits && t < 26 && (x.size >> t) > target) t++;
      // tests reach the large-input plans (two nine-bit digits, 18-bit suffixes at k = 21) on small inputs
      if (sw.min_top) { const uint32_t m = sw.min_top; if (x.size && t < m) t = m < rem_bits ? m : rem_bits; }
      // fstream (round 6): the file takes the DISTINCT-sized count (hash_count_stream_kernel: up to 4094 keys per sub-bucket streamed
      // through a table that holds ~1280 distinct suffixes) and with it one grouping bit fewer -- sub-buckets of 1152..2304 k-mers on
      // average instead of 576..1152, so that a file of up to 302 M k-mers groups by an eight-bit first digit (256-byte runs out of
      // the 16384-key tiles instead of 128-byte ones).  Narrowed files whose suffix fits the packed entry (8..20 bits).
      if (stream_on && x.size) {
        uint32_t ts = 0;
        while (ts < rem_bits && ts < 26 && (x.size >> ts) > starget) ts++;
        if (sw.min_top) { const uint32_t m = sw.min_top; if (ts < m) ts = m < rem_bits ? m : rem_bits; }
        x.top_str = ts;                                                // (clamped and validated once the file's kind of passes is known)
      }
    }
    if (c.homopoly_compress && t && !x.hpc) {
      // homopolymer-compressed sequence never repeats a base: every 2-bit group after the first takes 3 of its 4 values, so only
      // (3/4)^(t/2) of the 2^t top-bit patterns occur and the occupied sub-buckets are that much larger than planned: log2(4/3)/2 =
      // 0.2075 of every key bit carries no information
      const double scale = 1.0 / (1.0 - 0.2075);
      const uint32_t tc = (uint32_t)((double)t * scale + 0.5);
      t = tc < rem_bits ? (tc < 26 ? tc : 26) : rem_bits;
    }
    return t;
  }

  // `compress` with dense-rank digits: the high-digit-first passes where the dense-rank histogram is at hand
  void plan_hpc_kind(FilePlan &x) {
    mgc::make_hpc_group_plan(rem_bits - x.top, x.top / 10, &x.sp);
    // (sub-bucket numbers made of dense ranks are no key bits: the kernels that put a k-mer's top bits back from its sub-bucket
    // number -- 32-bit suffixes -- stay with the low digit first)
    const bool wide = fine_hpc && nb <= 256 && x.top == 20 && (kw == 2 || rem_bits - x.top >= 32) &&
                      mgc::finish_uses_hash(kw, rem_bits - x.top) && mgc::sort_plan_wide_msd(x.sp, x.size, sw.wide_msd);
    x.kind = wide ? Group::WIDE : Group::SORT;
    // (above the index-claimed tables' reach: the distinct-sized count whatever the coverage; below: a candidate the probe file decides on)
    if (x.hpc_stream && wide) { x.stream = true; prof.stream_files++; }
    else if (hpc_stream_ok && wide && x.top == 20 && x.size < (1ull << 30)) x.hpc_cand = true;
    // hpc_mixed: a candidate bucket of a size at which 3^9 sub-buckets (dense-rank high digit + the plain eight bits of four bases)
    // average what the distinct-sized count likes (0.3 .. 1 of its target: 700 .. 2304 k-mers) -- 3^10 of them hold a few hundred
    // k-mers each at 5 Gbp and the count kernel's per-sub-bucket steps dominate.  Taken where the probe says coverage is high.
    if ((x.hpc_cand || (x.stream && sw.hash_stream == 1)) && hpc_mixed_ok && x.size >= 19683ull * (starget * 3 / 10) &&
        x.size <= 19683ull * starget) {
      mgc::SortPlan mp;
      mgc::make_hpc_mixed_plan(rem_bits - 18, &mp);
      x.hpc_mixed = mgc::sort_plan_wide_msd(mp, x.size, sw.wide_msd);
      if (x.hpc_mixed && sw.hash_stream == 1) { take_coarser(x); x.hpc_mixed = x.hpc_cand = false; }   // (tests, A/B: no probe)
    }
  }

  // bit digits: narrowed, whole keys high digit first, or the stable LSB passes; the coarser candidate validated
  void plan_bit_kind(FilePlan &x) {
    x.sp = group_plan(rem_bits - x.top);
    fit_split(x);
    const uint32_t low = rem_bits - x.top;
    if (low < 32 && mgc::finish_uses_hash(kw, low) && mgc::sort_plan_narrows(x.sp, x.size, kw, sw.narrow)) x.kind = Group::NARROW;
    // (only the hash-count kernels translate the sub-bucket numbers of whole keys)
    else if (fine && nb <= 256 && x.msd_ok && mgc::finish_uses_hash(kw, low) && mgc::sort_plan_wide_msd(x.sp, x.size, sw.wide_msd)) x.kind = Group::WIDE;
    else x.kind = Group::SORT;
    if (!x.top_str) return;
    // the coarser plan stays a candidate if the file narrows under BOTH plans, its suffix then has to fit the packed 32-bit entry
    // (20 bits) -- or if its whole 8-byte k-mers take the high-digit-first passes under both (k = 24..32: 64-bit entries, 52 bits)
    const bool narrow = x.kind == Group::NARROW;
    uint32_t ts = x.top_str;
    const uint32_t t = x.top, max_low = narrow ? 20u : 52u;
    if (rem_bits - ts > max_low) ts = rem_bits - max_low;
    // (a plan that does not coarsen the file keeps the kernels it has -- unless MGC_HASH_STREAM=1 asks for the new one)
    bool ok = ts >= 1 && ts <= t && ts <= 18 && (ts < t || sw.hash_stream == 1) && (narrow || (x.kind == Group::WIDE && kw == 1 && sw.hash_stream != 2)) &&
              x.size < (1ull << 32) && mgc::finish_stream_ok(kw, rem_bits - ts, narrow) && mgc::finish_uses_hash(kw, rem_bits - ts);
    if (ok) {
      const mgc::SortPlan sp = group_plan(rem_bits - ts);
      if (narrow) ok = mgc::sort_plan_narrows(sp, x.size, kw, sw.narrow);
      else {
        // (whole keys need the high digit's histogram at hand under the coarser plan as well: fit_split's test)
        const bool split_ok = !(fine && sp.num_passes == 2 && sp.pass_bits[1] > fine_bits && ts - fine_bits > 9);
        ok = split_ok && mgc::sort_plan_wide_msd(sp, x.size, sw.wide_msd);
      }
    }
    x.top_str = ok ? ts : 0;
  }

  void plan_files() {
    init();
    for (FilePlan &x : files) {
      x.top = plan_top(x);
      if (x.size == 0 || x.top == 0) continue;
      if (x.hpc) plan_hpc_kind(x);
      else plan_bit_kind(x);
    }
    // a file's sub-bucket tables are laid out for the FINER of its two plans (2^top slots); ngf() of them are in use
    for (FilePlan &x : files) {
      x.slots = x.ngf();
      x.gbase = ng_total; x.sbase = ns_total;
      ng_total += x.slots;
      ns_total += x.slots ? x.slots + 1 : 0;
    }
  }

  // The coarser plan becomes the file's: the distinct-sized count (the probe's outcome, or MGC_HASH_STREAM=1 without a probe)
  void take_coarser(FilePlan &x) {
    if (!x.stream) { x.stream = true; prof.stream_files++; }
    if (x.top_str) {                                     // (its kind of passes stays as it is)
      x.top = x.top_str;
      x.sp = group_plan(rem_bits - x.top);
      x.msd_ok = true;
      fit_split(x);
    } else if (x.hpc_mixed) {                            // (`compress`: the other count kernel, on 3^9 sub-buckets)
      x.top = 18;
      mgc::make_hpc_mixed_plan(rem_bits - 18, &x.sp);
      prof.hpc_mixed_files++;
    }
  }

  // Which plan?  The distinct-sized count pays off when a sub-bucket's distinct suffixes are few against its keys (measured at 10 Gbp,
  // profiles/r06_coverage_ab.txt: D / N = 0.14 -> -3.6 ms, 0.24 -> -1.5, 0.45 -> +3, 0.72 -> +50: above its table the retry launch
  // counts the sub-bucket a second time), and D / N is not known before something has been counted: ONE file -- the PROBE file, the
  // smallest one that is still a fair sample -- goes through its passes and its count first, on the finer plan; its distinct /
  // instances ratio decides for the others (apply_probe).  MGC_HASH_STREAM=1: every candidate, no probe; 0: none.  -1: no probe.
  int choose_probe() {
    bool any_cand = false;
    for (const FilePlan &x : files) any_cand = any_cand || x.top_str != 0 || x.hpc_cand;
    if (!any_cand) return -1;
    if (sw.hash_stream == 1) {
      for (FilePlan &x : files) if (x.top_str) take_coarser(x);
      return -1;
    }
    int probe = -1;
    uint64_t best = ~0ull;
    for (uint32_t b = 0; b < nb; b++)
      if (files[b].size >= max_bucket / 16 && files[b].size >= 4096 && files[b].size < best) { best = files[b].size; probe = (int)b; }
    return probe;
  }
  void apply_probe(uint32_t probe) {                     // the probe found coverage high enough
    for (uint32_t b = 0; b < nb; b++)
      if (b != probe && (files[b].top_str || (files[b].hpc_cand && !files[b].stream))) take_coarser(files[b]);
  }

  // 5-byte layout: 8-byte keys with 33..40 bits below the file (k = 20..23), every non-empty file on the narrowed passes with the high
  // digit first off the fifteen-bit histogram (the instrumented instantiation reads whole keys).  MGC_SOA5=0: whole keys.
  // The mask of the key bits above the low 32 (0: whole keys).
  uint32_t soa_mask(bool plain_input) const {
    bool soa = sw.soa5 && plain_input && kw == 1 && nb == 64 && fine && rem_bits > 32 && rem_bits <= 40;
    for (const FilePlan &x : files) if (x.size && !(x.kind == Group::NARROW && x.top)) soa = false;
    return soa ? (1u << (rem_bits - 32)) - 1u : 0u;
  }
  // K96 records (round 5): 16-byte keys with at most 96 bits below the file (k = 33..51), every non-empty file on the whole-key
  // high-digit-first passes: 12 of the 16 bytes leave the partition, go through both passes and into the count kernel (mgc_common.hpp
  // K96; the region of a file stays 16 bytes per k-mer, so a file can be widened back in place).  A small file keeps 16-byte keys.
  // MGC_K96=0: whole keys.  True if any file takes them.
  bool k96_layout(bool plain_input) {
    if (!(sw.k96 && plain_input && kw == 2 && nb == 64 && fine && rem_bits <= 96 && !c.homopoly_compress)) return false;
    bool any = false;
    for (FilePlan &x : files) if (x.size && x.kind == Group::WIDE && x.top) { x.k96 = true; any = true; prof.k96_files++; }
    return any;
  }
};

// The count of one session: its buffers, its streams and its stages.
struct Count {
  mgc_session *s;
  const mgc::CountInput &in;
  hipStream_t st;
  const mgc_count_config &c;
  const mgc::Switches &sw;
  mgc_profile &prof;
  const uint32_t k, kw, bucket_bits, nb, rem_bits;
  const size_t kbytes;
  CountPlan plan;
  StageTimer tm;
  hipEvent_t ev_all[2] = {nullptr, nullptr};

  const uint8_t *d_bases;
  uint64_t n_bases, N = 0, nd = 0;
  void *part_ws = nullptr, *sort_ws = nullptr, *rle_ws = nullptr;
  uint64_t *d_counts64 = nullptr, *d_starts = nullptr;
  std::vector<uint64_t> h_meta;                          // [nb] starts, [nb] K96 flags: copied to d_starts (lives until the count returns)
  const uint64_t *d_fine = nullptr, *d_fine_hpc = nullptr;
  void *d_packed = nullptr;                              // the packed base stream (mgc_device.h, kp_packed_bytes); nullptr: the partition reads ASCII
  mgc::SortPlan full{};                                  // the stable sort of all bits below the bucket
  bool use_finish;
  unsigned char *X = nullptr, *Y = nullptr;
  size_t sort_ws_bytes = 0;
  uint32_t *d_err = nullptr;
  uint32_t soa_hi_mask = 0;                              // nonzero: the files lie in the 5-byte layout
  static constexpr uint32_t ev_per_file = 2 * 16;        // room for 16 passes per file
  std::vector<hipEvent_t> pass_ev;
  uint32_t sort_launch_groups = 0;
  size_t y_base_bytes = 0;                               // what Y holds without batched launches (one file's keys, or all of them)
  std::vector<unsigned char> h_batch_tables;             // the batched launches' descriptor tables (copied from here: lives until the count returns)
  int group_dbg_left = 2;                                // MGC_GROUP_DBG: instrumented files this count may still run (GroupFile::dbg)

  // the finish path
  int probe = -1;
  uint64_t *d_substart = nullptr, *d_group = nullptr, *d_stats = nullptr, *d_retrycnt = nullptr;
  uint32_t *d_large = nullptr, *d_nz = nullptr;
  const size_t hdr_bytes = mgc::sort_header_bytes();
  unsigned char *d_nws = nullptr, *d_nhdrs = nullptr;
  std::vector<mgc::DBuf> cnt_extra;
  bool fork_huge = false, forked = false, need_join = false;   // forked: stream2 is ordered after everything st holds that it must see
  static constexpr int NH = 1 + S::HUGE_EXTRA;
  hipStream_t hstream[NH] = {};
  unsigned char *halt[NH] = {};
  void *hws[NH] = {nullptr, nullptr, nullptr, nullptr};  // the sliced count of gigantic sub-buckets: one plan workspace per stream
  size_t hws_bytes = 0;
  int n_huge_streams = 1, huge_next = 0;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> fin_ev; // profiling: around every file's count-kernel launch
  uint64_t fin_keys = 0, fin_in_bytes = 0; bool fin_narrow = false;
  // early packing (mgc_pack_plan.hpp): the files are packed on pack_st, in index order, while later files are still counted
  bool early = false;
  std::vector<uint32_t> chain;                           // the files that hold k-mers, in index order: the packing chain
  std::vector<int> chain_pos;                            // a file's place in it (-1: empty)
  std::vector<char> pack_ev2;                            // the file has a second event to wait for (s->pack_ev[nb + b])
  uint64_t *d_pstate = nullptr;                          // mgc_device.h, launch_pack_gate_scan
  hipStream_t pack_st = nullptr;
  uint64_t early_cap = 0;                                // k-mers the result had room for when the chain was queued
  hipEvent_t ev_pack[2] = {nullptr, nullptr};            // profiling: around what the count kernels do not hide of the packing

  Count(mgc_session *s_, const mgc::CountInput &in_, uint32_t bucket_bits_)
      : s(s_), in(in_), st(s_->stream), c(s_->cfg), sw(s_->sw), prof(s_->prof), k(c.k), kw(s_->key_words), bucket_bits(bucket_bits_),
        nb(1u << bucket_bits_), rem_bits(2 * c.k - bucket_bits_), kbytes(sizeof(uint64_t) * kw), plan(c, sw, s_->prof, kw, bucket_bits_),
        tm(s_->profiling, s_->stream), d_bases(s_->d_bases), n_bases(s_->n_bases), h_meta(2 * (size_t)nb, 0), use_finish(sw.finish) {}

  void *seg(uint32_t b) const { return X + kbytes * plan.files[b].start; }
  uint32_t low(const FilePlan &x) const { return rem_bits - x.top; }
  // the list of non-empty sub-buckets pays off only when a good part of the 2^t grid is empty (`compress`: 59049 of 2^20); tests run the
  // dense-grid instantiations of the count kernels on small inputs (whose 2^t grids are mostly empty)
  const uint32_t *nz_list(const FilePlan &x) const { return (4 * x.nzcount < 3 * x.ngf() && !sw.nolist) ? d_nz + x.gbase : nullptr; }
  // files whose high digit goes first off the histogram at hand: each has a header and look-back scratch
  bool msd_file(const FilePlan &x) const {
    return d_fine_hpc ? x.kind == Group::WIDE : (x.kind == Group::NARROW || x.kind == Group::WIDE) && x.msd_ok;
  }
  mgc::FinishFile finish_desc(uint32_t b, bool stream, hipStream_t fst, int hsel) const;
  void take_stats(uint32_t b) {
    const uint64_t *h = s->h_stats + 3 * (size_t)b;
    plan.files[b].maxsub = h[0]; plan.files[b].nlarge = h[1]; plan.files[b].nzcount = h[2];
  }

  // the stages, in the order they run (every one returns an MGC_* code)
  int run();
  int compress_bases(); int histogram(); int buffers(); int partition(bool soa, bool k96);
  int count_full();                                      // MGC_FINISH=0
  int count_finish(); int finish_buffers(); int prepare_headers(); int narrow_prepare(int only, int skip);
  int probe_file(); int group_file(uint32_t b); int stats_file(uint32_t b); int group_all();
  mgc::GroupFile group_desc(uint32_t b); bool batch_file(uint32_t b) const; int group_batches();
  int huge_setup(); int huge_sync_all(); int huge_join_all();
  int finish_file(uint32_t b); int oversized_streams(uint32_t b, bool *stream); int widen_back(uint32_t b, bool *unordered);
  int count_file(uint32_t b, bool stream); int fallback_file(uint32_t b, bool unordered);
  int trace_slices(); int retry(); int scan_pack(); void finish_profile();
  int pack_file(uint32_t b, hipStream_t ps, const uint64_t *d_gate = nullptr, uint64_t gate_above = 0);
  int pack_events(); int pack_plan(); int pack_step(uint32_t b); int pack_finish(); int pack_done();
  int block_offsets(); void collect_profile();
};

// ---- `compress`: homopolymer-compress the base stream on the device (merylInput.C:261-268) ----
int Count::compress_bases() {
  if (!c.homopoly_compress || !n_bases || in.keys) return MGC_OK;
  HIP_TRY(s, s->ensure(S::B_HPC, n_bases));
  HIP_TRY(s, s->ensure(S::B_HPC_WS, mgc::hpc_workspace_bytes(n_bases)));
  uint8_t *d_hpc = reinterpret_cast<uint8_t *>(s->buf[S::B_HPC].p);
  void *hws_ = s->buf[S::B_HPC_WS].p;
  HIP_TRY(s, mgc::launch_homopoly_compress(d_bases, n_bases, d_hpc, hws_, st));
  uint64_t n_out = 0;
  HIP_TRY(s, hipMemcpyAsync(&n_out, hws_, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(s, hipStreamSynchronize(st));
  d_bases = d_hpc;
  n_bases = n_out;
  return MGC_OK;
}

// ---- pass 1: per-file histogram ----
int Count::histogram() {
  HIP_TRY(s, s->ensure(S::B_PART_WS, mgc::kp_workspace_bytes(bucket_bits)));
  HIP_TRY(s, s->ensure(S::B_META, sizeof(uint64_t) * nb * 3));        // counts, starts, per-file K96 flags
  part_ws = s->buf[S::B_PART_WS].p;
  d_counts64 = reinterpret_cast<uint64_t *>(s->buf[S::B_META].p);
  d_starts = d_counts64 + nb;
  std::vector<uint64_t> h_counts(nb);
  // (two digits cover at most 18 bits: beyond 2k - 6 = 41 nothing narrows -- the files' WHOLE keys then take the same high-digit-first
  // passes, mgc::launch_group_wide, 16-byte keys included; MGC_WIDE_MSD=0: low digit first off a histogram read of the keys, as
  // `compress` always does: its digits are dense ranks)
  const bool wide_msd_on = sw.wide_msd && !c.homopoly_compress;
  if (!in.keys) {
    // The narrowed grouping passes (k <= ~25) group a file by its TOP digit first when that digit's histogram is at hand: the file
    // histogram then counts fifteen top bits instead of six (one kernel, same read of the bases) and the 8 B/k-mer digit-histogram
    // read of every file goes away.
    // The packed base stream (MGC_PACKED_BASES=0: off): the histogram kernel stores the 2-bit codes and invalid-base masks it has to
    // make anyway, and the partition stages its tiles from them instead of decoding the ASCII bases a second time.  Only where the
    // arena can grow by it beside what the count itself is budgeted at (2 + 14 bytes per key word and base, mgc_input.cpp: input_setup);
    // a count that cannot have it runs as before.
    if (sw.packed_bases && n_bases) {
      const size_t pb = mgc::kp_packed_bytes(n_bases);
      bool room = s->buf[S::B_PACKED].cap >= pb;
      if (!room) {
        size_t free_b = 0, total_b = 0;
        room = hipMemGetInfo(&free_b, &total_b) == hipSuccess &&
               (double)free_b + (double)s->arena_bytes() >= (double)n_bases * (double)(2 + 14ull * kw) + (double)pb;
      }
      if (room) {
        if (s->ensure(S::B_PACKED, pb) == hipSuccess) d_packed = s->buf[S::B_PACKED].p;
        else (void)hipGetLastError();
      }
    }
    tm.begin(MGC_STAGE_HISTOGRAM);
    if (n_bases >= (1u << 22) && ((kw == 1 && 2 * k - bucket_bits <= 41) || wide_msd_on) && mgc::kmer_histogram_fine_ok(k, bucket_bits, s->sfx_mask, sw)) {
      HIP_TRY(s, s->ensure(S::B_FINE, sizeof(uint64_t) << 15));
      uint64_t *fine = reinterpret_cast<uint64_t *>(s->buf[S::B_FINE].p);
      HIP_TRY(s, mgc::launch_kmer_histogram_fine(d_bases, n_bases, k, c.mode, d_counts64, fine, part_ws, st, sw.const_k, 6, d_packed));
      d_fine = fine;
    } else if (c.homopoly_compress && n_bases >= (1u << 22) && (2 * k - bucket_bits) % 2 == 0 && 2 * k - bucket_bits >= 20 &&
               sw.hpc_digits && mgc::kmer_histogram_hpc_ok(k, bucket_bits, s->sfx_mask, sw)) {
      // `compress`: k-mers per (bucket, dense-rank digit below it) -- the buckets' high digit goes first as well (MGC_HPC_MSD=0: off)
      HIP_TRY(s, s->ensure(S::B_FINE, sizeof(uint64_t) * std::max<size_t>((size_t)1 << 15, mgc::kmer_histogram_hpc_entries(bucket_bits))));
      uint64_t *fine = reinterpret_cast<uint64_t *>(s->buf[S::B_FINE].p);
      HIP_TRY(s, mgc::launch_kmer_histogram_hpc(d_bases, n_bases, k, c.mode, bucket_bits, d_counts64, fine, part_ws, st, sw.const_k, d_packed));
      d_fine_hpc = fine;
    } else
    HIP_TRY(s, mgc::launch_kmer_histogram(d_bases, n_bases, k, c.mode, bucket_bits, d_counts64, part_ws, st, s->sfx_mask, s->sfx_test, d_packed));
    tm.end(MGC_STAGE_HISTOGRAM);
    prof.stage_launches[MGC_STAGE_HISTOGRAM] = 1;
    HIP_TRY(s, hipMemcpyAsync(h_counts.data(), d_counts64, sizeof(uint64_t) * nb, hipMemcpyDeviceToHost, st));
    HIP_TRY(s, hipStreamSynchronize(st));
  } else {
    memcpy(h_counts.data(), in.counts, sizeof(uint64_t) * nb);
    // the owner side of a sharded count: the senders' fifteen-bit histograms, summed over the ranks (mgc_count_buckets_into), give
    // every bucket's first grouping digit -- 15 - bucket_bits bits of it -- so that nobody reads the keys for a histogram here either
    uint64_t n_ext = 0;
    for (uint32_t b = 0; b < nb; b++) n_ext += h_counts[b];
    if (in.fine && sw.fine_hist && bucket_bits <= 8 && n_ext >= (1u << 22) && s->sfx_mask == 0 && !c.homopoly_compress &&
        2 * k >= 15 + 2 && ((kw == 1 && 2 * k - bucket_bits <= 41) || wide_msd_on))
      d_fine = in.fine;
  }
  memset(s->file_instances, 0, sizeof(s->file_instances));
  for (uint32_t b = 0; b < nb; b++) {
    plan.files[b].size = h_counts[b];
    plan.files[b].start = h_meta[b] = N;
    N += h_counts[b];
    plan.max_bucket = std::max(plan.max_bucket, h_counts[b]);
    s->file_instances[b >> (bucket_bits - MGC_NUM_FILES_BITS)] += h_counts[b];
  }
  s->n_instances = N;
  plan.fine = d_fine != nullptr;
  plan.fine_hpc = d_fine_hpc != nullptr;
  return MGC_OK;
}

// Two ways from file-grouped k-mers to the (k-mer, count) stream:
//   finish (default): LSB-sort only the top t bits of every file globally, then sort the low bits of every sub-bucket in LDS with the
//                     run-length count fused in (mgc_finish.hip);
//   full   (MGC_FINISH=0, and the fallback for files with an oversized sub-bucket): LSB-sort all 2k-6 bits globally, then the
//                     separate run-length kernels.
int Count::buffers() {
  mgc::make_sort_plan(0, rem_bits, &full);
  const bool odd = !use_finish && (full.num_passes & 1u) != 0;
  if (!in.keys) HIP_TRY(s, s->ensure(S::B_X, kbytes * N));
  y_base_bytes = kbytes * (odd ? N : plan.max_bucket);
  HIP_TRY(s, s->ensure(S::B_Y, y_base_bytes));
  X = in.keys ? reinterpret_cast<unsigned char *>(in.keys) : reinterpret_cast<unsigned char *>(s->buf[S::B_X].p);
  Y = reinterpret_cast<unsigned char *>(s->buf[S::B_Y].p);
  sort_ws_bytes = mgc::sort_workspace_bytes(plan.max_bucket) + 256;
  HIP_TRY(s, s->ensure(S::B_SORT_WS, sort_ws_bytes));
  sort_ws = s->buf[S::B_SORT_WS].p;
  // device flags: [0] look-back timeout, [1] scratch answer of the hash probe, [2] overflow of a streamed sub-bucket;
  // [FIN_HUGE_STATS_AT ...]: the path counters of the gigantic sub-buckets (mgc_device.h), zero when the count begins
  d_err = reinterpret_cast<uint32_t *>(reinterpret_cast<unsigned char *>(sort_ws) + sort_ws_bytes - 256);
  static_assert(sizeof(uint32_t) * (mgc::FIN_HUGE_STATS_AT + mgc::FIN_HUGE_STATS) <= 256, "the flag block holds the path counters");
  HIP_TRY(s, hipMemsetAsync(d_err, 0, sizeof(uint32_t) * (mgc::FIN_HUGE_STATS_AT + mgc::FIN_HUGE_STATS), st));
  if (s->profiling) {
    pass_ev.resize((size_t)nb * ev_per_file);
    for (auto &e : pass_ev) (void)hipEventCreate(&e);
  }
  return MGC_OK;
}

// ---- pass 2: pack + scatter into per-file regions ----
// Launched once the plan of the files is known: when every file takes the narrowed passes its k-mers leave as 5 bytes (u32 + u8 per
// file) instead of 8 -- the file's first grouping pass puts them together again.
int Count::partition(bool soa, bool k96) {
  if (in.keys) return MGC_OK;
  HIP_TRY(s, hipMemcpyAsync(d_starts, h_meta.data(), sizeof(uint64_t) * nb, hipMemcpyHostToDevice, st));
  uint64_t *d_k96flags = d_starts + nb;
  if (k96) HIP_TRY(s, hipMemcpyAsync(d_k96flags, h_meta.data() + nb, sizeof(uint64_t) * nb, hipMemcpyHostToDevice, st));
  tm.begin(MGC_STAGE_PARTITION);
  HIP_TRY(s, mgc::launch_kmer_partition(d_bases, n_bases, k, c.mode, bucket_bits, d_starts, (void *)X, part_ws, st,
                                        s->sfx_mask, s->sfx_test, k96 ? d_k96flags : (soa ? d_counts64 : nullptr), sw.const_k, d_packed));
  tm.end(MGC_STAGE_PARTITION);
  const uint64_t packed_b = d_packed ? mgc::kp_packed_bytes(n_bases) : 0;    // stored by the histogram, read by the partition in place of the bases
  prof.hist_bytes = n_bases + packed_b;
  prof.partition_bytes = d_packed ? packed_b : n_bases;
  for (uint32_t b = 0; b < nb; b++) prof.partition_bytes += plan.files[b].size * (soa ? 5u : ((k96 && plan.files[b].k96) ? 12u : (uint64_t)kbytes));
  prof.stage_launches[MGC_STAGE_PARTITION] = 2;
  return MGC_OK;
}

// MGC_FINISH=0: the stable sort of all bits of every file, then the run-length kernels
int Count::count_full() {
  TRY(partition(false, false));
  const bool odd = (full.num_passes & 1u) != 0;
  tm.begin(MGC_STAGE_SORT);
  for (uint32_t b = 0; b < nb; b++) {
    FilePlan &x = plan.files[b];
    if (x.size == 0) continue;
    void *alt = odd ? (void *)(Y + kbytes * x.start) : (void *)Y;
    int in_alt = 0;   // odd pass count: every file ends in Y at the same offsets; even: back in X
    hipEvent_t *pe = s->profiling ? &pass_ev[(size_t)b * ev_per_file] : nullptr;
    HIP_TRY(s, mgc::launch_radix_sort(seg(b), alt, x.size, kw, full, sort_ws, sort_ws_bytes - 256, d_err, &in_alt, st, pe));
    x.passes = full.num_passes;
    sort_launch_groups++;
  }
  tm.end(MGC_STAGE_SORT);
  void *d_sorted = odd ? (void *)Y : (void *)X;

  // ---- run-length count ----
  HIP_TRY(s, s->ensure(S::B_RLE_WS, mgc::rle_workspace_bytes(N)));
  rle_ws = s->buf[S::B_RLE_WS].p;
  tm.begin(MGC_STAGE_RLE);
  HIP_TRY(s, mgc::launch_rle_count(d_sorted, N, kw, rle_ws, st));
  HIP_TRY(s, mgc::rle_read_total(rle_ws, &nd, st));
  s->n_distinct = nd;
  HIP_TRY(s, s->ensure(S::B_UNIQUE, kbytes * nd));
  HIP_TRY(s, s->ensure(S::B_COUNTS, sizeof(uint32_t) * nd));
  s->d_unique = s->buf[S::B_UNIQUE].p;
  s->d_counts = reinterpret_cast<uint32_t *>(s->buf[S::B_COUNTS].p);
  HIP_TRY(s, mgc::launch_rle_emit(d_sorted, N, kw, rle_ws, s->d_unique, s->d_counts, st));
  tm.end(MGC_STAGE_RLE);
  prof.stage_launches[MGC_STAGE_RLE] = 3;
  return MGC_OK;
}

// The sub-bucket tables, the statistics and the counts' buffers.
int Count::finish_buffers() {
  const uint64_t ng_total = plan.ng_total;
  HIP_TRY(s, s->ensure(S::B_SUBSTART, sizeof(uint64_t) * (plan.ns_total + 1)));
  HIP_TRY(s, s->ensure(S::B_GROUPS, sizeof(uint64_t) * (ng_total + 2 + 3 * (uint64_t)nb)));
  HIP_TRY(s, s->ensure(S::B_LARGE, sizeof(uint32_t) * (ng_total + 1)));
  HIP_TRY(s, s->ensure(S::B_NONEMPTY, sizeof(uint32_t) * (ng_total + 1) + sizeof(uint64_t) * 2 * ((uint64_t)nb + 1)));
  HIP_TRY(s, s->ensure(S::B_GSCAN, mgc::finish_scan_scratch_bytes(ng_total + 1)));
  HIP_TRY(s, s->ensure(S::B_RLE_WS, mgc::rle_workspace_bytes(plan.max_bucket)));
  d_substart = reinterpret_cast<uint64_t *>(s->buf[S::B_SUBSTART].p);
  d_group    = reinterpret_cast<uint64_t *>(s->buf[S::B_GROUPS].p);   // [ng_total+1], then the files' statistics
  // per file, three words side by side (one small copy brings a file's back): [0] its largest sub-bucket, [1] how many are above the
  // persistent kernels' capacity, [2] how many are not empty
  d_stats    = d_group + ng_total + 1;
  d_large    = reinterpret_cast<uint32_t *>(s->buf[S::B_LARGE].p);
  d_retrycnt = reinterpret_cast<uint64_t *>(s->buf[S::B_NONEMPTY].p) + nb + 1;  // [nb] retry lists of the count kernels
  d_nz       = reinterpret_cast<uint32_t *>(d_retrycnt + nb + 1);                 // [ng_total] (a dense file's part: its retry list)
  HIP_TRY(s, hipMemsetAsync(s->buf[S::B_NONEMPTY].p, 0, sizeof(uint64_t) * 2 * ((size_t)nb + 1), st));
  HIP_TRY(s, hipMemsetAsync(d_group, 0, sizeof(uint64_t) * (ng_total + 1 + 3 * (size_t)nb), st));   // empty sub-buckets stay 0
  rle_ws = s->buf[S::B_RLE_WS].p;
  return MGC_OK;
}

// high digit first: the headers of all files in one launch (with a probe file: its header first, the others' once their plan is
// known), their look-back granules zeroed in one memset
int Count::prepare_headers() {
  if ((!d_fine && !d_fine_hpc) || nb > 256) return MGC_OK;
  uint64_t on[4] = {0, 0, 0, 0};
  size_t off = 0;
  bool any = false;
  for (uint32_t b = 0; b < nb; b++) {
    FilePlan &x = plan.files[b];
    x.nws_off = off;
    if (!msd_file(x)) continue;
    any = true;
    on[b >> 6] |= 1ull << (b & 63u);
    off += ((x.kind == Group::NARROW ? mgc::narrow_scratch_bytes(x.size) : mgc::wide_scratch_bytes(x.size, kw)) + 255) / 256 * 256;
  }
  if (!any) return MGC_OK;
  HIP_TRY(s, s->ensure(S::B_SORT_HDRS, hdr_bytes * nb));
  HIP_TRY(s, s->ensure(S::B_NARROW_WS, off));
  d_nhdrs = reinterpret_cast<unsigned char *>(s->buf[S::B_SORT_HDRS].p);
  d_nws = reinterpret_cast<unsigned char *>(s->buf[S::B_NARROW_WS].p);
  if (d_fine) TRY(narrow_prepare(probe, -1));
  else HIP_TRY(s, mgc::launch_hpc_prepare(d_fine_hpc, bucket_bits, on, d_nhdrs, st));
  HIP_TRY(s, hipMemsetAsync(d_nws, 0, off, st));
  return MGC_OK;
}

int Count::narrow_prepare(int only, int skip) {
  unsigned char bits_a[256] = {0}, on[256] = {0};
  bool any = false;
  for (uint32_t b = 0; b < nb; b++) {
    if (!msd_file(plan.files[b]) || (only >= 0 && (int)b != only) || (int)b == skip) continue;
    on[b] = 1; bits_a[b] = (unsigned char)plan.files[b].sp.pass_bits[1]; any = true;
  }
  if (any) HIP_TRY(s, mgc::launch_narrow_prepare(d_fine, nb, bits_a, on, d_nhdrs, st));
  return MGC_OK;
}

// what the grouping launchers are told about file b (mgc_device.h, GroupFile)
mgc::GroupFile Count::group_desc(uint32_t b) {
  FilePlan &x = plan.files[b];
  const bool msd = d_nhdrs && d_nws && (x.kind == Group::WIDE || x.msd_ok);
  mgc::GroupFile f;
  f.keys = seg(b); f.alt = (void *)Y; f.n = x.size; f.plan = &x.sp;
  f.layout = x.k96 ? mgc::GroupKeys::K96 : (kw == 2 ? mgc::GroupKeys::K128 : (soa_hi_mask ? mgc::GroupKeys::SOA5 : mgc::GroupKeys::U64));
  f.soa_hi_mask = soa_hi_mask;
  f.d_error = d_err; f.d_sub_starts = d_substart + x.sbase; f.st = st;
  f.pass_events = s->profiling ? &pass_ev[(size_t)b * ev_per_file] : nullptr;
  f.prepared = msd ? (void *)(d_nhdrs + hdr_bytes * b) : nullptr; f.scratch = msd ? (void *)(d_nws + x.nws_off) : nullptr;
  f.ws = sort_ws; f.ws_bytes = sort_ws_bytes - 256;
  f.pipe = sw.group_pipe; f.stagger = sw.pass_stagger;
  f.dbg = sw.group_dbg && msd && x.kind == Group::NARROW && group_dbg_left > 0;     // (developer output: the first two such files of a count)
  return f;
}

// ---- A. grouping passes of one file: global passes on its top bits only (the finish only needs the file grouped by them) ----
int Count::group_file(uint32_t b) {
  FilePlan &x = plan.files[b];
  if (x.size == 0) return MGC_OK;
  void *src = seg(b);
  mgc::GroupFile f = group_desc(b);
  hipEvent_t *pe = f.pass_events;
  switch (x.kind) {
  case Group::NONE:                                        // (a file of one sub-bucket: nothing to group)
    return MGC_OK;
  case Group::NARROW:                                      // X (8 B) -> Y (4 B) -> front of X (4 B); boundaries included
    HIP_TRY(s, mgc::launch_group_narrow(f));
    if (f.dbg) group_dbg_left--;
    x.tr_a = f.tr_a; x.tr_b = f.tr_b;
    x.passes = 2;
    x.narrowed = true;
    break;
  case Group::WIDE:                                        // X -> Y -> X, whole keys; boundaries included
    if (d_nhdrs) {
      HIP_TRY(s, mgc::launch_group_wide(f));
      x.tr_a = f.tr_a; x.tr_b = f.tr_b;
      x.passes = 2;
      x.k96_passes = x.k96;
      prof.wide_msd_files++;
      prof.wide_digit_widths |= (1u << x.sp.pass_bits[1]) | (1u << (16 + x.sp.pass_bits[0]));
      break;
    }
    x.kind = Group::SORT;
    [[fallthrough]];
  case Group::SORT: {
    int in_alt = 0;
    HIP_TRY(s, mgc::launch_radix_sort(src, (void *)Y, x.size, kw, x.sp, sort_ws, sort_ws_bytes - 256, d_err, &in_alt, st, pe));
    if (in_alt) HIP_TRY(s, hipMemcpyAsync(src, Y, kbytes * x.size, hipMemcpyDeviceToDevice, st));
    x.passes = x.sp.num_passes;
    break;
  }
  }
  sort_launch_groups++;
  return MGC_OK;
}

// ---- B/C. a file's sub-bucket boundaries and its statistics ----
int Count::stats_file(uint32_t b) {
  const FilePlan &x = plan.files[b];
  if (x.size == 0) return MGC_OK;
  uint64_t *ds = d_stats + 3 * (size_t)b;
  if (x.kind == Group::NARROW || x.kind == Group::WIDE)
    HIP_TRY(s, mgc::launch_subbucket_max(d_substart + x.sbase, kw, low(x), x.top, ds, d_large + x.gbase, ds + 1, d_nz + x.gbase, ds + 2, st,
                                         x.stream ? mgc::finish_stream_capacity() : 0));
  else
    HIP_TRY(s, mgc::launch_subbucket_bounds(seg(b), x.size, kw, low(x), x.top, d_substart + x.sbase, ds, d_large + x.gbase, ds + 1,
                                            d_nz + x.gbase, ds + 2, st));
  return MGC_OK;
}

// the probe file: passes, statistics, count -- then its distinct / instances ratio (one 8-byte copy) chooses the others' plan
int Count::probe_file() {
  const uint32_t pb = (uint32_t)probe;
  const FilePlan &x = plan.files[pb];
  TRY(group_file(pb));
  TRY(stats_file(pb));
  HIP_TRY(s, hipMemcpyAsync(s->h_stats + 3 * (size_t)pb, d_stats + 3 * (size_t)pb, sizeof(uint64_t) * 3, hipMemcpyDeviceToHost, st));
  HIP_TRY(s, hipStreamSynchronize(st));
  take_stats(pb);
  TRY(finish_file(pb));
  if (need_join) TRY(huge_join_all());
  forked = false;                                        // (the second stream has to be ordered behind the other files' passes again)
  uint64_t h_pd = 0;
  HIP_TRY(s, mgc::launch_sum_u64(d_group + x.gbase, x.slots, d_group + plan.ng_total, st));
  HIP_TRY(s, hipMemcpyAsync(&h_pd, d_group + plan.ng_total, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(s, hipStreamSynchronize(st));
  const double ratio = (double)h_pd / (double)x.size;
  prof.probe_ratio = ratio;
  if (sw.finish_trace) fprintf(stderr, "[finish] probe file %u: %llu distinct of %llu k-mers (%.3f): the other files take the %s plan\n", pb,
                               (unsigned long long)h_pd, (unsigned long long)x.size, ratio, ratio <= 0.30 ? "distinct-sized" : "finer");
  if (ratio <= 0.30) plan.apply_probe(pb);
  if (d_fine && nb <= 256 && d_nhdrs) TRY(narrow_prepare(-1, probe));
  return MGC_OK;
}

// Stage after stage: the passes of all files go to the session stream back to back, one synchronisation brings the files' statistics
// back, then the count kernels run.  (A pipelined form -- a file's count kernel on another stream as soon as its statistics are back,
// beside the passes of the files after it -- was built in round 4, measured slower and removed in round 5: profiles/r04y_pipe_ab.txt,
// DESIGN_HISTORY.md.)
// The grouping passes themselves: the narrowed files of the judged form go through them in BATCHES -- one launch per pass over the
// tiles of all files of a batch, so that the device does not drain and fill again 128 times per count (mgc_sort.hip, radix_group_body,
// BATCH; which files share a launch and where their words lie in Y meanwhile: mgc_group_batch.hpp).  Every other file, and every
// file that is alone in its batch, keeps the per-file launches.
bool Count::batch_file(uint32_t b) const {
  const FilePlan &x = plan.files[b];
  return (int)b != probe && x.size && x.top && x.kind == Group::NARROW && x.msd_ok && d_nhdrs && d_nws && soa_hi_mask != 0 &&
         mgc::group_batch_form(true, true, sw.group_pipe, sw.group_dbg, sw.pass_stagger);
}

int Count::group_batches() {
  std::vector<mgc::BatchFile> bf(nb);
  for (uint32_t b = 0; b < nb; b++) {
    const FilePlan &x = plan.files[b];
    // (shifts and digit widths are arguments of a launch: the key is the plan's digits, which also fix both instantiations)
    bf[b] = mgc::BatchFile{x.size, x.sp.pass_shift[0] | (x.sp.pass_bits[0] << 8) | (x.sp.pass_bits[1] << 16), batch_file(b)};
  }
  const uint64_t tile_keys = (uint64_t)mgc::GROUP_BLOCK * mgc::GROUP_KPT_NARROW0P;
  // Y has to hold the words of all files of a batch at once.  Where the arena cannot grow to the budget the budget is halved, down to
  // single files (which fit the Y every count has).  Nothing uses Y at this point: the probe file's kernels have been joined.
  uint64_t budget = sw.group_batch_bytes;
  std::vector<mgc::Batch> batches;
  for (;;) {
    batches = mgc::group_plan_batches(bf, budget, sw.group_batch_files, tile_keys);
    const size_t need = std::max<size_t>(y_base_bytes, (size_t)mgc::group_batches_y_bytes(batches));
    if (s->buf[S::B_Y].cap >= need) break;
    const hipError_t e = s->ensure(S::B_Y, need);
    if (e == hipSuccess) break;
    (void)hipGetLastError();
    if (need <= y_base_bytes) HIP_TRY(s, e);
    budget /= 2;
  }
  Y = reinterpret_cast<unsigned char *>(s->buf[S::B_Y].p);
  halt[0] = Y;
  if (sw.finish_trace) {
    uint32_t ne = 0, shared = 0;
    for (const mgc::BatchFile &f : bf) ne += f.eligible && f.n;
    for (const mgc::Batch &bt : batches) if (bt.files.size() > 1) shared += (uint32_t)bt.files.size();
    fprintf(stderr, "[finish] grouping passes: %u files take the batched form, %u of them share launches, %zu batches, %llu bytes of the pass buffer "
                    "(budget %llu), 5-byte mask %x, headers %d\n", ne, shared, batches.size(),
            (unsigned long long)mgc::group_batches_y_bytes(batches), (unsigned long long)budget, soa_hi_mask, d_nhdrs && d_nws ? 1 : 0);
  }
  size_t table_bytes = 0, nbatch = 0;
  for (const mgc::Batch &bt : batches) if (bt.files.size() > 1) { table_bytes += mgc::group_batch_table_bytes((uint32_t)bt.files.size()); nbatch++; }
  if (!nbatch) return MGC_OK;
  // device: [16 bytes of control words per batch, zeroed][the tables]
  const size_t ctl_bytes = (nbatch * 16 + 255) / 256 * 256;
  HIP_TRY(s, s->ensure(S::B_GROUP_BATCH, ctl_bytes + table_bytes));
  unsigned char *d_gb = reinterpret_cast<unsigned char *>(s->buf[S::B_GROUP_BATCH].p);
  HIP_TRY(s, hipMemsetAsync(d_gb, 0, ctl_bytes, st));
  h_batch_tables.assign(table_bytes, 0);
  size_t at = 0, bi = 0;
  std::vector<mgc::GroupFile> gf;
  for (const mgc::Batch &bt : batches) {
    if (bt.files.size() < 2) continue;
    const uint32_t lead = bt.files[0].file;
    gf.clear();
    for (const mgc::BatchSlot &sl : bt.files) {
      gf.push_back(group_desc(sl.file));
      gf.back().alt = (void *)(Y + sl.y_off);
      gf.back().pass_events = nullptr;
    }
    mgc::GroupBatch gb;
    gb.files = gf.data(); gb.nfiles = (uint32_t)gf.size();
    gb.d_table = d_gb + ctl_bytes + at; gb.h_table = h_batch_tables.data() + at;
    gb.d_ctl = reinterpret_cast<uint32_t *>(d_gb + 16 * bi);
    gb.d_error = d_err; gb.st = st;
    gb.pass_events = s->profiling ? &pass_ev[(size_t)lead * ev_per_file] : nullptr;
    HIP_TRY(s, mgc::launch_group_narrow_batch(gb));
    for (size_t j = 0; j < gf.size(); j++) {
      FilePlan &x = plan.files[bt.files[j].file];
      x.tr_a = gf[j].tr_a; x.tr_b = gf[j].tr_b;
      x.passes = 2; x.narrowed = true; x.batch_lead = (int)lead;
      sort_launch_groups++;
    }
    at += mgc::group_batch_table_bytes(gb.nfiles); bi++;
  }
  return MGC_OK;
}

int Count::group_all() {
  TRY(group_batches());
  for (uint32_t b = 0; b < nb; b++) if ((int)b != probe && plan.files[b].batch_lead < 0) TRY(group_file(b));   // (the probe file went first)
  tm.end(MGC_STAGE_SORT);
  tm.begin(MGC_STAGE_RLE);
  // the small statistics kernels of all files back to back: they run beside each other
  for (uint32_t b = 0; b < nb; b++) if ((int)b != probe) TRY(stats_file(b));
  HIP_TRY(s, hipMemcpyAsync(s->h_stats, d_stats, sizeof(uint64_t) * 3 * (size_t)nb, hipMemcpyDeviceToHost, st));
  HIP_TRY(s, hipStreamSynchronize(st));
  for (uint32_t b = 0; b < nb; b++) if ((int)b != probe) take_stats(b);
  return huge_setup();
}

// Round 6: the streaming kernels of different files on up to FOUR streams, each with a second buffer of its own.  One gigantic sub-bucket
// (a repeat family's k-mers: 266 K keys at 30x of a 10 % repeat genome) occupies ONE workgroup for ~600 us; with every file's streaming
// launch queued on one stream those tails added up to 39 ms of a 57 ms count stage (profiles/r06y: BASELINE config 3's read shape at
// 10 Gbp) while the device had room for all of them at once.  MGC_HUGE_STREAMS=1: one stream (round 5).
// (The streams are created on first need, behind all the others: HIP maps streams onto a few hardware queues in creation order, and
// three more of them created at mgc_open put the two count streams on ONE queue -- their kernels no longer ran side by side, the judged
// count stage went 25.4 -> 28.8 ms, profiles/r06_ab_runs.txt r06z.  Needed only where several files hold a GIGANTIC sub-bucket: the many
// slightly oversized ones of an ordinary file -- 615 of up to 1946 keys in a dense file of the judged workload -- are short.)
int Count::huge_setup() {                                // once the files' statistics are back
  uint32_t files_gigantic = 0;
  for (uint32_t b = 0; b < nb; b++) if (plan.files[b].size && s->h_stats[3 * (size_t)b + 1] != 0 && s->h_stats[3 * (size_t)b] > 16384) files_gigantic++;
  if (files_gigantic && sw.huge_slices) {
    HIP_TRY(s, s->ensure(S::B_HWS0, hws_bytes));
    hws[0] = s->buf[S::B_HWS0].p;
  }
  const int want = (int)std::min<uint64_t>((uint64_t)sw.huge_streams, (uint64_t)NH);
  if (!fork_huge || want <= 1 || files_gigantic < 2) return MGC_OK;
  for (int i = 1; i < want; i++) {
    if (!s->stream_h[i - 1] && hipStreamCreateWithFlags(&s->stream_h[i - 1], hipStreamNonBlocking) != hipSuccess) { s->stream_h[i - 1] = nullptr; (void)hipGetLastError(); }
    if (!s->stream_h[i - 1]) break;
    const int id = S::B_Y2 + (i - 1);
    HIP_TRY(s, s->ensure(id, kbytes * plan.max_bucket));
    hstream[i] = s->stream_h[i - 1];
    halt[i] = reinterpret_cast<unsigned char *>(s->buf[id].p);
    if (sw.huge_slices) { HIP_TRY(s, s->ensure(S::B_HWS0 + i, hws_bytes)); hws[i] = s->buf[S::B_HWS0 + i].p; }
    n_huge_streams = i + 1;
  }
  return MGC_OK;
}

int Count::huge_sync_all() {                             // (the host waits for every streaming kernel: Y and its siblings are free)
  for (int i = 0; i < n_huge_streams; i++) HIP_TRY(s, hipStreamSynchronize(hstream[i]));
  return MGC_OK;
}

int Count::huge_join_all() {                             // (st is ordered behind every streaming kernel)
  for (int i = 0; i < n_huge_streams; i++) {
    HIP_TRY(s, hipEventRecord(s->ev_join, hstream[i]));
    HIP_TRY(s, hipStreamWaitEvent(st, s->ev_join, 0));
  }
  return MGC_OK;
}

// ---- D. finish one file: LDS sort + count, or the full-sort fallback ----
int Count::finish_file(uint32_t b) {
  FilePlan &x = plan.files[b];
  x.fallback = false;
  if (x.size == 0) return MGC_OK;
  bool stream = false, unordered = false;
  TRY(oversized_streams(b, &stream));
  if (x.nlarge > 0 && !stream && (x.k96 || x.kind == Group::NARROW)) TRY(widen_back(b, &unordered));
  // whole keys in (low digit : high digit) order whose oversized sub-buckets nothing streams: the stable sort of all bits
  if (x.kind == Group::WIDE && x.nlarge > 0 && !stream) unordered = true;
  if ((x.maxsub <= plan.cap || stream) && !unordered) return count_file(b, stream);
  return fallback_file(b, unordered);
}

// Sub-buckets above the persistent kernels' capacity (a k-mer repeated thousands of times, a dense corner of the key space) are streamed
// through a large hash table, in several suffix ranges if their distinct k-mers do not fit at once.  Only a gigantic one is asked about
// first (one pass must do), before anything touches the file.
int Count::oversized_streams(uint32_t b, bool *stream) {
  const FilePlan &x = plan.files[b];
  *stream = mgc::finish_uses_hash(kw, low(x)) && x.nlarge > 0;
  if (*stream && x.maxsub > sw.stream_max && kw == 2) {
    *stream = false;                                     // no probe for 16-byte keys: a sub-bucket that large takes the sort
  } else if (*stream && x.maxsub > sw.stream_max) {
    uint32_t h_fail[3] = {0, 0, 0};                      // [0] answer, [2] most distinct suffixes met (diagnostics)
    HIP_TRY(s, hipMemsetAsync(d_err + 4, 0, 12, st));
    HIP_TRY(s, mgc::launch_finish_probe(finish_desc(b, true, st, 0), sw.stream_max, d_err + 4));
    HIP_TRY(s, hipMemcpyAsync(h_fail, d_err + 4, 12, hipMemcpyDeviceToHost, st));
    HIP_TRY(s, hipStreamSynchronize(st));
    *stream = (h_fail[0] == 0);
    if (sw.finish_trace)
      fprintf(stderr, "[finish] bucket %u: largest sub-bucket %llu > %llu, up to %u distinct in one: %s\n", b,
              (unsigned long long)x.maxsub, (unsigned long long)sw.stream_max, h_fail[2],
              *stream ? "streamed through the hash tables" : "too many distinct: stable-sort fallback");
  } else if (sw.finish_trace && x.maxsub > plan.cap) {
    fprintf(stderr, "[finish] bucket %u: largest sub-bucket %llu > %llu: %s\n", b, (unsigned long long)x.maxsub,
            (unsigned long long)plan.cap, *stream ? "streamed through the hash tables" : "stable-sort fallback");
  }
  return MGC_OK;
}

// An oversized sub-bucket that nothing streams: the LDS sort / the stable-sort fallback want whole k-mers back.  K96 records are widened
// in their own (16 bytes per k-mer) region and the file goes on as a launch_group_wide file; a narrowed file's words are widened
// back by sub-bucket and the file is whole keys from then on.  Both go through Y, the streaming kernels' second buffer.
int Count::widen_back(uint32_t b, bool *unordered) {
  FilePlan &x = plan.files[b];
  if (need_join) TRY(huge_sync_all());
  forked = false;
  if (x.k96) {
    const unsigned __int128 fb = (unsigned __int128)b << rem_bits;
    HIP_TRY(s, mgc::launch_widen_k96(seg(b), x.size, (uint64_t)fb, (uint64_t)(fb >> 64), (void *)Y, st));
  } else {
    HIP_TRY(s, mgc::launch_widen_groups(seg(b), d_substart + x.sbase, x.ngf(), (uint64_t)b << rem_bits, low(x), (void *)Y, st, x.tr_a, x.tr_b));
  }
  HIP_TRY(s, hipMemcpyAsync(seg(b), Y, kbytes * x.size, hipMemcpyDeviceToDevice, st));
  if (x.k96) {
    x.k96 = false;
    prof.k96_widened_files++;
    return MGC_OK;
  }
  x.kind = Group::SORT;
  *unordered = x.tr_a != 0;        // grouped, but not in key order: only the stable sort of all bits can take it from here
  // (the coarser plan's oversized list was cut at ITS capacity: the whole-key kernels would miss the sub-buckets in between)
  if (x.stream) { x.stream = false; *unordered = true; }
  cnt_extra.emplace_back();        // the back half of its region holds k-mers again: counts of its own
  HIP_TRY(s, cnt_extra.back().ensure(sizeof(uint32_t) * x.size));
  x.cnt = reinterpret_cast<uint32_t *>(cnt_extra.back().p);
  return MGC_OK;
}

// The streaming kernel of a file's oversized sub-buckets goes to a second stream: it touches other sub-buckets than the persistent
// kernel, and one gigantic sub-bucket occupies ONE workgroup for hundreds of microseconds -- beside the persistent kernels of this and
// the next files that tail costs nothing.  The persistent kernels of odd files go to the second stream too, so that the tail of one
// file's launch overlaps the head of the next: finish stage 58.5 -> 54.2 ms per 10 Gbp.  All streaming kernels stay on stream2: they
// share one second buffer.
// What the count-stage launchers are told about file b (mgc_device.h, FinishFile).  stream: its oversized list goes through the streaming
// kernels, on streaming stream hsel with that stream's second buffer and workspace; fst: where its persistent kernels go.
mgc::FinishFile Count::finish_desc(uint32_t b, bool stream, hipStream_t fst, int hsel) const {
  const FilePlan &x = plan.files[b];
  mgc::FinishFile f;
  f.keys = seg(b); f.alt = halt[hsel];
  f.layout = x.kind == Group::NARROW ? mgc::FinishKeys::NARROW32 : x.k96 ? mgc::FinishKeys::K96 : kw == 2 ? mgc::FinishKeys::WHOLE16 : mgc::FinishKeys::WHOLE8;
  f.starts = d_substart + x.sbase; f.ng = x.ngf(); f.low_bits = low(x); f.tr_a = x.tr_a; f.tr_b = x.tr_b;
  f.n_keys = x.size; f.max_sub = x.maxsub;
  f.cnt_tmp = x.cnt; f.group_distinct = d_group + x.gbase;
  f.large_list = d_large + x.gbase; f.n_large = x.nlarge; f.stream = stream;
  f.nonempty_list = nz_list(x); f.nonempty_count = d_stats + 3 * (size_t)b + 2;
  // (the distinct-sized count's retry list: behind the file's oversized list -- a sub-bucket is on one of them at most)
  f.retry_list = x.stream ? d_large + x.gbase + x.nlarge : d_nz + x.gbase; f.retry_count = d_retrycnt + b;
  f.stream_cap = x.stream ? mgc::finish_stream_capacity() : 0;
  f.huge_ws = hws[hsel]; f.huge_ws_bytes = hws_bytes; f.huge_ws_keys = plan.max_bucket; f.d_error = d_err;
  f.st = fst; f.st_huge = hstream[hsel];
  f.hash_multi = sw.hash_multi; f.hash_dbg = sw.hash_dbg;
  return f;
}

int Count::count_file(uint32_t b, bool stream) {
  const FilePlan &x = plan.files[b];
  const bool on_second = fork_huge && (b & 1u);
  if ((stream || on_second) && fork_huge && !forked) {   // everything the forked kernels read is complete at this point of st
    HIP_TRY(s, hipEventRecord(s->ev_fork, st));
    for (int i = 0; i < n_huge_streams; i++) HIP_TRY(s, hipStreamWaitEvent(hstream[i], s->ev_fork, 0));
    forked = need_join = true;
  }
  hipStream_t fst = on_second ? s->stream2 : st;
  const int hsel = (stream && x.nlarge > 0 && n_huge_streams > 1) ? (huge_next++ % n_huge_streams) : 0;
  const bool narrow = x.kind == Group::NARROW;
  if (s->profiling) {
    fin_ev.emplace_back(); (void)hipEventCreate(&fin_ev.back().first); (void)hipEventCreate(&fin_ev.back().second);
    (void)hipEventRecord(fin_ev.back().first, fst);
    fin_keys += x.size;
    fin_in_bytes += x.size * (narrow ? 4u : (x.k96 ? 12u : (uint64_t)kbytes));
    fin_narrow = fin_narrow || narrow;
  }
  HIP_TRY(s, mgc::launch_finish_file(finish_desc(b, stream, fst, hsel)));
  if (s->profiling) (void)hipEventRecord(fin_ev.back().second, fst);
  if ((size_t)nb + b < s->pack_ev.size()) {              // (the packing chain waits for them: pack_step)
    HIP_TRY(s, hipEventRecord(s->pack_ev[b], fst));
    pack_ev2[b] = stream && x.nlarge > 0 && hstream[hsel] != fst;          // ... the streaming launch of its oversized list
    if (pack_ev2[b]) HIP_TRY(s, hipEventRecord(s->pack_ev[(size_t)nb + b], hstream[hsel]));
  }
  return MGC_OK;
}

// a sub-bucket does not fit in LDS (heavily repeated k-mers): finish this file the long way
int Count::fallback_file(uint32_t b, bool unordered) {
  FilePlan &x = plan.files[b];
  x.fallback = true;
  if (need_join) TRY(huge_sync_all());                   // the sort below uses Y, the streaming kernels' second buffer
  forked = false;                                        // ... and the next streaming kernel must wait for that sort
  if (low(x) || unordered) {
    // LSD order: the low bits cannot be sorted after the top bits, so the whole key is redone
    int in_alt = 0;
    HIP_TRY(s, mgc::launch_radix_sort(seg(b), (void *)Y, x.size, kw, full, sort_ws, sort_ws_bytes - 256, d_err, &in_alt, st, nullptr));
    if (in_alt) HIP_TRY(s, hipMemcpyAsync(seg(b), Y, kbytes * x.size, hipMemcpyDeviceToDevice, st));
  }
  uint64_t distinct = 0;
  HIP_TRY(s, mgc::launch_rle_count(seg(b), x.size, kw, rle_ws, st));
  HIP_TRY(s, mgc::rle_read_total(rle_ws, &distinct, st));
  HIP_TRY(s, hipMemsetAsync(d_group + x.gbase, 0, sizeof(uint64_t) * x.slots, st));
  HIP_TRY(s, hipMemcpyAsync(d_group + x.gbase, &distinct, sizeof(uint64_t), hipMemcpyHostToDevice, st));
  HIP_TRY(s, hipStreamSynchronize(st));
  return MGC_OK;
}

int Count::trace_slices() {                              // what the LAST sliced file on every streaming stream did (diagnostics)
  if (!sw.finish_trace || !hws[0]) return MGC_OK;
  HIP_TRY(s, hipStreamSynchronize(st));
  for (int i = 0; i < n_huge_streams; i++) {
    if (!hws[i]) continue;
    mgc::HugeTrace t;
    HIP_TRY(s, mgc::finish_huge_trace(hws[i], plan.max_bucket, &t));
    fprintf(stderr, "[finish] sliced count, stream %d: the last file had %u sub-buckets cut into %u slices; %u of them dense (counted by ranges)\n", i, t.cut, t.slices, t.dense);
  }
  return MGC_OK;
}

// the sub-buckets hash_count_stream_kernel could not hold (more distinct suffixes than its table: low coverage, D ~ N): their numbers
// are on the device -- one small copy brings the counts back, the files that have any get the retry launch
int Count::retry() {
  bool any_stream = false;
  for (const FilePlan &x : plan.files) any_stream = any_stream || (x.stream && !x.fallback && x.size);
  if (!any_stream) return MGC_OK;
  std::vector<uint64_t> h_retry(nb, 0);
  HIP_TRY(s, hipMemcpyAsync(h_retry.data(), d_retrycnt, sizeof(uint64_t) * nb, hipMemcpyDeviceToHost, st));
  HIP_TRY(s, hipStreamSynchronize(st));
  for (uint32_t b = 0; b < nb; b++) {
    const FilePlan &x = plan.files[b];
    if (!x.stream || x.fallback || h_retry[b] == 0) continue;
    prof.stream_retries += h_retry[b];
    HIP_TRY(s, mgc::launch_finish_retry(finish_desc(b, true, st, 0), h_retry[b]));
  }
  return MGC_OK;
}

// ---- E/F. offsets of every sub-bucket in the packed result; G/H. pack ----
int Count::scan_pack() {
  if (s->profiling) { (void)hipEventCreate(&ev_pack[0]); (void)hipEventCreate(&ev_pack[1]); (void)hipEventRecord(ev_pack[0], st); }
  HIP_TRY(s, mgc::launch_finish_scan(d_group, plan.ng_total, s->buf[S::B_GSCAN].p, st));
  HIP_TRY(s, hipMemcpyAsync(&nd, d_group + plan.ng_total, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(s, hipStreamSynchronize(st));
  if (plan.ng_total == 0) nd = 0;
  s->n_distinct = nd;
  if (in.out_keys && in.out_counts && nd <= in.out_cap) {
    // (mgc_count_buckets_into: the packing kernels write the caller's pre-sized result -- no copy out of the arena afterwards)
    s->d_unique = in.out_keys;
    s->d_counts = in.out_counts;
  } else {
    HIP_TRY(s, s->ensure(S::B_UNIQUE, kbytes * nd));
    HIP_TRY(s, s->ensure(S::B_COUNTS, sizeof(uint32_t) * nd));
    s->d_unique = s->buf[S::B_UNIQUE].p;
    s->d_counts = reinterpret_cast<uint32_t *>(s->buf[S::B_COUNTS].p);
  }
  for (uint32_t b = 0; b < nb; b++) TRY(pack_file(b, st));
  return pack_done();
}

int Count::pack_done() {
  if (s->profiling) (void)hipEventRecord(ev_pack[1], st);
  tm.end(MGC_STAGE_RLE);
  prof.stage_launches[MGC_STAGE_RLE] = 4 * nb;
  if (s->profiling) {
    HIP_TRY(s, hipStreamSynchronize(st));
    { float pms = 0; if (hipEventElapsedTime(&pms, ev_pack[0], ev_pack[1]) == hipSuccess) prof.pack_ms = pms; }
    (void)hipEventDestroy(ev_pack[0]); (void)hipEventDestroy(ev_pack[1]);
    finish_profile();
  }
  return MGC_OK;
}

int Count::pack_file(uint32_t b, hipStream_t ps, const uint64_t *d_gate, uint64_t gate_above) {
  const FilePlan &x = plan.files[b];
  if (x.size == 0) return MGC_OK;
  void *sg = seg(b);
  if (x.kind == Group::NARROW) {
    HIP_TRY(s, mgc::launch_compact_groups_narrow(sg, x.cnt, d_substart + x.sbase, d_group + x.gbase, x.ngf(), (uint64_t)b << rem_bits, low(x),
                                                 s->d_unique, s->d_counts, ps, x.tr_a, x.tr_b, nz_list(x), x.nzcount, d_gate, gate_above));
  } else if (!x.fallback && x.k96) {
    const unsigned __int128 fb = (unsigned __int128)b << rem_bits;
    HIP_TRY(s, mgc::launch_compact_groups_k96(sg, x.cnt, d_substart + x.sbase, d_group + x.gbase, x.ngf(), (uint64_t)fb, (uint64_t)(fb >> 64),
                                              s->d_unique, s->d_counts, ps, x.tr_a, x.tr_b, nz_list(x), x.nzcount, d_gate, gate_above));
  } else if (!x.fallback) {
    HIP_TRY(s, mgc::launch_compact_groups(sg, kw, x.cnt, d_substart + x.sbase, d_group + x.gbase, x.ngf(), s->d_unique, s->d_counts, ps,
                                          x.tr_a, x.tr_b, nz_list(x), x.nzcount, d_gate, gate_above));
  } else {                                               // (never early: mgc_pack_plan.hpp, pack_file_ok)
    HIP_TRY(s, mgc::launch_rle_count(sg, x.size, kw, rle_ws, ps));
    HIP_TRY(s, mgc::launch_rle_emit(sg, x.size, kw, rle_ws, s->d_unique, s->d_counts, ps, d_group + x.gbase));
  }
  return MGC_OK;
}

// ---- early packing: a file is packed while the files after it are still being counted ----
// The count kernels are bound by instruction issue, the packing kernels by memory: behind each other each leaves idle what the other
// needs.  Nothing but a file's offset in the result makes them serial, and that is the sum of the distinct k-mers of the files before
// it.  So the files are packed in index order on a third stream (pack_st), file i as soon as its count kernel and those of
// the files before it have ended: a gate and the scan of its slice of d_group with the carry-in base[i] (mgc_finish.hip,
// pack_gate_scan_kernel), then the packing launch of file i - 1 -- one step behind, because the last sub-bucket of a
// file ends at d_group[first slot of the next file], which the next file's scan writes.  d_group ends up as the scan of all files
// leaves it.  What can still go wrong once the chain is queued is decided on the device and is sticky (a file with sub-buckets on the
// retry list, or a result without room: that file and every later one stay untouched); pack_finish then takes the serial path from
// there.  Which counts take it at all, and how much room the result gets beforehand: mgc_pack_plan.hpp.
int Count::pack_events() {                               // once per session: two events per file, behind its count launch(es)
  if (!sw.pack_overlap) return MGC_OK;
  pack_ev2.assign(nb, 0);
  while (s->pack_ev.size() < 2 * (size_t)nb) {
    hipEvent_t e = nullptr;
    HIP_TRY(s, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    s->pack_ev.push_back(e);
  }
  return MGC_OK;
}

int Count::pack_plan() {                                 // the statistics of all files are back, nothing but the probe file is counted
  if (!sw.pack_overlap || s->pack_ev.size() < 2 * (size_t)nb) return MGC_OK;
  std::vector<mgc::PackFile> pf(nb);
  uint32_t listed = 0;
  for (uint32_t b = 0; b < nb; b++) {
    const FilePlan &x = plan.files[b];
    pf[b] = mgc::PackFile{x.size, x.maxsub, x.nlarge, mgc::finish_uses_hash(kw, low(x)), x.fallback};
    listed += x.size && x.nlarge ? 1u : 0u;
  }
  const bool eligible = mgc::pack_overlap_eligible(pf, plan.cap, sw.stream_max, true);
  if (sw.finish_trace) fprintf(stderr, "[finish] early packing: %u files have an oversized list; the count is %s\n", listed, eligible ? "eligible" : "not eligible");
  if (!eligible) return MGC_OK;
  // The stream: the session's input stream, which has a hardware queue to itself (created at mgc_open between the two count streams)
  // and is idle while the caller's own thread counts (mgc_count has waited for everything queued there).  Not while the worker
  // thread counts a batch: the caller is then pushing the next one through it.  A stream of its own, created on first need behind
  // all the others, shares a hardware queue with a count stream -- four queues, the note at huge_setup -- and the chain's waits
  // then hold that stream's count kernels back: measured slower than no early packing at all (profiles/pack_overlap_ab.txt).
  // For the same reason not where huge_setup has created further streams for gigantic sub-buckets: one of them may share the
  // chain's queue (not measured).  Decided before the arena is touched: such a count keeps the result buffers it has.
  if (s->worker_active || !s->st_in || n_huge_streams > 1) return MGC_OK;
  pack_st = s->st_in;
  const bool caller = in.out_keys && in.out_counts;
  auto arena_kmers = [&]() { return mgc::pack_buffers_kmers(s->buf[S::B_UNIQUE].cap, s->buf[S::B_COUNTS].cap, kbytes); };
  const double ratio = probe >= 0 ? prof.probe_ratio : (double)sw.pack_ratio / 1000.0;
  const uint64_t est = mgc::pack_estimate(ratio, N, sw.pack_margin);
  const uint64_t want = mgc::pack_arena_want(caller, est, arena_kmers());
  if (want && (s->ensure(S::B_UNIQUE, kbytes * want) != hipSuccess || s->ensure(S::B_COUNTS, sizeof(uint32_t) * want) != hipSuccess))
    (void)hipGetLastError();                             // (the arena cannot grow: what is there has to do)
  early_cap = mgc::pack_capacity(caller, in.out_cap, arena_kmers());
  if (sw.finish_trace) fprintf(stderr, "[finish] early packing: %llu k-mers, %llu distinct expected (%s %.4f, margin %lld/1000), room for %llu%s\n",
                               (unsigned long long)N, (unsigned long long)est, probe >= 0 ? "probe file's ratio" : (sw.pack_ratio ? "MGC_PACK_RATIO" : "no probe file: ratio"), ratio, (long long)sw.pack_margin,
                               (unsigned long long)early_cap, caller ? " in the caller's buffers" : "");
  if (early_cap == 0) return MGC_OK;
  if (!s->ev_pack_done && hipEventCreateWithFlags(&s->ev_pack_done, hipEventDisableTiming) != hipSuccess) { s->ev_pack_done = nullptr; (void)hipGetLastError(); return MGC_OK; }
  chain_pos.assign(nb, -1);
  for (uint32_t b = 0; b < nb; b++) if (plan.files[b].size) { chain_pos[b] = (int)chain.size(); chain.push_back(b); }
  uint64_t max_slice = 0;
  for (size_t i = 0; i < chain.size(); i++)
    max_slice = std::max(max_slice, (i + 1 < chain.size() ? plan.files[chain[i + 1]].gbase : plan.ng_total) - plan.files[chain[i]].gbase);
  HIP_TRY(s, s->ensure(S::B_PACK_STATE, mgc::pack_state_bytes((uint32_t)chain.size(), max_slice)));
  d_pstate = reinterpret_cast<uint64_t *>(s->buf[S::B_PACK_STATE].p);
  s->d_unique = caller ? in.out_keys : s->buf[S::B_UNIQUE].p;
  s->d_counts = caller ? in.out_counts : reinterpret_cast<uint32_t *>(s->buf[S::B_COUNTS].p);
  HIP_TRY(s, mgc::launch_pack_state_init(d_pstate, early_cap, pack_st));
  early = true;
  return MGC_OK;
}

int Count::pack_step(uint32_t b) {                       // file b's count launch is queued (the probe file's ended long ago)
  if (!early || chain_pos[b] < 0) return MGC_OK;
  const FilePlan &x = plan.files[b];
  const uint64_t i = (uint64_t)chain_pos[b], m = chain.size();
  hipStream_t ps = pack_st;
  HIP_TRY(s, hipStreamWaitEvent(ps, s->pack_ev[b], 0));
  if (pack_ev2[b]) HIP_TRY(s, hipStreamWaitEvent(ps, s->pack_ev[(size_t)nb + b], 0));
  const uint64_t g1 = i + 1 < m ? plan.files[chain[i + 1]].gbase : plan.ng_total;
  HIP_TRY(s, mgc::launch_pack_gate_scan(d_group + x.gbase, g1 - x.gbase, d_pstate, (uint32_t)m, (uint32_t)i, x.stream ? d_retrycnt + b : nullptr,
                                        i + 1 == m ? d_group + plan.ng_total : nullptr, false, ps));
  if (i > 0) TRY(pack_file(chain[i - 1], ps, d_pstate, mgc::pack_gate_threshold(i - 1, m)));
  if (i + 1 == m) TRY(pack_file(b, ps, d_pstate, mgc::pack_gate_threshold(i, m)));
  return MGC_OK;
}

// The session stream is behind every count kernel here.  One copy brings the chain's state back: the first deferred file q and every
// file's place in the result.  q == m: everything is packed.  Otherwise the serial path from q on: the retry launches, the scans of the
// files from q on (carry-in base[q]), the result grown if it has to be, and the packing launches of the files the chain left out --
// of ALL files if the result moved (the packing launches do not modify their source).
int Count::pack_finish() {
  const uint64_t m = chain.size(), none = mgc::pack_state_none();
  if (s->profiling) { (void)hipEventCreate(&ev_pack[0]); (void)hipEventCreate(&ev_pack[1]); (void)hipEventRecord(ev_pack[0], st); }
  HIP_TRY(s, hipEventRecord(s->ev_pack_done, pack_st));
  HIP_TRY(s, hipStreamWaitEvent(st, s->ev_pack_done, 0));
  std::vector<uint64_t> h(3 + m + 1, 0);
  HIP_TRY(s, hipMemcpyAsync(h.data(), d_pstate, sizeof(uint64_t) * h.size(), hipMemcpyDeviceToHost, st));
  HIP_TRY(s, hipStreamSynchronize(st));
  const uint64_t q = h[0] == none ? m : std::min<uint64_t>(h[0], m);
  for (uint64_t i = 0; i < m; i++) prof.early_pack_files += mgc::pack_ran_early(i, q, m) ? 1u : 0u;
  prof.early_pack_deferred = (uint32_t)(m - q);
  if (sw.finish_trace) {
    double lo = 2.0, hi = 0.0;                           // (the spread the margin of the estimate is chosen from: mgc_pack_plan.hpp)
    for (uint64_t i = 0; i < q; i++) { const double r = (double)(h[3 + i + 1] - h[3 + i]) / (double)plan.files[chain[i]].size; lo = std::min(lo, r); hi = std::max(hi, r); }
    fprintf(stderr, "[finish] early packing: %llu of %llu files scanned before the last count kernel ended (%u packed), %llu distinct in them, "
                    "distinct / instances per file %.4f .. %.4f\n", (unsigned long long)q, (unsigned long long)m, prof.early_pack_files,
            (unsigned long long)h[3 + q], q ? lo : 0.0, hi);
  }
  if (q == m) {
    nd = h[3 + m];
    s->n_distinct = nd;
    return pack_done();
  }
  TRY(retry());
  if (s->profiling) (void)hipEventRecord(ev_pack[0], st);  // (the retry launches belong to the count, as on the serial path)
  for (uint64_t i = q; i < m; i++) {
    const FilePlan &x = plan.files[chain[i]];
    const uint64_t g1 = i + 1 < m ? plan.files[chain[i + 1]].gbase : plan.ng_total;
    HIP_TRY(s, mgc::launch_pack_gate_scan(d_group + x.gbase, g1 - x.gbase, d_pstate, (uint32_t)m, (uint32_t)i, nullptr,
                                          i + 1 == m ? d_group + plan.ng_total : nullptr, true, st));
  }
  HIP_TRY(s, hipMemcpyAsync(&nd, d_group + plan.ng_total, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(s, hipStreamSynchronize(st));
  s->n_distinct = nd;
  const void *was_keys = s->d_unique; const uint32_t *was_counts = s->d_counts;
  bool moved = false;
  if (in.out_keys && in.out_counts && nd <= in.out_cap) {
    s->d_unique = in.out_keys;
    s->d_counts = in.out_counts;
  } else {
    // (a buffer that grows is a new one, even where the allocator hands the old address out again)
    moved = s->buf[S::B_UNIQUE].cap < std::max<size_t>(kbytes * nd, 256) || s->buf[S::B_COUNTS].cap < std::max<size_t>(sizeof(uint32_t) * nd, 256);
    HIP_TRY(s, s->ensure(S::B_UNIQUE, kbytes * nd));
    HIP_TRY(s, s->ensure(S::B_COUNTS, sizeof(uint32_t) * nd));
    s->d_unique = s->buf[S::B_UNIQUE].p;
    s->d_counts = reinterpret_cast<uint32_t *>(s->buf[S::B_COUNTS].p);
  }
  moved = moved || s->d_unique != was_keys || s->d_counts != was_counts;
  if (moved) prof.early_pack_files = 0;
  for (uint64_t i = moved ? 0 : mgc::pack_late_from(q, m); i < m; i++) TRY(pack_file(chain[i], st));
  return pack_done();
}

void Count::finish_profile() {
  for (auto &pe : fin_ev) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, pe.first, pe.second) == hipSuccess) { prof.finish_ms += ms; prof.finish_launches++; }
    (void)hipEventDestroy(pe.first); (void)hipEventDestroy(pe.second);
  }
  prof.finish_keys = fin_keys;
  prof.finish_bytes = fin_in_bytes + nd * (fin_narrow ? 8u : (uint64_t)kbytes + 4u);
  // which way the gigantic sub-buckets went (the caller has just waited for the stream: every count kernel is done)
  uint32_t h_huge[mgc::FIN_HUGE_STATS] = {};
  if (d_err && hipMemcpy(h_huge, d_err + mgc::FIN_HUGE_STATS_AT, sizeof(h_huge), hipMemcpyDeviceToHost) == hipSuccess) {
    prof.huge_cut += h_huge[0]; prof.huge_slices += h_huge[1]; prof.huge_dense += h_huge[2];
    for (int m = 0; m < 4; m++) prof.huge_repasses[m] += h_huge[3 + m];
    prof.huge_empty_ranges += h_huge[7];
  }
}

// The default path: every file grouped by its top bits, then its sub-buckets sorted and counted in LDS (or streamed through the hash
// tables), then packed.
int Count::count_finish() {
  plan.plan_files();
  probe = plan.choose_probe();
  TRY(finish_buffers());
  soa_hi_mask = plan.soa_mask(!in.keys && s->sfx_mask == 0);
  const bool k96 = plan.k96_layout(!in.keys && s->sfx_mask == 0);
  for (uint32_t b = 0; b < nb; b++) h_meta[nb + b] = plan.files[b].k96 ? 1 : 0;
  TRY(partition(soa_hi_mask != 0, k96));
  // Where the counts of a file's distinct k-mers wait for the packing step (one uint32 per k-mer instance position).  A NARROWED file
  // keeps 4-byte words in the front half of its 8-byte region from the first grouping pass on: the back half is free and takes the
  // counts -- no buffer of its own (35 GB of the 123 GB arena at 10 Gbp; a large first hipMalloc is the slowest thing a freshly started
  // process does, profiles/r03m_e2e_io.txt).  The other files share B_CNT_TMP; a narrowed file that has to be widened back later (a
  // sub-bucket nothing can stream) gets a buffer of its own then.
  uint64_t wide_total = 0;
  for (const FilePlan &x : plan.files) if (x.kind != Group::NARROW) wide_total += x.size;
  HIP_TRY(s, s->ensure(S::B_CNT_TMP, sizeof(uint32_t) * wide_total));
  uint32_t *wide = reinterpret_cast<uint32_t *>(s->buf[S::B_CNT_TMP].p);
  uint64_t at = 0;
  for (uint32_t b = 0; b < nb; b++) {
    FilePlan &x = plan.files[b];
    if (x.kind == Group::NARROW) x.cnt = reinterpret_cast<uint32_t *>(seg(b)) + x.size;
    else { x.cnt = wide + at; at += x.size; }
  }
  tm.begin(MGC_STAGE_SORT);
  TRY(prepare_headers());
  if (s->h_stats_cap < 3 * (size_t)nb) {
    if (s->h_stats) { (void)hipHostFree(s->h_stats); s->h_stats = nullptr; s->h_stats_cap = 0; }
    HIP_TRY(s, hipHostMalloc(reinterpret_cast<void **>(&s->h_stats), sizeof(uint64_t) * 3 * (size_t)nb, hipHostMallocDefault));
    s->h_stats_cap = 3 * (size_t)nb;
  }
  fork_huge = s->stream2 != nullptr;
  hstream[0] = fork_huge ? s->stream2 : st;
  halt[0] = Y;
  hws_bytes = mgc::finish_huge_workspace_bytes(plan.max_bucket);
  TRY(pack_events());
  prof.probe_file = probe;
  if (probe >= 0) TRY(probe_file());
  TRY(group_all());
  TRY(pack_plan());
  for (uint32_t b = 0; b < nb; b++) {
    if ((int)b != probe) TRY(finish_file(b));
    TRY(pack_step(b));
  }
  if (need_join) TRY(huge_join_all());
  TRY(trace_slices());
  if (early) return pack_finish();
  TRY(retry());
  return scan_pack();
}

// ---- block offsets, and the look-back flag ----
int Count::block_offsets() {
  HIP_TRY(s, s->ensure(S::B_BLOCKS, sizeof(uint64_t) * (c.n_prefix + 1)));
  s->d_block_start = reinterpret_cast<uint64_t *>(s->buf[S::B_BLOCKS].p);
  tm.begin(MGC_STAGE_BLOCKS);
  HIP_TRY(s, mgc::launch_block_offsets(s->d_unique, nd, kw, c.w_data, c.n_prefix, s->d_block_start, st));
  tm.end(MGC_STAGE_BLOCKS);
  prof.stage_launches[MGC_STAGE_BLOCKS] = 1;
  uint32_t h_err[3] = {0, 0, 0};
  HIP_TRY(s, hipMemcpyAsync(h_err, d_err, sizeof(h_err), hipMemcpyDeviceToHost, st));
  if (s->profiling) (void)hipEventRecord(ev_all[1], st);
  HIP_TRY(s, hipStreamSynchronize(st));
  if (h_err[0]) { mgc::set_err(&s->err, "radix sort look-back timed out"); return MGC_ETIMEOUT; }
  if (h_err[2]) { mgc::set_err(&s->err, "count stage: the retry table of the distinct-sized count filled up, a sub-bucket was not counted"); return MGC_EHIP; }
  return MGC_OK;
}

void Count::collect_profile() {
  float ms = 0;
  for (int i = 0; i < MGC_NUM_STAGES; i++)
    if (tm.used[i] && hipEventElapsedTime(&ms, tm.ev[i][0], tm.ev[i][1]) == hipSuccess) prof.stage_ms[i] = ms;
  if (hipEventElapsedTime(&ms, ev_all[0], ev_all[1]) == hipSuccess) prof.total_ms = ms;
  // (from the plan of all bits, whichever path ran)
  prof.stage_launches[MGC_STAGE_SORT] = sort_launch_groups * (full.num_passes + 2);
  for (uint32_t b = 0; b < nb; b++) {
    const FilePlan &x = plan.files[b];
    if (x.size == 0) continue;
    // (a file of a batched launch counts as a launch of its own here -- the fields keep their meaning of one per file and pass -- and
    // the batch's first file carries the launch's duration; the kernel launches themselves: pass_kernel_launches)
    const bool follower = x.batch_lead >= 0 && (uint32_t)x.batch_lead != b;
    for (uint32_t p = 0; p < x.passes; p++) {
      hipEvent_t *pe = &pass_ev[(size_t)b * ev_per_file + 2 * p];
      ms = 0;
      if (!follower && hipEventElapsedTime(&ms, pe[0], pe[1]) != hipSuccess) continue;
      if (!follower) prof.pass_kernel_launches[p ? 1 : 0]++;
      prof.sort_pass_ms_total += ms;
      prof.sort_pass_launches++;
      prof.sort_pass_keys += x.size;
      const int pi = p ? 1 : 0;
      prof.pass_ms[pi] += ms;
      prof.pass_launches[pi]++;
      prof.pass_keys[pi] += x.size;
      if (x.narrowed && !p) prof.narrow_digit_widths |= 1u << (x.tr_a ? x.tr_a : x.sp.pass_bits[0]);
      prof.pass_bytes[pi] += x.size * (x.narrowed ? (p ? 8u : (soa_hi_mask ? 9u : 12u)) : (x.k96_passes ? 24u : 2u * kbytes));
    }
  }
  for (auto &e : pass_ev) (void)hipEventDestroy(e);
  (void)hipEventDestroy(ev_all[0]); (void)hipEventDestroy(ev_all[1]);
  // (an elapsed-time query on an event pair a small file never recorded fails, harmlessly -- but the runtime keeps the error for the
  // thread's next hipGetLastError(): the CLI's -V on a batched count failed in the run store's first launch that way)
  (void)hipGetLastError();
}

int Count::run() {
  TRY(compress_bases());
  if (s->profiling) { (void)hipEventCreate(&ev_all[0]); (void)hipEventCreate(&ev_all[1]); (void)hipEventRecord(ev_all[0], st); }
  TRY(histogram());
  TRY(buffers());
  TRY(use_finish ? count_finish() : count_full());
  TRY(block_offsets());
  if (s->profiling) collect_profile();
  return MGC_OK;                                         // the caller marks the session counted (a batch is not the result yet)
}
}  // namespace

// One pass over bases that are resident in HBM (s->d_bases / s->n_bases), or over the keys of in.keys: results stay in HBM.
int mgc::count_device(mgc_session *s, const CountInput &in) {
  s->join_prepare();
  s->free_result();
  HIP_TRY(s, hipSetDevice(s->device));
  const uint32_t bucket_bits = in.keys ? in.bucket_bits : plan_bucket_bits(s->cfg, s->sw, s->n_bases);
  memset(&s->prof, 0, sizeof(s->prof));
  s->prof.probe_file = -1;
  Count count(s, in, bucket_bits);
  return count.run();
}
