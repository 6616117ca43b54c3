// mgc_session.hpp -- the session object behind include/meryl_gpu_count.h and the helpers its translation units
// (mgc_api.cpp: configuration, open / close, count, results; mgc_input.cpp: input staging + batches; mgc_textfile.cpp: whole-file readers; mgc_count.cpp: counting; mgc_stream.cpp: delivery of the result,
// database streaming; mgc_eval.cpp: operations over databases) share.  The owning device buffer they use, mgc::DBuf, is mgc_devbuf.hpp's;
// the session's arena below is a different thing (grow-only for the session's life, traced by MGC_IO_TRACE).  Internal.
#pragma once

#include "../../include/meryl_gpu_count.h"
#include "mgc_bam_walk.hpp"
#include "mgc_clock.hpp"
#include "mgc_devbuf.hpp"
#include "mgc_device.h"
#include "mgc_gzip_crc.hpp"
#include "mgc_input.hpp"

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

namespace mgc {
// last error of the calling thread (mgc_last_error(NULL)); defined in mgc_api.cpp
std::string &thread_last_error();
// simple mode swaps the configured block geometry for countSimple's (mgc_api.cpp); false + thread error when k is too small
bool effective_geometry(mgc_count_config *c);

inline void set_err(std::string *dst, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (dst) {                                         // a session's error string is written by its worker thread and by the pushing thread
    static std::mutex mu;
    std::lock_guard<std::mutex> g(mu);
    *dst = buf;
  }
  thread_last_error() = buf;
}
}  // namespace mgc

#define HIP_TRY(s, expr)                                                                         \
  do {                                                                                           \
    hipError_t e__ = (expr);                                                                     \
    if (e__ != hipSuccess) {                                                                     \
      mgc::set_err((s) ? &(s)->err : nullptr, "%s:%d: %s -> %s", __FILE__, __LINE__, #expr,      \
                   hipGetErrorString(e__));                                                      \
      return (e__ == hipErrorOutOfMemory) ? MGC_ENOMEM : MGC_EHIP;                               \
    }                                                                                            \
  } while (0)

struct mgc_session {
  mgc_count_config cfg;
  int              device = -1;
  hipStream_t      stream = nullptr;
  uint64_t         sfx_mask = 0, sfx_test = 0;   // count-suffix= filter (0, 0: none)
  mgc::Switches    sw;                   // the MGC_* switches of the count path, read once by mgc_open (mgc_device.h)
  static constexpr int HUGE_EXTRA = 3;
  hipStream_t      stream_h[HUGE_EXTRA] = {nullptr, nullptr, nullptr};   // more streams for the streaming kernels of oversized sub-buckets (count_device)
  hipStream_t      stream2 = nullptr;    // the streaming hash-count of a file's oversized sub-buckets runs beside its persistent kernel
  hipEvent_t       ev_fork = nullptr, ev_join = nullptr;
  // early packing (mgc_count.cpp, Count::pack_plan): the events behind every file's count launches, created once, and the one behind
  // the packing chain's last launch.  The chain itself runs on st_in (below), which is idle while the caller's own thread counts
  std::vector<hipEvent_t> pack_ev;
  hipEvent_t       ev_pack_done = nullptr;
  uint64_t        *h_stats = nullptr;    // pinned: per file {largest sub-bucket, oversized sub-buckets, non-empty sub-buckets}
  size_t           h_stats_cap = 0;
  std::string      err;

  // input: what count_device reads (a staging buffer of this session, or the caller's device buffer)
  const uint8_t    *d_bases = nullptr;
  uint64_t          n_bases = 0;
  bool              borrowed = false;

  // result
  bool      counted = false;
  uint64_t  n_instances = 0, n_distinct = 0;
  uint64_t  file_instances[MGC_NUM_FILES];
  void     *d_unique = nullptr;           // uint64[D] (k <= 32) or {lo,hi}[D] (k > 32)
  uint32_t *d_counts = nullptr;
  uint64_t *d_block_start = nullptr;
  uint32_t  key_words = 1;

  // device arena: buffers survive between mgc_count calls (grow-only), so a
  // repeated count does not pay hipMalloc/hipFree of tens of GB every time
  struct Buf { void *p = nullptr; size_t cap = 0; };
  enum { B_PART_WS, B_META, B_X, B_Y, B_SORT_WS, B_RLE_WS, B_UNIQUE, B_COUNTS, B_BLOCKS, B_HPC, B_HPC_WS,
         B_SUBSTART, B_GROUPS, B_GSCAN, B_CNT_TMP, B_LARGE, B_NONEMPTY, B_STAGE0, B_STAGE1, B_TEXT_IN0, B_TEXT_IN1, B_TEXT_WS,
         B_TEXT_STATE, B_RK, B_RC, B_R2K, B_R2C, B_MERGE_WS, B_SORT_HDRS, B_FINE, B_NARROW_WS, B_Y2, B_Y3, B_Y4, B_HWS0, B_HWS1, B_HWS2, B_HWS3,
         B_PACKED /* the count's packed base stream: 2-bit codes + invalid-base masks, written by the histogram, read by the partition */,
         B_GROUP_BATCH /* the batched grouping launches' control words and descriptor tables (mgc_count.cpp, group_batches) */,
         B_BAM_SEG0, B_BAM_SEG1 /* the segment tables of the two BAM pieces in flight (mgc_bam_walk.hpp) */,
         B_GZ_SYM0, B_GZ_SYM1 /* the unresolved symbols of the two gzip pieces in flight (mgc_gzip.hip) */, B_GZ_TAB0, B_GZ_TAB1 /* their CRC
         piece tables and results */, B_GZ_WIN /* two 32 KiB windows, ping-pong, and the error word */,
         B_PACK_STATE /* early packing: the gate's state and the files' places in the result (mgc_device.h, launch_pack_gate_scan) */, B_NUM };
  Buf buf[B_NUM];
  size_t arena_bytes() const { size_t t = 0; for (const auto &b : buf) t += b.cap; return t; }
  double tr_alloc = 0;                   // seconds inside hipMalloc / hipFree of the arena (MGC_IO_TRACE)
  uint64_t tr_alloc_bytes = 0;
  hipError_t ensure(int which, size_t bytes) {
    Buf &b = buf[which];
    if (bytes < 256) bytes = 256;
    if (b.cap >= bytes) return hipSuccess;
    const double t0 = mgc::now_s();
    if (b.p) { (void)hipFree(b.p); b.p = nullptr; b.cap = 0; }
    hipError_t e = hipMalloc(&b.p, bytes);
    if (e == hipSuccess) b.cap = bytes;
    tr_alloc += mgc::now_s() - t0;
    tr_alloc_bytes += bytes;
    return e;
  }
  void free_arena() { for (auto &b : buf) { if (b.p) (void)hipFree(b.p); b.p = nullptr; b.cap = 0; } }
  // Grows a staging buffer whose first `keep` bytes must survive (device-to-device copy on stream `on`, synchronised).
  // Growth is by 4x up to the batch size, and the old buffer is NOT freed here: hipFree waits for the whole device -- i.e.
  // for the batch the worker thread is counting -- and twenty growth steps of that cost 4.9 of the 5.2 s a 6 Gbp host
  // push took (profiles/r02i).  The old buffers go when the count is done (free_garbage).
  std::vector<void *> garbage;
  hipError_t ensure_preserve(int which, size_t bytes, size_t keep, hipStream_t on) {
    Buf &b = buf[which];
    if (b.cap >= bytes) return hipSuccess;
    struct Tm { double *acc; double t0; Tm(double *a) : acc(a), t0(mgc::now_s()) {} ~Tm() { *acc += mgc::now_s() - t0; } } tm_(&tr_grow);
    size_t want = b.cap * 4;
    const size_t full = batch_limit ? (size_t)batch_limit + 4 * PIN_CHUNK : 0;       // what a whole batch needs
    if (full && want > full && full >= bytes) want = full;
    if (want < bytes) want = bytes;
    void *np = nullptr;
    hipError_t e = hipMalloc(&np, want);
    if (e != hipSuccess && want > bytes) { want = bytes; e = hipMalloc(&np, want); }
    if (e != hipSuccess) return e;
    if (b.p && keep) e = hipMemcpyAsync(np, b.p, keep, hipMemcpyDeviceToDevice, on);
    if (e == hipSuccess) e = hipStreamSynchronize(on);
    if (b.p) garbage.push_back(b.p);
    b.p = np; b.cap = want;
    return e;
  }
  void free_garbage() { for (void *p : garbage) (void)hipFree(p); garbage.clear(); }

  // ---- input staging -------------------------------------------------------------------------------------------
  // Everything pushed (bases from the host, text parsed on the device) lands in ONE base stream in HBM, stage[fill],
  // '.' after every sequence.  The device-side parse state (B_TEXT_STATE) holds the stream's length: text chunks
  // advance it on the device, plain appends set it; the host's fill_len is exact unless text was parsed since the last
  // read-back (len_inexact) -- then it is an upper bound.  All of it runs on st_in, a stream of its own, so that
  // uploads and parsing overlap the count of the previous batch (which runs on `stream`, from the worker thread).
  static constexpr size_t TEXT_CHUNK = 32u << 20;
  static constexpr size_t PIN_CHUNK  = 32u << 20;
  hipStream_t st_in = nullptr;
  bool        state_ready = false;       // parse state allocated and reset
  int         fill = 0;
  uint64_t    fill_len = 0;
  bool        len_inexact = false;
  bool        input_seen = false;
  // the open file: text (mgc_begin_text; a plain gzip file is one) or BAM (mgc_begin_bam; format TEXT_BAM) -- one "open file" state for
  // both: the cut inside a file, the rollback point in the device's parse state
  bool        text_open = false, text_cut_in_file = false;
  int         text_format = 0;
  static constexpr int TEXT_BAM = -1;                      // (not one of MGC_TEXT_FASTA / _FASTQ / _SAM)
  static constexpr int TEXT_RING_MAX = mgc::InputRing::FILE_SLOTS_MAX;
  mgc::InputRing in;                                      // the two piece slots every route's pieces go through (mgc_input.hpp)
  // BAM: pieces are inflated BAM bytes, walked on the host, decoded on the device (mgc_bam.hip) from a segment table that travels with the piece
  mgc::BamWalker bam_walker;
  std::vector<mgc::BamSegment> bam_segs;                 // of the piece being walked
  double      tr_bam_walk = 0;                           // seconds in the walker, this file (MGC_IO_TRACE)
  // gzip (mgc_push_text_gzip_file): pieces come with the symbols of an unresolved prefix; they are resolved on the device before the
  // parse kernels read them, and the CRC-32 of every member is computed there over the resolved text and held against its trailer here
  int         gz_win = 0;                                 // which of the two windows holds the text before the next piece
  mgc::GzCrcLedger gz;                                    // (mgc_gzip_crc.hpp)
  double      tr_gz_copy = 0, tr_gz_collect = 0, tr_gz_wait = 0;   // seconds of this file's submits in the symbol copy, in folding the CRCs, waiting for the device (MGC_IO_TRACE)
  // host-pushed bases: two pinned chunks, the upload of one overlaps the filling of the other
  char       *pin[2] = {nullptr, nullptr};
  size_t      pin_len = 0;
  int         pin_cur = 0;
  hipEvent_t  pin_ev[2] = {nullptr, nullptr};
  bool        pin_used[2] = {false, false};

  // ---- out-of-core batches (the analogue of writeBatch's spill, merylOp-countThreads.C:323-379, and of
  // merylBlockWriter::finish() merging the iterations) ---------------------------------------------------------
  // When the staged bases reach batch_limit, everything up to the last sequence boundary is counted as one batch by
  // the WORKER thread while the caller keeps pushing into the other staging buffer; the batch's (k-mer, count) result
  // is parked as a sorted run -- in HBM while there is room, in pinned host DRAM otherwise -- and the runs are merged once,
  // at the end (mgc_runs.cpp): into one device-resident result when that fits, chunk by chunk into the consumer otherwise.
  uint64_t    batch_limit = 0;            // bases per batch; 0 = derive from free HBM at the first input
  uint64_t    no_cut_below = 0;           // a cut found no sequence boundary: do not scan again before the stream is this long
  bool        have_r = false;             // at least one batch result has been parked
  struct mgc_runs *runs = nullptr;        // the parked batch results (mgc_runs.cpp)
  bool        ooc = false;                // counted, and the result exists only as runs (too large to collapse into HBM)
  uint64_t    result_budget = 0;          // bytes of runs that may stay in HBM; 0 = 60 % of what is free at the first batch's end
  uint64_t    total_bases = 0, total_instances = 0;
  uint64_t    total_file_instances[MGC_NUM_FILES];
  uint32_t    n_batches = 0;
  double      merge_ms = 0;
  std::thread worker;
  double      tr_memcpy = 0, tr_flush = 0, tr_cut = 0, tr_join = 0, tr_grow = 0;   // MGC_IO_TRACE: where the pushing thread's time went
  bool        worker_active = false;      // a batch is being counted (join before touching count state)
  int         worker_rc = MGC_OK;

  // mgc_prepare: the count's largest buffers allocated by a helper thread while the input is still being read
  std::thread prep_thread;
  bool        prep_active = false;
  void join_prepare() { if (prep_active) { prep_thread.join(); prep_active = false; } }

  // profiling
  bool        profiling = false;
  mgc_profile prof;

  void free_result() {            // result views point into the arena
    d_unique = nullptr; d_counts = nullptr; d_block_start = nullptr;
    counted = false;
  }
};

namespace mgc {
// The owner side of a sharded count (mgc_count_buckets[_into]): k-mers already extracted and grouped by bucket by the caller --
// extraction and partition are skipped, the caller's buffer is processed in place.  Default: the session's own input.
struct CountInput {
  void           *keys = nullptr;
  const uint64_t *counts = nullptr;                 // [1 << bucket_bits]
  uint32_t        bucket_bits = MGC_NUM_FILES_BITS;
  const uint64_t *fine = nullptr;                   // the senders' summed fifteen-bit histogram (the first grouping digit of every bucket)
  void           *out_keys = nullptr;               // where the packed result goes when it fits (out_cap k-mers): the caller's buffers
  uint32_t       *out_counts = nullptr;
  uint64_t        out_cap = 0;
};
// One count over the bases resident in HBM (s->d_bases / s->n_bases) or over in.keys: the result stays in the session's arena
// (mgc_count.cpp).  The caller marks the session counted.
int count_device(mgc_session *s, const CountInput &in = CountInput());

// ---- input staging (mgc_input.cpp) --------------------------------------------------------------------------------------------
inline int stage_id(int which) { return which ? mgc_session::B_STAGE1 : mgc_session::B_STAGE0; }
inline uint8_t *stage_ptr(mgc_session *s, int which) { return reinterpret_cast<uint8_t *>(s->buf[stage_id(which)].p); }
// Everything pushed so far is in stage[fill], its exact length in fill_len, and no batch is being counted: an empty stream is set up if
// nothing was pushed, the pinned chunk of host-pushed bases is flushed, the length is read back, the worker thread is joined.
int settle_input(mgc_session *s);
// one batch: stage[which][0, n) -> count -> park (mgc_api.cpp; cut_batch runs it on the worker thread)
int count_staged_batch(mgc_session *s, int which, uint64_t n);

// What the whole-file readers (mgc_textfile.cpp) use of the open file besides mgc_begin_text / mgc_end_text / mgc_begin_bam.  Each
// submit takes one piece (<= TEXT_CHUNK bytes, in pinned memory) and returns once its upload and kernels are queued.
int text_submit(mgc_session *s, const char *pinned_src, size_t piece);
// Waits for both pieces in flight: after a file's last piece (the uploads still read from their pinned sources), and FOR a piece that
// queues nothing (see mgc_input.cpp).
void text_drain(mgc_session *s);
// closes the open file and takes it back out of the stream; MGC_EINVAL when part of it was already counted
int text_rollback(mgc_session *s);
// text_rollback and the session's error: MGC_EFORMAT with "'what': why" + format_tail, or MGC_EINVAL with "'what': why" + joint +
// "after part of the file was counted (input larger than one batch)" when it cannot be taken back
int refuse_file(mgc_session *s, const char *what, const std::string &why, const char *joint = ", ", const char *format_tail = "");
// The open BAM file: the piece is walked on the host, uploaded with its segment table and decoded into the stream.  BAM_REFUSED (> 0):
// the walker refuses the stream (s->bam_walker.error()); nothing of the piece was queued, the file is still open (bam_refuse closes it).
constexpr int BAM_REFUSED = 1;
int bam_submit(mgc_session *s, const char *pinned_src, size_t piece);
// refuse_file with the walker's words
int bam_refuse(mgc_session *s, const char *what);
// mgc_end_bam with the name the refusal of a stream that ends inside the header or a record is reported under
int bam_end(mgc_session *s, const char *what);
// The open text file as a gzip stream (gzip_begin after mgc_begin_text): a piece of its text whose first n_symbols bytes are unresolved
// -- `symbols` holds them (mgc_gzip_par.hpp) -- window_valid bytes of its gzip member before it, and the members that end inside it.
// Uploads text, symbols and CRC table, queues resolve -> window -> CRC and the parse kernels.  GZIP_REFUSED (> 0): a CRC32 / ISIZE of
// an earlier piece did not match its trailer or the device met an unresolvable symbol (s->gz.verdict); the file is still open
// (gzip_refuse closes it).
constexpr int GZIP_REFUSED = 1;
int gzip_begin(mgc_session *s);
int gzip_submit(mgc_session *s, const char *pinned_text, size_t piece, const uint16_t *symbols, size_t n_symbols, uint32_t window_valid,
                const GzMemberEnd *ends, size_t n_ends, uint64_t comp_off);
// waits for the pieces in flight and checks what they brought back; GZIP_REFUSED as above
int gzip_finish(mgc_session *s);
// refuse_file once the pieces in flight are done and forgotten
int gzip_refuse(mgc_session *s, const char *what, const char *why);
}  // namespace mgc

