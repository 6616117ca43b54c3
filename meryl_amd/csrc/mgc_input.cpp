// mgc_input.cpp -- input staging of a session (include/meryl_gpu_count.h; the state is described in mgc_session.hpp and mgc_input.hpp):
// host-pushed bases, text parsed on the device, BAM decoded on the device, gzip text resolved on the device -- all into ONE base stream
// in HBM, stage[fill], cut into batches that a worker thread counts (count_staged_batch, mgc_api.cpp) while the caller goes on pushing.
// Text, BAM and gzip pieces share one slot protocol, written once below (acquire_slot, queue_piece, text_drain); the routes supply what
// differs.  The whole-file readers on top of it are mgc_textfile.cpp's.
#include "../../include/meryl_gpu_count.h"
#include "mgc_device.h"
#include "mgc_sam_fsm.hpp"
#include "mgc_session.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>

using mgc::set_err;
using mgc::stage_id;
using mgc::stage_ptr;
using mgc::count_staged_batch;
using mgc::PieceSlot;

struct HostParseState { uint64_t out_len, file_start_len; uint32_t state, prev_nl, error, pad; };

// ---- the input ring's own memory (mgc_input.hpp) ----------------------------------------------------------------------------------
hipError_t mgc::SideTable::reserve(mgc_session *s, size_t want, size_t grow_to) {
  if (cap < want) {
    if (host) { (void)hipHostFree(host); host = nullptr; cap = 0; }
    const hipError_t e = hipHostMalloc(reinterpret_cast<void **>(&host), grow_to, hipHostMallocDefault);
    if (e != hipSuccess) return e;
    cap = grow_to;
  }
  return s->ensure(dev, cap);
}

mgc::InputRing::InputRing() {
  slot[0].dev_in = mgc_session::B_TEXT_IN0; slot[0].bam_seg.dev = mgc_session::B_BAM_SEG0; slot[0].gz_sym.dev = mgc_session::B_GZ_SYM0; slot[0].gz_tab.dev = mgc_session::B_GZ_TAB0;
  slot[1].dev_in = mgc_session::B_TEXT_IN1; slot[1].bam_seg.dev = mgc_session::B_BAM_SEG1; slot[1].gz_sym.dev = mgc_session::B_GZ_SYM1; slot[1].gz_tab.dev = mgc_session::B_GZ_TAB1;
}

hipError_t mgc::InputRing::setup(size_t chunk) {
  hipError_t e = hipSuccess;
  if (!st_up) e = hipStreamCreateWithFlags(&st_up, hipStreamNonBlocking);
  for (int i = 1; i >= 0 && e == hipSuccess; i--) {          // slot[0].pinned last: it says that all of this is there
    PieceSlot &sl = slot[i];
    if (!sl.done_ev) e = hipEventCreateWithFlags(&sl.done_ev, hipEventDisableTiming);
    if (e == hipSuccess && !sl.up_ev) e = hipEventCreateWithFlags(&sl.up_ev, hipEventDisableTiming);
    if (e == hipSuccess && !sl.pinned) e = hipHostMalloc(reinterpret_cast<void **>(&sl.pinned), chunk, hipHostMallocDefault);
  }
  return e;
}

char *mgc::InputRing::alloc_file_slot(int device, size_t chunk) {
  char *p = nullptr;
  (void)hipSetDevice(device);
  return hipHostMalloc(reinterpret_cast<void **>(&p), chunk, hipHostMallocDefault) == hipSuccess ? p : nullptr;
}

mgc::InputRing::~InputRing() {
  for (PieceSlot &sl : slot) {
    if (sl.pinned) (void)hipHostFree(sl.pinned);
    if (sl.done_ev) (void)hipEventDestroy(sl.done_ev);
    if (sl.up_ev) (void)hipEventDestroy(sl.up_ev);
  }
  for (char *p : file_slots) if (p) (void)hipHostFree(p);
  if (st_up) { (void)hipStreamSynchronize(st_up); (void)hipStreamDestroy(st_up); }
}

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

int mgc::settle_input(mgc_session *s) {
  int rc = MGC_OK;
  if (!s->state_ready) { rc = input_setup(s); if (rc != MGC_OK) return rc; }     // nothing was pushed: an empty stream
  rc = flush_pinned(s);
  if (rc == MGC_OK) rc = resolve_length(s);
  const int wrc = join_worker(s);
  return rc != MGC_OK ? rc : wrc;
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
  if (!s->in.slot[0].pinned) {
    for (const PieceSlot &sl : s->in.slot) HIP_TRY(s, s->ensure(sl.dev_in, mgc_session::TEXT_CHUNK));
    HIP_TRY(s, s->ensure(mgc_session::B_TEXT_WS, mgc::text_parse_workspace_bytes(mgc_session::TEXT_CHUNK)));
    HIP_TRY(s, s->in.setup(mgc_session::TEXT_CHUNK));
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
  if (!s || (format != MGC_TEXT_FASTA && format != MGC_TEXT_FASTQ && format != MGC_TEXT_SAM)) return MGC_EINVAL;
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

// ---- the piece protocol (mgc_input.hpp), written once for text, BAM and gzip ------------------------------------------------------
// The slot the next piece goes through, free again: a submit into slot b first waits for the done event of the piece two before it
// (that piece's pinned source is free with it).
static int acquire_slot(mgc_session *s, PieceSlot **slot) {
  PieceSlot &sl = s->in.slot[s->in.next & 1u];
  if (sl.used) HIP_TRY(s, hipEventSynchronize(sl.done_ev));
  *slot = &sl;
  return MGC_OK;
}

// Waits for both pieces in flight: after a file's last piece, whose upload still reads from its pinned source -- and for every
// piece that queues NOTHING (a BAM piece without a segment: header bytes, names, qualities, aux; a gzip piece without text: an empty
// member, the end of the file).  The whole-file readers' rings give a slot back two pieces after its submit BECAUSE a submit waits
// for the piece two before it; a piece that queues nothing does not advance `next`, would break that count, and so waits for both.
void mgc::text_drain(mgc_session *s) {
  for (PieceSlot &sl : s->in.slot) if (sl.used) (void)hipEventSynchronize(sl.done_ev);
}

// One piece (<= TEXT_CHUNK bytes at pinned_src) through the acquired slot: it adds `adds` bytes to the stream -- exactly (the decode
// writes at the stream's end and the parse state is told the new length) or at most (the decode goes through the parse state, which
// keeps the length on the device).  uploads(st_up): what travels with the piece; launches(d_in, d_out, st_in): its decode, d_out
// being the stage buffer (exact: its end).
template <class Uploads, class Launches>
static int queue_piece(mgc_session *s, PieceSlot &sl, const char *pinned_src, size_t piece, uint64_t adds, bool exact, Uploads uploads, Launches launches) {
  // grown before any pointer into it is taken: ensure_preserve may move it
  HIP_TRY(s, s->ensure_preserve(stage_id(s->fill), s->fill_len + adds + 4096, s->fill_len, s->st_in));
  uint8_t *d_in = reinterpret_cast<uint8_t *>(s->buf[sl.dev_in].p);
  // the copy runs on its own stream, so that chunk c travels while chunk c-1 is parsed (one stream did them in turn: 0.56 ms
  // of copy + 0.4 ms of parse per 32 MiB, 0.6 s of the 20 GB file -> database run; profiles/r03m_e2e_io.txt)
  HIP_TRY(s, hipMemcpyAsync(d_in, pinned_src, piece, hipMemcpyHostToDevice, s->in.st_up));
  int rc = uploads(s->in.st_up);
  if (rc != MGC_OK) return rc;
  HIP_TRY(s, hipEventRecord(sl.up_ev, s->in.st_up));
  HIP_TRY(s, hipStreamWaitEvent(s->st_in, sl.up_ev, 0));
  rc = launches(d_in, stage_ptr(s, s->fill) + (exact ? s->fill_len : 0), s->st_in);
  if (rc != MGC_OK) return rc;
  s->fill_len += adds;
  if (exact) HIP_TRY(s, mgc::launch_text_set_len(s->buf[mgc_session::B_TEXT_STATE].p, s->fill_len, 0, s->st_in));
  else s->len_inexact = true;                               // an upper bound: headers, qualities and line ends are dropped
  HIP_TRY(s, hipEventRecord(sl.done_ev, s->st_in));         // behind the last thing the piece queued
  sl.used = true;
  s->in.next++;
  if (s->fill_len >= s->batch_limit) return cut_batch(s);
  return MGC_OK;
}

static int launch_parse(mgc_session *s, const uint8_t *d_in, size_t piece, uint8_t *d_stage, hipStream_t st) {
  HIP_TRY(s, mgc::launch_text_parse(d_in, piece, s->text_format, s->buf[mgc_session::B_TEXT_STATE].p,
                                    s->buf[mgc_session::B_TEXT_WS].p, d_stage, st));
  return MGC_OK;
}

// the caller's bytes in pieces through the slots' pinned blocks: submit(pinned, piece) != MGC_OK ends it
template <class Submit>
static int push_pieces(mgc_session *s, const char *src, size_t len, Submit submit) {
  while (len) {
    const size_t piece = len < mgc_session::TEXT_CHUNK ? len : mgc_session::TEXT_CHUNK;
    PieceSlot *sl = nullptr;
    int rc = acquire_slot(s, &sl);                          // pinned + device buffer are free again
    if (rc != MGC_OK) return rc;
    memcpy(sl->pinned, src, piece);
    rc = submit(sl->pinned, piece);
    if (rc != MGC_OK) return rc;
    src += piece;
    len -= piece;
  }
  return MGC_OK;
}

int mgc::text_submit(mgc_session *s, const char *pinned_src, size_t piece) {
  PieceSlot *sl = nullptr;
  const int rc = acquire_slot(s, &sl);
  if (rc != MGC_OK) return rc;
  return queue_piece(s, *sl, pinned_src, piece, piece, false, [](hipStream_t) { return (int)MGC_OK; },
                     [&](const uint8_t *d_in, uint8_t *d_stage, hipStream_t st) { return launch_parse(s, d_in, piece, d_stage, st); });
}

extern "C" int mgc_push_text(mgc_session *s, const char *text, size_t len) {
  if (!s || (!text && len)) return MGC_EINVAL;
  if (!s->text_open || s->text_format == mgc_session::TEXT_BAM) { set_err(&s->err, "mgc_push_text without mgc_begin_text"); return MGC_ESTATE; }
  HIP_TRY(s, hipSetDevice(s->device));
  return push_pieces(s, text, len, [s](const char *p, size_t n) { return mgc::text_submit(s, p, n); });
}

// Closes the open file and takes what it has put into the stream back out.  MGC_EINVAL, and the stream as it is, when part
// of the file went into a batch that is already counted: that cannot be taken back.
int mgc::text_rollback(mgc_session *s) {
  s->text_open = false;
  if (s->text_cut_in_file) return MGC_EINVAL;
  HIP_TRY(s, mgc::launch_text_file_op(s->buf[mgc_session::B_TEXT_STATE].p, stage_ptr(s, s->fill), 2, s->st_in));
  return resolve_length(s);
}

int mgc::refuse_file(mgc_session *s, const char *what, const std::string &why, const char *joint, const char *format_tail) {
  const std::string w = why;                                // (why may be one of the session's own strings)
  const int rc = mgc::text_rollback(s);
  if (rc == MGC_EINVAL) set_err(&s->err, "'%s': %s%safter part of the file was counted (input larger than one batch)", what, w.c_str(), joint);
  if (rc != MGC_OK) return rc;
  set_err(&s->err, "'%s': %s%s", what, w.c_str(), format_tail);
  return MGC_EFORMAT;
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
  if (h.error && s->text_format == MGC_TEXT_SAM) {
    const char *why = (h.error & mgc::SAM_ERR_CR_LINE_START) ? "line starts with a carriage return" : "alignment line with fewer than 10 columns";
    rc = mgc::text_rollback(s);
    if (rc == MGC_EINVAL)
      set_err(&s->err, "the SAM file is refused (%s) after part of it was counted (input larger than one batch): "
                       "convert it, or feed it through mgc_push_bases from the start", why);
    if (rc != MGC_OK) return rc;
    set_err(&s->err, "the SAM file is refused: %s: feed it through mgc_push_bases (meryl_seq.h reader)", why);
    return MGC_EFORMAT;
  }
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
  const size_t nseg = s->bam_segs.size(), seg_bytes = nseg * sizeof(mgc::BamSegment);
  if (nseg == 0) { mgc::text_drain(s); return MGC_OK; }     // nothing for the device
  PieceSlot *sl = nullptr;
  const int rc = acquire_slot(s, &sl);
  if (rc != MGC_OK) return rc;
  mgc::SideTable &seg = sl->bam_seg;                        // grow-only, with room to spare: records of one file are alike
  HIP_TRY(s, seg.reserve(s, seg_bytes, (nseg + nseg / 2 + 4096) * sizeof(mgc::BamSegment)));
  memcpy(seg.host, s->bam_segs.data(), seg_bytes);
  void *d_seg = s->buf[seg.dev].p;
  return queue_piece(s, *sl, pinned_src, piece, out_bytes, true,
                     [&](hipStream_t up) { HIP_TRY(s, hipMemcpyAsync(d_seg, seg.host, seg_bytes, hipMemcpyHostToDevice, up)); return (int)MGC_OK; },
                     [&](const uint8_t *d_in, uint8_t *d_out, hipStream_t st) {
                       HIP_TRY(s, mgc::launch_bam_decode(d_in, piece, d_seg, nseg, out_bytes, d_out, st));
                       return (int)MGC_OK;
                     });
}

int mgc::bam_refuse(mgc_session *s, const char *what) { return mgc::refuse_file(s, what, s->bam_walker.error()); }

extern "C" int mgc_push_bam(mgc_session *s, const void *bam_bytes, size_t len) {
  if (!s || (!bam_bytes && len)) return MGC_EINVAL;
  if (!s->text_open || s->text_format != mgc_session::TEXT_BAM) { set_err(&s->err, "mgc_push_bam without mgc_begin_bam"); return MGC_ESTATE; }
  HIP_TRY(s, hipSetDevice(s->device));
  const int rc = push_pieces(s, static_cast<const char *>(bam_bytes), len, [s](const char *p, size_t n) { return mgc::bam_submit(s, p, n); });
  return rc == mgc::BAM_REFUSED ? mgc::bam_refuse(s, "mgc_push_bam") : rc;
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

// ---- gzip input, inflated by several host threads, resolved on the device (mgc_gzip_par.hpp, mgc_gzip.hip) ----------------------
// The open gzip file IS an open text file (mgc_begin_text): its pieces go through the parse kernels as text_submit's do.  Before they
// read a piece, its unresolved prefix is patched from the window the device keeps of the text before it; the CRC-32 of the resolved
// text comes back when the piece's slot is acquired again (or at gzip_finish) and is held against the members' trailers then
// (mgc_gzip_crc.hpp).
static uint32_t *gz_error_word(mgc_session *s) { return reinterpret_cast<uint32_t *>(static_cast<uint8_t *>(s->buf[mgc_session::B_GZ_WIN].p) + 2 * mgc::GZ_WINDOW); }

int mgc::gzip_begin(mgc_session *s) {
  HIP_TRY(s, s->ensure(mgc_session::B_GZ_WIN, 2 * mgc::GZ_WINDOW + 256));
  HIP_TRY(s, hipMemsetAsync(s->buf[mgc_session::B_GZ_WIN].p, 0, 2 * mgc::GZ_WINDOW + 256, s->st_in));
  s->gz_win = 0;
  s->tr_gz_copy = s->tr_gz_collect = s->tr_gz_wait = 0;
  s->gz.reset();
  return MGC_OK;
}

// the CRC values of the piece that went through slot b have arrived (its done event was waited for)
static void gz_collect(mgc_session *s, uint32_t b) {
  const PieceSlot &sl = s->in.slot[b];
  if (s->gz.pending[b].empty()) return;
  const double t0 = mgc::now_s();
  const size_t cap = sl.gz_tab_entries();
  const uint32_t *crc = reinterpret_cast<const uint32_t *>(sl.gz_tab.host + 12 * cap);
  s->gz.collect((int)b, crc, crc[cap]);
  s->tr_gz_collect += mgc::now_s() - t0;
}

int mgc::gzip_finish(mgc_session *s) {
  const double t0 = mgc::now_s();
  mgc::text_drain(s);
  s->tr_gz_wait += mgc::now_s() - t0;
  const uint32_t older = s->in.next & 1u;
  gz_collect(s, older);
  gz_collect(s, older ^ 1u);
  return s->gz.refused() ? mgc::GZIP_REFUSED : MGC_OK;
}

int mgc::gzip_submit(mgc_session *s, const char *pinned_text, size_t piece, const uint16_t *symbols, size_t n_symbols, uint32_t window_valid,
                     const mgc::GzMemberEnd *ends, size_t n_ends, uint64_t comp_off) {
  if (piece == 0) {                                         // nothing for the device: the trailers are checked here
    if (mgc::gzip_finish(s) != MGC_OK) return mgc::GZIP_REFUSED;
    s->gz.empty_piece(ends, n_ends);
    return s->gz.refused() ? mgc::GZIP_REFUSED : MGC_OK;
  }
  if (piece > mgc_session::TEXT_CHUNK || n_symbols > piece || window_valid > mgc::GZ_WINDOW) { set_err(&s->err, "gzip_submit: a piece out of bounds"); return MGC_EINVAL; }
  const double w0 = mgc::now_s();
  PieceSlot *sl = nullptr;
  const int rc = acquire_slot(s, &sl);
  if (rc != MGC_OK) return rc;
  s->tr_gz_wait += mgc::now_s() - w0;
  const uint32_t b = s->in.next & 1u;
  gz_collect(s, b);                                         // the slot is free: what the piece that used it brought back
  if (s->gz.refused()) return mgc::GZIP_REFUSED;
  const size_t want_tab = mgc::GzCrcLedger::table_room(piece, n_ends);
  HIP_TRY(s, sl->gz_tab.reserve(s, PieceSlot::gz_tab_bytes(want_tab), PieceSlot::gz_tab_bytes(want_tab + want_tab / 2 + 1024)));
  const size_t cap = sl->gz_tab_entries();
  char *h_tab = sl->gz_tab.host;
  const long n_tab = s->gz.build_table((int)b, piece, ends, n_ends, comp_off, reinterpret_cast<uint64_t *>(h_tab), reinterpret_cast<uint32_t *>(h_tab + 8 * cap), cap);
  if (n_tab < 0) { set_err(&s->err, "gzip_submit: member ends out of order"); return MGC_EINVAL; }
  HIP_TRY(s, sl->gz_sym.reserve(s, n_symbols * 2, std::min<size_t>(2 * mgc_session::TEXT_CHUNK, n_symbols * 3 + (1u << 20))));
  const double c0 = mgc::now_s();
  if (n_symbols) memcpy(sl->gz_sym.host, symbols, n_symbols * 2);
  s->tr_gz_copy += mgc::now_s() - c0;
  const uint16_t *d_sym = static_cast<const uint16_t *>(s->buf[sl->gz_sym.dev].p);
  uint8_t *d_tab = static_cast<uint8_t *>(s->buf[sl->gz_tab.dev].p);
  uint8_t *d_win = static_cast<uint8_t *>(s->buf[mgc_session::B_GZ_WIN].p);
  return queue_piece(s, *sl, pinned_text, piece, piece, false,
                     [&](hipStream_t up) {
                       if (n_symbols) HIP_TRY(s, hipMemcpyAsync(const_cast<uint16_t *>(d_sym), sl->gz_sym.host, n_symbols * 2, hipMemcpyHostToDevice, up));
                       HIP_TRY(s, hipMemcpyAsync(d_tab, h_tab, (size_t)n_tab * 8, hipMemcpyHostToDevice, up));
                       HIP_TRY(s, hipMemcpyAsync(d_tab + 8 * cap, h_tab + 8 * cap, (size_t)n_tab * 4, hipMemcpyHostToDevice, up));
                       return (int)MGC_OK;
                     },
                     [&](uint8_t *d_in, uint8_t *d_stage, hipStream_t st) {
                       HIP_TRY(s, mgc::launch_gzip_resolve(d_in, piece, d_sym, n_symbols, d_win + (size_t)s->gz_win * mgc::GZ_WINDOW, window_valid,
                                                           d_win + (size_t)(s->gz_win ^ 1) * mgc::GZ_WINDOW, gz_error_word(s), st));
                       s->gz_win ^= 1;
                       HIP_TRY(s, mgc::launch_gzip_crc32(d_in, reinterpret_cast<const uint64_t *>(d_tab), reinterpret_cast<const uint32_t *>(d_tab + 8 * cap),
                                                         (size_t)n_tab, reinterpret_cast<uint32_t *>(d_tab + 12 * cap), st));
                       HIP_TRY(s, hipMemcpyAsync(h_tab + 12 * cap, d_tab + 12 * cap, (size_t)n_tab * 4, hipMemcpyDeviceToHost, st));
                       HIP_TRY(s, hipMemcpyAsync(h_tab + 16 * cap, gz_error_word(s), 4, hipMemcpyDeviceToHost, st));
                       return launch_parse(s, d_in, piece, d_stage, st);
                     });
}

int mgc::gzip_refuse(mgc_session *s, const char *what, const char *why) {
  const std::string w = why;                                // (why may point into the ledger's verdict)
  mgc::text_drain(s);
  s->gz.forget_pending();
  return mgc::refuse_file(s, what, w);
}

extern "C" int mgc_push_bases_device(mgc_session *s, const uint8_t *d_bases, uint64_t n_bases) {
  if (!s || (!d_bases && n_bases)) return MGC_EINVAL;
  if (s->borrowed || s->input_seen || s->counted) { set_err(&s->err, "device input must be the only input"); return MGC_ESTATE; }
  s->d_bases = d_bases;
  s->n_bases = n_bases;
  s->borrowed = true;
  return MGC_OK;
}
