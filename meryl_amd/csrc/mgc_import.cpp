// mgc_import.cpp -- C-ABI layer of include/meryl_import.h and include/meryl_import_labelled.h: the bare device steps and the
// text -> database drivers.
//
// Reference side: main() of src/meryl-import/meryl-import.C:137-256 -- read a line, push (suffix, value) into one of 1024
// merylCountArrays, then countKmers + dumpCountedKmers per prefix into a wPrefix = 10 database.  Here the text goes to the
// device in batches cut at a line end; every batch is parsed, sorted and reduced there (mgc_import.hip); one batch is handed
// straight to the database stream, several are parked as runs and merged once (include/meryl_db.h).  Nothing is created at
// the output path before the whole input has been accepted.
//
// The meryl 2 dialect with labels (include/meryl_import_labelled.h) shares the device steps' bodies, the reader, the front
// half of a batch (ImportBase) and the entry points; its driver keeps every batch's triples on the device and sorts and
// reduces once, since the run store carries no labels.
#include "../../include/meryl_import_labelled.h"
#include "../../include/meryl_db.h"
#include "mgc_import_dev.hpp"
#include "mgc_runs.hpp"

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstdlib>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#include <zlib.h>

using mgc::set_err;

namespace {
using mgc::now_s;

int hip_rc(hipError_t e, const char *what) {
  if (e == hipSuccess) return MGC_OK;
  set_err(nullptr, "%s: %s", what, hipGetErrorString(e));
  return (e == hipErrorOutOfMemory) ? MGC_ENOMEM : MGC_EHIP;
}
bool k_ok(uint32_t k, int w_prefix = MGC_IMPORT_W_PREFIX) {
  if (k >= MGC_IMPORT_MIN_K && k <= MGC_IMPORT_MAX_K) return true;
  set_err(nullptr, "meryl-import: k=%u out of range (%d..%d: a %d-bit prefix must leave a suffix)", k, MGC_IMPORT_MIN_K, MGC_IMPORT_MAX_K, w_prefix);
  return false;
}
bool label_width_ok(uint32_t lw) {
  if (lw >= MGC_IMPORT_MIN_LABEL_WIDTH && lw <= MGC_IMPORT_MAX_LABEL_WIDTH) return true;
  set_err(nullptr, "meryl-import: label width %u out of range (%d..%d)", lw, MGC_IMPORT_MIN_LABEL_WIDTH, MGC_IMPORT_MAX_LABEL_WIDTH);
  return false;
}
const char *bad_text(uint32_t kind, const mgc::Import2State &) {
  switch (kind) {
    case MGC_IMPORT_BAD_BASE:   return "the k-mer holds a byte that is not one of ACGTacgt";
    case MGC_IMPORT_BAD_SHORT:  return "the k-mer is shorter than k";
    case MGC_IMPORT_BAD_VALUE:  return "the value is not a number (123, 123d, 7bh, 173o, 1111011b) of at most 4294967295";
    case MGC_IMPORT_BAD_LABEL:  return "the label is not a number (123, 123d, 7bh, 173o, 1111011b) that fits the label width";
    case MGC_IMPORT_BAD_ASSIGN: return "the number of a 'value=' / 'label=' line is missing, malformed or out of range";
  }
  return "malformed";
}
const char *bad_text(uint32_t kind, const mgc::ImportState &) {
  switch (kind) {
    case MGC_IMPORT_BAD_BASE:  return "the k-mer holds a byte that is not one of ACGTacgt";
    case MGC_IMPORT_BAD_SHORT: return "the k-mer is shorter than k";
    case MGC_IMPORT_BAD_VALUE: return "the value is not a decimal number of at most 4294967295";
    case MGC_IMPORT_BAD_HASH:  return "the number after '#' is not a decimal number of at most 4294967295";
  }
  return "malformed";
}
}  // namespace

// ================================================================================================
//  device steps
// ================================================================================================
extern "C" const char *mgc_import_error(void) { return mgc::thread_last_error().c_str(); }

namespace {
// the persistent words that hold after the chunk the count pass saw last
uint32_t value_after(const mgc::ImportState &h) { return h.chunk_has ? h.chunk_val : h.persistent; }
uint32_t value_after(const mgc::Import2State &h) { return h.chunk_vhas ? h.chunk_val : h.persistent_value; }
uint64_t label_after(const mgc::ImportState &) { return 0; }
uint64_t label_after(const mgc::Import2State &h) { return h.chunk_lhas ? h.chunk_lab : h.persistent_label; }

// The bodies of the parse steps, once for both dialects: S is the dialect's state, `name` what the step is called in messages;
// k and the label width are checked by the callers.  An empty chunk launches nothing but the reset of the chunk words: it
// holds nothing and moves nothing.
template <typename S>
int parse_count(const char *name, const uint8_t *d_text, uint64_t n_text, uint32_t k, uint32_t label_width, void *d_state, void *d_ws,
                size_t ws_bytes, mgc_import_parse_result *res, uint64_t *persistent_label, void *stream) {
  if (!d_state || !d_ws || !res || (n_text && !d_text) || n_text > 0xFFFFFFFFull || ws_bytes < mgc::parse_workspace_bytes<S>(n_text)) {
    set_err(nullptr, "mgc_dev_%s_count: bad arguments (a chunk holds fewer than 2^32 bytes)", name);
    return MGC_EINVAL;
  }
  const std::string what = std::string(name) + "_count";
  hipStream_t st = (hipStream_t)stream;
  S *ds = reinterpret_cast<S *>(d_state);
  hipError_t e = mgc::launch_parse_count<S>(d_text, n_text, k, label_width, ds, d_ws, st);
  if (e != hipSuccess) return hip_rc(e, what.c_str());
  S h;
  e = hipMemcpyAsync(&h, ds, sizeof(h), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return hip_rc(e, (what + " sync").c_str());
  res->n_lines = h.chunk_lines;
  res->n_records = h.chunk_records;
  res->bad_line = h.first_bad == ~0ull ? 0 : h.first_bad >> 3;
  res->bad_kind = h.first_bad == ~0ull ? 0u : (uint32_t)(h.first_bad & 7);
  res->persistent_value = value_after(h);
  if (persistent_label) *persistent_label = label_after(h);
  return MGC_OK;
}

template <typename S>
int parse_emit(const char *name, const uint8_t *d_text, uint64_t n_text, uint32_t k, int mode, uint32_t label_width, void *d_state, void *d_ws,
               size_t ws_bytes, void *d_keys, uint32_t *d_values, uint64_t *d_labels, void *stream) {
  if (mode < 0 || mode > 2 || !d_state || !d_ws || (n_text && !d_text) || n_text > 0xFFFFFFFFull ||
      ws_bytes < mgc::parse_workspace_bytes<S>(n_text)) {
    set_err(nullptr, "mgc_dev_%s: bad arguments", name);
    return MGC_EINVAL;
  }
  if (n_text == 0) return MGC_OK;
  return hip_rc(mgc::launch_parse_emit<S>(d_text, n_text, k, mode, label_width, reinterpret_cast<S *>(d_state), d_ws, d_keys, d_values,
                                          d_labels, (hipStream_t)stream), name);
}
}  // namespace

extern "C" size_t mgc_dev_import_parse_state_bytes(void) { return sizeof(mgc::ImportState); }
extern "C" size_t mgc_dev_import_parse_workspace_bytes(uint64_t n_text) { return mgc::parse_workspace_bytes<mgc::ImportState>(n_text); }
extern "C" size_t mgc_dev_import2_parse_state_bytes(void) { return sizeof(mgc::Import2State); }
extern "C" size_t mgc_dev_import2_parse_workspace_bytes(uint64_t n_text) { return mgc::parse_workspace_bytes<mgc::Import2State>(n_text); }

extern "C" int mgc_dev_import_parse_begin(void *d_state, void *stream) {
  if (!d_state) return MGC_EINVAL;
  return hip_rc(mgc::launch_parse_begin(reinterpret_cast<mgc::ImportState *>(d_state), (hipStream_t)stream), "import_parse_begin");
}
extern "C" int mgc_dev_import2_parse_begin(void *d_state, void *stream) {
  if (!d_state) return MGC_EINVAL;
  return hip_rc(mgc::launch_parse_begin(reinterpret_cast<mgc::Import2State *>(d_state), (hipStream_t)stream), "import2_parse_begin");
}

extern "C" int mgc_dev_import_parse_count(const uint8_t *d_text, uint64_t n_text, uint32_t k, void *d_state, void *d_ws,
                                          size_t ws_bytes, mgc_import_parse_result *res, void *stream) {
  if (!k_ok(k)) return MGC_EINVAL;
  return parse_count<mgc::ImportState>("import_parse", d_text, n_text, k, 0, d_state, d_ws, ws_bytes, res, nullptr, stream);
}
extern "C" int mgc_dev_import2_parse_count(const uint8_t *d_text, uint64_t n_text, uint32_t k, uint32_t label_width, void *d_state,
                                           void *d_ws, size_t ws_bytes, mgc_import_parse_result *res, uint64_t *persistent_label,
                                           void *stream) {
  if (!k_ok(k, MGC_IMPORT2_W_PREFIX) || !label_width_ok(label_width)) return MGC_EINVAL;
  return parse_count<mgc::Import2State>("import2_parse", d_text, n_text, k, label_width, d_state, d_ws, ws_bytes, res, persistent_label, stream);
}

extern "C" int mgc_dev_import_parse(const uint8_t *d_text, uint64_t n_text, uint32_t k, int mode, void *d_state, void *d_ws,
                                    size_t ws_bytes, void *d_keys, uint32_t *d_values, void *stream) {
  if (!k_ok(k)) return MGC_EINVAL;
  return parse_emit<mgc::ImportState>("import_parse", d_text, n_text, k, mode, 0, d_state, d_ws, ws_bytes, d_keys, d_values, nullptr, stream);
}
extern "C" int mgc_dev_import2_parse(const uint8_t *d_text, uint64_t n_text, uint32_t k, int mode, uint32_t label_width, void *d_state,
                                     void *d_ws, size_t ws_bytes, void *d_keys, uint32_t *d_values, uint64_t *d_labels, void *stream) {
  if (!k_ok(k, MGC_IMPORT2_W_PREFIX) || !label_width_ok(label_width)) return MGC_EINVAL;
  return parse_emit<mgc::Import2State>("import2_parse", d_text, n_text, k, mode, label_width, d_state, d_ws, ws_bytes, d_keys, d_values, d_labels,
                                       stream);
}

extern "C" size_t mgc_dev_sort_pairs_workspace_bytes(uint64_t n) { return mgc::sort_pairs_workspace_bytes(n); }

extern "C" int mgc_dev_sort_pairs(void *d_keys, uint32_t *d_values, void *d_alt_keys, uint32_t *d_alt_values, uint64_t n,
                                  uint32_t key_words, uint32_t begin_bit, uint32_t end_bit, void *d_ws, size_t ws_bytes,
                                  int *result_in_alt, void *stream) {
  if (!result_in_alt || begin_bit > end_bit || (key_words != 1 && key_words != 2) || end_bit > 64 * key_words) return MGC_EINVAL;
  *result_in_alt = 0;
  if (n == 0 || begin_bit == end_bit) return MGC_OK;
  if (!d_keys || !d_values || !d_alt_keys || !d_alt_values || !d_ws || ws_bytes < mgc::sort_pairs_workspace_bytes(n)) return MGC_EINVAL;
  return hip_rc(mgc::launch_sort_pairs(d_keys, d_values, d_alt_keys, d_alt_values, n, key_words, begin_bit, end_bit, d_ws, result_in_alt,
                                       (hipStream_t)stream), "sort_pairs");
}

extern "C" size_t mgc_dev_sort_triples_workspace_bytes(uint64_t n) { return mgc::sort_triples_workspace_bytes(n); }

extern "C" int mgc_dev_sort_triples(void *d_keys, uint32_t *d_values, uint64_t *d_labels, void *d_alt_keys, uint32_t *d_alt_values,
                                    uint64_t *d_alt_labels, uint64_t n, uint32_t key_words, uint32_t begin_bit, uint32_t end_bit,
                                    void *d_ws, size_t ws_bytes, int *result_in_alt, void *stream) {
  if (!result_in_alt || begin_bit > end_bit || (key_words != 1 && key_words != 2) || end_bit > 64 * key_words) {
    set_err(nullptr, "mgc_dev_sort_triples: bad key words or bit range");
    return MGC_EINVAL;
  }
  *result_in_alt = 0;
  if (n == 0 || begin_bit == end_bit) return MGC_OK;
  if (n > MGC_SORT_TRIPLES_MAX_N) {
    set_err(nullptr, "mgc_dev_sort_triples: %llu triples, one sort takes at most %llu (32-bit record numbers)", (unsigned long long)n,
            (unsigned long long)MGC_SORT_TRIPLES_MAX_N);
    return MGC_EINVAL;
  }
  if (!d_keys || !d_values || !d_labels || !d_alt_keys || !d_alt_values || !d_alt_labels || !d_ws ||
      ws_bytes < mgc::sort_triples_workspace_bytes(n)) {
    set_err(nullptr, "mgc_dev_sort_triples: NULL buffer or workspace too small");
    return MGC_EINVAL;
  }
  return hip_rc(mgc::launch_sort_triples(d_keys, d_values, d_labels, d_alt_keys, d_alt_values, d_alt_labels, n, key_words, begin_bit, end_bit,
                                         d_ws, result_in_alt, (hipStream_t)stream), "sort_triples");
}

extern "C" size_t mgc_dev_reduce_pairs_workspace_bytes(uint64_t n) { return mgc::reduce_pairs_workspace_bytes(n); }
extern "C" size_t mgc_dev_reduce_triples_workspace_bytes(uint64_t n) { return mgc::reduce_triples_workspace_bytes(n); }

namespace {
// the count pass and its number of distinct keys, for arguments the caller has checked.  d_labels: NULL for pairs
int reduce_count(const char *what, const void *d_keys, const uint32_t *d_values, const uint64_t *d_labels, uint64_t n, uint32_t key_words,
                 void *d_ws, uint64_t *n_distinct, void *stream) {
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = mgc::launch_reduce_count(d_keys, d_values, d_labels, n, key_words, d_ws, st);
  if (e != hipSuccess) return hip_rc(e, what);
  e = hipMemcpyAsync(n_distinct, d_ws, sizeof(uint64_t), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  return hip_rc(e, (std::string(what) + " sync").c_str());
}
}  // namespace

extern "C" int mgc_dev_reduce_pairs_count(const void *d_keys, const uint32_t *d_values, uint64_t n, uint32_t key_words, void *d_ws,
                                          size_t ws_bytes, uint64_t *n_distinct, void *stream) {
  if (!n_distinct || !d_ws || ws_bytes < mgc::reduce_pairs_workspace_bytes(n) || (n && (!d_keys || !d_values)) ||
      (key_words != 1 && key_words != 2)) return MGC_EINVAL;
  return reduce_count("reduce_pairs_count", d_keys, d_values, nullptr, n, key_words, d_ws, n_distinct, stream);
}

extern "C" int mgc_dev_reduce_pairs_emit(const void *d_keys, const uint32_t *d_values, uint64_t n, uint32_t key_words, void *d_ws,
                                         size_t ws_bytes, void *d_out_keys, uint32_t *d_out_values, void *stream) {
  if (!d_ws || ws_bytes < mgc::reduce_pairs_workspace_bytes(n) || (n && (!d_keys || !d_values || !d_out_keys || !d_out_values)) ||
      (key_words != 1 && key_words != 2)) return MGC_EINVAL;
  return hip_rc(mgc::launch_reduce_emit(d_keys, d_values, nullptr, n, key_words, 0, d_ws, d_out_keys, d_out_values, nullptr,
                                        (hipStream_t)stream), "reduce_pairs_emit");
}

extern "C" int mgc_dev_reduce_triples_count(const void *d_keys, const uint32_t *d_values, const uint64_t *d_labels, uint64_t n,
                                            uint32_t key_words, void *d_ws, size_t ws_bytes, uint64_t *n_distinct, void *stream) {
  if (!n_distinct || (key_words != 1 && key_words != 2)) { set_err(nullptr, "mgc_dev_reduce_triples_count: bad arguments"); return MGC_EINVAL; }
  *n_distinct = 0;
  if (n == 0) return MGC_OK;
  if (!d_ws || ws_bytes < mgc::reduce_triples_workspace_bytes(n) || !d_keys || !d_values || !d_labels) {
    set_err(nullptr, "mgc_dev_reduce_triples_count: NULL buffer or workspace too small");
    return MGC_EINVAL;
  }
  return reduce_count("reduce_triples_count", d_keys, d_values, d_labels, n, key_words, d_ws, n_distinct, stream);
}

extern "C" int mgc_dev_reduce_triples_emit(const void *d_keys, const uint32_t *d_values, const uint64_t *d_labels, uint64_t n,
                                           uint32_t key_words, uint32_t label_width, void *d_ws, size_t ws_bytes, void *d_out_keys,
                                           uint32_t *d_out_values, uint64_t *d_out_labels, void *stream) {
  if (!label_width_ok(label_width)) return MGC_EINVAL;
  if (key_words != 1 && key_words != 2) { set_err(nullptr, "mgc_dev_reduce_triples_emit: bad arguments"); return MGC_EINVAL; }
  if (n == 0) return MGC_OK;
  if (!d_ws || ws_bytes < mgc::reduce_triples_workspace_bytes(n) || !d_keys || !d_values || !d_labels || !d_out_keys || !d_out_values ||
      !d_out_labels) {
    set_err(nullptr, "mgc_dev_reduce_triples_emit: NULL buffer or workspace too small");
    return MGC_EINVAL;
  }
  return hip_rc(mgc::launch_reduce_emit(d_keys, d_values, d_labels, n, key_words, label_width, d_ws, d_out_keys, d_out_values, d_out_labels,
                                        (hipStream_t)stream), "reduce_triples_emit");
}

// ================================================================================================
//  text -> database
// ================================================================================================
namespace {

struct Source {                                            // bytes, 0 at the end, < 0 on a read error
  virtual int64_t read(char *dst, size_t cap) = 0;
  virtual ~Source() {}
};
struct MemSource : Source {
  const char *p; uint64_t n, at = 0;
  MemSource(const char *p_, uint64_t n_) : p(p_), n(n_) {}
  int64_t read(char *dst, size_t cap) override {
    const size_t m = (size_t)std::min<uint64_t>(cap, n - at);
    if (m) memcpy(dst, p + at, m);
    at += m;
    return (int64_t)m;
  }
};
struct GzSource : Source {                                 // plain files pass through zlib unchanged
  gzFile gz = nullptr;
  ~GzSource() override { if (gz) gzclose(gz); }
  int64_t read(char *dst, size_t cap) override {
    size_t got = 0;
    while (got < cap) {
      const unsigned want = (unsigned)std::min<size_t>(cap - got, 1u << 30);
      const int r = gzread(gz, dst + got, want);
      if (r < 0) return -1;
      if (r == 0) break;
      got += (size_t)r;
    }
    return (int64_t)got;
  }
};

// Two pinned buffers filled by a reader thread: a batch is everything up to the last '\n' that fits; what follows it is
// carried into the next batch; a line longer than the buffer grows it.
struct Reader {
  struct Slot { char *p = nullptr; size_t cap = 0, n = 0; bool last = false, full = false; };
  Slot slot[2];
  Source *src = nullptr;
  std::mutex mu;
  std::condition_variable cv;
  std::thread th;
  bool stop = false, failed = false;
  double read_s = 0;
  int device = 0;

  ~Reader() {
    { std::lock_guard<std::mutex> g(mu); stop = true; }
    cv.notify_all();
    if (th.joinable()) th.join();
    for (Slot &s : slot) if (s.p) (void)hipHostFree(s.p);
  }
  bool grow(Slot &s, size_t cap, size_t keep) {
    void *q = nullptr;
    if (hipHostMalloc(&q, cap, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return false; }
    if (keep) memcpy(q, s.p, keep);
    if (s.p) (void)hipHostFree(s.p);
    s.p = reinterpret_cast<char *>(q); s.cap = cap;
    return true;
  }
  bool start(Source *s, size_t batch, int dev) {
    src = s; device = dev;
    for (Slot &sl : slot) if (!grow(sl, batch, 0)) return false;
    th = std::thread([this] { main(); });
    return true;
  }
  void main() {
    (void)hipSetDevice(device);
    std::vector<char> tail;
    bool eof = false;
    for (int i = 0; !eof; i ^= 1) {
      Slot &s = slot[i];
      {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return stop || !s.full; });
        if (stop) return;
      }
      const double t0 = now_s();
      size_t have = tail.size();
      bool bad = false;
      if (have > s.cap && !grow(s, 2 * have, 0)) bad = true;
      if (!bad && have) memcpy(s.p, tail.data(), have);
      tail.clear();
      size_t cut = 0;
      while (!bad) {
        const int64_t r = src->read(s.p + have, s.cap - have);
        if (r < 0) { bad = true; break; }
        have += (size_t)r;
        if (have < s.cap) { eof = true; cut = have; break; }
        size_t j = have;
        while (j > 0 && s.p[j - 1] != '\n') j--;
        if (j > 0) { cut = j; break; }
        if (s.cap >= (0xFFFFFFFFull >> 1) || !grow(s, 2 * s.cap, have)) bad = true;      // one line longer than the batch
      }
      read_s += now_s() - t0;
      std::lock_guard<std::mutex> g(mu);
      if (bad) { failed = true; s.n = 0; s.last = true; s.full = true; cv.notify_all(); return; }
      if (cut < have) tail.assign(s.p + cut, s.p + have);
      s.n = cut; s.last = eof; s.full = true;
      cv.notify_all();
    }
  }
  Slot *wait(int i) {
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [&] { return slot[i].full; });
    return &slot[i];
  }
  void release(int i) {
    { std::lock_guard<std::mutex> g(mu); slot[i].full = false; }
    cv.notify_all();
  }
};

#define IM_TRY(expr) do { hipError_t e__ = (expr); if (e__ != hipSuccess) {                                        \
    set_err(nullptr, "%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(e__));                      \
    return (e__ == hipErrorOutOfMemory) ? MGC_ENOMEM : MGC_EHIP; } } while (0)

struct ImportArgs {
  uint32_t k; int mode;
  bool labelled; uint32_t label_width;                     // the meryl 2 dialect and its label width
  const char *output; int device, host_threads;
};

// What both drivers do the same way: the device and its stream, the batches of text, and the parse of one batch around
// whatever the driver does between its two passes.  S: the dialect's state
template <typename S>
struct ImportBase {
  typedef mgc::DBuf DBuf;
  uint32_t k = 0, kw = 1, label_width = 0;
  int mode = 0, device = -1, host_threads = 0;
  hipStream_t st = nullptr;
  hipEvent_t ev[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // 0..4: the parse; 5, 6: the driver's
  DBuf d_text, d_state, d_pws;
  size_t free_b = 0;                                       // device memory free when the run began
  double t_begin = 0;
  mgc_import_info info;

  ~ImportBase() {
    (void)hipSetDevice(device);
    for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
    if (st) (void)hipStreamDestroy(st);
  }

  // device, stream, events and the parser's state; -> the bytes of text a batch holds
  int open(uint64_t *batch_bytes) {
    t_begin = now_s();
    memset(&info, 0, sizeof(info));
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { set_err(nullptr, "meryl-import: no HIP device"); return MGC_EHIP; }
    if (device < 0) (void)hipGetDevice(&device);
    IM_TRY(hipSetDevice(device));
    IM_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    for (hipEvent_t &e : ev) IM_TRY(hipEventCreate(&e));
    size_t total_b = 0;
    IM_TRY(hipMemGetInfo(&free_b, &total_b));
    // per byte of text: the text itself, two (key, value) buffer pairs (a record takes at least k + 1 >= 7 bytes) and the
    // runs; with labels the triples a batch leaves stay on the device, the text does not.
    // At most 256 MiB: the reader fills the next batch while this one is uploaded and worked on, and pinning the two
    // buffers is paid before the first byte moves (one 1 GiB batch took twice the wall clock of seven 128 MiB ones)
    *batch_bytes = std::min<uint64_t>(std::max<uint64_t>(free_b / 12, 1u << 20), 256ull << 20);
    if (const char *e = getenv("MGC_IMPORT_BATCH")) { if (*e) *batch_bytes = strtoull(e, nullptr, 10); }
    *batch_bytes = std::min<uint64_t>(std::max<uint64_t>(*batch_bytes, 64), 1ull << 31);
    IM_TRY(d_state.ensure(sizeof(S)));
    IM_TRY(mgc::launch_parse_begin(d_state.as<S>(), st));
    return MGC_OK;
  }

  // on_batch(text, n, slot, last) for every batch that holds text; it releases the slot once the text has left it
  template <typename F>
  int each_batch(Reader &rd, Source *src, uint64_t batch_bytes, F &&on_batch) {
    if (!rd.start(src, (size_t)batch_bytes, device)) { set_err(nullptr, "meryl-import: no pinned memory for batches of %llu bytes", (unsigned long long)batch_bytes); return MGC_ENOMEM; }
    for (int i = 0;; i ^= 1) {
      Reader::Slot *s = rd.wait(i);
      if (rd.failed) { set_err(nullptr, "meryl-import: reading the input failed"); return MGC_EINVAL; }
      const bool last = s->last;
      const size_t n = s->n;
      info.text_bytes += n;
      if (n == 0) { rd.release(i); if (last) break; continue; }
      info.n_batches++;
      const int rc = on_batch(s->p, n, i, last);
      if (rc != MGC_OK) return rc;
      if (last) break;
    }
    info.read_s = rd.read_s;
    return MGC_OK;
  }

  // the front half of a batch of whole lines: upload, count pass, refusal -> *nr records to make room for
  int count_pass(const char *h_text, size_t n, Reader *rd, int slot, uint64_t *nr) {
    IM_TRY(d_text.ensure(n + 64));
    IM_TRY(d_pws.ensure(mgc::parse_workspace_bytes<S>(n)));
    IM_TRY(hipEventRecord(ev[0], st));
    IM_TRY(hipMemcpyAsync(d_text.p, h_text, n, hipMemcpyHostToDevice, st));
    IM_TRY(hipEventRecord(ev[1], st));
    IM_TRY(mgc::launch_parse_count(d_text.as<uint8_t>(), n, k, label_width, d_state.as<S>(), d_pws.p, st));
    IM_TRY(hipEventRecord(ev[2], st));
    S h;
    IM_TRY(hipMemcpyAsync(&h, d_state.p, sizeof(h), hipMemcpyDeviceToHost, st));
    IM_TRY(hipStreamSynchronize(st));
    rd->release(slot);                                      // the text has left the pinned buffer
    info.n_lines += h.chunk_lines;
    if (h.first_bad != ~0ull) {
      info.bad_line = h.first_bad >> 3; info.bad_kind = (uint32_t)(h.first_bad & 7);
      set_err(nullptr, "meryl-import: line %llu: %s", (unsigned long long)info.bad_line, bad_text(info.bad_kind, h));
      return MGC_EFORMAT;
    }
    info.n_records += h.chunk_records;
    *nr = h.chunk_records;
    return MGC_OK;
  }

  // the emit pass over the batch count_pass saw, into room for its records (d_labels: meryl 2)
  int emit_pass(size_t n, void *d_keys, uint32_t *d_values, uint64_t *d_labels) {
    IM_TRY(hipEventRecord(ev[3], st));
    IM_TRY(mgc::launch_parse_emit(d_text.as<uint8_t>(), n, k, mode, label_width, d_state.as<S>(), d_pws.p, d_keys, d_values, d_labels, st));
    IM_TRY(hipEventRecord(ev[4], st));
    return MGC_OK;
  }

  // once ev[4] has passed: the upload and both parse passes of the batch into the info
  int add_parse_times() {
    float up = 0, p1 = 0, p2 = 0;
    IM_TRY(hipEventElapsedTime(&up, ev[0], ev[1]));
    IM_TRY(hipEventElapsedTime(&p1, ev[1], ev[2]));
    IM_TRY(hipEventElapsedTime(&p2, ev[3], ev[4]));
    info.upload_ms += up; info.parse_ms += p1 + p2;
    return MGC_OK;
  }
};

// meryl 1: every batch sorted and reduced on its own; one batch goes straight to the database stream, several through the run store
struct Importer : ImportBase<mgc::ImportState> {
  DBuf d_k[2], d_v[2], d_sws, d_rws;
  mgc_runs *runs = nullptr;

  ~Importer() {
    (void)hipSetDevice(device);
    if (runs) mgc_runs_close(runs);
  }

  // one batch of whole lines -> *out_k / *out_v: nd ascending distinct k-mers and their summed values (device memory of this object)
  int batch(const char *h_text, size_t n, Reader *rd, int slot, const void **out_k, const uint32_t **out_v, uint64_t *nd) {
    *out_k = nullptr; *out_v = nullptr; *nd = 0;
    uint64_t nr = 0;
    int rc = count_pass(h_text, n, rd, slot, &nr);
    if (rc != MGC_OK) return rc;
    const size_t kb = sizeof(uint64_t) * kw;
    for (int i = 0; i < 2; i++) { IM_TRY(d_k[i].ensure(kb * nr)); IM_TRY(d_v[i].ensure(sizeof(uint32_t) * nr)); }
    IM_TRY(d_sws.ensure(mgc::sort_pairs_workspace_bytes(nr)));
    IM_TRY(d_rws.ensure(mgc::reduce_pairs_workspace_bytes(nr)));
    rc = emit_pass(n, d_k[0].p, d_v[0].as<uint32_t>(), nullptr);
    if (rc != MGC_OK) return rc;
    int in_alt = 0;
    IM_TRY(mgc::launch_sort_pairs(d_k[0].p, d_v[0].as<uint32_t>(), d_k[1].p, d_v[1].as<uint32_t>(), nr, kw, 0, 2 * k, d_sws.p, &in_alt, st));
    IM_TRY(hipEventRecord(ev[5], st));
    const int s = in_alt ? 1 : 0, o = s ^ 1;
    IM_TRY(mgc::launch_reduce_count(d_k[s].p, d_v[s].as<uint32_t>(), nullptr, nr, kw, d_rws.p, st));
    IM_TRY(mgc::launch_reduce_emit(d_k[s].p, d_v[s].as<uint32_t>(), nullptr, nr, kw, 0, d_rws.p, d_k[o].p, d_v[o].as<uint32_t>(), nullptr,
                                   st));                    // (synchronises for the count)
    IM_TRY(hipMemcpyAsync(nd, d_rws.p, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    IM_TRY(hipEventRecord(ev[6], st));
    IM_TRY(hipEventSynchronize(ev[6]));
    rc = add_parse_times();
    if (rc != MGC_OK) return rc;
    float sm = 0, rm = 0;
    IM_TRY(hipEventElapsedTime(&sm, ev[4], ev[5]));
    IM_TRY(hipEventElapsedTime(&rm, ev[5], ev[6]));
    info.sort_ms += sm; info.reduce_ms += rm;
    *out_k = d_k[o].p; *out_v = d_v[o].as<uint32_t>();
    return MGC_OK;
  }

  int run(Source *src, const char *output) {
    uint64_t batch_bytes = 0;
    int rc = open(&batch_bytes);
    if (rc != MGC_OK) return rc;
    Reader rd;
    const void *bk = nullptr; const uint32_t *bv = nullptr; uint64_t bn = 0;
    bool single = false;
    rc = each_batch(rd, src, batch_bytes, [&](const char *text, size_t n, int slot, bool last) {
      int rc = batch(text, n, &rd, slot, &bk, &bv, &bn);
      if (rc != MGC_OK) return rc;
      if (last && info.n_batches == 1) { single = true; return MGC_OK; }
      if (!runs) {
        runs = mgc_runs_open(k, MGC_IMPORT_W_PREFIX, device, free_b / 3, 0);
        if (!runs) { set_err(nullptr, "meryl-import: %s", mgc_runs_error(nullptr)); return MGC_EHIP; }
      }
      rc = mgc_runs_add(runs, bk, bv, bn, st);
      if (rc != MGC_OK) set_err(nullptr, "meryl-import: %s", mgc_runs_error(runs));
      return rc;
    });
    if (rc != MGC_OK) return rc;

    // the whole input is accepted: only now does anything appear at the output path
    const double t_write = now_s();
    mgc_db_stream *d = mgc_db_stream_open(output, k, MGC_IMPORT_W_PREFIX, 0, 0, 0, 1, host_threads, device);
    if (!d) { set_err(nullptr, "meryl-import: %s", mgc_db_stream_error(nullptr)); return MGC_EINVAL; }
    std::string msg;
    const uint64_t n_prefix = 1ull << MGC_IMPORT_W_PREFIX;
    if (runs) {
      for (DBuf *b : {&d_text, &d_k[0], &d_k[1], &d_v[0], &d_v[1], &d_sws}) b->release();     // room for the merge
      rc = mgc_runs_write(runs, d, 0, n_prefix);
      if (rc != MGC_OK) msg = mgc_runs_error(runs);
      mgc_runs_profile rp;
      if (rc == MGC_OK && mgc_runs_get_profile(runs, &rp) == MGC_OK) info.n_distinct = rp.n_merged;
    } else {
      rc = mgc_db_stream_write(d, single ? bk : nullptr, single ? bv : nullptr, single ? bn : 0, 0, n_prefix);
      if (rc != MGC_OK) msg = mgc_db_stream_error(d);
      info.n_distinct = single ? bn : 0;
    }
    const int rc2 = mgc_db_stream_close(d, nullptr);
    if (rc == MGC_OK && rc2 != MGC_OK) { rc = rc2; msg = mgc_db_stream_error(nullptr); }
    if (rc != MGC_OK) set_err(nullptr, "meryl-import: %s", msg.c_str());
    info.write_s = now_s() - t_write;
    info.total_s = now_s() - t_begin;
    return rc;
  }
};

// meryl 2: the run store carries no labels, so every batch's triples stay on the device and are sorted and reduced once
struct LabelledImporter : ImportBase<mgc::Import2State> {
  DBuf d_k[2], d_v[2], d_l[2], d_sws, d_rws;
  uint64_t n_total = 0, cap = 0;                           // triples held in d_k[0] / d_v[0] / d_l[0], and how many fit

  size_t triple_bytes() const { return sizeof(uint64_t) * kw + sizeof(uint32_t) + sizeof(uint64_t); }

  // `need` more bytes of device memory, or the refusal that names them
  int room_for(uint64_t need, const char *what) {
    size_t free_now = 0, total_b = 0;
    IM_TRY(hipMemGetInfo(&free_now, &total_b));
    if (need <= free_now) return MGC_OK;
    set_err(nullptr, "meryl-import: %llu triples do not fit the device: %s needs %llu bytes, %llu are free", (unsigned long long)n_total, what,
            (unsigned long long)need, (unsigned long long)free_now);
    return MGC_ENOMEM;
  }

  // room for `want` triples in the [0] arrays, what they hold kept
  int reserve(uint64_t want) {
    if (want <= cap) return MGC_OK;
    const uint64_t ncap = std::max<uint64_t>(want, 2 * cap);
    const int rc = room_for(ncap * triple_bytes() + 3 * 256, "appending a batch");
    if (rc != MGC_OK) return rc;
    DBuf nk, nv, nl;
    const size_t kb = sizeof(uint64_t) * kw;
    IM_TRY(nk.ensure(kb * ncap)); IM_TRY(nv.ensure(sizeof(uint32_t) * ncap)); IM_TRY(nl.ensure(sizeof(uint64_t) * ncap));
    if (n_total) {
      IM_TRY(hipMemcpyAsync(nk.p, d_k[0].p, kb * n_total, hipMemcpyDeviceToDevice, st));
      IM_TRY(hipMemcpyAsync(nv.p, d_v[0].p, sizeof(uint32_t) * n_total, hipMemcpyDeviceToDevice, st));
      IM_TRY(hipMemcpyAsync(nl.p, d_l[0].p, sizeof(uint64_t) * n_total, hipMemcpyDeviceToDevice, st));
      IM_TRY(hipStreamSynchronize(st));
    }
    d_k[0] = std::move(nk); d_v[0] = std::move(nv); d_l[0] = std::move(nl);
    cap = ncap;
    return MGC_OK;
  }

  // one batch of whole lines: its triples appended in input order
  int batch(const char *h_text, size_t n, Reader *rd, int slot) {
    uint64_t nr = 0;
    int rc = count_pass(h_text, n, rd, slot, &nr);
    if (rc != MGC_OK) return rc;
    rc = reserve(n_total + nr);
    if (rc != MGC_OK) return rc;
    const size_t kb = sizeof(uint64_t) * kw;
    rc = emit_pass(n, reinterpret_cast<unsigned char *>(d_k[0].p) + kb * n_total, d_v[0].as<uint32_t>() + n_total,
                   d_l[0].as<uint64_t>() + n_total);
    if (rc != MGC_OK) return rc;
    IM_TRY(hipEventSynchronize(ev[4]));
    rc = add_parse_times();
    if (rc != MGC_OK) return rc;
    n_total += nr;
    return MGC_OK;
  }

  // all triples -> *nd ascending distinct k-mers with their sums, back in the [0] arrays
  int sort_and_reduce(uint64_t *nd) {
    *nd = 0;
    if (n_total == 0) return MGC_OK;
    if (n_total > MGC_SORT_TRIPLES_MAX_N) {
      set_err(nullptr, "meryl-import: %llu records, one labelled import takes at most %llu (the triple sort carries 32-bit record numbers)",
              (unsigned long long)n_total, (unsigned long long)MGC_SORT_TRIPLES_MAX_N);
      return MGC_EUNSUPPORTED;
    }
    d_text.release(); d_pws.release();
    const size_t kb = sizeof(uint64_t) * kw;
    const size_t sws = mgc::sort_triples_workspace_bytes(n_total), rws = mgc::reduce_triples_workspace_bytes(n_total);
    const int rc = room_for(n_total * triple_bytes() + sws + rws + 5 * 256, "the sort");
    if (rc != MGC_OK) return rc;
    IM_TRY(d_k[1].ensure(kb * n_total)); IM_TRY(d_v[1].ensure(sizeof(uint32_t) * n_total)); IM_TRY(d_l[1].ensure(sizeof(uint64_t) * n_total));
    IM_TRY(d_sws.ensure(sws)); IM_TRY(d_rws.ensure(rws));
    IM_TRY(hipEventRecord(ev[0], st));
    int in_alt = 0;
    IM_TRY(mgc::launch_sort_triples(d_k[0].p, d_v[0].as<uint32_t>(), d_l[0].as<uint64_t>(), d_k[1].p, d_v[1].as<uint32_t>(),
                                    d_l[1].as<uint64_t>(), n_total, kw, 0, 2 * k, d_sws.p, &in_alt, st));
    IM_TRY(hipEventRecord(ev[1], st));
    const int s = in_alt ? 1 : 0, o = s ^ 1;
    IM_TRY(mgc::launch_reduce_count(d_k[s].p, d_v[s].as<uint32_t>(), d_l[s].as<uint64_t>(), n_total, kw, d_rws.p, st));
    IM_TRY(mgc::launch_reduce_emit(d_k[s].p, d_v[s].as<uint32_t>(), d_l[s].as<uint64_t>(), n_total, kw, label_width, d_rws.p,
                                   d_k[o].p, d_v[o].as<uint32_t>(), d_l[o].as<uint64_t>(), st));   // (synchronises for the count)
    IM_TRY(hipMemcpyAsync(nd, d_rws.p, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    IM_TRY(hipEventRecord(ev[2], st));
    IM_TRY(hipEventSynchronize(ev[2]));
    float sm = 0, rm = 0;
    IM_TRY(hipEventElapsedTime(&sm, ev[0], ev[1]));
    IM_TRY(hipEventElapsedTime(&rm, ev[1], ev[2]));
    info.sort_ms += sm; info.reduce_ms += rm;
    if (o != 0) { std::swap(d_k[0], d_k[1]); std::swap(d_v[0], d_v[1]); std::swap(d_l[0], d_l[1]); }
    return MGC_OK;
  }

  int run(Source *src, const char *output) {
    uint64_t batch_bytes = 0;
    int rc = open(&batch_bytes);
    if (rc != MGC_OK) return rc;
    Reader rd;
    rc = each_batch(rd, src, batch_bytes, [&](const char *text, size_t n, int slot, bool) { return batch(text, n, &rd, slot); });
    if (rc != MGC_OK) return rc;

    uint64_t nd = 0;
    rc = sort_and_reduce(&nd);
    if (rc != MGC_OK) return rc;

    // the whole input is accepted and reduced: only now does anything appear at the output path
    const double t_write = now_s();
    mgc_db_stream *d = mgc_db_stream_open(output, k, MGC_IMPORT2_W_PREFIX, label_width, 0, 0, 1, host_threads, device);
    if (!d) { set_err(nullptr, "meryl-import: %s", mgc_db_stream_error(nullptr)); return MGC_EINVAL; }
    std::string msg;
    rc = mgc_db_stream_write_labelled(d, nd ? d_k[0].p : nullptr, nd ? d_v[0].as<uint32_t>() : nullptr, nd ? d_l[0].as<uint64_t>() : nullptr,
                                      nd, 0, 1ull << MGC_IMPORT2_W_PREFIX);
    if (rc != MGC_OK) msg = mgc_db_stream_error(d);
    const int rc2 = mgc_db_stream_close(d, nullptr);
    if (rc == MGC_OK && rc2 != MGC_OK) { rc = rc2; msg = mgc_db_stream_error(nullptr); }
    if (rc != MGC_OK) set_err(nullptr, "meryl-import: %s", msg.c_str());
    info.n_distinct = nd;
    info.write_s = now_s() - t_write;
    info.total_s = now_s() - t_begin;
    return rc;
  }
};
#undef IM_TRY

// ---- the entry points: argument checks, the source, the driver of the dialect ----
bool import_args_ok(const ImportArgs &a) {
  if (a.labelled ? (!k_ok(a.k, MGC_IMPORT2_W_PREFIX) || !label_width_ok(a.label_width)) : !k_ok(a.k)) return false;
  if (a.mode < 0 || a.mode > 2 || !a.output || !*a.output) { set_err(nullptr, "meryl-import: bad mode or no output path"); return false; }
  return true;
}

template <typename I>
int run_import(Source *src, const ImportArgs &a, mgc_import_info *info) {
  I im;
  im.k = a.k; im.kw = a.k > 32 ? 2u : 1u; im.label_width = a.label_width; im.mode = a.mode; im.device = a.device; im.host_threads = a.host_threads;
  const int rc = im.run(src, a.output);
  if (info) *info = im.info;
  return rc;
}

int import_from(Source *src, const ImportArgs &a, mgc_import_info *info) {
  return a.labelled ? run_import<LabelledImporter>(src, a, info) : run_import<Importer>(src, a, info);
}

int import_file(const char *path, const ImportArgs &a, mgc_import_info *info) {
  if (info) memset(info, 0, sizeof(*info));
  if (!path || !*path) { set_err(nullptr, "meryl-import: no input path"); return MGC_EINVAL; }
  if (!import_args_ok(a)) return MGC_EINVAL;
  GzSource src;
  const std::string p(path);
  src.gz = (p == "-") ? gzdopen(0, "rb") : gzopen(path, "rb");
  if (!src.gz) { set_err(nullptr, "meryl-import: cannot open '%s'", path); return MGC_EINVAL; }
  (void)gzbuffer(src.gz, 1u << 20);
  return import_from(&src, a, info);
}

int import_text(const char *text, uint64_t n_text, const ImportArgs &a, mgc_import_info *info) {
  if (info) memset(info, 0, sizeof(*info));
  if (!text && n_text) { set_err(nullptr, "meryl-import: NULL text"); return MGC_EINVAL; }
  if (!import_args_ok(a)) return MGC_EINVAL;
  MemSource src(text, n_text);
  return import_from(&src, a, info);
}
}  // namespace

extern "C" int mgc_import_file(const char *path, uint32_t k, int mode, const char *output, int device, int host_threads,
                               mgc_import_info *info) {
  return import_file(path, ImportArgs{k, mode, false, 0, output, device, host_threads}, info);
}
extern "C" int mgc_import_text(const char *text, uint64_t n_text, uint32_t k, int mode, const char *output, int device,
                               int host_threads, mgc_import_info *info) {
  return import_text(text, n_text, ImportArgs{k, mode, false, 0, output, device, host_threads}, info);
}
extern "C" int mgc_import_labelled_file(const char *path, uint32_t k, int mode, uint32_t label_width, const char *output, int device,
                                        int host_threads, mgc_import_info *info) {
  return import_file(path, ImportArgs{k, mode, true, label_width, output, device, host_threads}, info);
}
extern "C" int mgc_import_labelled_text(const char *text, uint64_t n_text, uint32_t k, int mode, uint32_t label_width, const char *output,
                                        int device, int host_threads, mgc_import_info *info) {
  return import_text(text, n_text, ImportArgs{k, mode, true, label_width, output, device, host_threads}, info);
}
