// mgc_analyze.cpp -- C-ABI layer of include/meryl_analyze.h: the accumulator, the database loop and the report files.
//
// Reference side: src/meryl-analyze/meryl-analyze.C -- one thread walks the database with nextMer(), scores every k-mer and
// inserts its value into a std::map per (histogram, score) (:171-223, :257-322, :359-424); printHist (:139-152) writes the
// maps out.  Here a file's raw bytes are read by host threads, uploaded and decoded on the device (mgc_decode.hip) while
// the next files are read; the decoded arrays go through the score + histogram kernel (mgc_analyze.hip); what its dense tier
// does not take goes through the one list tier of mgc_hist_list.hpp: sorted and run-length counted on the device, merged into a
// sorted host list.
#include "../../include/meryl_analyze.h"
#include "../../include/meryl_db.h"
#include "mgc_analyze_dev.hpp"
#include "mgc_dbfile.hpp"
#include "mgc_device.h"
#include "mgc_hist_list.hpp"
#include "mgc_runs.hpp"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

using mgc::set_err;

namespace {
using mgc::now_s;

bool type_ok(int type) { return type == MGC_ANALYZE_GC || type == MGC_ANALYZE_GA || type == MGC_ANALYZE_GT; }
bool k_ok(uint32_t k) {
  if (k >= 1 && k <= MGC_ANALYZE_MAX_K) return true;
  set_err(nullptr, "meryl-analyze: k=%u out of range (1..%d)", k, MGC_ANALYZE_MAX_K);
  return false;
}
bool have_device() {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0) return true;
  (void)hipGetLastError();
  set_err(nullptr, "meryl-analyze: no HIP device");
  return false;
}

constexpr uint64_t CHUNK = 1ull << 26;      // entries per kernel pass: bounds the overflow list (three 8-byte entries per k-mer at worst)
typedef mgc::HistPair Row;                  // key = analyze_pack(histogram, score, value)
}  // namespace

struct mgc_analyze {
  typedef mgc::DBuf DBuf;
  uint32_t k = 0, kw = 1, dense = MGC_ANALYZE_DENSE_VALUES, n_cus = 1;
  int type = 0, device = -1;
  bool ready = false;
  hipStream_t st_own = nullptr;
  hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  DBuf d_dense;                                                       // the accumulator: the dense tier ...
  mgc::ListTier ovf{"meryl-analyze"};                                 // ... and what went through the overflow list
  mgc::DbFileScratch file_scratch;                                    // one database file
  DBuf d_keys, d_vals;
  std::vector<Row> rows[3];                 // result cache per histogram
  bool rows_ok[3] = {false, false, false};
  mgc_analyze_info info;

  ~mgc_analyze() {                          // (the buffers go after this body, on the device it selects)
    if (st_own) (void)hipSetDevice(device);               // (init got as far as the device)
    for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
    if (st_own) (void)hipStreamDestroy(st_own);
  }

#define AN_TRY(expr) do { hipError_t e__ = (expr); if (e__ != hipSuccess) {                                         \
    set_err(nullptr, "%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(e__));                      \
    return (e__ == hipErrorOutOfMemory) ? MGC_ENOMEM : MGC_EHIP; } } while (0)

  size_t dense_bytes() const { return sizeof(uint64_t) * mgc::ANALYZE_HISTS * mgc::ANALYZE_SCORES * MGC_ANALYZE_DENSE_VALUES; }

  int init() {                              // the first touch of the device
    if (ready) { AN_TRY(hipSetDevice(device)); return MGC_OK; }
    if (!have_device()) return MGC_EHIP;
    if (device < 0) (void)hipGetDevice(&device);
    AN_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    AN_TRY(hipGetDeviceProperties(&prop, device));
    n_cus = (uint32_t)std::max(prop.multiProcessorCount, 1);
    AN_TRY(hipStreamCreateWithFlags(&st_own, hipStreamNonBlocking));
    for (hipEvent_t &e : ev) AN_TRY(hipEventCreate(&e));
    AN_TRY(d_dense.ensure(dense_bytes()));
    AN_TRY(hipMemset(d_dense.p, 0, dense_bytes()));
    ready = true;
    return MGC_OK;
  }

  int add_chunk(const void *keys, const uint32_t *vals, uint64_t n, hipStream_t st) {
    const uint32_t nh = mgc::analyze_device_hists(type);
    // the list starts at an eighth of the worst case (all of it when the dense tier is off) and grows to what a pass asked for
    const uint64_t first_cap = dense ? std::max<uint64_t>(n * nh / 8, 1u << 16) : n * nh;
    AN_TRY(ovf.reserve(first_cap));
    uint64_t cap = ovf.capacity(), need = 0;
    AN_TRY(ovf.reset(st));
    AN_TRY(hipEventRecord(ev[0], st));
    AN_TRY(mgc::launch_analyze_hist(keys, vals, n, k, type, dense, true, d_dense.as<uint64_t>(), ovf.list(), cap, ovf.list_n(), n_cus, st));
    AN_TRY(hipMemcpyAsync(&need, ovf.list_n(), 8, hipMemcpyDeviceToHost, st));
    AN_TRY(hipStreamSynchronize(st));
    if (need > cap) {                                       // the dense tier has counted its share: only the list is redone
      AN_TRY(ovf.reserve(need));
      cap = ovf.capacity();
      AN_TRY(ovf.reset(st));
      AN_TRY(mgc::launch_analyze_hist(keys, vals, n, k, type, dense, false, d_dense.as<uint64_t>(), ovf.list(), cap, ovf.list_n(), n_cus, st));
      uint64_t again = 0;
      AN_TRY(hipMemcpyAsync(&again, ovf.list_n(), 8, hipMemcpyDeviceToHost, st));
      AN_TRY(hipStreamSynchronize(st));
      if (again != need) { set_err(nullptr, "meryl-analyze: the overflow list changed size between passes"); return MGC_EHIP; }
      info.n_overflow_retries++;
    }
    AN_TRY(hipEventRecord(ev[1], st));
    info.n_overflow_kmers += need / nh;
    const int rc = ovf.drain(need, mgc::ANALYZE_KEY_BITS, st, ev[2]);
    if (rc != MGC_OK) return rc;
    float ms = 0;
    AN_TRY(hipEventElapsedTime(&ms, ev[0], ev[1])); info.hist_ms += ms;
    AN_TRY(hipEventElapsedTime(&ms, ev[1], ev[2])); info.overflow_ms += ms;
    return MGC_OK;
  }

  int add(const void *keys, const uint32_t *vals, uint64_t n, hipStream_t st) {
    for (bool &b : rows_ok) b = false;
    const unsigned char *kp = reinterpret_cast<const unsigned char *>(keys);
    for (uint64_t o = 0; o < n; o += CHUNK) {
      const uint64_t m = std::min<uint64_t>(CHUNK, n - o);
      const int rc = add_chunk(kp + o * 8 * kw, vals + o, m, st);
      if (rc != MGC_OK) return rc;
    }
    info.n_kmers += n;
    return MGC_OK;
  }

  // ---- the database loop ----------------------------------------------------------------------------------------
  struct Slot { mgc::DbFile f; bool done = false; };

  int one_file(Slot &s, const mdb_info &inf) {
    const uint64_t n = s.f.n;
    if (n == 0) return MGC_OK;
    hipStream_t st = st_own;
    AN_TRY(d_keys.ensure(8 * (size_t)kw * n));
    AN_TRY(d_vals.ensure(4 * n));
    AN_TRY(hipEventRecord(ev[3], st));
    uint32_t h_err = 0;
    AN_TRY(mgc::dbfile_upload(s.f, inf, kw, file_scratch, d_keys.p, d_vals.as<uint32_t>(), nullptr, &h_err, st));
    AN_TRY(hipEventRecord(ev[4], st));
    AN_TRY(hipStreamSynchronize(st));                       // the host copies may go
    std::string msg;
    if (mgc::dbfile_decode_rc(h_err, &msg) != MGC_OK) { set_err(nullptr, "meryl-analyze: %s", msg.c_str()); return MGC_EINVAL; }
    float ms = 0;
    AN_TRY(hipEventElapsedTime(&ms, ev[3], ev[4])); info.decode_ms += ms;
    s.f.drop();
    return add(d_keys.p, d_vals.as<uint32_t>(), n, st);
  }

  int add_database(const char *path, const mdb_info &inf, int host_threads) {
    const bool host_decode = mgc::decode_on_host();         // (tests) read once per call
    const uint32_t nf = MGC_NUM_FILES;
    const int nth = std::max(1, std::min(host_threads <= 0 ? 4 : host_threads, 16));
    const uint32_t ahead = (uint32_t)nth + 1;               // files read but not yet consumed
    std::vector<Slot> slot(nf);
    std::mutex mu;
    std::condition_variable cv;
    uint32_t next = 0, consumed = 0;
    bool stop = false;
    double read_s = 0;
    auto reader = [&]() {
      mdb_reader *r = mdb_reader_open(path);                // one reader per thread: a reader is not shared
      for (;;) {
        uint32_t ff;
        {
          std::unique_lock<std::mutex> lk(mu);
          cv.wait(lk, [&] { return stop || next >= nf || next < consumed + ahead; });
          if (stop || next >= nf) break;
          ff = next++;
        }
        Slot &s = slot[ff];
        const double t0 = now_s();
        if (!r) { s.f.rc = MGC_EINVAL; s.f.msg = mdb_last_error(); }
        else mgc::dbfile_read(r, ff, kw, host_decode, false, &s.f);
        const double dt = now_s() - t0;
        { std::lock_guard<std::mutex> g(mu); s.done = true; read_s += dt; }
        cv.notify_all();
      }
      if (r) mdb_reader_close(r);
    };
    std::vector<std::thread> pool;
    for (int i = 0; i < nth; i++) pool.emplace_back(reader);
    int rc = MGC_OK;
    for (uint32_t ff = 0; ff < nf && rc == MGC_OK; ff++) {
      {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return slot[ff].done; });
      }
      Slot &s = slot[ff];
      if (s.f.rc != MGC_OK) { set_err(nullptr, "meryl-analyze: '%s': %s", path, s.f.msg.c_str()); rc = s.f.rc; }
      else { rc = one_file(s, inf); info.n_files++; }
      s.f.drop();
      { std::lock_guard<std::mutex> g(mu); consumed = ff + 1; }
      cv.notify_all();
    }
    { std::lock_guard<std::mutex> g(mu); stop = true; }
    cv.notify_all();
    for (auto &t : pool) t.join();
    info.read_s += read_s;
    return rc;
  }

  // ---- results ----------------------------------------------------------------------------------------------------
  // `which` of the report -> rows ascending by (score, value), packed with histogram 0
  int build(int which) {
    if (rows_ok[which]) return MGC_OK;
    // -gc keeps the GC histogram only: AT is the same k-mers at score k - GC
    const bool mirror = type == MGC_ANALYZE_GC && which == MGC_ANALYZE_REVERSE;
    const uint32_t h = type == MGC_ANALYZE_GC ? 0u : (uint32_t)which;
    std::vector<Row> &out = rows[which];
    out.clear();
    auto put = [&](uint32_t score, uint32_t value, uint64_t n) { out.push_back(Row{mgc::analyze_pack(0, mirror ? k - score : score, value), n}); };
    if (ready) {
      AN_TRY(hipSetDevice(device));
      std::vector<uint64_t> hd((size_t)mgc::ANALYZE_SCORES * MGC_ANALYZE_DENSE_VALUES);
      AN_TRY(hipMemcpy(hd.data(), d_dense.as<uint64_t>() + (size_t)h * hd.size(), hd.size() * 8, hipMemcpyDeviceToHost));
      for (uint32_t s = 0; s <= k; s++)
        for (uint32_t v = 0; v < MGC_ANALYZE_DENSE_VALUES; v++)
          if (const uint64_t c = hd[(size_t)s * MGC_ANALYZE_DENSE_VALUES + v]) put(s, v, c);
    }
    const uint64_t lo = mgc::analyze_pack(h, 0, 0), hi = mgc::analyze_pack(h + 1, 0, 0);
    auto it = std::lower_bound(ovf.acc.begin(), ovf.acc.end(), lo, [](const Row &a, uint64_t key) { return a.key < key; });
    for (; it != ovf.acc.end() && it->key < hi; ++it) put((uint32_t)(it->key >> 32) & 127u, (uint32_t)it->key, it->n);
    // both tiers may hold the same (score, value) when the dense bound was switched between adds; rows are unique after this
    std::sort(out.begin(), out.end(), [](const Row &a, const Row &b) { return a.key < b.key; });
    size_t w = 0;
    for (size_t i = 0; i < out.size(); i++) {
      if (w && out[w - 1].key == out[i].key) out[w - 1].n += out[i].n;
      else out[w++] = out[i];
    }
    out.resize(w);
    rows_ok[which] = true;
    return MGC_OK;
  }
#undef AN_TRY
};

namespace {
bool which_ok(const mgc_analyze *a, int which) {
  if (which == MGC_ANALYZE_FORWARD || which == MGC_ANALYZE_REVERSE || (which == MGC_ANALYZE_COMBINED && a->type != MGC_ANALYZE_GC)) return true;
  set_err(nullptr, "meryl-analyze: no histogram %d in this report (-gc has forward and reverse only)", which);
  return false;
}
}  // namespace

extern "C" const char *mgc_analyze_error(void) { return mgc::thread_last_error().c_str(); }

extern "C" int mgc_dev_analyze_scores(const void *d_keys, uint64_t n, uint32_t k, int type, uint8_t *d_fscore, uint8_t *d_rscore, void *stream) {
  if (!k_ok(k)) return MGC_EINVAL;
  if (!type_ok(type)) { set_err(nullptr, "meryl-analyze: unknown report type %d", type); return MGC_EINVAL; }
  if (n && (!d_keys || !d_fscore || !d_rscore)) { set_err(nullptr, "mgc_dev_analyze_scores: NULL array"); return MGC_EINVAL; }
  if (n == 0) return MGC_OK;
  const hipError_t e = mgc::launch_analyze_scores(d_keys, n, k, type, d_fscore, d_rscore, (hipStream_t)stream);
  if (e == hipSuccess) return MGC_OK;
  set_err(nullptr, "analyze_scores: %s", hipGetErrorString(e));
  return MGC_EHIP;
}

extern "C" int mgc_analyze_open(uint32_t k, int type, int device, mgc_analyze **out) {
  if (out) *out = nullptr;
  if (!k_ok(k)) return MGC_EINVAL;
  if (!type_ok(type)) { set_err(nullptr, "meryl-analyze: unknown report type %d", type); return MGC_EINVAL; }
  if (!out) { set_err(nullptr, "mgc_analyze_open: NULL result pointer"); return MGC_EINVAL; }
  mgc_analyze *a = new mgc_analyze();
  a->k = k; a->kw = k > 32 ? 2u : 1u; a->type = type; a->device = device;
  memset(&a->info, 0, sizeof(a->info));
  // MGC_ANALYZE_DENSE=0 (measurements): no dense tier, every value takes the overflow list.  Read once, here.
  if (const char *e = getenv("MGC_ANALYZE_DENSE")) { if (e[0] == '0') a->dense = 0; }
  *out = a;
  return MGC_OK;
}

extern "C" void mgc_analyze_close(mgc_analyze *a) { delete a; }

extern "C" int mgc_analyze_add_device(mgc_analyze *a, const void *d_keys, const uint32_t *d_values, uint64_t n, void *stream) {
  if (!a) { set_err(nullptr, "mgc_analyze_add_device: NULL accumulator"); return MGC_EINVAL; }
  if (n && (!d_keys || !d_values)) { set_err(nullptr, "mgc_analyze_add_device: NULL array"); return MGC_EINVAL; }
  if (n == 0) return MGC_OK;
  const double t0 = now_s();
  int rc = a->init();
  if (rc == MGC_OK) rc = a->add(d_keys, d_values, n, (hipStream_t)stream);
  a->info.total_s += now_s() - t0;
  return rc;
}

extern "C" int mgc_analyze_add_database(mgc_analyze *a, const char *path, int host_threads) {
  if (!a) { set_err(nullptr, "mgc_analyze_add_database: NULL accumulator"); return MGC_EINVAL; }
  if (!path || !*path) { set_err(nullptr, "meryl-analyze: no database path"); return MGC_EINVAL; }
  mdb_reader *r = mdb_reader_open(path);
  if (!r) { set_err(nullptr, "meryl-analyze: cannot open '%s': %s", path, mdb_last_error()); return MGC_EINVAL; }
  mdb_info inf;
  mdb_reader_info(r, &inf);
  mdb_reader_close(r);
  if (inf.k != a->k) { set_err(nullptr, "meryl-analyze: '%s' holds %u-mers, the accumulator %u-mers", path, inf.k, a->k); return MGC_EINVAL; }
  const double t0 = now_s();
  int rc = a->init();
  if (rc == MGC_OK) rc = a->add_database(path, inf, host_threads);
  a->info.total_s += now_s() - t0;
  return rc;
}

extern "C" int mgc_analyze_result_rows(mgc_analyze *a, int which, uint64_t *n_rows) {
  if (!a || !n_rows) { set_err(nullptr, "mgc_analyze_result_rows: NULL argument"); return MGC_EINVAL; }
  if (!which_ok(a, which)) return MGC_EINVAL;
  const int rc = a->build(which);
  if (rc == MGC_OK) *n_rows = a->rows[which].size();
  return rc;
}

extern "C" int mgc_analyze_result(mgc_analyze *a, int which, uint32_t *scores, uint32_t *values, uint64_t *occurrences) {
  if (!a) { set_err(nullptr, "mgc_analyze_result: NULL accumulator"); return MGC_EINVAL; }
  if (!which_ok(a, which)) return MGC_EINVAL;
  const int rc = a->build(which);
  if (rc != MGC_OK) return rc;
  const std::vector<Row> &rows = a->rows[which];
  if (!rows.empty() && (!scores || !values || !occurrences)) { set_err(nullptr, "mgc_analyze_result: NULL array"); return MGC_EINVAL; }
  for (size_t i = 0; i < rows.size(); i++) {
    scores[i] = (uint32_t)(rows[i].key >> 32);
    values[i] = (uint32_t)rows[i].key;
    occurrences[i] = rows[i].n;
  }
  return MGC_OK;
}

extern "C" int mgc_analyze_write(mgc_analyze *a, const char *prefix) {
  if (!a) { set_err(nullptr, "mgc_analyze_write: NULL accumulator"); return MGC_EINVAL; }
  if (!prefix || !*prefix) { set_err(nullptr, "meryl-analyze: no output prefix"); return MGC_EINVAL; }
  struct Out { const char *name; int which; };
  static const Out gc[] = {{"GC", MGC_ANALYZE_FORWARD}, {"AT", MGC_ANALYZE_REVERSE}};
  static const Out ga[] = {{"GA_TC", MGC_ANALYZE_COMBINED}, {"GA", MGC_ANALYZE_FORWARD}, {"TC", MGC_ANALYZE_REVERSE}};
  static const Out gt[] = {{"GT_AC", MGC_ANALYZE_COMBINED}, {"GT", MGC_ANALYZE_FORWARD}, {"AC", MGC_ANALYZE_REVERSE}};
  const Out *outs = a->type == MGC_ANALYZE_GC ? gc : (a->type == MGC_ANALYZE_GA ? ga : gt);
  const int n_outs = a->type == MGC_ANALYZE_GC ? 2 : 3;
  for (int i = 0; i < n_outs; i++) {
    const int rc = a->build(outs[i].which);
    if (rc != MGC_OK) return rc;
  }
  for (int i = 0; i < n_outs; i++) {
    const std::string name = std::string(prefix) + "." + outs[i].name + ".hist";
    FILE *f = fopen(name.c_str(), "w");
    if (!f) { set_err(nullptr, "meryl-analyze: cannot create '%s'", name.c_str()); return MGC_EINVAL; }
    for (const Row &r : a->rows[outs[i].which])
      fprintf(f, "%u\t%u\t%lu\n", (unsigned)(r.key >> 32), (unsigned)(uint32_t)r.key, (unsigned long)r.n);
    if (fclose(f) != 0) { set_err(nullptr, "meryl-analyze: writing '%s' failed", name.c_str()); return MGC_EINVAL; }
  }
  return MGC_OK;
}

extern "C" int mgc_analyze_get_info(const mgc_analyze *a, mgc_analyze_info *info) {
  if (!a || !info) { set_err(nullptr, "mgc_analyze_get_info: NULL argument"); return MGC_EINVAL; }
  *info = a->info;
  return MGC_OK;
}
