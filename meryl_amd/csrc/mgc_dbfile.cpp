// mgc_dbfile.cpp -- the one loader of a database's data files (mgc_dbfile.hpp): read by a host thread, then uploaded and decoded
// on the device (mgc_decode.hip: one thread per block) or, where only the host decoder follows the file's framing, uploaded as arrays.
#include "mgc_dbfile.hpp"

#include <cstdlib>
#include <cstring>

namespace mgc {
bool decode_on_host() { const char *e = getenv("MGC_DECODE_HOST"); return e && e[0] == '1'; }

void DbFile::drop() {
  mdb_free(bytes); mdb_free(blocks); mdb_free(vals); mdb_free(labels);
  bytes = nullptr; blocks = nullptr; vals = nullptr; labels = nullptr;
  std::vector<uint64_t>().swap(keys);
}

DbFile &DbFile::operator=(DbFile &&o) noexcept {
  if (this == &o) return *this;
  drop();
  bytes = o.bytes; blocks = o.blocks; vals = o.vals; labels = o.labels;
  o.bytes = nullptr; o.blocks = nullptr; o.vals = nullptr; o.labels = nullptr;
  size = o.size; nb = o.nb; n = o.n; raw = o.raw; rc = o.rc;
  keys = std::move(o.keys);
  msg = std::move(o.msg);
  return *this;
}

void dbfile_read(mdb_reader *r, uint32_t ff, uint32_t kw, bool host_decode, bool want_labels, DbFile *f) {
  f->drop();
  f->size = f->nb = f->n = 0; f->raw = false; f->rc = MGC_OK; f->msg.clear();
  mdb_info inf;
  mdb_reader_info(r, &inf);
  if (!host_decode) {
    const int rc = mdb_reader_raw_file(r, ff, &f->bytes, &f->size, &f->blocks, &f->nb, &f->n);
    if (rc == MGC_OK) { f->raw = true; return; }
    if (rc != MGC_EUNSUPPORTED) { f->rc = rc; f->msg = mdb_last_error(); return; }
  }
  uint64_t *lo = nullptr, *hi = nullptr;
  f->rc = mdb_reader_read_file_ex(r, ff, &lo, &hi, &f->vals, (want_labels && inf.label_size) ? &f->labels : nullptr, &f->n);
  if (f->rc != MGC_OK) f->msg = mdb_last_error();
  else {
    f->keys.resize((size_t)kw * f->n);
    if (kw == 1) { if (f->n) memcpy(f->keys.data(), lo, 8 * f->n); }
    else for (uint64_t j = 0; j < f->n; j++) { f->keys[2 * j] = lo[j]; f->keys[2 * j + 1] = hi[j]; }
  }
  mdb_free(lo); mdb_free(hi);
}

int dbfile_decode_rc(uint32_t err_word, std::string *msg) {
  if (!err_word) return MGC_OK;
  *msg = "corrupt block in a database file (device decoder, code " + std::to_string(err_word) + ")";
  return MGC_EINVAL;
}
}  // namespace mgc

#ifndef MGC_DBFILE_HOST_ONLY
#include "mgc_device.h"

namespace mgc {
hipError_t dbfile_upload(const DbFile &f, const mdb_info &inf, uint32_t kw, DbFileScratch &sc, void *d_keys, uint32_t *d_vals,
                         uint64_t *d_labels, uint32_t *h_err, hipStream_t st) {
  *h_err = 0;
  if (!f.n) return hipSuccess;
  hipError_t e;
  if (f.raw) {
    e = sc.file.ensure(f.size + 16);
    if (e == hipSuccess) e = sc.blocks.ensure(sizeof(mdb_raw_block) * f.nb);
    if (e == hipSuccess) e = sc.err.ensure(256);
    if (e == hipSuccess) e = hipMemsetAsync(sc.err.p, 0, 4, st);
    if (e == hipSuccess) e = hipMemcpyAsync(sc.file.p, f.bytes, f.size + 16, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(sc.blocks.p, f.blocks, sizeof(mdb_raw_block) * f.nb, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = launch_decode_blocks(sc.file.p, sc.blocks.p, f.nb, inf.suffix_size, inf.label_size, kw, d_keys, d_vals, sc.err.as<uint32_t>(), st, d_labels);
    if (e == hipSuccess) e = hipMemcpyAsync(h_err, sc.err.p, 4, hipMemcpyDeviceToHost, st);
  } else {
    e = hipMemcpyAsync(d_keys, f.keys.data(), 8 * (size_t)kw * f.n, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_vals, f.vals, 4 * f.n, hipMemcpyHostToDevice, st);
    if (e == hipSuccess && d_labels && f.labels) e = hipMemcpyAsync(d_labels, f.labels, 8 * f.n, hipMemcpyHostToDevice, st);
  }
  return e;
}
}  // namespace mgc
#endif
