// mgc_dbfile.hpp -- data file `ff` of a database -> (k-mers, values[, labels]) in HBM, for everything that consumes whole databases
// (mgc_eval.cpp, mgc_analyze.cpp, mgc_lookup.hip).  Two steps, because the callers thread them differently: READ (host threads; no
// HIP -- with MGC_DBFILE_HOST_ONLY this header and mgc_dbfile.cpp compile without it) and UPLOAD + DECODE (the device).  Internal.
#pragma once

#include "../../include/meryl_db.h"

#include <string>
#include <utility>
#include <vector>

namespace mgc {
// MGC_DECODE_HOST=1 (tests): every file takes the host decoder.  Every entry point reads it once per call.
bool decode_on_host();

// One data file as a host thread read it: raw (the file's bytes and one descriptor per block that holds k-mers; decoded on the
// device, mgc_decode.hip) or host-decoded (a file framed in a way only the host decoder follows, or decode_on_host()).
struct DbFile {
  unsigned char *bytes = nullptr; mdb_raw_block *blocks = nullptr;     // raw
  uint64_t size = 0, nb = 0;
  std::vector<uint64_t> keys;                                         // host-decoded: kw words per k-mer, {lo, hi} interleaved
  uint32_t *vals = nullptr;
  uint64_t *labels = nullptr;                                         //   only when asked for and the database stores some
  uint64_t n = 0;                                                     // k-mers in the file
  bool raw = false;
  int rc = MGC_OK;
  std::string msg;                                                    // mdb_last_error() of the read that failed

  DbFile() = default;
  DbFile(const DbFile &) = delete;
  DbFile &operator=(const DbFile &) = delete;
  DbFile(DbFile &&o) noexcept { *this = std::move(o); }
  DbFile &operator=(DbFile &&o) noexcept;
  ~DbFile() { drop(); }
  void drop();                                                        // the host copies go; n, rc and msg stay
};

// raw unless host_decode; MGC_EUNSUPPORTED from the raw reader -> the host decoder; anything else is the file's error (f->rc, f->msg)
void dbfile_read(mdb_reader *r, uint32_t ff, uint32_t kw, bool host_decode, bool want_labels, DbFile *f);

// a non-zero error word of the device decoder -> MGC_EINVAL and the one message
int dbfile_decode_rc(uint32_t err_word, std::string *msg);
}  // namespace mgc

#ifndef MGC_DBFILE_HOST_ONLY
#include "mgc_devbuf.hpp"

namespace mgc {
struct DbFileScratch { DBuf file, blocks, err; };                     // a raw file's bytes, its block array, the decoder's error word

// Queues one file's way to d_keys / d_vals / d_labels (null: no labels wanted) on st.  Raw: error word cleared, bytes and block
// array copied, decoded, error word copied back to *h_err; host-decoded: the arrays copied, *h_err = 0.  Nothing is synchronised:
// the caller waits for st before it reuses the scratch or drops f, and before it reads *h_err.
hipError_t dbfile_upload(const DbFile &f, const mdb_info &inf, uint32_t kw, DbFileScratch &sc, void *d_keys, uint32_t *d_vals,
                         uint64_t *d_labels, uint32_t *h_err, hipStream_t st);
}  // namespace mgc
#endif
