// The read half of the one database-file loader (meryl_amd/csrc/mgc_dbfile.cpp, built with MGC_DBFILE_HOST_ONLY) against
// mdb_reader_read_file_ex, on small databases whose data files are framed canonically, framed in a way only the host decoder
// follows (the 8-byte lenmax field of a block's object doubled), or truncated.  Stand-alone; run under the address and
// undefined-behaviour sanitizers by tests/test_dbfile_host.py.   usage: dbfile_host <work directory>
#include "../../meryl_amd/csrc/mgc_dbfile.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <filesystem>
#include <string>
#include <vector>

namespace fs = std::filesystem;

static uint64_t g_checks = 0;
#define CHECK(c) do { g_checks++; if (!(c)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

struct Shape { const char *name; uint32_t k, w_prefix, label_size; uint32_t per_block; uint32_t skip_every; };

static std::string data_name(const std::string &dir, uint32_t ff) {
  std::string b = "/0x";
  for (int i = 5; i >= 0; i--) b += ((ff >> i) & 1) ? '1' : '0';
  return dir + b + ".merylData";
}

// every block: up to per_block ascending distinct suffixes; every skip_every-th prefix holds nothing (so some files are empty at w_prefix = 6)
static void write_db(const std::string &path, const Shape &s) {
  mdb_writer *w = mdb_writer_open_ex(path.c_str(), s.k, s.w_prefix, s.label_size, 0, 1);
  CHECK(w);
  const uint32_t sbits = 2 * s.k - s.w_prefix;
  for (uint64_t prefix = 0; prefix < (1ull << s.w_prefix); prefix++) {
    if (s.skip_every && prefix % s.skip_every == 1) continue;
    std::vector<uint64_t> lo, hi, lab;
    std::vector<uint32_t> cn;
    const uint64_t span = sbits >= 64 ? ~0ull : (1ull << sbits) - 1;
    const uint32_t n = (uint32_t)std::min<uint64_t>(1 + rnd() % s.per_block, span < 8 ? span + 1 : 8);
    uint64_t cur_lo = 0, cur_hi = 0;
    for (uint32_t i = 0; i < n; i++) {
      if (sbits <= 8) cur_lo = i;                                               // a handful: consecutive suffixes
      else { const uint64_t step = 1 + rnd() % (span / (2 * n) + 1); cur_lo += step; if (sbits > 64 && (rnd() & 3) == 0) cur_hi += 1 + rnd() % 5; }
      lo.push_back(cur_lo); hi.push_back(sbits > 64 ? (cur_hi & ((1ull << (sbits - 64)) - 1)) : 0);
      cn.push_back(1 + (uint32_t)(rnd() % 5));
      lab.push_back(rnd() & ((1ull << (s.label_size ? s.label_size : 1)) - 1));
    }
    const int rc = s.label_size ? mdb_writer_add_block_labelled(w, prefix, n, lo.data(), sbits > 64 ? hi.data() : nullptr, cn.data(), lab.data(), 0)
                                : mdb_writer_add_block(w, prefix, n, lo.data(), sbits > 64 ? hi.data() : nullptr, cn.data());
    CHECK(rc == MGC_OK);
  }
  CHECK(mdb_writer_close(w) == MGC_OK);
}

// doubles lenmax of the first block of file ff that holds k-mers; false: the file is empty
static bool make_host_only(const std::string &path, uint32_t ff) {
  mdb_reader *r = mdb_reader_open(path.c_str());
  CHECK(r);
  mdb_info inf;
  mdb_reader_info(r, &inf);
  std::vector<mdb_index_entry> idx((size_t)1 << inf.num_blocks_bits);
  CHECK(mdb_reader_file_index(r, ff, idx.data()) == MGC_OK);
  mdb_reader_close(r);
  for (const mdb_index_entry &e : idx) {
    if (!e.n_kmers) continue;
    FILE *f = fopen(data_name(path, ff).c_str(), "r+b");
    CHECK(f);
    uint64_t lenmax = 0;
    CHECK(fseek(f, (long)e.position, SEEK_SET) == 0 && fread(&lenmax, 8, 1, f) == 1);
    lenmax *= 2;
    CHECK(fseek(f, (long)e.position, SEEK_SET) == 0 && fwrite(&lenmax, 8, 1, f) == 1);
    CHECK(fclose(f) == 0);
    return true;
  }
  return false;
}

// every file of `path` through dbfile_read, against mdb_reader_read_file_ex; host_only[ff]: the file's framing is not canonical
static void check_db(const std::string &path, const std::vector<bool> &host_only, bool host_decode, bool want_labels) {
  mdb_reader *r = mdb_reader_open(path.c_str());
  CHECK(r);
  mdb_info inf;
  mdb_reader_info(r, &inf);
  const uint32_t kw = inf.k > 32 ? 2u : 1u;
  std::vector<mgc::DbFile> files(64);
  for (uint32_t ff = 0; ff < 64; ff++) {
    mgc::DbFile f;
    mgc::dbfile_read(r, ff, kw, host_decode, want_labels, &f);
    CHECK(f.rc == MGC_OK && f.msg.empty());
    uint64_t *lo = nullptr, *hi = nullptr, *lab = nullptr, n = 0;
    uint32_t *cn = nullptr;
    CHECK(mdb_reader_read_file_ex(r, ff, &lo, &hi, &cn, &lab, &n) == MGC_OK);
    CHECK(f.n == n);
    CHECK(f.raw == !(host_decode || host_only[ff]));
    if (f.raw) {
      CHECK(f.bytes && f.blocks && f.keys.empty() && !f.vals && !f.labels);
      CHECK(f.size == (uint64_t)fs::file_size(data_name(path, ff)));
      uint64_t total = 0;
      for (uint64_t b = 0; b < f.nb; b++) { CHECK(f.blocks[b].out_offset == total && f.blocks[b].n_kmers > 0); total += f.blocks[b].n_kmers; }
      CHECK(total == n);
      for (int i = 0; i < 16; i++) CHECK(f.bytes[f.size + i] == 0);                 // the slack the device decoder may read
    } else {
      CHECK(!f.bytes && !f.blocks && f.keys.size() == (size_t)kw * n);
      for (uint64_t j = 0; j < n; j++) {
        CHECK(f.keys[kw * j] == lo[j]);
        if (kw == 2) CHECK(f.keys[2 * j + 1] == hi[j]);
        CHECK(f.vals[j] == cn[j]);
      }
      if (want_labels && inf.label_size) { CHECK(f.labels); for (uint64_t j = 0; j < n; j++) CHECK(f.labels[j] == lab[j]); }
      else CHECK(!f.labels);                                                         // absent when not asked for, or not stored
    }
    mdb_free(lo); mdb_free(hi); mdb_free(cn); mdb_free(lab);
    files[ff] = std::move(f);                                                        // records move: the vector frees them
    CHECK(!f.bytes && !f.vals && f.keys.empty());
  }
  mgc::DbFile again = std::move(files[3]);
  mgc::dbfile_read(r, 5, kw, host_decode, want_labels, &again);                      // a record is reusable
  CHECK(again.rc == MGC_OK && again.n == files[5].n);
  mdb_reader_close(r);
}

int main(int argc, char **argv) {
  if (argc != 2) { fprintf(stderr, "usage: dbfile_host <work directory>\n"); return 2; }
  const std::string work = argv[1];
  const Shape shapes[] = {{"k4", 4, 6, 0, 4, 3}, {"k16", 16, 12, 0, 6, 0}, {"k40", 40, 8, 9, 7, 0}};
  CHECK(!mgc::decode_on_host() || getenv("MGC_DECODE_HOST"));
  for (const Shape &s : shapes) {
    const std::string orig = work + "/" + s.name + ".meryl", mixed = work + "/" + s.name + ".mixed.meryl", all = work + "/" + s.name + ".all.meryl";
    write_db(orig, s);
    fs::copy(orig, mixed, fs::copy_options::recursive);
    fs::copy(orig, all, fs::copy_options::recursive);
    std::vector<bool> none(64, false), some(64, false), every(64, false);
    for (uint32_t ff : {0u, 5u, 33u, 63u}) some[ff] = make_host_only(mixed, ff);
    uint32_t n_every = 0;
    for (uint32_t ff = 0; ff < 64; ff++) { every[ff] = make_host_only(all, ff); n_every += every[ff]; }
    CHECK(some[5] || some[0] || some[33] || some[63]);
    CHECK(n_every >= 32);
    if (s.k == 4) CHECK(n_every < 64);                                               // this shape has empty files
    for (int labels = 0; labels < 2; labels++) {
      check_db(orig, none, false, labels);
      check_db(mixed, some, false, labels);
      check_db(all, every, false, labels);
      check_db(orig, none, true, labels);
      check_db(mixed, some, true, labels);
      check_db(all, every, true, labels);
    }
    // a truncated data file: the file's error and message, nothing kept
    const std::string cut = work + "/" + s.name + ".cut.meryl";
    fs::copy(orig, cut, fs::copy_options::recursive);
    uint32_t victim = 9;
    while (fs::file_size(data_name(cut, victim)) == 0) victim++;
    fs::resize_file(data_name(cut, victim), fs::file_size(data_name(cut, victim)) / 2);
    mdb_reader *r = mdb_reader_open(cut.c_str());
    CHECK(r);
    for (int host_decode = 0; host_decode < 2; host_decode++) {
      mgc::DbFile f;
      mgc::dbfile_read(r, victim, s.k > 32 ? 2u : 1u, host_decode != 0, true, &f);
      CHECK(f.rc != MGC_OK && f.rc != MGC_EUNSUPPORTED && !f.msg.empty());
      CHECK(!f.raw && !f.bytes && !f.blocks);
      mgc::dbfile_read(r, victim - 1, s.k > 32 ? 2u : 1u, host_decode != 0, true, &f);       // its neighbour is fine, in the same record
      CHECK(f.rc == MGC_OK && f.msg.empty());
    }
    mdb_reader_close(r);
  }
  std::string msg;
  CHECK(mgc::dbfile_decode_rc(0, &msg) == MGC_OK && msg.empty());
  CHECK(mgc::dbfile_decode_rc(3, &msg) == MGC_EINVAL && msg == "corrupt block in a database file (device decoder, code 3)");
  printf("ok %llu\n", (unsigned long long)g_checks);
  return 0;
}
