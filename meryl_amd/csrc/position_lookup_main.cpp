// position_lookup_main.cpp -- `position-lookup`: where the k-mers of query sequences land on a reference, and how often.
//
// Keeps the reference tool's surface (src/meryl-lookup/position-lookup.C:398-423):
//   position-lookup -m <db.meryl> -s <ref.fa[.gz]> [-hpq out] [-mpb out] [-qpb out] <query.fa|fq[.gz]> ...
//     -hpq  per query, in input order:  nPer <TAB> tCov <TAB> length <TAB> ident                          (:262)
//           tCov = its k-mers found in the database, nPer = the sum of their numbers of positions on the reference
//     -mpb  per reference base with a non-zero count:  position <BLANK> count                             (:345-348)
//           count = the query k-mers, over all queries, equal to the k-mer that begins at the base
//     -qpb  the same with the number of distinct query sequences                                          (:360-363)
// A word that is neither an option nor an existing file is "unknown option '<w>'", exit 1, as there.  Positions are 0-based
// inside their sequence.  With one reference sequence -mpb / -qpb are the reference's files byte for byte; with several, the
// reference folds them onto one axis -- here a line `# <ident>` precedes the lines of every sequence that has any (an
// extension).  Only the canonical k-mer of a window is looked up (:198), and a k-mer's number of positions is counted on the
// reference given with -s, not taken from its value (include/meryl_positions.h).  Outputs are written uncompressed.
//
// The database goes into the device-resident lookup table, the reference into the position index over it
// (mgc_posidx_build); the queries go to the device in batches of whole sequences (mgc_paint_add).  The reference's batches are
// 4096 sequences or 16 Mbp (:373), sized for its worker threads; here a batch is up to 128 Mi bases with no limit on the
// sequences (MGC_POSLOOKUP_BATCH overrides the number of bases) -- the results do not depend on it.  The text is formatted on
// the host: the lines are sparse.
#include "../../include/meryl_gpu_count.h"
#include "../../include/meryl_positions.h"

#include <hip/hip_runtime.h>

#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace {
[[noreturn]] void die(const char *fmt, const char *a = "") {
  fprintf(stderr, fmt, a);
  fprintf(stderr, "\n");
  exit(1);
}
}  // namespace

#include "mgc_fastx.hpp"               // Seqs, parse_text, read_fastx_text (they call die)

namespace {
bool compressed_name(const std::string &n) {
  for (const char *suf : {".gz", ".bz2", ".xz", ".zst"})
    if (n.size() > strlen(suf) && n.compare(n.size() - strlen(suf), std::string::npos, suf) == 0) return true;
  return false;
}
bool file_exists(const char *path) {
  FILE *f = fopen(path, "rb");
  if (!f) return false;
  fclose(f);
  return true;
}
void hip(hipError_t e, const char *what) {
  if (e != hipSuccess) { fprintf(stderr, "ERROR: %s: %s\n", what, hipGetErrorString(e)); exit(1); }
}
FILE *open_out(const std::string &name) {
  FILE *f = fopen(name.c_str(), "w");
  if (!f) die("ERROR: cannot write '%s'.", name.c_str());
  return f;
}
void close_out(FILE *f, const std::string &name) {
  if (fclose(f) != 0) die("ERROR: cannot write '%s'.", name.c_str());
}

// saveMerPerBase / saveQueryPerBase (:340-364): `position count` for every base with a non-zero count
void write_per_base(const std::string &name, const std::vector<uint32_t> &count, const Seqs &ref) {
  FILE *f = open_out(name);
  const uint64_t n_seq = ref.names.size();
  for (uint64_t s = 0; s < n_seq; s++) {
    bool any = false;
    for (uint64_t i = ref.start[s]; i < ref.start[s + 1]; i++) {
      if (!count[i]) continue;
      if (!any && n_seq > 1) fprintf(f, "# %s\n", ref.names[s].c_str());
      any = true;
      fprintf(f, "%" PRIu64 " %u\n", i - ref.start[s], count[i]);
    }
  }
  close_out(f, name);
}
}  // namespace

int main(int argc, char **argv) {
  std::string db, ref_name, hpq_name, mpb_name, qpb_name;
  std::vector<std::string> queries;
  for (int a = 1; a < argc; a++) {
    const std::string w = argv[a];
    if (w == "-m" && a + 1 < argc) db = argv[++a];
    else if (w == "-s" && a + 1 < argc) ref_name = argv[++a];
    else if (w == "-hpq" && a + 1 < argc) hpq_name = argv[++a];
    else if (w == "-mpb" && a + 1 < argc) mpb_name = argv[++a];
    else if (w == "-qpb" && a + 1 < argc) qpb_name = argv[++a];
    else if (file_exists(argv[a])) queries.push_back(w);
    else { fprintf(stderr, "unknown option '%s'\n", argv[a]); return 1; }          // :420-421
  }
  // before any database or device is touched
  const char *usage = "usage: %s -m <db.meryl> -s <ref.fa[.gz]> [-hpq out] [-mpb out] [-qpb out] <query.fa|fq[.gz]> ...\n";
  if (db.empty()) { fprintf(stderr, "No meryl database (-m) supplied.\n"); fprintf(stderr, usage, argv[0]); return 1; }
  if (ref_name.empty()) { fprintf(stderr, "No reference sequence (-s) supplied.\n"); fprintf(stderr, usage, argv[0]); return 1; }
  if (hpq_name.empty() && mpb_name.empty() && qpb_name.empty()) {
    fprintf(stderr, "No output (-hpq, -mpb, -qpb) supplied.\n");
    fprintf(stderr, usage, argv[0]);
    return 1;
  }
  for (const std::string *o : {&hpq_name, &mpb_name, &qpb_name})
    if (compressed_name(*o)) die("ERROR: output '%s' names a compressed file; this build writes position reports uncompressed only.", o->c_str());
  uint64_t batch_bases = 128ull << 20;
  if (getenv("MGC_POSLOOKUP_BATCH")) batch_bases = strtoull(getenv("MGC_POSLOOKUP_BATCH"), nullptr, 10);
  if (batch_bases >= (1ull << 32)) batch_bases = (1ull << 32) - 1;

  fprintf(stderr, "\nLoading kmers from '%s' into lookup table.\n", db.c_str());
  mgc_lookup *table = mgc_lookup_load(db.c_str(), 0, UINT64_MAX, -1, 0);
  if (!table) die("ERROR: %s", mgc_lookup_error());

  Seqs ref;
  {
    std::string text;
    read_fastx_text(ref_name, text);
    parse_text(text, ref);
  }
  uint8_t *d_ref = nullptr;
  hip(hipMalloc(reinterpret_cast<void **>(&d_ref), ref.bases.size() + 1), "hipMalloc");
  hip(hipMemcpy(d_ref, ref.bases.data(), ref.bases.size(), hipMemcpyHostToDevice), "upload");
  fprintf(stderr, "Loading positions of those kmers in '%s'.\n", ref_name.c_str());
  mgc_posidx *idx = mgc_posidx_build(table, d_ref, ref.bases.size(), nullptr);
  if (!idx) die("ERROR: %s", mgc_lookup_error());
  (void)hipFree(d_ref);
  mgc_posidx_info info;
  mgc_posidx_get_info(idx, &info);
  fprintf(stderr, "  %" PRIu64 " %u-mers, %" PRIu64 " reference bases, %" PRIu64 " positions in %" PRIu64 " lists (longest %" PRIu64 ").\n",
          info.n_kmers, info.k, info.n_ref_bases, info.n_placed, info.n_slots_used, info.longest_list);

  const uint32_t what = (hpq_name.empty() ? 0u : MGC_PAINT_HITS) | (mpb_name.empty() ? 0u : MGC_PAINT_MERS) | (qpb_name.empty() ? 0u : MGC_PAINT_QUERIES);
  mgc_paint *paint = mgc_paint_open(idx, what);
  if (!paint) die("ERROR: %s", mgc_lookup_error());
  FILE *hpq = hpq_name.empty() ? nullptr : open_out(hpq_name);

  uint8_t *d_bases = nullptr;
  uint64_t *d_start = nullptr;
  uint32_t *d_per = nullptr, *d_cov = nullptr;
  uint64_t cap_bases = 0, cap_seq = 0, batch_id = 0;
  std::vector<uint64_t> start;
  std::vector<uint32_t> per, cov;
  for (const std::string &qn : queries) {
    Seqs q;
    {
      std::string text;
      read_fastx_text(qn, text);
      parse_text(text, q);
    }
    const uint64_t n_seq = q.names.size();
    for (uint64_t s0 = 0; s0 < n_seq;) {                        // loadBatch (:154-186): whole sequences, at least one
      uint64_t s1 = s0 + 1;
      while (s1 < n_seq && q.start[s1 + 1] - q.start[s0] <= batch_bases) s1++;
      const uint64_t b0 = q.start[s0], nb = q.start[s1] - b0, ns = s1 - s0;
      if (nb >= (1ull << 32)) die("ERROR: a sequence of '%s' holds 2^32 bases or more.", qn.c_str());
      if (nb > cap_bases) {
        if (d_bases) (void)hipFree(d_bases);
        hip(hipMalloc(reinterpret_cast<void **>(&d_bases), nb + 1), "hipMalloc");
        cap_bases = nb;
      }
      if (ns > cap_seq) {
        if (d_start) { (void)hipFree(d_start); (void)hipFree(d_per); (void)hipFree(d_cov); }
        hip(hipMalloc(reinterpret_cast<void **>(&d_start), 8 * (ns + 1)), "hipMalloc");
        hip(hipMalloc(reinterpret_cast<void **>(&d_per), 4 * ns), "hipMalloc");
        hip(hipMalloc(reinterpret_cast<void **>(&d_cov), 4 * ns), "hipMalloc");
        cap_seq = ns;
      }
      start.resize(ns + 1);
      for (uint64_t s = 0; s <= ns; s++) start[s] = q.start[s0 + s] - b0;
      hip(hipMemcpy(d_bases, q.bases.data() + b0, nb, hipMemcpyHostToDevice), "upload");
      hip(hipMemcpy(d_start, start.data(), 8 * (ns + 1), hipMemcpyHostToDevice), "upload");
      fprintf(stderr, "Loaded batch %4" PRIu64 " with %5" PRIu64 " sequences and %8" PRIu64 " bases.\n", batch_id++, ns, nb - ns);
      if (mgc_paint_add(paint, d_bases, nb, d_start, ns, d_per, d_cov, nullptr) != MGC_OK) die("ERROR: %s", mgc_lookup_error());
      if (hpq) {
        per.resize(ns); cov.resize(ns);
        hip(hipMemcpy(per.data(), d_per, 4 * ns, hipMemcpyDeviceToHost), "download");
        hip(hipMemcpy(cov.data(), d_cov, 4 * ns, hipMemcpyDeviceToHost), "download");
        for (uint64_t s = 0; s < ns; s++)                       // :262; a sequence's bases are followed by one '.'
          fprintf(hpq, "%u\t%u\t%" PRIu64 "\t%s\n", per[s], cov[s], start[s + 1] - start[s] - 1, q.names[s0 + s].c_str());
      }
      s0 = s1;
    }
  }
  if (hpq) close_out(hpq, hpq_name);

  if (!mpb_name.empty() || !qpb_name.empty()) {
    uint32_t *d_out = nullptr;
    std::vector<uint32_t> count(ref.bases.size());
    hip(hipMalloc(reinterpret_cast<void **>(&d_out), 4 * (ref.bases.size() + 1)), "hipMalloc");
    for (int which = 0; which < 2; which++) {
      const std::string &name = which ? qpb_name : mpb_name;
      if (name.empty()) continue;
      if (mgc_paint_get(paint, which ? MGC_PAINT_QUERIES : MGC_PAINT_MERS, d_out, nullptr) != MGC_OK) die("ERROR: %s", mgc_lookup_error());
      hip(hipDeviceSynchronize(), "paint");
      if (!count.empty()) hip(hipMemcpy(count.data(), d_out, 4 * count.size(), hipMemcpyDeviceToHost), "download");
      write_per_base(name, count, ref);
    }
    (void)hipFree(d_out);
  }
  if (d_bases) (void)hipFree(d_bases);
  if (d_start) { (void)hipFree(d_start); (void)hipFree(d_per); (void)hipFree(d_cov); }
  mgc_paint_close(paint);
  mgc_posidx_free(idx);
  mgc_lookup_free(table);
  return 0;
}
