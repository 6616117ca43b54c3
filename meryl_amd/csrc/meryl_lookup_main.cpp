// meryl_lookup_main.cpp -- `meryl-lookup`: the k-mers of the sequences of a FASTA/FASTQ file looked up in meryl databases.
//
// Keeps the reference tool's surface (src/meryl-lookup/meryl-lookup.C:150-368 options and their checks) for these modes:
//   meryl-lookup -existence -sequence <in.fa[.gz]> -mers <db.meryl> [<db2.meryl> ...] [-min v] [-max v] [-output out.tsv]
//     per sequence:  name <TAB> kmersInSequence { <TAB> kmersInDB <TAB> kmersFound } per database   (existence.C:48-132)
//   meryl-lookup -bed | -bed-runs -sequence <in.fa> -mers <db.meryl> [...] [-labels <l1> ...] [-min v] [-max v] [-output out.bed]
//     one line per k-mer (per run of k-mers) found, per database when labels are given           (dump.C:251-364)
//   meryl-lookup -wig-count | -wig-depth -sequence <in.fa> -mers <db.meryl> [...] [-min v] [-max v] [-output out.wig]
//     per base: the summed value of the k-mer starting there / the depth of found k-mers of the FIRST database over it
//                                                                                                  (dump.C:139-244, 368-405)
// Every database is loaded into the device-resident exact lookup table (include/meryl_lookup.h = merylExactLookup); the
// sequences go to the device as one base stream with '.' after each.  The position reports are formatted on the device
// (mgc_lookup_report) and written as they come; -output is optional (stdout) and must not name a compressed file.
//   meryl-lookup -include | -exclude [-10x] -sequence <R1.fq[.gz]> [<R2.fq[.gz]>] -mers <db.meryl> [-min v] [-max v] -output <o1> [<o2>]
//     the reads (read pairs) with at least one / without any k-mer of the database, "ident nKmers=<found>" as the header;
//     -10x leaves the first 23 bases of the first input out                                          (include-exclude.C)
//     streamed in pieces through mgc_lookup_filter_files: records are found, looked up and written as text on the device.
// -dump (no option of the reference tool) is not part of this build.
#include "../../include/meryl_gpu_count.h"
#include "../../include/meryl_lookup.h"
#include "../../include/meryl_seq.h"

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
enum Op { OP_NONE, OP_EXISTENCE, OP_BED, OP_BED_RUNS, OP_WIG_COUNT, OP_WIG_DEPTH, OP_INCLUDE, OP_EXCLUDE };

const char *op_name(Op op) {                                  // toString(lookupOp), meryl-lookup.H:38-50 (-bed-runs is opBED)
  switch (op) {
    case OP_EXISTENCE: return "-existence";
    case OP_BED: case OP_BED_RUNS: return "-bed";
    case OP_WIG_COUNT: return "-wig-count";
    case OP_WIG_DEPTH: return "-wig-depth";
    case OP_INCLUDE: return "-include";
    case OP_EXCLUDE: return "-exclude";
    default: return "(not supplied)";
  }
}

bool compressed_name(const std::string &n) {
  for (const char *suf : {".gz", ".bz2", ".xz", ".zst"})
    if (n.size() > strlen(suf) && n.compare(n.size() - strlen(suf), std::string::npos, suf) == 0) return true;
  return false;
}

int write_piece(const void *data, uint64_t n, void *user) {
  return fwrite(data, 1, (size_t)n, static_cast<FILE *>(user)) == (size_t)n ? 0 : 1;
}
}  // namespace

int main(int argc, char **argv) {
  std::string seq_name, seq_name2, out_name, out_name2;
  std::vector<std::string> dbs, labels;
  uint64_t vmin = 0, vmax = UINT64_MAX;
  Op op = OP_NONE;
  bool estimate = false, is10x = false;
  double max_memory_gb = 0.0;                                 // -memory: 0 = whatever the device has
  for (int a = 1; a < argc; a++) {
    const std::string w = argv[a];
    if (w == "-existence") op = OP_EXISTENCE;
    else if (w == "-bed") op = OP_BED;
    else if (w == "-bed-runs") op = OP_BED_RUNS;
    else if (w == "-wig-count") op = OP_WIG_COUNT;
    else if (w == "-wig-depth") op = OP_WIG_DEPTH;
    else if (w == "-include") op = OP_INCLUDE;
    else if (w == "-exclude") op = OP_EXCLUDE;
    else if (w == "-10x") is10x = true;
    else if (w == "-sequence" && a + 1 < argc) {              // meryl-lookup.C:160-164: an optional second input
      seq_name = argv[++a];
      if (a + 1 < argc && argv[a + 1][0] != '-') seq_name2 = argv[++a];
    } else if (w == "-output" && a + 1 < argc) {              // :174-178
      out_name = argv[++a];
      if (a + 1 < argc && argv[a + 1][0] != '-') out_name2 = argv[++a];
    }
    else if (w == "-min" && a + 1 < argc) vmin = strtoull(argv[++a], nullptr, 10);
    else if (w == "-max" && a + 1 < argc) vmax = strtoull(argv[++a], nullptr, 10);
    else if (w == "-threads" && a + 1 < argc) ++a;
    else if (w == "-memory" && a + 1 < argc) max_memory_gb = strtod(argv[++a], nullptr);
    else if (w == "-estimate") estimate = true;
    else if (w == "-mers") { while (a + 1 < argc && argv[a + 1][0] != '-') dbs.push_back(argv[++a]); }
    else if (w == "-labels") { while (a + 1 < argc && argv[a + 1][0] != '-') labels.push_back(argv[++a]); }
    else if (w == "-dump")
      die("ERROR: mode '%s' is not part of this build (-existence, -bed, -bed-runs, -wig-count, -wig-depth, -include, -exclude only).", w.c_str());
    else die("ERROR: unknown option '%s'.", w.c_str());
  }
  // lookupGlobal::checkInvalid (meryl-lookup.C:306-368), before any database or device is touched
  if (op == OP_NONE && !estimate) die("No report-type (-bed, -wig-count, -wig-depth, -existence, -include, -exclude) supplied.");
  const bool filtering = op == OP_INCLUDE || op == OP_EXCLUDE;
  if (filtering) {                                            // :328-330, :346-358, :362-367
    if (!seq_name.empty() && out_name.empty()) die("No output file (-output) supplied.");
    if (!seq_name2.empty() && out_name2.empty()) die("No second output file (-output) supplied for second input (-input) file.");
    if (seq_name2.empty() && !out_name2.empty()) die("No second input file (-input) supplied for second output (-output) file.");
    if (dbs.size() > 1) die("Only one meryl database (-mers) supported for %s.", op_name(op));
    if (!labels.empty()) die("Labels (-labels) not supported for %s.", op_name(op));
    for (const std::string *o : {&out_name, &out_name2})
      if (compressed_name(*o)) die("ERROR: output '%s' names a compressed file; this build writes position reports uncompressed only.", o->c_str());
  } else if (op != OP_NONE) {
    if (!seq_name2.empty()) die("Only one input sequence (-sequence) supported for %s.", op_name(op));
    if (!out_name2.empty()) die("Only one output file (-output) supported for %s.", op_name(op));
    if (op != OP_BED && op != OP_BED_RUNS && !labels.empty()) die("Labels (-labels) not supported for %s.", op_name(op));
    if (op != OP_EXISTENCE && compressed_name(out_name))
      die("ERROR: output '%s' names a compressed file; this build writes position reports uncompressed only.", out_name.c_str());
    if (dbs.size() > MGC_LOOKUP_MAX_TABLES && op != OP_EXISTENCE) die("ERROR: at most 32 databases (-mers) for %s.", op_name(op));
  }
  if (op == OP_NONE || (seq_name.empty() && !estimate) || dbs.empty()) {
    fprintf(stderr, "usage: %s -existence | -bed | -bed-runs | -wig-count | -wig-depth -sequence <in.fa|fq[.gz]> -mers <db.meryl> [...] "
                    "[-labels l ...] [-min v] [-max v] [-memory GB] [-estimate] [-output out]\n"
                    "       %s -include | -exclude [-10x] -sequence <in1> [<in2>] -mers <db.meryl> [-min v] [-max v] -output <out1> [<out2>]\n",
            argv[0], argv[0]);
    return 1;
  }

  // meryl-lookup.C:62-87: the memory every table will need, BEFORE anything is loaded (here: device memory, from the databases'
  // own value histograms -- no device is touched); -estimate stops after the report, -memory is the limit it is held against
  double required_gb = 0.0;
  for (const std::string &d : dbs) {
    fprintf(stderr, "\nEstimating memory usage for '%s'.\n", d.c_str());
    mgc_lookup_info est;
    if (mgc_lookup_estimate(d.c_str(), vmin, vmax, &est) != MGC_OK) die("ERROR: %s", mgc_lookup_error());
    fprintf(stderr, "  %" PRIu64 " of %" PRIu64 " %u-mers kept, %.3f GB of device memory.\n", est.n_kmers, est.n_kmers_in_db, est.k,
            (double)est.device_bytes / 1024.0 / 1024.0 / 1024.0);
    required_gb += (double)est.device_bytes / 1024.0 / 1024.0 / 1024.0;
  }
  fprintf(stderr, "\nMemory required:  %.3f GB\n", required_gb);
  if (max_memory_gb > 0.0) {
    fprintf(stderr, "Memory limit:     %.3f GB\n", max_memory_gb);
    if (required_gb > max_memory_gb) { fprintf(stderr, "\nNot enough memory to load databases.  Increase -memory.\n"); return 1; }
  }
  if (estimate) { fprintf(stderr, "\nStopping after memory estimated reported; -estimate option enabled.\n"); return 0; }

  if (filtering) {                                            // filter(), include-exclude.C:137-154
    FILE *outs[2] = {nullptr, nullptr};
    const std::string *onames[2] = {&out_name, &out_name2};
    const uint32_t n_in = seq_name2.empty() ? 1u : 2u;
    for (uint32_t i = 0; i < n_in; i++)
      if (!(outs[i] = fopen(onames[i]->c_str(), "w"))) die("ERROR: cannot write '%s'.", onames[i]->c_str());
    fprintf(stderr, "\nLoading kmers from '%s' into lookup table.\n", dbs[0].c_str());
    mgc_lookup *t = mgc_lookup_load(dbs[0].c_str(), vmin, vmax, -1, 0);
    if (!t) die("ERROR: %s", mgc_lookup_error());
    if (is10x)
      fprintf(stderr, "\nRunning in 10x mode. The first 23 bp of every sequence in %s will be ignored while looking up.\n", seq_name.c_str());
    uint64_t batch = 0;                                       // bytes per piece of input (MGC_LOOKUP_BATCH overrides the default)
    if (getenv("MGC_LOOKUP_BATCH")) batch = strtoull(getenv("MGC_LOOKUP_BATCH"), nullptr, 10);
    mgc_filter_result tot;
    const int rc = mgc_lookup_filter_files(t, op == OP_INCLUDE ? MGC_FILTER_INCLUDE : MGC_FILTER_EXCLUDE, is10x ? 23u : 0u, seq_name.c_str(),
                                           n_in == 2 ? seq_name2.c_str() : nullptr, batch, write_piece, outs[0],
                                           n_in == 2 ? write_piece : nullptr, outs[1], &tot);
    for (uint32_t i = 0; i < n_in; i++)
      if (fclose(outs[i]) != 0) die("ERROR: cannot write '%s'.", onames[i]->c_str());
    if (rc != MGC_OK) die("ERROR: %s", mgc_lookup_error());
    // the reference passes the two numbers the other way round (include-exclude.C:153); here the sentence is true
    fprintf(stderr, "\nIncluding %" PRIu64 " reads (or read pairs) out of %" PRIu64 ".\n", tot.n_kept, tot.n_records);
    mgc_lookup_free(t);
    return 0;
  }

  std::string text;
  read_fastx_text(seq_name, text);
  Seqs sq;
  parse_text(text, sq);
  std::string().swap(text);
  const uint64_t n_seq = sq.names.size();
  auto hip = [](hipError_t e, const char *what) { if (e != hipSuccess) { fprintf(stderr, "ERROR: %s: %s\n", what, hipGetErrorString(e)); exit(1); } };

  if (op != OP_EXISTENCE) {                                   // dumpExistence (dump.C:430-441): every table at once, one report
    FILE *out = out_name.empty() ? stdout : fopen(out_name.c_str(), "w");
    if (!out) die("ERROR: cannot write '%s'.", out_name.c_str());
    std::vector<mgc_lookup *> tables;
    for (const std::string &d : dbs) {
      fprintf(stderr, "\nLoading kmers from '%s' into lookup table.\n", d.c_str());              // meryl-lookup.C:89
      mgc_lookup *t = mgc_lookup_load(d.c_str(), vmin, vmax, -1, 0);
      if (!t) die("ERROR: %s", mgc_lookup_error());
      tables.push_back(t);
    }
    uint8_t *d_bases = nullptr;
    hip(hipMalloc(reinterpret_cast<void **>(&d_bases), sq.bases.size() + 1), "hipMalloc");
    hip(hipMemcpy(d_bases, sq.bases.data(), sq.bases.size(), hipMemcpyHostToDevice), "upload");
    std::vector<const char *> names, labs;
    for (const std::string &n : sq.names) names.push_back(n.c_str());
    for (const std::string &l : labels) labs.push_back(l.c_str());
    uint64_t chunk = 64ull << 20;                             // bytes per piece of text (MGC_LOOKUP_CHUNK overrides)
    if (getenv("MGC_LOOKUP_CHUNK")) chunk = strtoull(getenv("MGC_LOOKUP_CHUNK"), nullptr, 10);
    const int mode = op == OP_BED ? MGC_REPORT_BED : op == OP_BED_RUNS ? MGC_REPORT_BED_RUNS
                   : op == OP_WIG_COUNT ? MGC_REPORT_WIG_COUNT : MGC_REPORT_WIG_DEPTH;
    if (mgc_lookup_report(tables.data(), (uint32_t)tables.size(), mode, labs.data(), (uint32_t)labs.size(), d_bases, sq.bases.size(),
                          sq.start.data(), names.data(), n_seq, chunk, write_piece, out) != MGC_OK)
      die("ERROR: %s", mgc_lookup_error());
    if (fflush(out) != 0 || (out != stdout && fclose(out) != 0)) die("ERROR: cannot write '%s'.", out_name.c_str());
    for (mgc_lookup *t : tables) mgc_lookup_free(t);
    (void)hipFree(d_bases);
    return 0;
  }

  uint8_t *d_bases = nullptr;
  uint64_t *d_start = nullptr, *d_total = nullptr, *d_found = nullptr;
  hip(hipMalloc(reinterpret_cast<void **>(&d_bases), sq.bases.size() + 1), "hipMalloc");
  hip(hipMalloc(reinterpret_cast<void **>(&d_start), 8 * (n_seq + 1)), "hipMalloc");
  hip(hipMalloc(reinterpret_cast<void **>(&d_total), 8 * (n_seq + 1)), "hipMalloc");
  hip(hipMalloc(reinterpret_cast<void **>(&d_found), 8 * (n_seq + 1)), "hipMalloc");
  hip(hipMemcpy(d_bases, sq.bases.data(), sq.bases.size(), hipMemcpyHostToDevice), "upload");
  hip(hipMemcpy(d_start, sq.start.data(), 8 * (n_seq + 1), hipMemcpyHostToDevice), "upload");

  std::vector<std::vector<uint64_t>> found(dbs.size());
  std::vector<uint64_t> total(n_seq), n_in_db(dbs.size());
  for (size_t d = 0; d < dbs.size(); d++) {
    fprintf(stderr, "\nLoading kmers from '%s' into lookup table.\n", dbs[d].c_str());          // meryl-lookup.C:89
    mgc_lookup *t = mgc_lookup_load(dbs[d].c_str(), vmin, vmax, -1, 0);
    if (!t) die("ERROR: %s", mgc_lookup_error());
    mgc_lookup_info info;
    mgc_lookup_get_info(t, &info);
    n_in_db[d] = info.n_kmers;
    if (mgc_lookup_existence(t, d_bases, sq.bases.size(), d_start, n_seq, d_total, d_found, nullptr) != MGC_OK) die("ERROR: %s", mgc_lookup_error());
    hip(hipDeviceSynchronize(), "lookup");
    found[d].resize(n_seq);
    if (n_seq) {
      hip(hipMemcpy(found[d].data(), d_found, 8 * n_seq, hipMemcpyDeviceToHost), "download");
      hip(hipMemcpy(total.data(), d_total, 8 * n_seq, hipMemcpyDeviceToHost), "download");
    }
    mgc_lookup_free(t);
  }
  FILE *out = out_name.empty() ? stdout : fopen(out_name.c_str(), "w");
  if (!out) die("ERROR: cannot write '%s'.", out_name.c_str());
  for (uint64_t s = 0; s < n_seq; s++) {                                                         // existence.C:96-113
    fprintf(out, "%s\t%" PRIu64, sq.names[s].c_str(), total[s]);
    for (size_t d = 0; d < dbs.size(); d++) fprintf(out, "\t%" PRIu64 "\t%" PRIu64, n_in_db[d], found[d][s]);
    fprintf(out, "\n");
  }
  if (out != stdout) fclose(out);
  (void)hipFree(d_bases); (void)hipFree(d_start); (void)hipFree(d_total); (void)hipFree(d_found);
  return 0;
}
