// meryl_analyze_main.cpp -- `meryl-analyze`: GC / GA / GT composition histograms of every k-mer of a meryl database.
//
// Keeps the reference tool's surface (src/meryl-analyze/meryl-analyze.C:444-521: the options, `usage:` first and the collected
// errors after it, exit 1; the narrative on stderr):
//   meryl-analyze -mers <db.meryl> -prefix <prefix> (-gc | -ga | -gt)
// The k-mers are decoded, scored and counted on the device (include/meryl_analyze.h); nothing here touches the device or
// creates a file before the command line is accepted.  Decisions where the reference's behaviour is undefined or of no use:
// a missing -prefix and a missing report type are refused (the reference formats a NULL pointer / opens the database and
// does nothing); of several report types the last one wins, as there; -verbose is an unknown option, as in the reference's
// option loop (its usage text names it, its loop does not read it -- and a line per k-mer is of no use at 10^9 k-mers).
#include "../../include/meryl_analyze.h"
#include "../../include/meryl_db.h"

#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace {
void usage(const char *prog, const std::vector<std::string> &err) {
  fprintf(stderr, "usage: %s -mers <meryldb> -prefix <prefix> (-gc | -ga | -gt)\n", prog);
  fprintf(stderr, "  -mers <meryldb>   the meryl database whose k-mers are analyzed.\n");
  fprintf(stderr, "  -prefix <prefix>  the output files are <prefix>.<NAME>.hist; required.\n");
  fprintf(stderr, "  -gc               histogram of the number of G and C bases per k-mer (GC.hist),\n");
  fprintf(stderr, "                    and of the A and T bases (AT.hist).\n");
  fprintf(stderr, "  -ga               histogram of the bases in GA microsatellite runs (GA.hist), in TC runs\n");
  fprintf(stderr, "                    (TC.hist), and of the larger of the two per k-mer (GA_TC.hist).\n");
  fprintf(stderr, "  -gt               the same for GT runs (GT.hist), AC runs (AC.hist) and the larger (GT_AC.hist).\n");
  fprintf(stderr, "                    One of -gc, -ga, -gt is required; of several the last one is used.\n");
  fprintf(stderr, "  (-verbose, one line per k-mer, is not an option of this program.)\n");
  fprintf(stderr, "output lines        : score (0..k) <tab> k-mer value <tab> number of k-mers\n");
  fprintf(stderr, "\n");
  for (const std::string &e : err) fputs(e.c_str(), stderr);
}
}  // namespace

int main(int argc, char **argv) {
  const char *db = nullptr, *prefix = nullptr;
  int type = -1;
  std::vector<std::string> err;

  for (int a = 1; a < argc; a++) {
    const std::string w = argv[a];
    auto value = [&]() -> const char * {
      if (a + 1 < argc) return argv[++a];
      err.push_back("Option '" + w + "' needs a value.\n");
      return nullptr;
    };
    if (w == "-mers") db = value();
    else if (w == "-prefix") prefix = value();
    else if (w == "-gc") type = MGC_ANALYZE_GC;
    else if (w == "-ga") type = MGC_ANALYZE_GA;
    else if (w == "-gt") type = MGC_ANALYZE_GT;
    else err.push_back("Unknown option '" + w + "'.\n");
  }
  if (!db) err.push_back("No query meryl database (-mers) supplied.\n");
  if (!prefix) err.push_back("No output prefix (-prefix) supplied.\n");
  if (type < 0) err.push_back("No report type (-gc | -ga | -gt) supplied.\n");
  if (!err.empty()) {
    usage(argv[0], err);
    return 1;
  }

  fprintf(stderr, "Open meryl database '%s'.\n", db);
  mdb_reader *r = mdb_reader_open(db);
  if (!r) {
    fprintf(stderr, "ERROR: cannot open '%s': %s\n", db, mdb_last_error());
    return 1;
  }
  mdb_info inf;
  mdb_reader_info(r, &inf);
  mdb_reader_close(r);

  mgc_analyze *an = nullptr;
  int rc = mgc_analyze_open(inf.k, type, -1, &an);
  if (rc == MGC_OK) rc = mgc_analyze_add_database(an, db, 0);
  if (rc != MGC_OK) {
    fprintf(stderr, "ERROR: %s\n", mgc_analyze_error());
    mgc_analyze_close(an);
    return 1;
  }
  mgc_analyze_info info;
  mgc_analyze_get_info(an, &info);
  fprintf(stderr, "Processed %li kmers in total.\n\n", (long)info.n_kmers);
  fprintf(stderr, "Output histogram\n");
  rc = mgc_analyze_write(an, prefix);
  if (rc != MGC_OK) {
    fprintf(stderr, "ERROR: %s\n", mgc_analyze_error());
    mgc_analyze_close(an);
    return 1;
  }
  fprintf(stderr, "Clean up..\n\n");
  mgc_analyze_close(an);
  fprintf(stderr, "Bye!\n");
  return 0;
}
