// meryl_import_main.cpp -- `meryl-import`: a text file of `kmer value` lines -> a meryl database.
//
// Keeps the reference tool's surface (src/meryl-import/meryl-import.C:44-135: options, their checks, the usage text):
//   meryl-import -k <K> -kmers <file | -> -output <db.meryl> [-forward | -reverse] [-threads t] [-maxvalue v] [-memory m]
// -kmers - reads standard input; plain text and gzip are read, other compressions are refused by their suffix.  The text is
// parsed, sorted and summed on the device (include/meryl_import.h); nothing here touches the device before the command
// line is accepted.  Where the reference's behaviour is undefined the input is refused with its line number (see the header).
// -multiset is not part of this build.
//
// -labelwidth <lw> (1..64) selects the meryl 2 tool (src/meryl2-import/meryl-import.C:62-67, :199-233: `kmer value label` lines,
// `value=` / `label=` lines; include/meryl_import_labelled.h); absent or 0 the tool is the meryl 1 one.  -valuewidth is
// accepted as 0 only: the writer's default value encoding is the only one this build has.
#include "../../include/meryl_import_labelled.h"

#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace {
void usage(const char *prog, const std::vector<std::string> &err) {
  fprintf(stderr, "usage: %s [...] -k <kmer-size> -kmers <input-kmers> -output <db.meryl>\n", prog);
  fprintf(stderr, "  Loads the kmers and values listed in <input-kmers> into a meryl kmer database.\n");
  fprintf(stderr, "\n");
  fprintf(stderr, "INPUTS and OUTPUTS\n");
  fprintf(stderr, "  -kmers <input-kmers>  A file consisting of kmers and values, one per line, separated\n");
  fprintf(stderr, "                        by white space ('AGTTGCC 4').  Order of kmers is not important.\n");
  fprintf(stderr, "                        The values of duplicate kmers are summed (modulo 2^32).\n");
  fprintf(stderr, "                        '-' reads standard input; gzip is read, other compressions are not.\n");
  fprintf(stderr, "\n");
  fprintf(stderr, "                        A persistent value can be specified as '#<value>' (e.g., '#3')\n");
  fprintf(stderr, "                        All kmers with no value after this line will use this value.\n");
  fprintf(stderr, "\n");
  fprintf(stderr, "  -k <size>             The size of a kmer, in bases (%d..%d).  A kmer in the input that is\n", MGC_IMPORT_MIN_K, MGC_IMPORT_MAX_K);
  fprintf(stderr, "                        shorter is refused with its line number; of a longer one the\n");
  fprintf(stderr, "                        right-most (last) <size> bases are used.\n");
  fprintf(stderr, "\n");
  fprintf(stderr, "  -output <db.meryl>    Create (or overwrite) meryl database 'database.meryl'.\n");
  fprintf(stderr, "\n");
  fprintf(stderr, "OPTIONS\n");
  fprintf(stderr, "  -multiset             (duplicate kmers as individual entries: not part of this build)\n");
  fprintf(stderr, "\n");
  fprintf(stderr, "  -maxvalue <value>     (accepted, a hint only)\n");
  fprintf(stderr, "\n");
  fprintf(stderr, "  -labelwidth <lw>      Store an <lw>-bit label (%d..%d) with each kmer, and read the meryl 2 dialect:\n", MGC_IMPORT_MIN_LABEL_WIDTH, MGC_IMPORT_MAX_LABEL_WIDTH);
  fprintf(stderr, "                        'kmer [value [label]]' lines; 'value=<n>' / 'label=<n>' lines set the persistent\n");
  fprintf(stderr, "                        value / label ('#' lines are not read); numbers are 123, 123d, 7bh, 173o or\n");
  fprintf(stderr, "                        1111011b; the labels of duplicate kmers add (modulo 2^lw).  0: no labels (default).\n");
  fprintf(stderr, "  -valuewidth <vw>      Only 0 (the default value encoding) is part of this build.\n");
  fprintf(stderr, "\n");
  fprintf(stderr, "  -forward              By default, the canonical kmer is loaded into the database.  These\n");
  fprintf(stderr, "  -reverse              options force either the forward or reverse-complement kmer to be\n");
  fprintf(stderr, "                        loaded instead.  These options are mutually exclusive.\n");
  fprintf(stderr, "\n");
  fprintf(stderr, "  -threads <t>          Use <t> host threads when writing data.\n");
  fprintf(stderr, "\n");
  fprintf(stderr, "  -memory <m>           (accepted, a hint only)\n");
  fprintf(stderr, "\n");
  for (const std::string &e : err) fputs(e.c_str(), stderr);
}

bool ends_with(const std::string &n, const char *suf) {
  return n.size() > strlen(suf) && n.compare(n.size() - strlen(suf), std::string::npos, suf) == 0;
}
}  // namespace

int main(int argc, char **argv) {
  const char *input = nullptr, *output = nullptr;
  uint32_t k = 0, label_width = 0;
  bool have_k = false, multiset = false;
  int mode = MGC_MODE_CANONICAL, threads = 0;
  std::vector<std::string> err;

  for (int a = 1; a < argc; a++) {
    const std::string w = argv[a];
    auto value = [&]() -> const char * {
      if (a + 1 < argc) return argv[++a];
      err.push_back("Option '" + w + "' needs a value.\n");
      return nullptr;
    };
    if (w == "-kmers") input = value();
    else if (w == "-output") output = value();
    else if (w == "-k") { if (const char *v = value()) { k = (uint32_t)strtoul(v, nullptr, 10); have_k = true; } }
    else if (w == "-maxvalue" || w == "-memory") (void)value();
    else if (w == "-labelwidth" || w == "-valuewidth") {
      if (const char *v = value()) {
        char *end = nullptr;
        const unsigned long x = strtoul(v, &end, 10);
        const bool number = *v >= '0' && *v <= '9' && end && *end == 0;
        if (w == "-labelwidth") {
          if (!number || x > MGC_IMPORT_MAX_LABEL_WIDTH) err.push_back("Label width (-labelwidth) '" + std::string(v) + "' is not a number in 0..64.\n");
          else label_width = (uint32_t)x;
        } else if (!number || x != 0) {
          err.push_back("Value width (-valuewidth) '" + std::string(v) + "': only 0, the default value encoding, is part of this build.\n");
        }
      }
    }
    else if (w == "-threads") { if (const char *v = value()) threads = atoi(v); }
    else if (w == "-multiset") multiset = true;
    else if (w == "-forward") mode = MGC_MODE_FORWARD;
    else if (w == "-reverse") mode = MGC_MODE_REVERSE;
    else err.push_back("Unknown option '" + w + "'.\n");
  }
  if (!input) err.push_back("No input kmer file (-kmers) supplied.\n");
  if (!output) err.push_back("No output database name (-output) supplied.\n");
  if (!have_k || k == 0) err.push_back("No kmer size (-k) supplied.\n");
  else if (k < MGC_IMPORT_MIN_K || k > MGC_IMPORT_MAX_K) {
    char b[160];
    snprintf(b, sizeof(b), "Kmer size (-k) %u is outside %d..%d (a 10-bit prefix must leave a suffix; kmers hold at most 64 bases).\n",
             k, MGC_IMPORT_MIN_K, MGC_IMPORT_MAX_K);
    err.push_back(b);
  }
  if (multiset) err.push_back("Option '-multiset' is not part of this build.\n");
  if (input) {
    const std::string n = input;
    for (const char *suf : {".bz2", ".xz", ".zst", ".lz4", ".zip"})
      if (ends_with(n, suf)) err.push_back("Input '" + n + "' is compressed with something other than gzip: decompress it into a pipe and use '-kmers -'.\n");
  }
  if (!err.empty()) {
    usage(argv[0], err);
    return 1;
  }

  mgc_import_info info;
  const int rc = label_width ? mgc_import_labelled_file(input, k, mode, label_width, output, -1, threads, &info)
                             : mgc_import_file(input, k, mode, output, -1, threads, &info);
  if (rc != MGC_OK) {
    fprintf(stderr, "ERROR: %s\n", mgc_import_error());
    return 1;
  }
  if (label_width) fprintf(stderr, "Added %" PRIu64 " kmers; incorrectly added 0 kmers.\n", info.n_records);   // meryl2-import/meryl-import.C:280
  else fprintf(stderr, "Found %" PRIu64 " kmers in the input.\n", info.n_records);
  fprintf(stderr, "\n");
  fprintf(stderr, "Bye.\n");
  return 0;
}
