// meryl_main.cpp -- `meryl` command-line front end for the MI355X count engine.
//
// Keeps the reference's CLI surface for the count path (north_star: `meryl count
// k=K <reads> output <db>`): the positional word grammar of
// src/meryl/meryl.C:30-87 and src/meryl/merylCommandBuilder.C (options :187-326,
// operations :346-385, `output` :440-461, sequence inputs :537-549, `[ ]`
// nesting :133-153), the stderr narrative of src/meryl/merylOp-count.C:324-401
// (including the line Canu parses, :398-401), and the debug verbs `print` and
// `dumpIndex` (src/meryl/meryl.C:36-46, src/meryl/merylOp-nextMer.C:665-677) on the
// databases it writes.  Beyond the count path: `histogram`, `dumpFile`, the set operations over
// databases (union[-min|-max|-sum], intersect[-min|-max|-sum], subtract, difference, symmetric-difference;
// merylOp-nextMer.C:559-613) and the single-input value filters / arithmetic (less-than ... modulo; :490-557), all merged on
// the device.  Set and value operations nest as in the reference: a whole tree of them over databases and finished counts
// runs as one evaluation with the intermediate results kept on the device (mgc_db_eval), `output` is optional on every
// one of them, and `print [operation]` prints the tree's result (quick-start.rst:327-333).  Labels (meryl2): `label=<word>`,
// `label=<word>#<const>` or `label=#<const>` after a set or value operation names how the label of a written k-mer comes from
// its inputs' labels (merylCommandBuilder-isAssign.C:124-156, merylOpCompute.C:286-395); a tree is evaluated with labels
// (mgc_db_eval_labelled) when `-l` was given, one of its operations carries such a word or one of its leaves stores labels,
// and as before otherwise.  Selectors (meryl2): `value:`, `label:`, `bases:` and `input:` words with `not`, `and`, `or` after a set
// or value operation (merylCommandBuilder-isSelect.C, merylSelector.C:72-156) are decoded by the library's parser
// (mgc_select_parse) once the operation's inputs are known, and a tree that holds any is evaluated through
// mgc_db_eval_selected; distinct= / word-frequency= / threshold= inside a selector stay on the value operations.  Value assignment
// (meryl2): `value=<word>`, `value=<word>#<const>` or `value=#<const>` after a set or value-filter operation names how the value of
// a written k-mer comes from its inputs' values (merylCommandBuilder-isAssign.C:44-103, merylOpCompute.C:136-282): the operation
// then gives the presence rule only, k-mers whose assigned value is 0 are not written, and selectors and the filter see the
// assigned value.  The text is decoded by the library's parser (mgc_value_assign_parse) and a tree that holds any is evaluated
// through mgc_db_eval_assigned; the arithmetic value operations and the counting operations refuse it.  Reports: `histogram` and
// `statistics` (src/meryl/merylOp-histogram.C:20-97) take a database -- the histogram its master index stores, host only -- or an
// operation, whose tree is then evaluated once with the value histogram of its root collected on the device (mgc_db_eval_reported);
// meryl2's `output:histogram[=file]` and `output:statistics[=file]` (merylCommandBuilder-processText.C:153-154,
// merylOpTemplate.C:168-209,285-307) ask the same of any set or value operation of a tree, to a file or (no file, or `-`) stdout.
// `print [operation]` of a tree without reports is the list of the tree's root (include/meryl_list.h): the lines are formatted on the
// device while the tree runs (mgc_db_eval_listed) and only text crosses to the host; a tree that also collects reports keeps
// mgc_db_eval_reported and its slice callback, and `print <db>` the host reader, which needs no device.
// What stays refused: output:list= and output:show, compare, ploidy, noise, printACGT, Canu sequence stores (segment=); CRAM only when no `samtools` is on the PATH.
#include "../../include/meryl_db.h"
#include "../../include/meryl_gpu_count.h"
#include "../../include/meryl_list.h"
#include "../../include/meryl_seq.h"

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <filesystem>
#include <string>
#include <sys/stat.h>
#include <thread>
#include <type_traits>
#include <unistd.h>
#include <chrono>
#include <vector>

namespace {
// wall-clock stamp of static initialisation (just before main()): what lies before the input is read -- the HIP runtime, the
// device, the session's streams -- is reported on its own in the -V TIMING line
const std::chrono::steady_clock::time_point g_t_main = std::chrono::steady_clock::now();

// ---- scaledNumber / scaledUnit / scaledName [meryl-utility, not in tree] ----
uint64_t scaledNumber(uint64_t n, uint32_t div = 1024) { for (int i = 0; i < 8 && n > 9999; i++) n /= div; return n; }
char scaledUnit(uint64_t n, uint32_t div = 1024) {
  const char u[] = { ' ', 'k', 'M', 'G', 'T', 'P', 'E', 'Z', 'Y' };
  int i = 0;
  for (; i < 8 && n > 9999; i++) n /= div;
  return u[i];
}
const char *scaledName(uint64_t n, uint32_t div = 1024) {
  const char *u[] = { "", " thousand", " million", " billion", " trillion", " quadrillion", " quintillion", "", "" };
  int i = 0;
  for (; i < 8 && n > 9999; i++) n /= div;
  return u[i];
}
uint64_t bits64(uint64_t v) { uint64_t b = 0; while (v) { b++; v >>= 1; } return b; }

bool file_exists(const std::string &p) { struct stat st; return stat(p.c_str(), &st) == 0 && !S_ISDIR(st.st_mode); }
bool dir_has_index(const std::string &p) { return file_exists(p + "/merylIndex"); }

bool has_compressed_suffix(const std::string &n) {
  for (const char *suf : { ".gz", ".bz2", ".xz", ".bgz", ".bgzf", ".zst" })
    if (n.size() > strlen(suf) && n.compare(n.size() - strlen(suf), strlen(suf), suf) == 0) return true;
  return false;
}

enum OpKind { OP_NONE, OP_COUNT, OP_COUNT_FORWARD, OP_COUNT_REVERSE, OP_PRINT, OP_DUMPINDEX, OP_HISTOGRAM, OP_STATISTICS, OP_DUMPFILE, OP_MERGE, OP_VALUE };

struct InputRef { std::string path; int child = -1; };      // a database on the command line, or the output of a child operation

struct Operation {
  OpKind                   kind = OP_NONE;
  std::vector<std::string> seq_inputs;      // sequence files (count ops)
  std::vector<bool>        seq_compress;    // `compress` is sticky per input (merylCommandBuilder.C:237-240,546)
  std::vector<InputRef>    inputs;          // databases and child operations, in command-line order
  std::vector<std::string> db_inputs;       // ... resolved to database paths once the children have run
  std::string              word;            // the operation as typed
  int                      merge_op = -1;   // MGC_MERGE_* (OP_MERGE)
  int                      value_op = -1;   // MGC_VALUE_* (OP_VALUE): less-than ... modulo
  uint64_t                 constant = ~0ull;   // its threshold / constant (merylCommandBuilder.C:216-233,291-294); ~0: not given
  double                   frac_distinct = -1, word_freq = -1;   // distinct=<f> / word-frequency=<f> thresholds (:278-289)
  int                      parent = -1;
  std::string              output;
  uint64_t                 exp_num_kmers = 0;   // n=
  std::string              count_suffix;        // count-suffix=
  uint64_t                 label = 0;           // label=#<n> (meryl2: the constant label of a count, merylCommandBuilder-isAssign.C:124)
  bool                     has_label_op = false;   // label=<word>[#<const>] on a set or value operation (:124-156)
  int                      label_op = MGC_LABEL_DEFAULT;
  uint64_t                 label_constant = 0;
  bool                     has_value_assign = false;   // value=<word>[#<const>] on a set or value-filter operation (:44-103)
  int                      value_assign = MGC_ASSIGN_NONE;
  uint64_t                 value_constant = 0;
  std::vector<std::string> select_words;        // value: label: bases: input: not and or, after a set or value operation (meryl2 selectors)
  bool                     has_hist_out = false, has_stats_out = false;   // output:histogram[=file] / output:statistics[=file] (meryl2)
  std::string              hist_out, stats_out;                            //   their files; "-": stdout
};

struct Globals {
  uint32_t k = 0;
  double   memory_gb;
  uint32_t threads;
  int      verbosity = 2;          // sayStandard
  bool     only_config = false;
  bool     compress = false;       // sticky
  uint32_t gpus = 1;               // gpus=<N> (this build only): ranks of ONE count spread over the node's devices
  uint32_t label_size = 0;         // -l <bits> (meryl2: kmerTiny::setLabelSize, merylGlobals.C:75-77)
  bool     label_size_given = false;
  bool     fast_exit = false;      // set when ONE count is all the command does (and MERYL_FAST_EXIT is not 0): see run_count
  Globals() {
    const long pages = sysconf(_SC_PHYS_PAGES), psz = sysconf(_SC_PAGE_SIZE);
    memory_gb = (pages > 0 && psz > 0) ? (double)pages * (double)psz / 1024.0 / 1024.0 / 1024.0 : 16.0;
    threads = std::thread::hardware_concurrency() ? std::thread::hardware_concurrency() : 1;
  }
};

void usage(const char *prog) {
  fprintf(stderr,
          "usage: %s [k=<K>] [memory=<GB>] [threads=<T>] [gpus=<N>] [n=<kmers>] [compress] [-l <label-bits>] [-C] [-Q] [-V]\n"
          "          count|count-forward|count-reverse [label=#<n>] <reads.fa|fq[.gz]|sam[.gz]|bam|cram> ... output <database.meryl>\n"
          "       %s print <database.meryl | [operation]>\n"
          "       %s histogram|statistics <database.meryl | [operation]>\n"
          "       %s dumpIndex <database.meryl>\n"
          "       %s dumpFile <database.meryl>/0x######\n"
          "       %s union[-min|-max|-sum]|intersect[-min|-max|-sum]|subtract|difference|symmetric-difference [value=<word>[#<n>]] [label=<word>[#<n>]] [selector ...] <db | [operation]> ... [output <db>]\n"
          "       %s less-than|greater-than|at-least|at-most|equal-to|not-equal-to <N | distinct=<f> | word-frequency=<f>> [value=<word>[#<n>]] [selector ...] <db | [operation]> [output <db>]\n"
          "       %s increase|decrease|multiply|divide|divide-round|modulo <N> <db | [operation]> [output <db>]\n"
          "\n"
          "  MI355X-native implementation of the `count` path of marbl/meryl.  Words are processed left to\n"
          "  right; options apply to the operations that follow.  A leading '[' and trailing ']' group the\n"
          "  words of one operation; an operation inside another one's brackets is its input.  A tree of set and value\n"
          "  operations is evaluated in one pass with its intermediate results on the device: only operations given\n"
          "  'output' write a database, and 'print [operation]' prints the result of the tree (distinct= and\n"
          "  word-frequency= need a database, or an input operation that writes one).  label=<word> on a set or value\n"
          "  operation (first selected min max and or xor difference lightest heaviest invert, with #<n> a constant;\n"
          "  label=#<n> sets it) combines the labels of its inputs; a count inside such a tree may omit 'output'.\n"
          "  value=<word> on a set operation or a value filter (first selected min max add sum sub dif mul div divzero mod rem\n"
          "  count, with #<n> a constant; value=#<n> sets it) computes the value of a written k-mer from the values of the\n"
          "  inputs that hold it; the operation then only decides where a k-mer must be present, a k-mer whose value\n"
          "  becomes 0 is dropped, and selectors and the filter see the new value -- e.g. intersect value=sub a b.\n"
          "  A selector after a set or value operation keeps, of what the operation would write, the k-mers for which a\n"
          "  sum of products of tests holds: value:[lhs]REL<rhs>, label:[lhs]REL<rhs> (a side: @<input>, #<n> or <n>; no lhs:\n"
          "  the output k-mer; REL: == eq != <> ne <= le >= ge < lt > gt), bases:<acgt>:REL<n>, input:<n|n-m|n-all|all|any|\n"
          "  first|@n|@a-@b>[:...], joined by 'and' (optional), 'or' and 'not' -- e.g. union input:3-all a b c d.\n"
          "  histogram and statistics report how the values of a database, or of the result of an operation, are\n"
          "  distributed (value <TAB> k-mers; the statistics table); of an operation the tree is evaluated once, the\n"
          "  histogram is collected on the device and nothing is written unless an operation says 'output'.\n"
          "  output:histogram[=file] and output:statistics[=file] on a set or value operation report that operation's\n"
          "  result while the tree runs on (no file, or '-': stdout) -- e.g. print [union-sum output:histogram=u.hist a b].\n"
          "  Other meryl operations (compare, ploidy, noise, printACGT) are\n"
          "  not part of this build.\n",
          prog, prog, prog, prog, prog, prog, prog, prog);
}

[[noreturn]] void die(const char *fmt, const char *a = "") {
  fprintf(stderr, fmt, a);
  fprintf(stderr, "\n");
  exit(1);
}

// ---- the configuration narrative, merylOp-count.C:118-165,231-295,324-401 ----
void print_configuration(const Globals &g, const Operation &op, uint64_t exp_num_kmers, const mgc_count_config &cfg) {
  const uint32_t k = g.k;
  fprintf(stderr, "\n");
  fprintf(stderr, "Counting %" PRIu64 " (estimated)%s %s%s%s %u-mers from %zu input file%s:\n",             // :324-330
          scaledNumber(exp_num_kmers), scaledName(exp_num_kmers),
          (op.kind == OP_COUNT) ? "canonical" : "", (op.kind == OP_COUNT_FORWARD) ? "forward" : "",
          (op.kind == OP_COUNT_REVERSE) ? "reverse" : "", k, op.seq_inputs.size(), (op.seq_inputs.size() == 1) ? "" : "s");
  for (const std::string &n : op.seq_inputs) fprintf(stderr, "  %15s: %s\n", "sequence-file", n.c_str());            // :332-333

  // SIMPLE MODE, :136-162
  fprintf(stderr, "\n\nSIMPLE MODE\n-----------\n\n");
  const uint32_t sl = cfg.count_suffix_length;
  if (2 * k - 2 * sl > 42) {
    fprintf(stderr, "  Not possible.\n");
  } else {
    const uint64_t n_entries = (uint64_t)1 << (2 * k - 2 * sl), low_bits = 16;
    const uint64_t exp_max = (uint64_t)(0.004 * (double)exp_num_kmers), exp_bits = bits64(exp_max) + 1;
    const uint64_t extra = (exp_bits < low_bits) ? 0 : exp_bits - low_bits;
    const uint64_t low_mem = n_entries * low_bits, high_mem = n_entries * extra, tot = (low_mem + high_mem) / 8;
    if (sl == 0) fprintf(stderr, "  %u-mers\n", k);                                                                 // :147-150
    else         fprintf(stderr, "  %u-mers with constant %u-mer suffix '%s'\n", k, sl, cfg.count_suffix);
    fprintf(stderr, "    -> %" PRIu64 " entries for counts up to %u.\n", n_entries, 65535u);
    fprintf(stderr, "    -> %" PRIu64 " %cbits memory used\n", scaledNumber(low_mem), scaledUnit(low_mem));
    fprintf(stderr, "\n  %" PRIu64 " input bases\n", exp_num_kmers);
    fprintf(stderr, "    -> expected max count of %" PRIu64 ", needing %" PRIu64 " extra bits.\n", exp_max, extra);
    if (extra > 0) fprintf(stderr, "    -> %" PRIu64 " %cbits memory used\n", scaledNumber(high_mem), scaledUnit(high_mem));
    else           fprintf(stderr, "    -> no memory used\n");
    fprintf(stderr, "\n  %" PRIu64 " %cB memory needed\n", scaledNumber(tot), scaledUnit(tot));
  }

  // COMPLEX MODE table, :245-293 (evaluated at expNumKmers / nBatches like findBestValues)
  if (k > 5) {
    const uint64_t n_est = exp_num_kmers / (cfg.n_batches ? cfg.n_batches : 1);
    const uint32_t seg_bits = 4096 * 8, seg_bytes = 4096;
    const uint64_t mem_used = cfg.use_simple ? UINT64_MAX : cfg.memory_used;
    fprintf(stderr, "\n\nCOMPLEX MODE\n------------\n\n");
    fprintf(stderr, "prefix     # of   struct   kmers/    segs/      min     data    total\n");
    fprintf(stderr, "  bits   prefix   memory   prefix   prefix   memory   memory   memory\n");
    fprintf(stderr, "------  -------  -------  -------  -------  -------  -------  -------\n");
    for (uint32_t wp = 1; wp < 2 * k - 1; wp++) {
      const uint64_t n_prefix = (uint64_t)1 << wp, kpp = n_est / n_prefix + 1, kps = seg_bits / (2 * k - wp), spp = kpp / kps + 1;
      if (wp + bits64(spp) + bits64(seg_bytes) >= 64) break;
      const uint64_t struct_mem = (uint64_t)3232 * n_prefix + 8 * n_prefix * spp, data_min = n_prefix * seg_bytes;
      const uint64_t data_mem = n_prefix * spp * seg_bytes, total = struct_mem + data_mem;
      fprintf(stderr, "%6u  %4" PRIu64 " %cP  %4" PRIu64 " %cB  %4" PRIu64 " %cM  %4" PRIu64 " %cS  %4" PRIu64 " %cB  %4" PRIu64 " %cB  %4" PRIu64 " %cB%s\n",
              wp, scaledNumber(n_prefix), scaledUnit(n_prefix), scaledNumber(struct_mem), scaledUnit(struct_mem),
              scaledNumber(kpp), scaledUnit(kpp), scaledNumber(spp), scaledUnit(spp),
              scaledNumber(data_min), scaledUnit(data_min), scaledNumber(data_mem), scaledUnit(data_mem),
              scaledNumber(total), scaledUnit(total), (wp == cfg.w_prefix && !cfg.use_simple) ? "  Best Value!" : "");
      if (total > (uint64_t)16 * mem_used) break;
    }
  }

  // FINAL CONFIGURATION, :390-401
  char line[256];
  mgc_format_configured_line(&cfg, line, sizeof(line));
  fprintf(stderr, "\n\nFINAL CONFIGURATION\n-------------------\n\n");
  fprintf(stderr, "Estimated to require %" PRIu64 " %cB memory out of %" PRIu64 " %cB allowed.\n",
          scaledNumber(cfg.memory_used), scaledUnit(cfg.memory_used), scaledNumber(cfg.memory_allowed), scaledUnit(cfg.memory_allowed));
  fprintf(stderr, "Estimated to require %u batch%s.\n", cfg.n_batches, (cfg.n_batches == 1) ? "" : "es");
  fprintf(stderr, "\n%s\n\n", line);
}

// one input of a count, or a byte window of it (a plain-text file read by one rank of a node count)
struct InputPiece { std::string name; uint64_t begin, end; };

static bool is_regular_file(const std::string &name) { struct stat st; return stat(name.c_str(), &st) == 0 && S_ISREG(st.st_mode); }

// Input: the file's raw text goes to the device and is parsed there (mgc_push_text*; a plain gzip file's is inflated by several threads
// and resolved there, mgc_push_text_gzip_file); a BGZF BAM file goes there as its
// inflated bytes and its SEQ fields are decoded there (mgc_push_bam_file); SAM text -- a .sam, a .sam.gz, stdin with an @HD line, a
// CRAM through `samtools view -h` -- takes the same text routes as MGC_TEXT_SAM and its SEQ column is extracted there; files the
// device routes refuse (multi-line FASTQ, a damaged BAM, a SAM line with fewer than 10 columns or "\r\n" blank lines ...), BAM in
// plain gzip or on stdin and MERYL_HOST_PARSER=1 take the host state machine of meryl_seq.cpp.  Returns the bytes / bases taken in (reported with -V -V).
int g_inflate_threads = 16;                                  // threads= of the command line: the BGZF inflaters (readers of plain text: at most 16)
bool g_gzip_parallel = true;                                 // false under gpus=N: every rank reads its files with the host reader's one gzread thread
uint64_t load_inputs(mgc_session *s, const std::vector<InputPiece> &pieces, int reader_threads) {
  const uint64_t buf_max = 2 * 1024 * 1024;                                                            // merylOp-countThreads.C:413
  std::vector<char> buf(buf_max);
  uint64_t total_bases = 0;
  const bool host_parser = getenv("MERYL_HOST_PARSER") && getenv("MERYL_HOST_PARSER")[0] == '1';
  auto load_on_host = [&](const std::string &name) {
    msr_reader *r = msr_open(name.c_str());
    if (!r) die("ERROR: %s", msr_last_error());
    for (;;) {                                                                                         // loader loop, :173-203
      uint64_t len = 0;                                                                                // 2 MiB of sequences, '.' after each
      const int rc = msr_load_stream(r, buf.data(), buf_max, &len);
      if (rc < 0) die("ERROR: %s", msr_last_error());
      if (rc == 0) break;
      if (mgc_push_bases(s, buf.data(), len, 0) != MGC_OK) die("ERROR: %s", mgc_last_error(s));
      total_bases += len;
    }
    mgc_push_bases(s, nullptr, 0, 1);                                                                  // end-of-file breaker, :196
    msr_close(r);
  };
  std::vector<char> text(host_parser ? 0 : (16u << 20));
  for (const InputPiece &pc : pieces) {
    const std::string &name = pc.name;
    const bool whole = pc.begin == 0 && pc.end == ~0ull;
    if (host_parser && whole) { load_on_host(name); continue; }
    msr_reader *r = msr_open(name.c_str());
    if (!r) die("ERROR: %s", msr_last_error());
    if (msr_format(r) == MSR_FORMAT_BAM && name != "-" && whole && is_regular_file(name) && mgc_is_bgzf_file(name.c_str()) && !getenv("MERYL_BGZF_GENERIC")) {
      // a BGZF BAM file: the library maps it, inflates its blocks with several threads straight into its pinned upload buffers, walks
      // the records and decodes their SEQ fields on the device.  A file it refuses is read again on the host, which says what is wrong.
      msr_close(r);
      const char *bt = getenv("MERYL_BGZF_THREADS");
      const int rc = mgc_push_bam_file(s, name.c_str(), bt ? atoi(bt) : std::max(reader_threads, g_inflate_threads));
      if (rc == MGC_EFORMAT) load_on_host(name);
      else if (rc != MGC_OK) die("ERROR: %s", mgc_last_error(s));
      struct stat fst;
      if (rc == MGC_OK && stat(name.c_str(), &fst) == 0) total_bases += (uint64_t)fst.st_size * 3;   // (a guess, as for bgzip'd text)
      continue;
    }
    if (msr_format(r) == MSR_FORMAT_BAM) { msr_close(r); load_on_host(name); continue; }     // BAM in plain gzip or on stdin: decoded on the host
    const bool sam = msr_format(r) == MSR_FORMAT_SAM;                                        // asked for by name: a leading '@' would be sniffed as FASTQ
    const int fmt = sam ? MGC_TEXT_SAM : 0;
    const bool cram = name.size() > 5 && name.compare(name.size() - 5, 5, ".cram") == 0;     // its SAM text comes through a pipe: the generic loop below
    if (name != "-" && !has_compressed_suffix(name) && !cram && !(sam && !is_regular_file(name))) {
      // plain text: the library reads the file itself, several threads straight into its pinned upload buffers
      msr_close(r);
      const int rc = whole ? mgc_push_text_file(s, name.c_str(), fmt, reader_threads)
                           : mgc_push_text_file_range(s, name.c_str(), fmt, reader_threads, pc.begin, pc.end);
      if (rc == MGC_EFORMAT && whole) load_on_host(name);
      else if (rc == MGC_EFORMAT) die("ERROR: '%s' is not strict four-line FASTQ / FASTA: it cannot be read in windows by several ranks (gpus=1 reads it)", name.c_str());
      else if (rc != MGC_OK) die("ERROR: %s", mgc_last_error(s));
      struct stat fst;
      if (whole) { if (stat(name.c_str(), &fst) == 0) total_bases += (uint64_t)fst.st_size; }
      else total_bases += pc.end - pc.begin;
      continue;
    }
    if (name != "-" && whole && !cram && mgc_is_bgzf_file(name.c_str()) && !getenv("MERYL_BGZF_GENERIC")) {
      // BGZF (bgzip'd FASTA / FASTQ): the library maps the file and inflates its blocks with several threads straight into its pinned
      // upload buffers (MERYL_BGZF_GENERIC=1: through the generic reader below, as every other compressed input)
      msr_close(r);
      const char *bt = getenv("MERYL_BGZF_THREADS");
      const int rc = mgc_push_text_bgzf_file(s, name.c_str(), fmt, bt ? atoi(bt) : std::max(reader_threads, g_inflate_threads));
      if (rc == MGC_EFORMAT) load_on_host(name);
      else if (rc != MGC_OK) die("ERROR: %s", mgc_last_error(s));
      struct stat fst;
      if (stat(name.c_str(), &fst) == 0) total_bases += (uint64_t)fst.st_size * 3;             // (text bytes, as the reference guesses them for .gz)
      continue;
    }
    if (name != "-" && whole && g_gzip_parallel && !cram && is_regular_file(name) && mgc_is_gzip_file(name.c_str()) && !getenv("MERYL_GZIP_GENERIC")) {
      // plain gzip: the library maps the file, several threads inflate it from guessed block starts straight into its pinned upload
      // buffers, the device resolves what they could not know and checks the CRC (MERYL_GZIP_GENERIC=1: one gzread thread, below)
      msr_close(r);
      const char *gt = getenv("MERYL_GZIP_THREADS");
      const int rc = mgc_push_text_gzip_file(s, name.c_str(), fmt, gt ? atoi(gt) : std::max(reader_threads, g_inflate_threads), nullptr);
      if (rc == MGC_EFORMAT) load_on_host(name);
      else if (rc != MGC_OK) die("ERROR: %s", mgc_last_error(s));
      struct stat fst;
      if (stat(name.c_str(), &fst) == 0) total_bases += (uint64_t)fst.st_size * 3;             // (text bytes, as the reference guesses them for .gz)
      continue;
    }
    bool begun = false, refused = false;
    for (;;) {
      const int64_t got = msr_read_text(r, text.data(), text.size());
      if (got < 0) die("ERROR: %s", msr_last_error());
      if (got == 0) break;
      if (!begun && sam) {
        if (mgc_begin_text(s, MGC_TEXT_SAM) != MGC_OK) die("ERROR: %s", mgc_last_error(s));
        begun = true;
      }
      if (!begun) {
        int64_t p = 0;
        while (p < got && (text[p] == '\n' || text[p] == '\r' || text[p] == ' ' || text[p] == '\t')) p++;
        const char c = p < got ? text[p] : '>';
        if (c != '>' && c != '@') {
          fprintf(stderr, "ERROR: '%s' is neither FASTA nor FASTQ (record starts with '%c')\n", name.c_str(), c);
          exit(1);
        }
        if (mgc_begin_text(s, c == '@' ? MGC_TEXT_FASTQ : MGC_TEXT_FASTA) != MGC_OK) die("ERROR: %s", mgc_last_error(s));
        begun = true;
      }
      if (mgc_push_text(s, text.data(), (size_t)got) != MGC_OK) die("ERROR: %s", mgc_last_error(s));
      total_bases += (uint64_t)got;                                                                    // text bytes (reported with -V -V)
    }
    msr_close(r);
    if (begun) {
      const int rc = mgc_end_text(s);
      if (rc == MGC_EFORMAT) refused = true;
      else if (rc != MGC_OK) die("ERROR: %s", mgc_last_error(s));
    }
    if (refused) load_on_host(name);
  }
  return total_bases;
}

// gpus=N: ONE count spread over the node's devices (this build only; the reference's node-scale recipe is "count pieces,
// then union-sum", src/meryl/merylOp-count.C:251-268).  Every rank READS ITS OWN share of the input through its own
// device's link -- plain-text files are cut into byte windows at record boundaries (mgc_text_record_start), inputs that
// cannot be cut (compressed, SAM/BAM, stdin) go whole to one rank each -- and stages it on its device; then
// mgc_count_node_batched: routing plan, per-batch partition / pulls / owner count, parked waves, one merge per owner,
// parts stitched into the 64-file directory.
int run_count_node(const Globals &g, const Operation &op, const mgc_count_config &cfg) {
  if (cfg.count_suffix_length) die("ERROR: %s", "count-suffix= and gpus= cannot be combined.");
  const uint32_t N = g.gpus;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) die("ERROR: %s", "no HIP device.");
  const auto t_start = std::chrono::steady_clock::now();
  // the share of every rank: windows of the plain-text files by bytes, the other inputs round-robin
  std::vector<std::vector<InputPiece>> share(N);
  std::vector<std::pair<std::string, uint64_t>> plain;
  uint64_t plain_total = 0;
  uint32_t rr = 0;
  for (const std::string &name : op.seq_inputs) {
    struct stat fst;
    bool cut = false;
    if (name != "-" && !has_compressed_suffix(name) && stat(name.c_str(), &fst) == 0 && S_ISREG(fst.st_mode) &&
        !(getenv("MERYL_HOST_PARSER") && getenv("MERYL_HOST_PARSER")[0] == '1')) {
      msr_reader *r = msr_open(name.c_str());
      if (!r) die("ERROR: %s", msr_last_error());
      cut = msr_format(r) == MSR_FORMAT_FASTX;
      msr_close(r);
    }
    if (cut) { plain.emplace_back(name, (uint64_t)fst.st_size); plain_total += (uint64_t)fst.st_size; }
    else share[rr++ % N].push_back(InputPiece{name, 0, ~0ull});
  }
  {
    uint64_t file_base = 0;                                   // position of the file in the concatenation of the plain files
    for (const auto &pf : plain) {
      const uint64_t size = pf.second;
      uint64_t prev = 0;
      for (uint32_t r = 0; r < N; r++) {
        // the rank's window of the concatenation, clipped to this file, moved up to the next record start
        const uint64_t hi_cat = (r + 1 == N) ? plain_total : (uint64_t)((unsigned __int128)plain_total * (r + 1) / N);
        uint64_t hi = hi_cat <= file_base ? 0 : std::min<uint64_t>(size, hi_cat - file_base);
        if (hi > 0 && hi < size && mgc_text_record_start(pf.first.c_str(), 0, hi, &hi) != MGC_OK) die("ERROR: %s", mgc_last_error(nullptr));
        if (hi < prev) hi = prev;
        if (hi > prev) share[r].push_back(InputPiece{pf.first, prev, hi});
        prev = hi;
      }
      file_base += size;
    }
  }
  std::vector<mgc_session *> sess(N, nullptr);
  std::vector<int> dev(N, 0);
  std::vector<uint64_t> taken(N, 0);
  const int readers = (int)std::max<uint32_t>(2, std::min<uint32_t>(g.threads, 16) / N);
  for (uint32_t r = 0; r < N; r++) {
    dev[r] = (int)(r % (uint32_t)ndev);
    mgc_count_config rc = cfg;
    rc.homopoly_compress = 0;                                 // the node count compresses every rank's stream itself
    sess[r] = mgc_open(&rc, dev[r]);
    if (!sess[r]) die("ERROR: %s", mgc_last_error(nullptr));
    mgc_set_batch_bases(sess[r], ~0ull >> 2);                // a rank's share is staged whole; the node count batches the counting
  }
  {
    std::vector<std::thread> th;
    g_gzip_parallel = false;
    for (uint32_t r = 0; r < N; r++) th.emplace_back([&, r] { taken[r] = load_inputs(sess[r], share[r], readers); });
    for (auto &t : th) t.join();
  }
  std::vector<const uint8_t *> ptr(N, nullptr);
  std::vector<uint64_t> len(N, 0);
  uint64_t total_bases = 0;
  for (uint32_t r = 0; r < N; r++) {
    if (mgc_staged_bases(sess[r], &ptr[r], &len[r]) != MGC_OK) die("ERROR: %s", mgc_last_error(sess[r]));
    total_bases += taken[r];
  }
  const auto t_loaded = std::chrono::steady_clock::now();
  if (g.verbosity > 0)
    fprintf(stderr, "\nInput complete.  Counting on %u ranks and writing results to '%s', using %u thread%s.\n",
            N, op.output.c_str(), g.threads, (g.threads == 1) ? "" : "s");
  uint64_t batch = 0;
  if (getenv("MERYL_BATCH_BASES") && *getenv("MERYL_BATCH_BASES")) batch = strtoull(getenv("MERYL_BATCH_BASES"), nullptr, 10);
  mgc_node_profile np;
  if (mgc_count_node_batched(&cfg, N, dev.data(), ptr.data(), len.data(), batch, op.output.c_str(), (int)g.threads, &np) != MGC_OK)
    die("ERROR: %s", mgc_last_error(nullptr));
  const auto t_done = std::chrono::steady_clock::now();
  if (g.verbosity > 2)
    fprintf(stderr, "\nTIMING  read+parse+stage=%.3f s (every rank its own share)   node count+write=%.3f s   (ranks=%u, routing bits=%u, "
                    "batches=%u, partition=%.3f s, exchange+count=%.3f s, merge of parked waves=%.3f s, files=%.3f s, stitch=%.3f s, "
                    "database_bytes=%" PRIu64 ")\n",
            std::chrono::duration<double>(t_loaded - t_start).count(), std::chrono::duration<double>(t_done - t_loaded).count(),
            np.n_ranks, np.bucket_bits, np.n_batches, np.partition_s, np.exchange_count_s, np.merge_runs_s, np.close_s, np.merge_parts_s,
            np.data_bytes);
  for (mgc_session *q : sess) mgc_close(q);
  if (g.verbosity > 0) {
    fprintf(stderr, "\nFinished counting.\n");
    if (g.verbosity > 2)
      fprintf(stderr, "  %" PRIu64 " bases, %" PRIu64 " k-mer instances, %" PRIu64 " distinct k-mers, prefix bits %u.\n",
              total_bases, np.n_instances, np.n_distinct, cfg.w_prefix);
  }
  return 0;
}

int run_count(const Globals &g, const Operation &op) {
  if (g.k == 0) die("ERROR: Kmer size not supplied with modifier k=<kmer-size>.");                    // merylOp-count.C:311-312
  if (op.output.empty() && !g.only_config) die("ERROR: No output specified for count operation.");     // :314-315

  uint64_t exp_num_kmers = op.exp_num_kmers;
  if (exp_num_kmers == 0)                                                                              // :317-318
    for (const std::string &n : op.seq_inputs) exp_num_kmers += msr_guess_number_of_kmers(n.c_str());

  mgc_count_config cfg;
  memset(&cfg, 0, sizeof(cfg));
  cfg.k = g.k;
  cfg.mode = (op.kind == OP_COUNT) ? MGC_MODE_CANONICAL : (op.kind == OP_COUNT_FORWARD) ? MGC_MODE_FORWARD : MGC_MODE_REVERSE;
  cfg.n_kmers_estimate = exp_num_kmers;
  cfg.memory_allowed = (uint64_t)(g.memory_gb * 1024.0 * 1024.0 * 1024.0);                            // merylCommandBuilder.C:299-302
  cfg.threads = g.threads;
  bool any_compress = false;
  for (bool c : op.seq_compress) any_compress = any_compress || c;
  for (bool c : op.seq_compress)
    if (c != any_compress) die("ERROR: `compress` must apply to all or none of the inputs of one count in this build.");
  cfg.homopoly_compress = any_compress ? 1 : 0;
  if (op.count_suffix.size() > MGC_MAX_COUNT_SUFFIX) die("ERROR: %s", "count-suffix of more than 32 bases.");
  cfg.count_suffix_length = (uint32_t)op.count_suffix.size();                                         // merylOp.H:139-147
  memcpy(cfg.count_suffix, op.count_suffix.c_str(), op.count_suffix.size());
  cfg.label_size = g.label_size;                                                                      // meryl2: every k-mer of a count
  cfg.label_constant = op.label;                                                                      // carries one constant label
  if (mgc_configure_counting(&cfg) != MGC_OK) die("ERROR: %s", mgc_last_error(nullptr));

  if (g.verbosity > 0) print_configuration(g, op, exp_num_kmers, cfg);
  if (g.only_config) return 0;                                                                         // -C, merylOp-countThreads.C:392-393

  if (g.verbosity > 0)
    fprintf(stderr, "Start counting with %s method.\n", cfg.use_simple ? "SIMPLE" : "THREADED");     // merylOp-nextMer.C:205-209

  if (g.gpus > 1) return run_count_node(g, op, cfg);

  mgc_session *s = mgc_open(&cfg, -1);
  if (!s) die("ERROR: %s", mgc_last_error(nullptr));

  if (getenv("MERYL_BATCH_BASES") && *getenv("MERYL_BATCH_BASES"))                                    // tests: force out-of-core batches
    mgc_set_batch_bases(s, strtoull(getenv("MERYL_BATCH_BASES"), nullptr, 10));
  uint64_t total_bases = 0;
  const auto t_start = std::chrono::steady_clock::now();
  uint64_t text_total = 0;
  for (const std::string &name : op.seq_inputs) text_total += msr_guess_number_of_kmers(name.c_str());
  const bool host_parser = getenv("MERYL_HOST_PARSER") && getenv("MERYL_HOST_PARSER")[0] == '1';
  if (!host_parser && text_total) (void)mgc_reserve_text(s, text_total);
  {
    // bases to expect: a FASTQ file is at most half sequence, anything else at most all of it (compressed: the reference's factors)
    uint64_t expect = 0;
    for (const std::string &name : op.seq_inputs) {
      uint64_t e = msr_guess_number_of_kmers(name.c_str());
      if (name != "-" && !has_compressed_suffix(name)) {
        FILE *f = fopen(name.c_str(), "rb");
        if (f) { const int c = fgetc(f); fclose(f); if (c == '@') e /= 2; }
      }
      expect += e;
    }
    if (expect && cfg.count_suffix_length == 0) (void)mgc_prepare(s, expect + 4096);
  }
  std::vector<InputPiece> pieces;
  for (const std::string &name : op.seq_inputs) pieces.push_back(InputPiece{name, 0, ~0ull});
  g_inflate_threads = (int)g.threads;
  total_bases = load_inputs(s, pieces, (int)std::min<uint32_t>(g.threads, 16));

  const auto t_loaded = std::chrono::steady_clock::now();
  if (g.verbosity > 2) (void)mgc_set_profiling(s, 1);           // -V: the device's own clock of the count beside the wall clock
  if (mgc_count(s) != MGC_OK) die("ERROR: %s", mgc_last_error(s));
  const auto t_counted = std::chrono::steady_clock::now();
  mgc_result_info info;
  mgc_get_result_info(s, &info);

  if (g.verbosity > 0) {
    fprintf(stderr, "\nInput complete.  Writing results to '%s', using %u thread%s.\n",                // :447-448
            op.output.c_str(), g.threads, (g.threads == 1) ? "" : "s");
  }
  mgc_db_write_profile wprof;
  if (mgc_write_database_profiled(s, op.output.c_str(), (int)g.threads, &wprof) != MGC_OK) {
    fprintf(stderr, "ERROR: writing '%s' failed: %s %s\n", op.output.c_str(), mdb_last_error(), mgc_last_error(s));
    exit(1);
  }
  const auto t_written = std::chrono::steady_clock::now();
  mgc_get_result_info(s, &info);                       // (an out-of-core result knows its distinct k-mers only once the runs are merged)
  if (g.verbosity > 2) {                                                                               // -V: where the wall clock went
    auto sec = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
      return std::chrono::duration<double>(b - a).count();
    };
    fprintf(stderr, "\nTIMING  read+parse+stage=%.3f s   count=%.3f s   encode+write=%.3f s   (device encode=%.4f s, copy+write=%.3f s, "
                    "database_bytes=%" PRIu64 ")   startup=%.3f s (main -> session open: HIP runtime, device, streams)\n",
            sec(t_start, t_loaded), sec(t_loaded, t_counted), sec(t_counted, t_written), wprof.encode_ms / 1e3,
            wprof.copy_write_s, wprof.data_bytes, sec(g_t_main, t_start));
  }
  if (g.verbosity > 2) {
    mgc_profile cp;
    if (mgc_get_profile(s, &cp) == MGC_OK && cp.total_ms > 0)
      fprintf(stderr, "        count on the device: %.1f ms (histogram %.1f, partition %.1f, grouping passes %.1f, sub-bucket count + packing %.1f); "
                      "the rest of count= is the host's: buffers the input did not size, the first launches, synchronisations\n",
              cp.total_ms, cp.stage_ms[MGC_STAGE_HISTOGRAM], cp.stage_ms[MGC_STAGE_PARTITION], cp.stage_ms[MGC_STAGE_SORT], cp.stage_ms[MGC_STAGE_RLE]);
    if (mgc_get_profile(s, &cp) == MGC_OK && cp.n_batches > 1)
      fprintf(stderr, "        counted in %u batches (memory-full spills, merylOp-countThreads.C:323-379), merged on the device in %.1f ms\n",
              cp.n_batches, cp.merge_ms);
  }
  // The database is complete and its files are closed.  When this count is all the command does, the process ends right away:
  // releasing a 120 GB arena, gigabytes of pinned ring and the runtime in an orderly way takes a good part of a second and gives
  // nothing back that process exit does not (MERYL_FAST_EXIT=0: the orderly way).
  if (!g.fast_exit) mgc_close(s);
  if (g.verbosity > 0) {
    fprintf(stderr, "\nFinished counting.\n");                                                         // :473
    if (g.verbosity > 2)
      fprintf(stderr, "  %" PRIu64 " bases, %" PRIu64 " k-mer instances, %" PRIu64 " distinct k-mers, prefix bits %u.\n",
              total_bases, info.n_instances, info.n_distinct, info.w_prefix);
  }
  return 0;
}

// one slice as `print` writes it: k-mer <TAB> value (merylOp-nextMer.C:673-676; meryl2 adds the label in binary,
// src/meryl2/merylOp-nextMer.C:36-43); hi / lb may be null
void print_kmers(uint32_t k, uint32_t label_size, const uint64_t *lo, const uint64_t *hi, const uint32_t *cn, const uint64_t *lb, uint64_t n) {
  static const char acgt[4] = { 'A', 'C', 'T', 'G' };
  std::vector<char> kstr(k + 1, 0);
  char lbits[72];
  for (uint64_t i = 0; i < n; i++) {
    const unsigned __int128 m = ((unsigned __int128)(hi ? hi[i] : 0) << 64) | lo[i];
    for (uint32_t b = 0; b < k; b++) kstr[b] = acgt[(unsigned)(m >> (2 * (k - 1 - b))) & 3];
    if (label_size == 0 || !lb) {
      fprintf(stdout, "%s\t%u\n", kstr.data(), cn[i]);
    } else {
      for (uint32_t b = 0; b < label_size; b++) lbits[b] = ((lb[i] >> (label_size - 1 - b)) & 1) ? '1' : '0';
      lbits[label_size] = 0;
      fprintf(stdout, "%s\t%u\t%s\n", kstr.data(), cn[i], lbits);
    }
  }
}

void print_database(const std::string &dbn) {
  mdb_reader *r = mdb_reader_open(dbn.c_str());
  if (!r) die("ERROR: %s", mdb_last_error());
  mdb_info info;
  mdb_reader_info(r, &info);
  for (uint32_t ff = 0; ff < MGC_NUM_FILES; ff++) {            // ascending == `threads=1 print` order (quick-start.rst:74-77)
    uint64_t *lo = nullptr, *hi = nullptr, *lb = nullptr, n = 0;
    uint32_t *cn = nullptr;
    if (mdb_reader_read_file_ex(r, ff, &lo, &hi, &cn, &lb, &n) != MGC_OK) die("ERROR: %s", mdb_last_error());
    print_kmers(info.k, info.label_size, lo, hi, cn, lb, n);
    mdb_free(lo); mdb_free(hi); mdb_free(cn); mdb_free(lb);
  }
  mdb_reader_close(r);
}

// ---- histogram / statistics (src/meryl/merylOp-histogram.C:20-97) ----
struct Histogram { std::vector<uint64_t> values, occurrences; uint64_t unique = 0, distinct = 0, total = 0; };

// the histogram the writer stored in a database's master index (quick-start.rst:144); *k: its k-mer size
Histogram stored_histogram(const std::string &dbn, uint32_t *k) {
  mdb_reader *r = mdb_reader_open(dbn.c_str());
  if (!r) die("ERROR: %s", mdb_last_error());
  mdb_info i;
  mdb_reader_info(r, &i);
  Histogram h;
  h.values.resize(i.hist_len); h.occurrences.resize(i.hist_len);
  if (i.hist_len && mdb_reader_histogram(r, h.values.data(), h.occurrences.data()) != 0) die("ERROR: %s", mdb_last_error());
  h.unique = i.num_unique; h.distinct = i.num_distinct; h.total = i.num_total;
  *k = i.k;
  mdb_reader_close(r);
  return h;
}

// value <TAB> number of distinct k-mers with that value, ascending (:39-42)
void write_histogram(FILE *f, const Histogram &h) {
  for (size_t ii = 0; ii < h.values.size(); ii++) fprintf(f, "%" PRIu64 "\t%" PRIu64 "\n", h.values[ii], h.occurrences[ii]);
}

// the statistics table (:65-93; the text is the library's, mdb_format_statistics)
void write_statistics(FILE *f, uint32_t k, const Histogram &h) {
  const size_t len = mdb_format_statistics(k, h.values.data(), h.occurrences.data(), h.values.size(), h.unique, h.distinct, h.total, nullptr, 0);
  std::vector<char> text(len + 1);
  mdb_format_statistics(k, h.values.data(), h.occurrences.data(), h.values.size(), h.unique, h.distinct, h.total, text.data(), text.size());
  fwrite(text.data(), 1, len, f);
}

// where a report goes: no name or "-" is stdout (merylOpTemplate.C:174-175)
FILE *open_report(const std::string &name) {
  if (name.empty() || name == "-") return stdout;
  FILE *f = fopen(name.c_str(), "w");
  if (!f) die("ERROR: cannot create the report file '%s'.", name.c_str());
  return f;
}
void close_report(FILE *f, const std::string &name) {
  if (f == stdout) { fflush(f); return; }
  if (fclose(f) != 0) die("ERROR: writing the report file '%s' failed.", name.c_str());
}

// `meryl histogram <db>` / `meryl statistics <db>`: from the stored histogram, on the host
int run_stored_report(OpKind verb, const std::string &dbn) {
  uint32_t k = 0;
  const Histogram h = stored_histogram(dbn, &k);
  if (verb == OP_HISTOGRAM) write_histogram(stdout, h); else write_statistics(stdout, k, h);
  return 0;
}

// `meryl dumpFile <db>/0x######`: the three tables of documentation/source/usage.rst:24-45 (src/meryl/meryl.C:41-45) --
// the file's index, every block's header, every k-mer as stored (unary prefix delta, accumulated prefix, the two halves
// of the binary remainder, value).
int run_dump_file(const Operation &op) {
  for (const std::string &arg : op.db_inputs) {
    const size_t slash = arg.find_last_of('/');
    const std::string dbn = (slash == std::string::npos) ? "." : arg.substr(0, slash);
    std::string base = (slash == std::string::npos) ? arg : arg.substr(slash + 1);
    const size_t dot = base.find('.');
    if (dot != std::string::npos) base.erase(dot);                                                    // 0x000000.merylData is fine too
    if (base.size() != 8 || base.compare(0, 2, "0x") != 0) die("ERROR: dumpFile wants <database>/0x###### (six binary digits), not '%s'.", arg.c_str());
    uint32_t ff = 0;
    for (int i = 2; i < 8; i++) { if (base[i] != '0' && base[i] != '1') die("ERROR: bad file name '%s'.", arg.c_str()); ff = (ff << 1) | (uint32_t)(base[i] - '0'); }
    mdb_reader *r = mdb_reader_open(dbn.c_str());
    if (!r) die("ERROR: %s", mdb_last_error());
    mdb_info info;
    mdb_reader_info(r, &info);
    const uint64_t nblocks = (uint64_t)1 << info.num_blocks_bits;
    std::vector<mdb_index_entry> idx(nblocks);
    if (mdb_reader_file_index(r, ff, idx.data()) != MGC_OK) die("ERROR: %s", mdb_last_error());
    fprintf(stdout, "\n    prefix    blkPos    nKmers\n---------- --------- ---------\n");
    for (const mdb_index_entry &e : idx) fprintf(stdout, "0x%08" PRIx64 " %9" PRIu64 " %9" PRIu64 "\n", e.prefix, e.position, e.n_kmers);
    fprintf(stdout, "\n            prefix   nKmers kCode uBits bBits                 k1 cCode                 c1                 c2\n"
                    "------------------ -------- ----- ----- ----- ------------------ ----- ------------------ ------------------\n");
    for (const mdb_index_entry &e : idx) {
      mdb_block_header h;
      if (mdb_reader_block_header(r, ff, e.position, &h) != MGC_OK) die("ERROR: %s", mdb_last_error());
      if (h.prefix != e.prefix) continue;                                                              // an index slot no block was written for
      fprintf(stdout, "0x%016" PRIx64 " %8" PRIu64 " %5u %5u %5u 0x%016" PRIx64 " %5u 0x%016" PRIx64 " 0x%016" PRIx64 "\n",
              h.prefix, h.n_kmers, h.k_code, h.unary_bits, h.binary_bits, h.k1, h.c_code, h.c1, h.c2);
    }
    fprintf(stdout, "\n kmerIdx prefixDelta      prefix |--- suffix-size and both suffixes ---|    value\n"
                    "-------- ----------- ----------- -- ---------------- -- ---------------- --------\n");
    for (const mdb_index_entry &e : idx) {
      mdb_block_header h;
      uint64_t *pd = nullptr, *tp = nullptr, *rh = nullptr, *rl = nullptr;
      uint32_t *vv = nullptr;
      if (mdb_reader_read_block_raw(r, ff, e.position, &h, &pd, &tp, &rh, &rl, &vv) != MGC_OK) die("ERROR: %s", mdb_last_error());
      if (h.prefix != e.prefix) h.n_kmers = 0;
      const uint32_t hi_bits = h.binary_bits > 64 ? h.binary_bits - 64 : 0, lo_bits = h.binary_bits > 64 ? 64 : h.binary_bits;
      for (uint64_t i = 0; i < h.n_kmers; i++)
        fprintf(stdout, "%8" PRIu64 " %11" PRIu64 " %011" PRIx64 " %2u %016" PRIx64 " %2u %016" PRIx64 " %8u\n",
                i, pd[i], tp[i], hi_bits, rh[i], lo_bits, rl[i], vv[i]);
      mdb_free(pd); mdb_free(tp); mdb_free(rh); mdb_free(rl); mdb_free(vv);
    }
    mdb_reader_close(r);
  }
  return 0;
}

int run_dump_index(const Operation &op) {
  for (const std::string &dbn : op.db_inputs) {
    mdb_reader *r = mdb_reader_open(dbn.c_str());
    if (!r) die("ERROR: %s", mdb_last_error());
    mdb_info i;
    mdb_reader_info(r, &i);
    fprintf(stdout, "Opened '%s'.\n", dbn.c_str());                                                    // shape of usage.rst:13-19
    fprintf(stdout, "  kmerSize       %u\n", i.k);
    fprintf(stdout, "  prefixSize     %u\n", i.prefix_size);
    fprintf(stdout, "  suffixSize     %u\n", i.suffix_size);
    fprintf(stdout, "  numFilesBits   %u (%u files)\n", i.num_files_bits, 1u << i.num_files_bits);
    fprintf(stdout, "  numBlocksBits  %u (%u blocks)\n", i.num_blocks_bits, 1u << i.num_blocks_bits);
    if (i.label_size) fprintf(stdout, "  labelSize      %u\n", i.label_size);
    fprintf(stdout, "  unique         %" PRIu64 "\n  distinct       %" PRIu64 "\n  total          %" PRIu64 "\n",
            i.num_unique, i.num_distinct, i.num_total);
    mdb_reader_close(r);
  }
  return 0;
}

// `union-sum a.meryl [greater-than 1 b.meryl] [count ... output c.meryl] output u.meryl`: a tree of the set operations
// (merylOp-nextMer.C:559-612) and the single-input value operations (:490-557) runs as ONE evaluation (mgc_db_eval): the
// slices of its leaves -- databases named on the command line, and the outputs of counts, which ran first (meryl.C:211-227
// turns a finished count into a pass-through over its new database) -- are loaded once per file, every operation's result
// stays on the device, and only operations given `output` write, as in the reference (:227).  `print` of such a tree
// receives the root's slices, files ascending.
bool is_tree_op(const Operation &op) { return op.kind == OP_MERGE || op.kind == OP_VALUE; }

struct EvalTree {
  std::vector<mgc_eval_node_assigned> nodes;              // the widest public node; run_tree narrows it for the entry point it calls
  std::vector<std::vector<uint32_t>>  kids;
  std::string                         first_leaf;
  bool                                label_words = false;    // an operation of the tree carries label=
  std::vector<mgc_select_term>        terms;                  // the selector programs of all nodes, one after the other
  bool                                value_words = false;    // an operation of the tree carries value=
  uint32_t                            leaf_label_size = 0;    // the largest label size among the leaves
  std::vector<int>                    node_op;                // the operation (index into ops) behind every node; -1: a database
};

// label=<word> | <word>#<const> | #<const> on a set or value operation (merylCommandBuilder-isAssign.C:124-156); without a
// constant the word's identity (:142-156, mgc_label_default_constant)
void parse_label_assign(const std::string &w, const std::string &val, Operation &op) {
  static const struct { const char *word; int code; } words[] = {
    {"first", MGC_LABEL_FIRST}, {"selected", MGC_LABEL_SELECTED}, {"min", MGC_LABEL_MIN}, {"max", MGC_LABEL_MAX}, {"and", MGC_LABEL_AND},
    {"or", MGC_LABEL_OR}, {"xor", MGC_LABEL_XOR}, {"difference", MGC_LABEL_DIFFERENCE}, {"lightest", MGC_LABEL_LIGHTEST},
    {"heaviest", MGC_LABEL_HEAVIEST}, {"invert", MGC_LABEL_INVERT}};
  const size_t hash = val.find('#');
  const std::string word = val.substr(0, hash);
  int code = -1;
  if (word.empty() && hash != std::string::npos) code = MGC_LABEL_SET;
  for (const auto &e : words) if (word == e.word) code = e.code;
  if (word == "shift-left" || word == "shift-right" || word == "rotate-left" || word == "rotate-right")
    die("ERROR: '%s': the shift and rotate label words are not part of this build (the reference's shift the wrong way and its rotate is a shift).", w.c_str());
  if (code < 0) die("ERROR: Unknown assign:label=<parameter> in '%s'.", w.c_str());                    // :160-163
  op.has_label_op = true;
  op.label_op = code;
  op.label_constant = (hash != std::string::npos) ? strtoull(val.c_str() + hash + 1, nullptr, 0) : mgc_label_default_constant(code);
}

// distinct=<f> / word-frequency=<f> turn into a threshold from the input's stored histogram (initializeThreshold, :65-118)
uint64_t threshold_from_histogram(const Operation &op, const std::string &in) {
  uint64_t c = op.constant;
  mdb_reader *r = mdb_reader_open(in.c_str());
  if (!r) die("ERROR: %s", mdb_last_error());
  mdb_info info;
  mdb_reader_info(r, &info);
  std::vector<uint64_t> hv(info.hist_len), ho(info.hist_len);
  if (info.hist_len) mdb_reader_histogram(r, hv.data(), ho.data());
  mdb_reader_close(r);
  if (op.frac_distinct >= 0) {                                             // :104-114
    const uint64_t target = (uint64_t)(op.frac_distinct * (double)info.num_distinct);
    uint64_t n = 0;
    for (uint64_t i = 0; i < info.hist_len; i++) { n += ho[i]; if (n >= target) { c = hv[i]; break; } }
  }
  if (op.word_freq >= 0) c = (uint64_t)(op.word_freq * (double)info.num_total);   // :116-118
  return c;
}

int run_tree(const Globals &g, const std::vector<Operation> &ops, int root, bool print, OpKind verb = OP_NONE);

uint32_t add_tree_node(const Globals &g, const std::vector<Operation> &ops, int i, EvalTree &t) {
  const Operation &op = ops[i];
  const bool by_histogram = op.kind == OP_VALUE && (op.frac_distinct >= 0 || op.word_freq >= 0);
  if (op.kind == OP_MERGE && op.inputs.empty()) die("ERROR: operation '%s' has no inputs.", op.word.c_str());
  if (op.kind == OP_VALUE && op.inputs.size() != 1) die("ERROR: operation '%s' takes exactly one input.", op.word.c_str());
  std::vector<uint32_t> kids;
  std::string leaf;
  for (const InputRef &in : op.inputs) {
    if (in.child >= 0 && is_tree_op(ops[in.child]) && !by_histogram) { kids.push_back(add_tree_node(g, ops, in.child, t)); continue; }
    if (in.child >= 0 && is_tree_op(ops[in.child])) {
      // a threshold from statistics needs a database (merylOp-nextMer.C:85-96); an input operation that writes one runs first
      if (ops[in.child].output.empty()) die("ERROR: input '%s' to operation most-frequent is not a meryl database.", ops[in.child].word.c_str());
      run_tree(g, ops, in.child, false);
    }
    leaf = in.child >= 0 ? ops[in.child].output : in.path;
    if (!dir_has_index(leaf)) die("ERROR: input '%s' is not a meryl database.", leaf.c_str());
    if (t.first_leaf.empty()) t.first_leaf = leaf;
    {
      mdb_reader *rd = mdb_reader_open(leaf.c_str());
      if (!rd) die("ERROR: %s", mdb_last_error());
      mdb_info info;
      mdb_reader_info(rd, &info);
      mdb_reader_close(rd);
      t.leaf_label_size = std::max(t.leaf_label_size, info.label_size);
    }
    mgc_eval_node_assigned nd;
    memset(&nd, 0, sizeof(nd));
    nd.kind = MGC_NODE_DATABASE;
    nd.path = in.child >= 0 ? ops[in.child].output.c_str() : in.path.c_str();
    t.nodes.push_back(nd);
    t.kids.emplace_back();
    t.node_op.push_back(-1);
    kids.push_back((uint32_t)t.nodes.size() - 1);
  }
  mgc_eval_node_assigned nd;
  memset(&nd, 0, sizeof(nd));
  nd.path = op.output.empty() ? nullptr : op.output.c_str();
  nd.label_op = op.label_op;
  nd.label_constant = op.label_constant;
  t.label_words = t.label_words || op.has_label_op;
  if (op.kind == OP_MERGE) {
    nd.kind = MGC_NODE_MERGE;
    nd.op = op.merge_op;
    if (g.verbosity > 0)
      fprintf(stderr, "\nPROCESSING %s of %zu input%s%s%s%s.\n", op.word.c_str(), kids.size(), kids.size() == 1 ? "" : "s",
              op.output.empty() ? "" : " into '", op.output.c_str(), op.output.empty() ? "" : "'");
  } else {
    nd.kind = MGC_NODE_VALUE;
    nd.op = op.value_op;
    nd.constant = by_histogram ? threshold_from_histogram(op, leaf) : op.constant;
    if (nd.constant == ~0ull) die("ERROR: operation '%s' needs a number (threshold / constant).", op.word.c_str());
    if (g.verbosity > 0)
      fprintf(stderr, "\nPROCESSING %s %" PRIu64 "%s%s%s.\n", op.word.c_str(), (uint64_t)nd.constant,
              op.output.empty() ? "" : " into '", op.output.c_str(), op.output.empty() ? "" : "'");
  }
  // the selector words are decoded once the number of inputs is known (`input:all`, `@n`), by the library's one parser
  nd.first_term = (uint32_t)t.terms.size();
  if (!op.select_words.empty()) {
    std::vector<const char *> words;
    for (const std::string &w : op.select_words) words.push_back(w.c_str());
    mgc_select_term terms[MGC_SELECT_MAX_TERMS];
    if (mgc_select_parse(words.data(), (uint32_t)words.size(), (uint32_t)kids.size(), terms, MGC_SELECT_MAX_TERMS, &nd.n_terms) != MGC_OK)
      die("ERROR: %s", ("operation '" + op.word + "': " + mgc_last_error(nullptr)).c_str());
    t.terms.insert(t.terms.end(), terms, terms + nd.n_terms);
  }
  nd.value_assign = op.value_assign;
  nd.value_constant = op.value_constant;
  t.nodes.push_back(nd);
  t.value_words = t.value_words || op.has_value_assign;
  t.kids.push_back(kids);
  t.node_op.push_back(i);
  return (uint32_t)t.nodes.size() - 1;
}

struct PrintCtx { uint32_t k, label_size; };
void print_slice(void *ctx, uint32_t, const uint64_t *lo, const uint64_t *hi, const uint32_t *values, uint64_t n) {
  print_kmers(static_cast<PrintCtx *>(ctx)->k, 0, lo, hi, values, nullptr, n);
}
void print_slice_labelled(void *ctx, uint32_t, const uint64_t *lo, const uint64_t *hi, const uint32_t *values, const uint64_t *labels, uint64_t n) {
  const PrintCtx *pc = static_cast<PrintCtx *>(ctx);
  print_kmers(pc->k, pc->label_size, lo, hi, values, labels, n);
}

// mgc_db_eval_listed's callback of `print [operation]`: a piece of the root's text, files ascending, pieces in order
int print_text(void *, uint32_t, uint32_t, const void *text, uint64_t n) { return fwrite(text, 1, n, stdout) == n ? 0 : 1; }

// the nodes as a narrower public struct: the fields it names, copied
template <typename T>
std::vector<T> narrowed(const std::vector<mgc_eval_node_assigned> &nodes) {
  std::vector<T> out(nodes.size());
  for (size_t v = 0; v < nodes.size(); v++) {
    const mgc_eval_node_assigned &s = nodes[v];
    T &d = out[v];
    memset(&d, 0, sizeof(d));
    d.kind = s.kind; d.op = s.op; d.constant = s.constant; d.path = s.path; d.first_child = s.first_child; d.n_children = s.n_children;
    if constexpr (!std::is_same<T, mgc_eval_node>::value) { d.label_op = s.label_op; d.label_constant = s.label_constant; }
    if constexpr (std::is_same<T, mgc_eval_node_selected>::value) { d.first_term = s.first_term; d.n_terms = s.n_terms; }
  }
  return out;
}

// the operation tree under ops[root] (paths point into `ops`, which outlives the call); verb: OP_HISTOGRAM / OP_STATISTICS when the
// tree is the input of that verb, whose report of the root goes to stdout
int run_tree(const Globals &g, const std::vector<Operation> &ops, int root, bool print, OpKind verb) {
  EvalTree t;
  const uint32_t r = add_tree_node(g, ops, root, t);
  std::vector<uint32_t> children;
  for (size_t v = 0; v < t.nodes.size(); v++) {
    t.nodes[v].first_child = (uint32_t)children.size();
    t.nodes[v].n_children = (uint32_t)t.kids[v].size();
    children.insert(children.end(), t.kids[v].begin(), t.kids[v].end());
  }
  // reports: the verb's on the root, output:histogram / output:statistics on any operation; their files exist before anything runs
  struct Report { uint32_t node; bool stats; std::string name; FILE *f; };
  std::vector<Report> reports;
  std::vector<uint8_t> want(t.nodes.size(), 0);
  for (uint32_t v = 0; v < t.nodes.size(); v++) {
    if (t.node_op[v] < 0) continue;
    const Operation &o = ops[t.node_op[v]];
    if (o.has_hist_out) reports.push_back(Report{v, false, o.hist_out, nullptr});
    if (o.has_stats_out) reports.push_back(Report{v, true, o.stats_out, nullptr});
  }
  if (verb != OP_NONE) reports.push_back(Report{r, verb == OP_STATISTICS, "-", nullptr});
  // deliberately before the evaluation, like the reference, which opens them while it reads the command (merylOpTemplate.C:187-188,
  // 207-208): a name that cannot be written stops the command before any work; an evaluation that fails leaves the file empty
  for (Report &rp : reports) { want[rp.node] = 1; rp.f = open_report(rp.name); }
  PrintCtx pc{0, 0};
  if (print || !reports.empty()) {                                                 // (every leaf holds the same k: mgc_db_eval checks)
    mdb_reader *rd = mdb_reader_open(t.first_leaf.c_str());
    if (!rd) die("ERROR: %s", mdb_last_error());
    mdb_info info;
    mdb_reader_info(rd, &info);
    mdb_reader_close(rd);
    pc.k = info.k;
  }
  // with labels only when something asks for them: -l, a label= word, or a leaf that stores labels; the outputs (and the
  // label column `print` adds) take -l bits, or the largest label size among the leaves
  const bool with_labels = g.label_size_given || t.label_words || t.leaf_label_size;
  const uint32_t n_nodes = (uint32_t)t.nodes.size(), n_children = (uint32_t)children.size(), n_terms = (uint32_t)t.terms.size();
  const uint32_t label_size = g.label_size_given ? g.label_size : 0;
  if (with_labels) pc.label_size = g.label_size_given && g.label_size ? g.label_size : t.leaf_label_size;
  int rc;
  std::vector<mgc_value_hist *> hists(t.nodes.size(), nullptr);
  if (print && reports.empty()) {                              // the root's text, formatted on the device; no slice leaves it as arrays
    std::vector<uint8_t> want_list(t.nodes.size(), 0);
    want_list[r] = 1;
    rc = mgc_db_eval_listed(t.nodes.data(), n_nodes, children.data(), n_children, r, t.terms.data(), n_terms, with_labels ? 1 : 0, label_size,
                            nullptr, nullptr, -1, (int)g.threads, nullptr, nullptr, want_list.data(), print_text, nullptr);
  }
  // a report somewhere: the entry point that collects them -- also under `print`, whose lines then come from the slice callback as before:
  // mgc_db_eval_listed could take want[] and hists[] as well, but what that form says when it fails without a device is pinned to name
  // mgc_db_eval_reported (tests/test_value_hist_host.py)
  else if (!reports.empty())
    rc = mgc_db_eval_reported(t.nodes.data(), n_nodes, children.data(), n_children, r, t.terms.data(), n_terms, with_labels ? 1 : 0, label_size,
                              print ? print_slice_labelled : nullptr, &pc, -1, (int)g.threads, want.data(), hists.data());
  else if (t.value_words)                                      // a value= somewhere: the tree through mgc_db_eval_assigned
    rc = mgc_db_eval_assigned(t.nodes.data(), n_nodes, children.data(), n_children, r, t.terms.data(), n_terms, with_labels ? 1 : 0, label_size,
                              print ? print_slice_labelled : nullptr, &pc, -1, (int)g.threads);
  else if (!t.terms.empty())                                   // a selector somewhere: the same tree through mgc_db_eval_selected
    rc = mgc_db_eval_selected(narrowed<mgc_eval_node_selected>(t.nodes).data(), n_nodes, children.data(), n_children, r, t.terms.data(), n_terms,
                              with_labels ? 1 : 0, label_size, print ? print_slice_labelled : nullptr, &pc, -1, (int)g.threads);
  else if (with_labels)
    rc = mgc_db_eval_labelled(narrowed<mgc_eval_node_labelled>(t.nodes).data(), n_nodes, children.data(), n_children, r, label_size,
                              print ? print_slice_labelled : nullptr, &pc, -1, (int)g.threads);
  else
    rc = mgc_db_eval(narrowed<mgc_eval_node>(t.nodes).data(), n_nodes, children.data(), n_children, r, print ? print_slice : nullptr, &pc, -1,
                     (int)g.threads);
  if (rc != MGC_OK) die("ERROR: %s", mgc_db_stream_error(nullptr));
  fflush(stdout);
  for (Report &rp : reports) {                                 // merylOpTemplate::finishAction, :295-307
    mgc_value_hist *hh = hists[rp.node];
    Histogram h;
    uint64_t len = 0;
    if (mgc_value_hist_len(hh, &len) != MGC_OK) die("ERROR: %s", mgc_db_stream_error(nullptr));
    h.values.resize(len); h.occurrences.resize(len);
    if (mgc_value_hist_get(hh, h.values.data(), h.occurrences.data()) != MGC_OK || mgc_value_hist_totals(hh, &h.unique, &h.distinct, &h.total) != MGC_OK)
      die("ERROR: %s", mgc_db_stream_error(nullptr));
    if (rp.stats) write_statistics(rp.f, pc.k, h); else write_histogram(rp.f, h);
    close_report(rp.f, rp.name);
  }
  for (mgc_value_hist *hh : hists) mgc_value_hist_close(hh);
  return 0;
}

// temporary databases (counts inside a tree that name no output): one directory each under $TMPDIR, removed at exit
std::vector<std::string> g_temp_dirs;
void remove_temp_dirs() {
  for (const std::string &d : g_temp_dirs) { std::error_code ec; std::filesystem::remove_all(d, ec); }
}
std::string temp_database() {
  const char *base = getenv("TMPDIR");
  std::string tmpl = std::string(base && base[0] ? base : "/tmp") + "/meryl-count-XXXXXX";
  if (!mkdtemp(&tmpl[0])) die("ERROR: cannot create a temporary directory '%s' for a count without 'output'.", tmpl.c_str());
  if (g_temp_dirs.empty()) atexit(remove_temp_dirs);
  g_temp_dirs.push_back(tmpl);
  return tmpl + "/count.meryl";
}

}  // namespace

int main(int argc, char **argv) {
  Globals g;
  std::vector<Operation> ops;
  std::vector<int> stack;            // merylCommandBuilder's _opStack: words attach to the operation on top
  bool expect_output_name = false;

  if (argc < 2) { usage(argv[0]); return 1; }

  auto top = [&]() -> int { return stack.empty() ? -1 : stack.back(); };
  auto is_counting = [&](int i) { return i >= 0 && ops[i].kind >= OP_COUNT && ops[i].kind <= OP_COUNT_REVERSE; };
  auto ensure_top = [&]() {                                                   // initialize(), :163-174: an empty root operation
    if (stack.empty()) { ops.emplace_back(); stack.push_back((int)ops.size() - 1); }
  };

  for (int a = 1; a < argc; a++) {
    std::string w = argv[a];
    // one leading '[' is ignored, trailing ']'s pop operations off the stack once the word is processed
    // (merylCommandBuilder.C:86-93,129-157)
    if (!w.empty() && w[0] == '[') w.erase(0, 1);
    int closing = 0;
    while (!w.empty() && w.back() == ']') { w.pop_back(); closing++; }

    if (!w.empty()) {
      const size_t eq = w.find('=');
      const std::string key = (eq == std::string::npos) ? w : w.substr(0, eq);
      const std::string val = (eq == std::string::npos) ? "" : w.substr(eq + 1);
      const int merge_code = (w == "union-sum") ? MGC_MERGE_UNION_SUM : (w == "union-min") ? MGC_MERGE_UNION_MIN :
                             (w == "union-max") ? MGC_MERGE_UNION_MAX : (w == "intersect-sum") ? MGC_MERGE_INTERSECT_SUM :
                             (w == "intersect-min") ? MGC_MERGE_INTERSECT_MIN : (w == "intersect-max") ? MGC_MERGE_INTERSECT_MAX :
                             (w == "union") ? MGC_MERGE_UNION : (w == "intersect") ? MGC_MERGE_INTERSECT :
                             (w == "subtract") ? MGC_MERGE_SUBTRACT : (w == "difference") ? MGC_MERGE_DIFFERENCE :
                             (w == "symmetric-difference") ? MGC_MERGE_SYMMETRIC_DIFFERENCE : -1;                 // merylCommandBuilder.C:364-378
      const int value_code = (w == "less-than") ? MGC_VALUE_LESS_THAN : (w == "greater-than") ? MGC_VALUE_GREATER_THAN :
                             (w == "at-least") ? MGC_VALUE_AT_LEAST : (w == "at-most") ? MGC_VALUE_AT_MOST :
                             (w == "equal-to") ? MGC_VALUE_EQUAL_TO : (w == "not-equal-to") ? MGC_VALUE_NOT_EQUAL_TO :
                             (w == "increase") ? MGC_VALUE_INCREASE : (w == "decrease") ? MGC_VALUE_DECREASE :
                             (w == "multiply") ? MGC_VALUE_MULTIPLY : (w == "divide") ? MGC_VALUE_DIVIDE :
                             (w == "divide-round") ? MGC_VALUE_DIVIDE_ROUND : (w == "modulo") ? MGC_VALUE_MODULO : -1;   // :350-362
      const bool is_number = !w.empty() && w.find_first_not_of("0123456789") == std::string::npos;

      if (expect_output_name) {                                             // `output <db>`, :440-461
        if (top() < 0 || ops[top()].kind == OP_NONE) die("ERROR: 'output' without an operation.");
        if (!ops[top()].output.empty()) die("ERROR: operation already has an output ('%s').", ops[top()].output.c_str());   // merylOp.C:256-257
        ops[top()].output = w;
        expect_output_name = false;
      }
      // meryl2's per-operation reports: output:histogram[=file], output:statistics[=file] (processText.C:153-154; any prefix of the
      // report's word that is not ambiguous, as the reference's {p} patterns take it)
      else if (w.compare(0, 7, "output:") == 0) {
        const size_t e2 = w.find('=');
        const std::string what = w.substr(7, e2 == std::string::npos ? std::string::npos : e2 - 7);
        const std::string file = (e2 == std::string::npos || e2 + 1 >= w.size()) ? "-" : w.substr(e2 + 1);
        const bool histo = !what.empty() && std::string("histogram").compare(0, what.size(), what) == 0;
        const bool stats = what.size() >= 2 && (std::string("statistics").compare(0, what.size(), what) == 0 || std::string("stats").compare(0, what.size(), what) == 0);
        if (what == "s") die("ERROR: '%s' is ambiguous; use output:show or output:stats.", w.c_str());              // :355
        if (!histo && !stats) die("ERROR: '%s': of the output: words only output:histogram[=file] and output:statistics[=file] are part of this build.", w.c_str());
        if (top() < 0 || !is_tree_op(ops[top()])) die("ERROR: '%s' needs a set or value operation before it.", w.c_str());
        Operation &o = ops[top()];
        if (histo ? o.has_hist_out : o.has_stats_out)                       // merylOpTemplate.C:180-185,200-205
          die("ERROR: %s", ("operation '" + o.word + "' already has '" + (histo ? "histogram" : "statistics") + "' output to file '" +
                            (histo ? o.hist_out : o.stats_out) + "', can't add another output to file '" + file + "'.").c_str());
        (histo ? o.has_hist_out : o.has_stats_out) = true;
        (histo ? o.hist_out : o.stats_out) = file;
      }
      // meryl2 selectors: value: label: bases: input: and the connectives, after a set or value operation (isSelect.C)
      else if (w.compare(0, 6, "value:") == 0 || w.compare(0, 6, "label:") == 0 || w.compare(0, 6, "bases:") == 0 || w.compare(0, 6, "input:") == 0) {
        if (top() < 0 || !is_tree_op(ops[top()])) die("ERROR: selector '%s' needs a set or value operation before it.", w.c_str());
        if (!ops[top()].inputs.empty()) die("ERROR: selector '%s' must come before the inputs of its operation.", w.c_str());
        ops[top()].select_words.push_back(w);
      }
      else if ((w == "not" || w == "and" || w == "or") && top() >= 0 && is_tree_op(ops[top()]) && ops[top()].inputs.empty()) {
        ops[top()].select_words.push_back(w);
      }
      // a bare number is the threshold / constant of the value operation on top ("greater-than 45", "divide 2"; :216-233)
      // (the reference takes an all-digits word as the number whenever the operation wants one, before it is ever looked at
      // as a file name -- a database directory called "5" cannot be an input of `less-than`)
      else if (is_number && top() >= 0 && ops[top()].kind == OP_VALUE && ops[top()].constant == ~0ull) {
        ops[top()].constant = strtoull(w.c_str(), nullptr, 10);
      }
      // threshold= / t= set the THRESHOLD only (setThreshold, :291-294): the arithmetic operations' constant is not touched
      else if ((key == "threshold" || key == "t") && eq != std::string::npos && top() >= 0 && ops[top()].kind == OP_VALUE) {
        if (ops[top()].value_op <= MGC_VALUE_NOT_EQUAL_TO) ops[top()].constant = strtoull(val.c_str(), nullptr, 10);
      }
      else if ((key == "distinct" || key == "d") && eq != std::string::npos && top() >= 0 && ops[top()].kind == OP_VALUE && ops[top()].value_op <= MGC_VALUE_NOT_EQUAL_TO) {
        ops[top()].frac_distinct = strtod(val.c_str(), nullptr);                                                    // :278-282
      }
      else if ((key == "word-frequency" || key == "f") && eq != std::string::npos && top() >= 0 && ops[top()].kind == OP_VALUE && ops[top()].value_op <= MGC_VALUE_NOT_EQUAL_TO) {
        ops[top()].word_freq = strtod(val.c_str(), nullptr);                                                        // :284-288
      }
      // ---- options, merylCommandBuilder.C:187-326 ----
      else if (w.compare(0, 2, "-V") == 0)   { g.verbosity += (int)w.size() - 1; }
      else if (w == "-Q")                    { g.verbosity = 0; }
      else if (w == "-P")                    { /* progress: accepted, unused by count (:206-209) */ }
      else if (w == "-C")                    { g.only_config = true; }
      else if (w == "-l") {                                                  // meryl2 global: label width in bits
        if (a + 1 >= argc) die("ERROR: -l needs the label size in bits.");
        g.label_size = (uint32_t)strtoul(argv[++a], nullptr, 10);
        if (g.label_size > 64) die("ERROR: label size of more than 64 bits.");
        g.label_size_given = true;
      }
      else if (key == "value" && eq != std::string::npos) {                  // value=<word>[#<const>]: how the operation computes the value
        if (is_counting(top())) die("ERROR: '%s': a counting operation takes no value assignment.", w.c_str());
        if (top() < 0 || !is_tree_op(ops[top()])) die("ERROR: '%s' needs a set or value-filter operation before it.", w.c_str());
        if (ops[top()].kind == OP_VALUE && ops[top()].value_op > MGC_VALUE_NOT_EQUAL_TO)
          die("ERROR: %s", ("operation '" + ops[top()].word + "' takes no '" + w + "': the operation is a value assignment itself.").c_str());
        if (mgc_value_assign_parse(val.c_str(), &ops[top()].value_assign, &ops[top()].value_constant) != MGC_OK)
          die("ERROR: %s", mgc_last_error(nullptr));
        ops[top()].has_value_assign = true;
      }
      else if (key == "label" && eq != std::string::npos && top() >= 0 && is_tree_op(ops[top()])) {
        parse_label_assign(w, val, ops[top()]);                              // how the operation combines its inputs' labels
      }
      else if (key == "label" && eq != std::string::npos) {                  // label=#<n>: the count's constant label
        if (!is_counting(top())) die("ERROR: option '%s' needs a counting operation before it.", w.c_str());
        if (val.empty() || val[0] != '#') die("ERROR: a count takes a constant label, label=#<integer>, not '%s'.", w.c_str());
        ops[top()].label = strtoull(val.c_str() + 1, nullptr, 0);
      }
      else if (key == "k" && eq != std::string::npos) {
        const uint32_t k = (uint32_t)strtoul(val.c_str(), nullptr, 10);
        if (k == 0 || k > 64) die("ERROR: k=%s is not a valid k-mer size (1..64).", val.c_str());
        if (g.k != 0 && g.k != k) die("ERROR: kmer size already set; cannot change it to '%s'.", val.c_str());   // :254-262
        g.k = k;
      }
      else if (key == "n" && eq != std::string::npos) {                     // :265-268: the operation on top
        ensure_top();
        ops[top()].exp_num_kmers = strtoull(val.c_str(), nullptr, 10);
      }
      else if (key == "memory" && eq != std::string::npos)  { g.memory_gb = strtod(val.c_str(), nullptr); }       // :299-302
      else if (key == "gpus" && eq != std::string::npos) {                                  // this build only (no reference counterpart)
        g.gpus = (uint32_t)strtoul(val.c_str(), nullptr, 10);
        if (g.gpus < 1 || g.gpus > 64) die("ERROR: %s", "gpus= takes 1..64.");
      }
      else if (key == "threads" && eq != std::string::npos) { g.threads = (uint32_t)strtoul(val.c_str(), nullptr, 10); if (!g.threads) g.threads = 1; }   // :306-310
      else if (w == "compress")              { g.compress = true; }                                               // :237-240
      else if (key == "count-suffix") {                                                                            // :271-272
        if (!is_counting(top())) die("ERROR: option '%s' needs a counting operation before it.", w.c_str());
        ops[top()].count_suffix = val;
      }
      else if (key == "segment") { die("ERROR: option '%s' (Canu sequence stores) is not supported in this build.", w.c_str()); }
      else if (top() >= 0 && ops[top()].kind == OP_DUMPFILE && ops[top()].inputs.empty()) {
        InputRef in; in.path = w;
        ops[top()].inputs.push_back(in);                                     // <database>/0x######
      }
      // ---- operations, :346-439 ----
      else if (w == "count" || w == "count-forward" || w == "count-reverse" || w == "print" || w == "dumpIndex" || w == "histogram" || w == "statistics" ||
               w == "dumpFile" || merge_code >= 0 || value_code >= 0) {
        const OpKind kind = (w == "count") ? OP_COUNT : (w == "count-forward") ? OP_COUNT_FORWARD :
                            (w == "count-reverse") ? OP_COUNT_REVERSE : (w == "print") ? OP_PRINT :
                            (w == "histogram") ? OP_HISTOGRAM : (w == "statistics") ? OP_STATISTICS : (w == "dumpFile") ? OP_DUMPFILE :
                            (w == "dumpIndex") ? OP_DUMPINDEX : (merge_code >= 0) ? OP_MERGE : OP_VALUE;
        ensure_top();
        if (is_counting(top())) { stack.pop_back(); ensure_top(); }         // :391-407: a counting operation takes no operation as input
        if (ops[top()].kind != OP_NONE) {                                    // :412-421: a new operation, input of the one on top
          const int parent = top();
          ops.emplace_back();
          const int me = (int)ops.size() - 1;
          if (ops[parent].kind == OP_DUMPINDEX || ops[parent].kind == OP_DUMPFILE)
            die("ERROR: operation '%s' cannot be the input of a debug operation.", w.c_str());
          InputRef in; in.child = me;
          ops[parent].inputs.push_back(in);
          ops[me].parent = parent;
          stack.push_back(me);
        }
        ops[top()].kind = kind;                                              // :422-431 (or it replaces the empty operation on top)
        ops[top()].word = w;
        ops[top()].merge_op = merge_code;
        ops[top()].value_op = value_code;
      }
      else if (w == "output")                { expect_output_name = true; }
      else if (w == "printACGT" || w == "compare" || w == "noise" || w == "ploidy") {
        die("ERROR: operation '%s' is not part of this build (count, the set operations, the value filters / arithmetic, histogram and statistics only).", w.c_str());
      }
      // ---- inputs ----
      else if (dir_has_index(w)) {                                           // :159,506-514
        const int t = top();
        if (t < 0 || (ops[t].kind != OP_PRINT && ops[t].kind != OP_DUMPINDEX && ops[t].kind != OP_HISTOGRAM && ops[t].kind != OP_STATISTICS && ops[t].kind != OP_MERGE && ops[t].kind != OP_VALUE))
          die("ERROR: database input '%s' needs a print, histogram, statistics, dumpIndex, set or value operation before it.", w.c_str());
        InputRef in; in.path = w;
        ops[t].inputs.push_back(in);
      }
      else if (file_exists(w) || w == "-") {                                 // :537-549: only counting ops take sequence
        if (!is_counting(top())) die("ERROR: sequence file '%s' supplied to a non-counting operation.", w.c_str());
        ops[top()].seq_inputs.push_back(w);
        ops[top()].seq_compress.push_back(g.compress);
      }
      else {                                                                  // meryl.C:84-86
        fprintf(stderr, "\nCan't interpret '%s': not a meryl command, option, or recognized input file.\n\n", argv[a]);
        usage(argv[0]);
        return 1;
      }
    }
    for (; closing > 0 && !stack.empty(); closing--) stack.pop_back();       // terminateOperation(), :86-93
  }
  if (expect_output_name) die("ERROR: 'output' needs a database name.");
  // print writes text by the gigabyte: a pipe or a file takes it in 1 MiB writes instead of stdio's 4 KiB ones (nothing has been written to
  // stdout yet); a terminal stays line buffered, and the other verbs keep stdio's buffer
  if (!isatty(STDOUT_FILENO) && std::any_of(ops.begin(), ops.end(), [](const Operation &op) { return op.kind == OP_PRINT; }))
    setvbuf(stdout, nullptr, _IOFBF, 1 << 20);

  if (g.verbosity > 0) {
    size_t n_trees = 0;
    for (const Operation &op : ops) if (op.kind != OP_NONE && op.parent < 0) n_trees++;
    fprintf(stderr, "\nFound %zu command tree%s.\n", n_trees, (n_trees == 1) ? "" : "s");              // meryl.C:181
  }

  int rc = 0;
  {
    size_t n_ops = 0, n_counts = 0;
    for (const Operation &op : ops) if (op.kind != OP_NONE) { n_ops++; if (op.kind >= OP_COUNT && op.kind <= OP_COUNT_REVERSE) n_counts++; }
    const char *fe = getenv("MERYL_FAST_EXIT");
    g.fast_exit = n_ops == 1 && n_counts == 1 && !g.only_config && g.gpus <= 1 && !(fe && fe[0] == '0');
  }
  // a count that is the input of a set or value operation may omit `output` (`union-sum label=or [count label=#1 a.fa]
  // [count label=#2 b.fa]`): its database is a temporary one, removed when the command ends
  if (!g.only_config)
    for (Operation &op : ops)
      if (op.kind >= OP_COUNT && op.kind <= OP_COUNT_REVERSE && op.output.empty() && op.parent >= 0 && is_tree_op(ops[op.parent]) &&
          !op.seq_inputs.empty() && g.k != 0)
        op.output = temp_database();
  for (const Operation &op : ops) {                                           // counting ops first, in list order (meryl.C:211-227)
    if (op.kind >= OP_COUNT && op.kind <= OP_COUNT_REVERSE) {
      if (op.seq_inputs.empty() && !g.only_config) die("ERROR: count operation has no sequence inputs.");
      rc |= run_count(g, op);
    }
  }
  if (g.only_config) {                                                        // -C: configure, report, stop (merylOp-countThreads.C:392-393)
    if (g.verbosity > 0) fprintf(stderr, "\nCleaning up.\n\nBye.\n");
    return rc;
  }
  auto is_report = [](const Operation &op) { return op.kind == OP_HISTOGRAM || op.kind == OP_STATISTICS; };
  for (const Operation &op : ops) {                                            // before anything runs
    if (is_report(op) && op.inputs.empty()) {
      fprintf(stderr, "ERROR: '%s' needs one input: a database, or an [operation] whose result it reports.\n\n", op.word.c_str());
      usage(argv[0]);
      return 1;
    }
    if (is_report(op) && op.inputs.size() > 1) die("ERROR: told to dump a histogram for more than one input!");   // merylOp-histogram.C:24-25
    if (op.kind == OP_DUMPINDEX || is_report(op) || op.kind == OP_DUMPFILE)
      for (const InputRef &in : op.inputs)                                     // (a report evaluates the tree that is its input itself)
        if (in.child >= 0 && ops[in.child].output.empty() && !(is_report(op) && is_tree_op(ops[in.child]))) die("ERROR: '%s' reads a database: its input operation needs an 'output <database>'.", op.word.c_str());
  }
  // the trees of set and value operations, one evaluation each; the tree under a `print`, `histogram` or `statistics` is evaluated by
  // that verb
  for (size_t i = ops.size(); i-- > 0;) {
    if (!is_tree_op(ops[i]) || (ops[i].parent >= 0 && (is_tree_op(ops[ops[i].parent]) || ops[ops[i].parent].kind == OP_PRINT || is_report(ops[ops[i].parent])))) continue;
    rc |= run_tree(g, ops, (int)i, false);
  }
  for (Operation &op : ops) {
    if (op.kind != OP_PRINT && op.kind != OP_DUMPINDEX && !is_report(op) && op.kind != OP_DUMPFILE) continue;
    if (op.kind == OP_PRINT) {
      for (const InputRef &in : op.inputs)
        if (in.child >= 0 && is_tree_op(ops[in.child])) rc |= run_tree(g, ops, in.child, true);
        else print_database(in.child >= 0 ? ops[in.child].output : in.path);
      continue;
    }
    if (is_report(op)) {
      for (const InputRef &in : op.inputs)
        if (in.child >= 0 && is_tree_op(ops[in.child])) rc |= run_tree(g, ops, in.child, false, op.kind);
        else rc |= run_stored_report(op.kind, in.child >= 0 ? ops[in.child].output : in.path);
      continue;
    }
    for (const InputRef &in : op.inputs) op.db_inputs.push_back(in.child >= 0 ? ops[in.child].output : in.path);
    if (op.kind == OP_DUMPINDEX) rc |= run_dump_index(op);
    if (op.kind == OP_DUMPFILE)  rc |= run_dump_file(op);
  }
  if (g.verbosity > 0) fprintf(stderr, "\nCleaning up.\n\nBye.\n");                                    // meryl.C:268,273
  if (g.fast_exit) { fflush(nullptr); _exit(rc); }                            // (every output file is closed; see run_count)
  return rc;
}
