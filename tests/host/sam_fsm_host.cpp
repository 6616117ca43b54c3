// The SAM parse as summaries that compose (meryl_amd/csrc/mgc_sam_fsm.hpp), held against a byte-at-a-time loop written here, on
// texts the test writes to files (tests/test_sam_fsm_host.py).  Usage: sam_fsm_host FILE [@centre ...] FILE [@centre ...] ...
// For every text:
//   - the whole text's summary, entered at a line start, emits and finds wrong what the loop does;
//   - cut in two at every offset within 18 bytes of a centre (and of the text's ends), composing the parts' summaries gives the
//     whole's; each part, entered in each of the twelve states, emits, finds wrong and exits as the loop does on its bytes;
//   - the same for a middle run cut in two round every centre (a run that begins inside a line has an open head, which the
//     second part goes on with), and for 300 seeded random cuts into 1 .. 5 parts composed in a random order of association;
//   - cut the way the kernels cut -- tiles of 16 KiB made of threads' 16 bytes summarised with 5-bit counters -- the composed
//     thread summaries give the whole's, and the exclusive composition of the threads' state functions gives every thread the
//     state the loop is in at its first byte.
// Prints "ok <texts> <two-part cuts> <random cuts> <entry checks>".
#include "../../meryl_amd/csrc/mgc_sam_fsm.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <set>
#include <string>
#include <vector>

using namespace mgc;
typedef SamSummary<SamSegWide> Wide;

static long g_entry_checks = 0;

[[noreturn]] static void fail(const std::string &text, const char *what, uint64_t a, uint64_t b, uint64_t c) {
  fprintf(stderr, "%s: %s (%llu, %llu, %llu)\n", text.c_str(), what, (unsigned long long)a, (unsigned long long)b, (unsigned long long)c);
  exit(1);
}

// ---- the loop: one byte at a time, the contract read off include/meryl_gpu_count.h -----------------------------------------------
struct Loop { uint64_t emitted; uint32_t wrong, state; };
static Loop loop(const uint8_t *b, uint64_t n, bool first_is_line_start, uint32_t state, std::vector<uint8_t> *states = nullptr) {
  Loop r = {0, 0, state};
  for (uint64_t i = 0; i < n; i++) {
    const uint8_t c = b[i];
    const bool ls = i == 0 ? first_is_line_start : b[i - 1] == '\n';
    if (states) (*states)[i] = ls ? 255 : (uint8_t)r.state;
    if (ls) {
      if (c == '\n') { r.state = 0; continue; }
      if (c == '@') { r.state = 11; continue; }
      if (c == '\r') r.wrong |= 2;
      r.state = c == '\t' ? 1 : 0;
      continue;
    }
    if (c == '\n') {
      if (r.state <= 8) r.wrong |= 1;
      else if (r.state <= 10) r.emitted++;
      r.state = 0;
      continue;
    }
    if (r.state == 11) continue;
    if (c == '\t') { if (r.state < 10) r.state++; continue; }
    if (r.state == 9 && c != '\r' && c != '*') r.emitted++;
  }
  return r;
}

static bool same(const Wide &a, const Wide &b) {
  return memcmp(a.seg.c, b.seg.c, sizeof(a.seg.c)) == 0 && a.tabs == b.tabs && a.rest == b.rest && a.fn == b.fn && a.flags == b.flags;
}

struct Text {
  std::string name;
  std::vector<uint8_t> b;
  bool ls_at(uint64_t p) const { return p == 0 || b[p - 1] == '\n'; }
  Wide sum(uint64_t p, uint64_t q) const { Wide s; sam_summarise(b.data() + p, q - p, ls_at(p), &s); return s; }
  // the run [p, q) entered in every state: the summary says what the loop does
  void check_entries(uint64_t p, uint64_t q, const Wide &s) const {
    for (uint32_t st = 0; st < 12; st++) {
      const Loop want = loop(b.data() + p, q - p, ls_at(p), st);
      uint32_t wrong = 0;
      const uint32_t emitted = sam_emit_for_entry(s, st, &wrong);
      if (emitted != want.emitted) fail(name, "bytes emitted for an entry state", p, q, st);
      if (wrong != want.wrong) fail(name, "what is found wrong for an entry state", p, q, st);
      if (q > p && sam_fn_apply(s.fn, st) != want.state) fail(name, "exit state for an entry state", p, q, st);
      g_entry_checks++;
    }
  }
};

static Wide compose_cuts(const Text &t, const std::vector<uint64_t> &edges, std::mt19937 *rng) {
  std::vector<Wide> parts;
  for (size_t i = 0; i + 1 < edges.size(); i++) { parts.push_back(t.sum(edges[i], edges[i + 1])); t.check_entries(edges[i], edges[i + 1], parts.back()); }
  while (parts.size() > 1) {                                 // any order of association gives the same
    const size_t i = rng ? (*rng)() % (parts.size() - 1) : 0;
    sam_compose(&parts[i], parts[i + 1]);
    parts.erase(parts.begin() + i + 1);
  }
  return parts[0];
}

int main(int argc, char **argv) {
  std::vector<Text> texts;
  std::vector<std::vector<uint64_t>> centres;
  for (int i = 1; i < argc; i++) {
    if (argv[i][0] == '@') { if (centres.empty()) return 2; centres.back().push_back(strtoull(argv[i] + 1, nullptr, 10)); continue; }
    FILE *f = fopen(argv[i], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[i]); return 2; }
    Text t;
    t.name = argv[i];
    uint8_t buf[65536];
    for (size_t got; (got = fread(buf, 1, sizeof(buf), f)) > 0;) t.b.insert(t.b.end(), buf, buf + got);
    fclose(f);
    texts.push_back(std::move(t));
    centres.emplace_back();
  }
  long two_part = 0, random_cuts = 0;
  for (size_t ti = 0; ti < texts.size(); ti++) {
    const Text &t = texts[ti];
    const uint64_t n = t.b.size();
    const Wide whole = t.sum(0, n);
    t.check_entries(0, n, whole);
    // the cut offsets: round every centre and both ends
    std::set<uint64_t> cuts;
    std::vector<uint64_t> cs = centres[ti];
    cs.push_back(0); cs.push_back(n);
    for (uint64_t c : cs)
      for (int d = -18; d <= 18; d++) { const int64_t p = (int64_t)c + d; if (p >= 1 && p < (int64_t)n) cuts.insert((uint64_t)p); }
    for (uint64_t p : cuts) {
      if (!same(compose_cuts(t, {0, p, n}, nullptr), whole)) fail(t.name, "two parts do not compose to the whole", p, 0, 0);
      two_part++;
    }
    // a middle run [c - 40, c + 40) cut at c + d: the first part may begin inside a line
    for (uint64_t c : centres[ti])
      for (int d = -18; d <= 18; d++) {
        const int64_t lo = (int64_t)c - 40, hi = (int64_t)c + 40, p = (int64_t)c + d;
        if (lo < 0 || hi > (int64_t)n) continue;
        for (int64_t from = lo; from < lo + 24 && from < p; from++) {
          Wide a = t.sum((uint64_t)from, (uint64_t)p);
          sam_compose(&a, t.sum((uint64_t)p, (uint64_t)hi));
          if (!same(a, t.sum((uint64_t)from, (uint64_t)hi))) fail(t.name, "two parts of a middle run do not compose to the run", from, p, hi);
        }
      }
    std::mt19937 rng(1234u + (uint32_t)ti);
    for (int r = 0; r < 300 && n > 0; r++) {
      const int parts = 1 + (int)(rng() % 5);
      std::set<uint64_t> e = {0, n};
      for (int k = 1; k < parts; k++) e.insert(rng() % (n + 1));
      std::vector<uint64_t> edges(e.begin(), e.end());
      const uint64_t from = edges.size() > 2 && (r & 1) ? edges[1] : 0;        // every other one: a run that begins anywhere
      if (from) edges.erase(edges.begin());
      if (!same(compose_cuts(t, edges, &rng), t.sum(from, n))) fail(t.name, "random parts do not compose to the run", r, from, parts);
      random_cuts++;
    }
    // the kernels' shape: 16-byte threads with packed counters, 1024 of them to a tile, the tiles composed
    std::vector<uint8_t> states(n);
    (void)loop(t.b.data(), n, true, 0, &states);
    Wide all;
    memset(&all, 0, sizeof(all));
    uint32_t file_fn = 0;
    for (uint64_t tile = 0; tile < n; tile += 16384) {
      Wide ts;
      memset(&ts, 0, sizeof(ts));
      uint32_t fn = 0;
      for (uint64_t p = tile; p < n && p < tile + 16384; p += 16) {
        const uint64_t q = p + 16 < n ? p + 16 : n;
        SamSummary<SamSegPacked> th;
        sam_summarise(t.b.data() + p, q - p, t.ls_at(p), &th);
        if (states[p] != 255 && sam_fn_apply(sam_fn_then(file_fn, fn), 0) != states[p]) fail(t.name, "entry state of a thread from the scan of state functions", p, states[p], fn);
        fn = sam_fn_then(fn, th.fn);
        sam_compose(&ts, th);
      }
      if (!same(ts, t.sum(tile, tile + 16384 < n ? tile + 16384 : n))) fail(t.name, "a tile's threads do not compose to the tile", tile, 0, 0);
      if (ts.fn != fn) fail(t.name, "a tile's state function is not the composition of its threads'", tile, ts.fn, fn);
      file_fn = sam_fn_then(file_fn, fn);
      sam_compose(&all, ts);
    }
    if (n && !same(all, whole)) fail(t.name, "the tiles do not compose to the whole", 0, 0, 0);
  }
  printf("ok %zu %ld %ld %ld\n", texts.size(), two_part, random_cuts, g_entry_checks);
  return 0;
}
