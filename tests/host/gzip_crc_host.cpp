// gzip_crc_host.cpp -- meryl_amd/csrc/mgc_gzip_crc.hpp stand-alone: the CRC ledger of the gzip input route with this program in the
// device's place (it computes zlib's crc32 of every table entry over a text it makes).  Single-threaded.  Prints "ok <checks>" and
// exits 0, or says which check failed and exits 1.  Built plain and with sanitizers by tests/test_gzip_crc_host.py.
//
//   gzip_crc_host combine | table | fold | empty
#include "../../meryl_amd/csrc/mgc_gzip_crc.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using mgc::GzCrcLedger;
using mgc::GzMemberEnd;

static long checks = 0;
#define CHECK(cond, ...)                                                                       \
  do {                                                                                         \
    checks++;                                                                                  \
    if (!(cond)) { printf("FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); exit(1); } \
  } while (0)

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() {                                      // xorshift64*
  rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
  return (uint32_t)((rng_state * 0x2545f4914f6cdd1dull) >> 32);
}

static uint32_t crc_of(const std::vector<uint8_t> &text, uint64_t begin, uint64_t len) {
  return (uint32_t)crc32(crc32(0L, Z_NULL, 0), text.data() + begin, (uInt)len);
}

// ---- combine ---------------------------------------------------------------------------------------------------------------
static void test_combine() {
  const uint32_t words[4] = {0u, 1u, 0x80000000u, 0xffffffffu};
  for (uint32_t a : words)
    for (uint32_t b : words)
      CHECK(mgc::crc32_combine_4096(a, b) == (uint32_t)crc32_combine(a, b, 4096), "%08x %08x", a, b);
  for (int i = 0; i < 100000; i++) {
    const uint32_t a = rnd(), b = rnd();
    CHECK(mgc::crc32_combine_4096(a, b) == (uint32_t)crc32_combine(a, b, 4096), "%08x %08x", a, b);
  }
}

// ---- table -----------------------------------------------------------------------------------------------------------------
static std::vector<GzMemberEnd> ends_at(const std::vector<uint64_t> &offs) {
  std::vector<GzMemberEnd> e;
  for (uint64_t o : offs) e.push_back({o, 0u, 0u, 1000 + o});
  return e;
}

static void test_table() {
  const uint64_t pieces[5] = {1, 4095, 4096, 4097, 12288};
  for (uint64_t piece : pieces) {
    const std::vector<std::vector<uint64_t>> sets = {{}, {0}, {piece}, {4096}, {100, 100}, {1, 1}, {100, 5000}};
    for (const std::vector<uint64_t> &set : sets) {
      std::vector<uint64_t> offs;
      for (uint64_t o : set) if (o <= piece) offs.push_back(o);         // only ends that lie within the piece
      const std::vector<GzMemberEnd> ends = ends_at(offs);
      const size_t room = GzCrcLedger::table_room(piece, ends.size());
      CHECK(room == piece / 4096 + 2 * ends.size() + 2, "room");
      std::vector<uint64_t> begin(room + 1, ~0ull);
      std::vector<uint32_t> len(room + 1, ~0u);
      GzCrcLedger g;
      const long n = g.build_table(1, piece, ends.data(), ends.size(), 77, begin.data(), len.data(), room);
      CHECK(n >= 0 && (size_t)n <= room, "piece %llu: %ld entries, room %zu", (unsigned long long)piece, n, room);
      CHECK(begin[(size_t)n] == ~0ull && len[(size_t)n] == ~0u, "wrote past its count");
      CHECK(g.pending[1].size() == (size_t)n && g.ends[1].size() == ends.size() && g.pending[0].empty() && g.piece_off[1] == 77, "remembered");
      uint64_t at = 0;
      size_t next_end = 0;
      uint64_t since_boundary = 0;                                       // text since the previous member end (or the piece's start)
      for (long i = 0; i < n; i++) {
        CHECK(begin[i] == at, "entry %ld begins at %llu, not %llu", i, (unsigned long long)begin[i], (unsigned long long)at);
        CHECK(len[i] <= 4096 && g.pending[1][i].len == len[i], "entry %ld is %u bytes", i, len[i]);
        if (next_end < offs.size()) CHECK(at + len[i] <= offs[next_end], "entry %ld crosses the end at %llu", i, (unsigned long long)offs[next_end]);
        if (len[i] == 0) CHECK(next_end < offs.size() && offs[next_end] == at && since_boundary == 0, "a 0-byte entry (%ld) that is no empty member's", i);
        at += len[i];
        since_boundary += len[i];
        // the entry that reaches a member's end closes it (the next end, and only that one)
        const bool closes = next_end < offs.size() && at == offs[next_end];
        CHECK(g.pending[1][i].end == (closes ? (int32_t)next_end : -1), "entry %ld closes end %d", i, g.pending[1][i].end);
        if (closes) { next_end++; since_boundary = 0; }
      }
      CHECK(at == piece && next_end == offs.size(), "the entries cover %llu of %llu bytes and %zu of %zu ends", (unsigned long long)at,
            (unsigned long long)piece, next_end, offs.size());
      // an end with no text since the previous boundary: exactly one entry of 0 bytes; no other 0-byte entries (none trails the last end)
      size_t zero_entries = 0, empty_ends = 0;
      for (long i = 0; i < n; i++) zero_entries += len[i] == 0;
      for (size_t e = 0; e < offs.size(); e++) empty_ends += offs[e] == (e ? offs[e - 1] : 0);
      CHECK(zero_entries == empty_ends, "%zu entries of 0 bytes for %zu ends without text", zero_entries, empty_ends);
      if (n) CHECK(len[n - 1] != 0 || g.pending[1][n - 1].end >= 0, "a 0-byte entry trails the last end");
    }
  }
  // bad arguments: nothing is remembered
  uint64_t begin[16];
  uint32_t len[16];
  GzCrcLedger g;
  const std::vector<GzMemberEnd> out_of_order = ends_at({200, 100}), beyond = ends_at({100, 5000});
  CHECK(g.build_table(0, 4096, out_of_order.data(), 2, 0, begin, len, 16) < 0, "ends out of order");
  CHECK(g.build_table(0, 4999, beyond.data(), 2, 0, begin, len, 16) < 0, "an end beyond the piece");
  CHECK(g.build_table(0, 12288, nullptr, 0, 0, begin, len, 4) < 0, "less room than the table may need");
  CHECK(g.pending[0].empty() && g.ends[0].empty(), "a refused table left something behind");
}

// ---- fold ------------------------------------------------------------------------------------------------------------------
struct Device {                                              // the two slots' tables as they come back
  std::vector<uint64_t> begin[2];
  std::vector<uint32_t> len[2], crc[2];
  long n[2] = {0, 0};
  void run(GzCrcLedger &g, int b, const std::vector<uint8_t> &text, uint64_t piece_begin, uint64_t piece, const std::vector<GzMemberEnd> &ends, uint64_t comp_off) {
    const size_t room = GzCrcLedger::table_room(piece, ends.size());
    begin[b].assign(room, 0); len[b].assign(room, 0); crc[b].assign(room, 0);
    n[b] = g.build_table(b, piece, ends.data(), ends.size(), comp_off, begin[b].data(), len[b].data(), room);
    CHECK(n[b] >= 0, "table");
    for (long i = 0; i < n[b]; i++) crc[b][i] = crc_of(text, piece_begin + begin[b][i], len[b][i]);
  }
};

// three members over two pieces: member 0 = text[0, 5000), member 1 = text[5000, 9000), member 2 = text[9000, 20000);
// piece 0 = text[0, 7000) in slot 0, piece 1 = text[7000, 20000) in slot 1.  damage: 0 none, 1 member 1's CRC, 2 member 2's ISIZE,
// 3 / 4 error word 1 / 2 on piece 1, 5 member 1's CRC and then member 2's ISIZE
static std::string fold(int damage, uint64_t *members) {
  std::vector<uint8_t> text(20000);
  for (uint8_t &c : text) c = (uint8_t)rnd();
  const uint64_t cut[4] = {0, 5000, 9000, 20000};
  uint32_t crc[3], isize[3];
  for (int m = 0; m < 3; m++) { crc[m] = crc_of(text, cut[m], cut[m + 1] - cut[m]); isize[m] = (uint32_t)(cut[m + 1] - cut[m]); }
  if (damage == 1 || damage == 5) crc[1] ^= 0x100;
  if (damage == 2 || damage == 5) isize[2] += 1;
  GzCrcLedger g;
  g.reset();
  Device d;
  d.run(g, 0, text, 0, 7000, {{5000, crc[0], isize[0], 111}}, 10);
  d.run(g, 1, text, 7000, 13000, {{2000, crc[1], isize[1], 222}, {13000, crc[2], isize[2], 333}}, 4242);
  g.collect(0, d.crc[0].data(), 0);
  CHECK(!g.refused() && g.members == 1 && g.pending[0].empty() && g.ends[0].empty(), "after piece 0");
  g.collect(1, d.crc[1].data(), damage == 3 ? 1u : damage == 4 ? 2u : 0u);
  g.collect(0, d.crc[0].data(), 7);                          // nothing pending in slot 0: nothing happens
  *members = g.members;
  CHECK(g.crc == 0 && g.member_len == 0, "a member is still running");
  return g.verdict;
}

static bool starts_with(const std::string &s, const char *p) { return s.compare(0, strlen(p), p) == 0; }

static void test_fold() {
  uint64_t members = 0;
  std::string v = fold(0, &members);
  CHECK(v.empty() && members == 3, "'%s', %llu members", v.c_str(), (unsigned long long)members);
  v = fold(1, &members);
  CHECK(starts_with(v, "CRC32 mismatch (member 1, trailer at compressed offset 222: ") && members == 3, "'%s'", v.c_str());
  v = fold(2, &members);
  CHECK(starts_with(v, "ISIZE mismatch (member 2, trailer at compressed offset 333: 11001, text 11000 bytes)"), "'%s'", v.c_str());
  v = fold(3, &members);
  CHECK(v == "the inflaters produced an invalid symbol (in the piece that starts at compressed offset 4242)", "'%s'", v.c_str());
  v = fold(4, &members);
  CHECK(v == "a back-reference reaches before the start of its gzip member (in the piece that starts at compressed offset 4242)", "'%s'", v.c_str());
  v = fold(5, &members);                                     // the first verdict stands
  CHECK(starts_with(v, "CRC32 mismatch (member 1,") && members == 3, "'%s'", v.c_str());
}

// ---- empty piece -----------------------------------------------------------------------------------------------------------
static void test_empty() {
  std::vector<uint8_t> text(6000);
  for (uint8_t &c : text) c = (uint8_t)rnd();
  for (int damage = 0; damage < 3; damage++) {               // 0 none, 1 the running member's CRC, 2 its ISIZE
    GzCrcLedger g;
    Device d;
    d.run(g, 0, text, 0, 6000, {}, 0);                       // the member's text, its end not yet seen
    g.collect(0, d.crc[0].data(), 0);
    CHECK(!g.refused() && g.members == 0 && g.member_len == 6000 && g.crc == crc_of(text, 0, 6000), "the running member");
    // ... its trailer and an empty member arrive with no text
    const GzMemberEnd ends[2] = {{0, crc_of(text, 0, 6000) ^ (damage == 1 ? 1u : 0u), 6000u + (damage == 2 ? 1u : 0u), 555}, {0, 0u, 0u, 575}};
    g.empty_piece(ends, 2);
    CHECK(g.members == 2 && g.crc == 0 && g.member_len == 0, "members");
    if (damage == 0) CHECK(!g.refused(), "'%s'", g.verdict.c_str());
    else CHECK(g.verdict == "CRC32 / ISIZE mismatch (member 0, trailer at compressed offset 555)", "'%s'", g.verdict.c_str());
  }
  GzCrcLedger g;                                             // an empty member that claims text
  const GzMemberEnd claims[2] = {{0, 0u, 0u, 18}, {0, 0u, 5u, 38}};
  g.empty_piece(claims, 2);
  CHECK(g.verdict == "CRC32 / ISIZE mismatch (member 1, trailer at compressed offset 38)" && g.members == 2, "'%s'", g.verdict.c_str());
  g.reset();
  CHECK(!g.refused() && g.members == 0, "reset");
}

int main(int argc, char **argv) {
  const std::string what = argc > 1 ? argv[1] : "";
  if (what == "combine") test_combine();
  else if (what == "table") test_table();
  else if (what == "fold") test_fold();
  else if (what == "empty") test_empty();
  else { fprintf(stderr, "usage: gzip_crc_host combine | table | fold | empty\n"); return 2; }
  printf("ok %ld\n", checks);
  return 0;
}
