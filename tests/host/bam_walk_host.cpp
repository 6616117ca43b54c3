// bam_walk_host.cpp -- the resumable BAM record walker (mgc_bam_walk.hpp) on its own.  tests/test_bam_walk_host.py builds this
// plain and with -fsanitize=address,undefined, and runs
//   bam_walk_host PIECE FILE [FILE ...]
// Every FILE holds an inflated BAM byte stream.  ONE walker object takes them in turn (reset() between them): each stream is fed
// in pieces of PIECE bytes (0: the whole stream at once), every piece from a heap block of exactly its size, so that a read outside
// the piece is a sanitizer report.  The segments of every piece are checked against what the header promises and "decoded" here, on
// the CPU.  Per file, on stdout:   ok <bytes> <records>\n<the bytes>\n    or    error <the walker's message>\n
// Exit status 1, and a FAILED line, when a segment breaks a promise.
#include "../../meryl_amd/csrc/mgc_bam_walk.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static int g_failed = 0;
#define CHECK(cond) do { if (!(cond)) { g_failed++; printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); } } while (0)

static bool read_file(const char *path, std::vector<unsigned char> *out) {
  FILE *f = fopen(path, "rb");
  if (!f) return false;
  unsigned char buf[1 << 16];
  size_t got;
  while ((got = fread(buf, 1, sizeof(buf), f)) > 0) out->insert(out->end(), buf, buf + got);
  fclose(f);
  return true;
}

int main(int argc, char **argv) {
  if (argc < 3) { fprintf(stderr, "usage: bam_walk_host PIECE FILE [FILE ...]\n"); return 2; }
  const size_t piece_arg = (size_t)strtoull(argv[1], nullptr, 10);
  static const char NT16[] = "=ACMGRSVTWYHKDBN";             // SAMv1 4.2
  mgc::BamWalker w;
  std::vector<mgc::BamSegment> segs;
  for (int a = 2; a < argc; a++) {
    std::vector<unsigned char> bam;
    if (!read_file(argv[a], &bam)) { fprintf(stderr, "cannot read %s\n", argv[a]); return 2; }
    w.reset();
    std::string stream;
    bool ok = true, continuing = false;                      // continuing: the previous piece ended inside a SEQ field
    const size_t step = piece_arg ? piece_arg : (bam.size() ? bam.size() : 1);
    for (size_t at = 0; at < bam.size() && ok; at += step) {
      const size_t n = bam.size() - at < step ? bam.size() - at : step;
      unsigned char *piece = static_cast<unsigned char *>(malloc(n));
      memcpy(piece, bam.data() + at, n);
      segs.clear();
      uint64_t out_bytes = ~0ull;
      ok = w.walk(piece, n, &segs, &out_bytes);
      if (ok) {
        uint64_t expect_off = 0;
        for (size_t i = 0; i < segs.size(); i++) {
          const mgc::BamSegment &sg = segs[i];
          const uint32_t nb = sg.n_bases_and_flag & 0x7fffffffu;
          const bool dot = (sg.n_bases_and_flag & mgc::BAM_SEG_DOT) != 0;
          CHECK(sg.out_off == expect_off);
          CHECK((uint64_t)sg.src_off + (nb + 1) / 2 <= n);
          CHECK(nb + (dot ? 1 : 0) >= 1);
          if (!dot) { CHECK(nb % 2 == 0); CHECK((uint64_t)sg.src_off + nb / 2 == n); CHECK(i + 1 == segs.size()); }
          if (continuing && i == 0) CHECK(sg.src_off == 0);
          if ((uint64_t)sg.src_off + (nb + 1) / 2 <= n)
            for (uint32_t j = 0; j < nb; j++) {
              const unsigned char b = piece[sg.src_off + j / 2];
              stream.push_back(NT16[(j & 1) ? (b & 15) : (b >> 4)]);
            }
          if (dot) stream.push_back('.');
          expect_off += nb + (dot ? 1 : 0);
        }
        CHECK(out_bytes == expect_off);
        if (!segs.empty()) continuing = (segs.back().n_bases_and_flag & mgc::BAM_SEG_DOT) == 0;
      } else {
        CHECK(out_bytes == 0);
        CHECK(w.failed() && !w.error().empty());
        std::vector<mgc::BamSegment> none;                   // a refused stream stays refused
        uint64_t ob = 1;
        CHECK(!w.walk(piece, n, &none, &ob) && none.empty() && ob == 0);
      }
      free(piece);
    }
    if (ok) ok = w.finish();
    if (ok) {
      CHECK(w.stream_bytes() == bam.size());
      printf("ok %zu %llu\n", stream.size(), (unsigned long long)w.records());
      fwrite(stream.data(), 1, stream.size(), stdout);
      printf("\n");
    } else {
      printf("error %s\n", w.error().c_str());
    }
  }
  return g_failed ? 1 : 0;
}
