// The base decoders of meryl_amd/csrc/mgc_bases.hpp (host forms: the byte select in plain C++) against the expressions they
// replaced, written out here: four zero-byte tests per word, one per letter.  Every byte value in every byte position of a word
// (beside every one of a set of neighbour bytes) and of a 16-byte group, then `argv[1]` random words and groups.
// Prints "ok <words compared> <groups compared>"; the first difference goes to stderr with exit status 1.
#include "../../meryl_amd/csrc/mgc_bases.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace old {
static uint32_t enc4(uint32_t w) { return (((w >> 1) & 0x03030303u) * 0x40100401u) >> 24; }
static uint32_t zero_bytes(uint32_t x) { return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu); }
static uint32_t inv4(uint32_t w) {
  const uint32_t u = w & 0xDFDFDFDFu;
  const uint32_t ok = zero_bytes(u ^ 0x41414141u) | zero_bytes(u ^ 0x43434343u) | zero_bytes(u ^ 0x47474747u) | zero_bytes(u ^ 0x54545454u);
  const uint32_t g = ((~ok) & 0x80808080u) >> 7;
  return ((g * 0x08040201u) >> 24) & 0xFu;
}
static void encode16(const uint32_t v[4], uint32_t &codes, uint32_t &inval) {
  codes = (enc4(v[0]) << 24) | (enc4(v[1]) << 16) | (enc4(v[2]) << 8) | enc4(v[3]);
  inval = (inv4(v[0]) << 12) | (inv4(v[1]) << 8) | (inv4(v[2]) << 4) | inv4(v[3]);
}
}  // namespace old

// what the definition says, byte by byte
static bool is_base(unsigned c) { return c == 'A' || c == 'C' || c == 'G' || c == 'T' || c == 'a' || c == 'c' || c == 'g' || c == 't'; }
static uint32_t plain_inv4(uint32_t w) {
  uint32_t m = 0;
  for (int i = 0; i < 4; i++) if (!is_base((w >> (8 * i)) & 0xFFu)) m |= 8u >> i;
  return m;
}

static unsigned long long n_words = 0, n_groups = 0;

static void check_word(uint32_t w) {
  const uint32_t ei = old::inv4(w), gi = mgc::inv4(w), ee = old::enc4(w), ge = mgc::enc4(w);
  if (ei != gi || ee != ge || gi != plain_inv4(w)) {
    fprintf(stderr, "word %08x: inv4 %x (old %x, plain %x) enc4 %02x (old %02x)\n", w, gi, ei, plain_inv4(w), ge, ee);
    exit(1);
  }
  n_words++;
}

static void check_group(const uint32_t v[4]) {
  uint32_t ec, ei, gc, gi;
  old::encode16(v, ec, ei);
  mgc::encode16(v[0], v[1], v[2], v[3], gc, gi);
  if (ec != gc || ei != gi) {
    fprintf(stderr, "group %08x %08x %08x %08x: codes %08x (old %08x) inval %04x (old %04x)\n", v[0], v[1], v[2], v[3], gc, ec, gi, ei);
    exit(1);
  }
  n_groups++;
}

int main(int argc, char **argv) {
  const unsigned long long n_random = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1000000ull;
  // neighbours: the eight bases, separators, the letters next to a base in the alphabet and with one bit flipped, the ends of the range
  static const unsigned char fill[] = {'A', 'C', 'G', 'T', 'a', 'c', 'g', 't', 'N', 'n', '.', '\n', 0x00, 0xFF, 0x7F, 0x80, 'B', 'U', 'E', '@', 0x01, 0x21,
                                       0xC1, 0xE7, 'D', 'F', 'S', 0x5F};
  const int nf = (int)sizeof(fill);
  for (int p = 0; p < 4; p++)
    for (unsigned v = 0; v < 256; v++)
      for (int f = 0; f < nf; f++)
        for (int f2 = 0; f2 < nf; f2++) {
          unsigned char b[4] = {fill[f], fill[f2], fill[(f + f2) % nf], fill[(f * 7 + f2 * 3 + 1) % nf]};
          b[p] = (unsigned char)v;
          uint32_t w;
          memcpy(&w, b, 4);
          check_word(w);
        }
  // every pair of byte values in two neighbouring positions (carries between the bytes of the word-wide arithmetic)
  for (int p = 0; p < 3; p++)
    for (unsigned v = 0; v < 256; v++)
      for (unsigned v2 = 0; v2 < 256; v2++) {
        unsigned char b[4] = {'A', 'c', 'N', 'T'};
        b[p] = (unsigned char)v; b[p + 1] = (unsigned char)v2;
        uint32_t w;
        memcpy(&w, b, 4);
        check_word(w);
      }
  for (int p = 0; p < 16; p++)
    for (unsigned v = 0; v < 256; v++)
      for (int f = 0; f < nf; f++) {
        unsigned char b[16];
        for (int i = 0; i < 16; i++) b[i] = fill[(f + i * (f + 1)) % nf];
        b[p] = (unsigned char)v;
        uint32_t g[4];
        memcpy(g, b, 16);
        check_group(g);
      }
  uint64_t x = 0x9E3779B97F4A7C15ull;                                   // xorshift64*
  auto next = [&]() { x ^= x >> 12; x ^= x << 25; x ^= x >> 27; return (uint32_t)((x * 0x2545F4914F6CDD1Dull) >> 32); };
  for (unsigned long long i = 0; i < n_random; i++) {
    uint32_t g[4] = {next(), next(), next(), next()};
    if (i & 1) for (int j = 0; j < 4; j++) g[j] &= 0x7F7F7F7Fu;         // half of them ASCII: more bases, more near misses
    if ((i & 3) == 3) {                                                 // a quarter mostly bases
      unsigned char b[16];
      memcpy(b, g, 16);
      for (int j = 0; j < 16; j++) if (b[j] & 0x0C) b[j] = fill[b[j] & 7];
      memcpy(g, b, 16);
    }
    for (int j = 0; j < 4; j++) check_word(g[j]);
    check_group(g);
  }
  printf("ok %llu %llu\n", n_words, n_groups);
  return 0;
}
