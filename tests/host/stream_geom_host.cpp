// Host check of meryl_amd/csrc/mgc_stream_geom.hpp, the geometry hash_count_stream_kernel takes per sub-bucket (no GPU): every
// sub-bucket size 1 .. 4094 at both table sizes (2048: the first launch, 8192: the retry launch), walked with the kernel's own
// chunk loop, and every state of a wave's pending-key queue.  Prints "ok <sizes checked> <queue states checked>".
#include "../../meryl_amd/csrc/mgc_stream_geom.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace mgc;

static int fail(const char *what, unsigned n, unsigned a, unsigned b) {
  fprintf(stderr, "FAIL %s: n=%u (%u, %u)\n", what, n, a, b);
  return 1;
}

int main() {
  const uint32_t BLOCK = 256, KPC = 6, CH = BLOCK * KPC, CAP = 4094;
  const uint32_t tables[2] = {2048, 8192};
  unsigned long sizes = 0, states = 0;
  for (uint32_t table : tables) {
    for (uint32_t max_size : {CAP, 2304u, 1536u, 300u}) {
      for (uint32_t n = 1; n <= CAP; n++) {
        const uint32_t csz = stream_chunk_size(n, max_size, CH, BLOCK);
        if (n > max_size) { if (csz != 0) return fail("a size above max_size is not this kernel's", n, csz, max_size); continue; }
        if (csz == 0 || csz % BLOCK != 0 || csz > CH) return fail("chunk: whole rows, at most CH keys", n, csz, CH);
        // the kernel's loop: keys [off, off + cnt) per round, the last round is the one whose rest fits
        std::vector<unsigned char> seen(n, 0);
        uint32_t off = 0, chunks = 0;
        for (;;) {
          const uint32_t rest = n - off, cnt = rest < csz ? rest : csz;
          const bool last = rest <= csz;
          if (cnt == 0) return fail("an empty chunk", n, off, csz);
          // rows of the chunk: row j is full when (j + 1) * BLOCK <= cnt, loaded when j * BLOCK < cnt
          for (uint32_t j = 0; j < KPC; j++) {
            const bool full = (j + 1) * BLOCK <= cnt, loaded = j * BLOCK < cnt;
            for (uint32_t t = 0; t < BLOCK; t++) {
              const bool act = j * BLOCK + t < cnt;              // the lane predicate of a partial row
              if ((full && !act) || (!loaded && act)) return fail("a full row needs no lane predicate, a row not loaded has no key", n, j, cnt);
              if (act) seen[off + j * BLOCK + t]++;
            }
          }
          if (cnt > KPC * BLOCK) return fail("a chunk is KPC rows", n, cnt, KPC * BLOCK);
          chunks++;
          if (last) break;
          off += csz;
        }
        if (chunks < 1 || chunks > 3) return fail("1..3 chunks", n, chunks, csz);
        for (uint32_t i = 0; i < n; i++) if (seen[i] != 1) return fail("every key once", n, i, seen[i]);

        const uint32_t s = stream_slots_for(n, table);
        if (s < 256 || s > table || (s & (s - 1)) != 0) return fail("slots: a power of two, 256 .. table", n, s, table);
        if (s < 2 * n && s != table) return fail("slots >= 2n wherever the table allows", n, s, table);
        if (s >= 512 && s / 2 >= 2 * n) return fail("slots: the SMALLEST such power of two", n, s, table);
        if (table == 8192 && s < 2 * n) return fail("the retry table is at most half full", n, s, table);
        sizes++;
      }
      if (stream_chunk_size(0, max_size, CH, BLOCK) != 0) return fail("an empty sub-bucket has no chunk", 0, 0, 0);
    }
  }
  // the queue: a row appends `row` keys (ranks 0 .. row - 1) at fill `fill`, after a drain (fill = 0) where it has to
  for (uint32_t wave = 0; wave < BLOCK / 64; wave++)
    for (uint32_t fill = 0; fill <= STREAM_QCAP; fill++)
      for (uint32_t row = 0; row <= 64; row++) {
        const uint32_t f = stream_queue_must_drain(fill, row) ? 0u : fill;
        if (stream_queue_must_drain(f, row)) return fail("a row fits an empty queue", row, f, STREAM_QCAP);
        for (uint32_t r = 0; r < row; r++) {
          const uint32_t i = stream_queue_index(wave, f, r);
          if (i < wave * STREAM_QCAP || i >= (wave + 1) * STREAM_QCAP) return fail("queue index inside the wave's segment", i, wave, f);
        }
        if (f + row > STREAM_QCAP) return fail("fill after the append", f, row, STREAM_QCAP);
        states++;
      }
  printf("ok %lu %lu\n", sizes, states);
  return 0;
}
