// input_host.cpp -- the host-only parts of whole-file text input on their own: the chunk ring (mgc_chunk_ring.hpp) and the
// BGZF block helpers (mgc_bgzf.hpp).  tests/test_input_host.py builds this plain, with -fsanitize=thread and with
// -fsanitize=address,undefined, and runs
//   input_host ring               every ring case; a line per failed check, exit status 1 if there was one
//   input_host bgzf FILE CAP      plans FILE with a text capacity of CAP bytes and inflates it; one line of key=value pairs
#include "../../meryl_amd/csrc/mgc_bgzf.hpp"
#include "../../meryl_amd/csrc/mgc_chunk_ring.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fcntl.h>
#include <string>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

using mgc::ChunkRingResult;

static std::atomic<int> g_failed{0};
#define CHECK(cond) do { if (!(cond)) { g_failed++; printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); } } while (0)

static const size_t SLOT = 64;
static unsigned char pattern(uint64_t c, size_t j) { return (unsigned char)(c * 131 + j * 7 + 1); }

// one pump over `slots` with callbacks that can be told to fail, and what they saw
struct Run {
  int      n_slots = 4, threads = 3, lag = 2;
  uint64_t n_chunks = 37;
  size_t   last_len = SLOT;
  int64_t  fill_fails_at = -1, consume_stops_at = -1;      // chunk numbers
  int      fill_detail = 0, consume_rc = 0, alloc_null_at_call = 0;

  std::vector<uint64_t> seen;                              // chunks in the order consume got them
  std::vector<std::string> saved;                          // their bytes, copied at their consume
  std::atomic<int> allocs{0};
  std::atomic<int64_t> max_filled{-1};
  bool bytes_ok = true, older_slots_intact = true;

  size_t len_of(uint64_t c) const { return c + 1 == n_chunks ? last_len : SLOT; }

  ChunkRingResult go(char **slots) {
    auto alloc = [&]() -> char * { return ++allocs == alloc_null_at_call ? nullptr : (char *)malloc(SLOT); };
    auto fill = [&](int t, uint64_t c, char *dst, int *detail) -> int64_t {
      CHECK(t >= 0 && t < threads);
      for (int64_t m = max_filled.load(); m < (int64_t)c && !max_filled.compare_exchange_weak(m, (int64_t)c);) {}
      if ((int64_t)c == fill_fails_at) { *detail = fill_detail; return -1; }
      for (size_t j = 0; j < len_of(c); j++) dst[j] = (char)pattern(c, j);
      return (int64_t)len_of(c);
    };
    auto consume = [&](uint64_t c, const char *p, size_t len) -> int {
      CHECK(p == slots[c % n_slots]);
      if (len != len_of(c)) bytes_ok = false;
      for (size_t j = 0; j < len && j < SLOT; j++) if ((unsigned char)p[j] != pattern(c, j)) bytes_ok = false;
      seen.push_back(c);
      saved.emplace_back(p, len);
      // the slots of the `lag` chunks before this one are not released yet: they still hold what their consume saw
      for (uint64_t back = 1; back <= (uint64_t)lag && back <= c && saved.size() > back; back++) {
        const std::string &was = saved[saved.size() - 1 - back];
        if (memcmp(slots[(c - back) % n_slots], was.data(), was.size()) != 0) older_slots_intact = false;
      }
      return (int64_t)c == consume_stops_at ? consume_rc : 0;
    };
    return mgc::run_chunk_ring(n_chunks, slots, n_slots, threads, lag, alloc, fill, consume);
  }
  bool seen_is_prefix(uint64_t n) const {                  // chunks 0 .. n-1, in order, once each
    if (seen.size() != n) return false;
    for (uint64_t i = 0; i < n; i++) if (seen[i] != i) return false;
    return true;
  }
};

static void free_slots(char **slots, int n) { for (int i = 0; i < n; i++) { free(slots[i]); slots[i] = nullptr; } }

static void ring_cases() {
  {  // 1. order and wrap; 2. the slots are reused by the next run
    char *slots[4] = {nullptr, nullptr, nullptr, nullptr};
    Run a; a.last_len = 17;
    ChunkRingResult r = a.go(slots);
    CHECK(r.end == ChunkRingResult::DONE);
    CHECK(a.seen_is_prefix(37));
    CHECK(a.bytes_ok);
    CHECK(a.older_slots_intact);
    CHECK(a.allocs == 4);
    CHECK(r.t_wait >= 0 && r.t_consume >= 0 && r.t_fill >= 0 && r.t_slot_wait >= 0);
    Run b; b.last_len = 17;
    r = b.go(slots);
    CHECK(r.end == ChunkRingResult::DONE && b.seen_is_prefix(37) && b.bytes_ok && b.older_slots_intact);
    CHECK(b.allocs == 0);
    free_slots(slots, 4);
  }
  {  // 3. a producer fails mid-file
    char *slots[4] = {nullptr, nullptr, nullptr, nullptr};
    Run a; a.fill_fails_at = 17; a.fill_detail = 5;
    const ChunkRingResult r = a.go(slots);
    CHECK(r.end == ChunkRingResult::FILL_FAILED && r.chunk == 17 && r.detail == 5);
    CHECK(a.seen.size() <= 17 && a.seen_is_prefix(a.seen.size()));
    CHECK(a.bytes_ok && a.older_slots_intact);
    free_slots(slots, 4);
  }
  {  // 4. the third slot allocation fails
    char *slots[4] = {nullptr, nullptr, nullptr, nullptr};
    Run a; a.alloc_null_at_call = 3;
    const ChunkRingResult r = a.go(slots);
    CHECK(r.end == ChunkRingResult::ALLOC_FAILED);
    CHECK(slots[r.chunk % 4] == nullptr);
    CHECK(a.seen.size() <= r.chunk && a.seen_is_prefix(a.seen.size()));          // in order, so nothing at or past the chunk that got no slot
    for (uint64_t c : a.seen) CHECK(slots[c % 4] != nullptr);
    CHECK(a.bytes_ok && a.older_slots_intact);
    free_slots(slots, 4);
  }
  {  // 5. the consumer stops early
    char *slots[4] = {nullptr, nullptr, nullptr, nullptr};
    Run a; a.consume_stops_at = 5; a.consume_rc = 7;
    const ChunkRingResult r = a.go(slots);
    CHECK(r.end == ChunkRingResult::CONSUMER_STOPPED && r.chunk == 5 && r.detail == 7);
    CHECK(a.seen_is_prefix(6));
    // consume(4) released chunk 2 and consume(5) released nothing: chunk 7 needs the slot of chunk 3, so no producer got past 6
    CHECK(a.max_filled <= 6);
    free_slots(slots, 4);
  }
  {  // 6. nothing to do
    char *slots[4] = {nullptr, nullptr, nullptr, nullptr};
    Run a; a.n_chunks = 0;
    const ChunkRingResult r = a.go(slots);
    CHECK(r.end == ChunkRingResult::DONE && a.seen.empty() && a.allocs == 0);
  }
  {  // 7. more threads than chunks; the smallest ring that works with lag 2
    char *slots[24] = {nullptr};
    Run a; a.n_slots = 24; a.threads = 16; a.n_chunks = 2;
    ChunkRingResult r = a.go(slots);
    CHECK(r.end == ChunkRingResult::DONE && a.seen_is_prefix(2) && a.bytes_ok && a.allocs == 2);
    free_slots(slots, 24);
    Run b; b.n_slots = 3; b.threads = 1; b.n_chunks = 10;
    r = b.go(slots);
    CHECK(r.end == ChunkRingResult::DONE && b.seen_is_prefix(10) && b.bytes_ok && b.older_slots_intact && b.allocs == 3);
    free_slots(slots, 24);
  }
  {  // 8. threads and slots
    const int RING_MAX = 64;
    for (int asked : {0, 16}) {
      const mgc::ChunkRingGeometry g = mgc::chunk_ring_geometry(asked, 1000, RING_MAX);
      CHECK(g.threads == 16 && g.slots == 24);
    }
    CHECK(mgc::chunk_ring_geometry(5, 1000, RING_MAX).slots == 13 && mgc::chunk_ring_geometry(5, 1000, RING_MAX).threads == 5);
    CHECK(mgc::chunk_ring_geometry(1000, 1000, RING_MAX).threads == RING_MAX - 8 && mgc::chunk_ring_geometry(1000, 1000, RING_MAX).slots == RING_MAX);
    for (int asked : {0, 1, 5, 16, 1000})
      for (uint64_t chunks : {0ull, 1ull, 2ull, 7ull, 100ull}) {
        const mgc::ChunkRingGeometry g = mgc::chunk_ring_geometry(asked, chunks, RING_MAX);
        CHECK(g.threads >= 1 && (uint64_t)g.threads <= (chunks ? chunks : 1) && g.threads <= g.slots - 2 && g.slots <= RING_MAX);
      }
  }
}

static int bgzf_case(const char *path, size_t cap) {
  const int fd = open(path, O_RDONLY);
  struct stat st;
  if (fd < 0 || fstat(fd, &st) != 0 || st.st_size == 0) { printf("cannot read %s\n", path); return 2; }
  const size_t size = (size_t)st.st_size;
  const unsigned char *map = (const unsigned char *)mmap(nullptr, size, PROT_READ, MAP_SHARED, fd, 0);
  if (map == MAP_FAILED) { printf("cannot map %s\n", path); return 2; }
  const mgc::BgzfPlan plan = mgc::bgzf_plan_chunks(map, size, cap);
  if (plan.bad != mgc::BGZF_BLOCK) {
    printf("refused=%s off=%llu isize=%u\n", plan.bad == mgc::BGZF_BAD_ISIZE ? "isize" : "not_a_block", (unsigned long long)plan.bad_off, plan.bad_isize);
  } else {
    // the chunks partition the block index, in order, and none holds more text than cap
    bool partition = !plan.chunks.empty() && plan.chunks.front().first == 0 && plan.chunks.back().last == plan.blocks.size();
    size_t max_text = 0;
    for (size_t c = 0; c < plan.chunks.size(); c++) {
      const mgc::BgzfChunk &ch = plan.chunks[c];
      if (ch.first >= ch.last || (c && ch.first != plan.chunks[c - 1].last)) partition = false;
      size_t text = 0;
      for (size_t i = ch.first; i < ch.last; i++) text += plan.blocks[i].isize;
      if (text != ch.text) partition = false;
      max_text = std::max(max_text, ch.text);
    }
    z_stream z;
    memset(&z, 0, sizeof(z));
    if (inflateInit2(&z, -15) != Z_OK) { printf("zlib\n"); return 2; }
    std::vector<unsigned char> chunk(cap ? cap : 1);
    std::string bad_blocks;
    unsigned long crc = crc32(0L, nullptr, 0);
    size_t len = 0;
    for (const mgc::BgzfChunk &ch : plan.chunks) {
      size_t at = 0;
      for (size_t i = ch.first; i < ch.last; i++) {
        const mgc::BgzfBlock &b = plan.blocks[i];
        if (at + b.isize > chunk.size()) { partition = false; break; }
        if (!mgc::bgzf_inflate_block(z, map + b.off, b, chunk.data() + at)) bad_blocks += (bad_blocks.empty() ? "" : ",") + std::to_string(i);
        at += b.isize;
      }
      crc = crc32(crc, chunk.data(), (unsigned)at);
      len += at;
    }
    inflateEnd(&z);
    printf("chunks=%zu blocks=%zu max_text=%zu partition=%d len=%zu crc=%lu bad_blocks=%s\n", plan.chunks.size(), plan.blocks.size(), max_text,
           partition ? 1 : 0, len, crc, bad_blocks.empty() ? "none" : bad_blocks.c_str());
  }
  munmap((void *)map, size);
  close(fd);
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 2 && !strcmp(argv[1], "ring")) {
    ring_cases();
    printf("%s\n", g_failed ? "ring: FAILED" : "ring: ok");
    return g_failed ? 1 : 0;
  }
  if (argc == 4 && !strcmp(argv[1], "bgzf")) return bgzf_case(argv[2], (size_t)strtoull(argv[3], nullptr, 10));
  fprintf(stderr, "usage: input_host ring | input_host bgzf FILE CAP\n");
  return 2;
}
