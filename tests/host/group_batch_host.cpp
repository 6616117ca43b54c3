// group_batch_host.cpp -- the batch planner of the grouping passes (meryl_amd/csrc/mgc_group_batch.hpp) over a grid of file-size
// vectors, launch keys, budgets and file caps, on the host (tests/test_group_batch_host.py builds it with the address and
// undefined-behaviour sanitizers).  Prints "ok <plans checked> <batches seen>".
#include "../../meryl_amd/csrc/mgc_group_batch.hpp"
#include "../../meryl_amd/csrc/mgc_group_route.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>

using namespace mgc;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s (vector %zu, budget %llu, cap %u)\n", __FILE__, __LINE__, #c, vi, (unsigned long long)budget, cap); exit(1); } } while (0)

int main() {
  const uint64_t T0 = (uint64_t)GROUP_BLOCK * GROUP_KPT_NARROW0P, T1 = (uint64_t)GROUP_BLOCK * GROUP_KPT_NARROW1, T16 = 16384;
  // keys as the count makes them: low shift | low digit's bits << 8 | high digit's bits << 16; the first pass's instantiation follows
  // from the high digit's width alone (mgc_group_route.hpp, group_pick_narrow_batch)
  const uint32_t K88 = 18u | (8u << 8) | (8u << 16), K98 = 17u | (9u << 8) | (8u << 16), K99 = 16u | (9u << 8) | (9u << 16);
  const uint64_t edge[] = {0, 1, 2, T16 - 1, T16, T16 + 1, T0 - 1, T0, T0 + 1, T1 - 1, T1 + 1, 2 * T0 - 1, 2 * T0, 2 * T0 + 1, 8 * T0 + 1, 81000, 135000000};
  const size_t ne = sizeof(edge) / sizeof(edge[0]);
  std::vector<std::vector<BatchFile>> vectors;
  vectors.push_back({});                                                  // no file at all
  for (size_t i = 0; i < ne; i++) vectors.push_back({BatchFile{edge[i], K88, true}});
  {                                                                       // every edge size beside every other, one key
    std::vector<BatchFile> v;
    for (size_t i = 0; i < ne; i++) for (size_t j = 0; j < ne; j++) { v.push_back(BatchFile{edge[i], K88, true}); v.push_back(BatchFile{edge[j], K88, true}); }
    vectors.push_back(v);
  }
  {                                                                       // three keys interleaved, empty and ineligible files between
    std::vector<BatchFile> v;
    const uint32_t keys[3] = {K88, K98, K99};
    for (size_t i = 0; i < 4 * ne; i++) v.push_back(BatchFile{edge[(i * 7) % ne], keys[i % 3], (i % 5) != 3});
    vectors.push_back(v);
  }
  {                                                                       // 64 files of a canonical count, pseudo-random sizes
    std::vector<BatchFile> v;
    uint64_t x = 88172645463325252ull;
    for (int i = 0; i < 64; i++) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; v.push_back(BatchFile{60000 + x % 50000, (x >> 20) % 4 ? K88 : K98, true}); }
    vectors.push_back(v);
  }
  const uint64_t budgets[] = {0, 1, 255, 256, 4 * T0, 4 * T0 + 256, 8 * T0, 1u << 20, 21u << 20, 8ull << 30, 35ull << 30, ~0ull >> 1};
  const uint32_t caps[] = {0, 1, 2, 3, 64};
  unsigned long long plans = 0, seen = 0;
  for (size_t vi = 0; vi < vectors.size(); vi++) {
    const std::vector<BatchFile> &files = vectors[vi];
    for (uint64_t budget : budgets) for (uint32_t cap : caps) {
      const std::vector<Batch> plan = group_plan_batches(files, budget, cap, T0);
      std::vector<int> in(files.size(), 0);
      uint64_t y_max = 0;
      for (const Batch &b : plan) {
        CHECK(!b.files.empty());
        CHECK(cap == 0 || b.files.size() <= cap);
        uint64_t y_end = 0, t_end = 0;
        GroupInst first0{}, second0{};
        for (size_t j = 0; j < b.files.size(); j++) {
          const BatchSlot &sl = b.files[j];
          CHECK(sl.file < files.size());
          const BatchFile &f = files[sl.file];
          in[sl.file]++;
          CHECK(f.eligible && f.n > 0 && f.key == b.key);
          CHECK(j == 0 || sl.file > b.files[j - 1].file);                     // files keep their order inside a batch
          // no batch mixes first-pass (or second-pass) instantiations
          GroupInst first{}, second{};
          CHECK(group_pick_narrow_batch((f.key >> 16) & 0xFF, (f.key >> 8) & 0xFF, &first, &second));
          if (j == 0) { first0 = first; second0 = second; }
          CHECK(first == first0 && second == second0 && first.batch && group_tile(first) == T0);
          // Y slices: disjoint, in order, aligned, long enough for the file's words
          CHECK(sl.y_off == y_end && sl.y_off % GROUP_BATCH_ALIGN == 0);
          CHECK(group_batch_slice_bytes(f.n) >= 4 * f.n);
          y_end = sl.y_off + group_batch_slice_bytes(f.n);
          // tile prefixes: strictly increasing, each file's tiles between its own and the next one's
          CHECK(sl.tile0 == t_end && (j == 0 || sl.tile0 > b.files[j - 1].tile0));
          t_end = sl.tile0 + (f.n + T0 - 1) / T0;
        }
        CHECK(b.y_bytes == y_end && b.tiles == t_end && b.tiles >= b.files.size());
        // inside the budget -- but for a batch of one file, which every budget takes
        CHECK(b.files.size() == 1 || b.y_bytes <= budget);
        y_max = std::max(y_max, b.y_bytes);
        seen++;
      }
      CHECK(group_batches_y_bytes(plan) == y_max);
      uint64_t largest = 0, two_smallest = ~0ull;
      for (size_t i = 0; i < files.size(); i++) {
        const bool takes = files[i].eligible && files[i].n > 0;
        CHECK(in[i] == (takes ? 1 : 0));                                    // every eligible file in exactly one batch, no other in any
        if (takes) largest = std::max(largest, group_batch_slice_bytes(files[i].n));
      }
      {                                                                     // a budget of one file: one file per batch
        std::vector<uint64_t> sl;
        for (const BatchFile &f : files) if (f.eligible && f.n) sl.push_back(group_batch_slice_bytes(f.n));
        std::sort(sl.begin(), sl.end());
        if (sl.size() >= 2) two_smallest = sl[0] + sl[1];
      }
      if (budget < two_smallest || cap == 1) for (const Batch &b : plan) CHECK(b.files.size() == 1);
      if (budget <= largest && !plan.empty()) CHECK(y_max == largest || y_max <= budget);
      plans++;
    }
  }
  printf("ok %llu %llu\n", plans, seen);
  return 0;
}
