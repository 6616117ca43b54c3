// The host merge of the histograms' list tier (meryl_amd/csrc/mgc_hist_list.hpp, built with MGC_HIST_LIST_HOST_ONLY: no HIP) against
// a std::map: passes of sorted distinct (key, count) merged one after the other into one vector, which must stay strictly ascending
// with every count summed.  Stand-alone; run under the address and undefined-behaviour sanitizers by tests/test_hist_list_host.py.
#include "../../meryl_amd/csrc/mgc_hist_list.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>

static uint64_t g_checks = 0;
#define CHECK(c) do { g_checks++; if (!(c)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

static const uint64_t KEY_U32_MAX = 0xFFFFFFFFull;
static const uint64_t KEY_PACKED40 = (1ull << 39) | (100ull << 32) | 0xFFFFFFFFull;      // histogram 1, score 100, value 2^32 - 1 as meryl-analyze packs them

struct Pass { std::vector<uint64_t> keys; std::vector<uint32_t> counts; };

static Pass make_pass(std::vector<uint64_t> keys, bool large_counts) {
  std::sort(keys.begin(), keys.end());
  keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
  Pass p;
  p.keys = keys;
  for (size_t i = 0; i < keys.size(); i++) p.counts.push_back(large_counts ? 0xFFFFFFFFu - (uint32_t)(rnd() % 3) : 1u + (uint32_t)(rnd() % 1000));
  return p;
}

static void merge_and_check(std::vector<mgc::HistPair> &acc, std::map<uint64_t, uint64_t> &ref, const Pass &p) {
  for (size_t i = 0; i < p.keys.size(); i++) ref[p.keys[i]] += p.counts[i];
  // (data() of an empty vector may be null: an empty pass passes exactly that)
  mgc::hist_merge(acc, p.keys.data(), p.counts.data(), p.keys.size());
  CHECK(acc.size() == ref.size());
  size_t i = 0;
  for (const auto &kv : ref) {
    CHECK(acc[i].key == kv.first && acc[i].n == kv.second);
    CHECK(i == 0 || acc[i - 1].key < acc[i].key);
    i++;
  }
}

int main() {
  uint64_t n_cases = 0, over_u32 = 0;
  for (int scenario = 0; scenario < 400; scenario++) {
    std::vector<mgc::HistPair> acc;
    std::map<uint64_t, uint64_t> ref;
    const uint64_t universe = scenario % 4 == 0 ? 16 : (scenario % 4 == 1 ? 300 : (scenario % 4 == 2 ? (1ull << 32) : (1ull << 40)));
    const int n_merges = 4 + (int)(rnd() % 8);
    for (int m = 0; m < n_merges; m++) {
      std::vector<uint64_t> keys;
      const int kind = (scenario == 0 && m < 2) ? 0 : (int)(rnd() % 7);
      const size_t len = rnd() % 40;
      switch (kind) {
        case 0: break;                                                                     // an empty pass (into an empty vector first)
        case 1: for (size_t i = 0; i < len; i++) keys.push_back(rnd() % universe); break;  // interleaved with what is there
        case 2: for (const mgc::HistPair &h : acc) keys.push_back(h.key); break;           // the identical key set
        case 3: {                                                                          // disjoint: all above, or all below
          const uint64_t top = acc.empty() ? 0 : acc.back().key, bottom = acc.empty() ? 1000 : acc.front().key;
          if (rnd() & 1) { for (size_t i = 0; i < len; i++) if (top + 1 + i > top) keys.push_back(top + 1 + i); }
          else { for (size_t i = 0; i < len && i < bottom; i++) keys.push_back(bottom - 1 - i); }
          break;
        }
        case 4: keys = {0, KEY_U32_MAX, KEY_PACKED40}; break;
        case 5: for (size_t i = 0; i < len; i++) keys.push_back(rnd() % universe); keys.push_back(0); keys.push_back(KEY_PACKED40); break;
        default: for (size_t i = 0; i < acc.size(); i += 2) keys.push_back(acc[i].key); keys.push_back(KEY_U32_MAX); break;   // every other key
      }
      merge_and_check(acc, ref, make_pass(keys, (scenario & 1) != 0));
      n_cases++;
    }
    for (const mgc::HistPair &h : acc) if (h.n > 0xFFFFFFFFull) over_u32++;
  }
  {
    // the same pass twice into an empty vector: every count doubles past 2^32
    std::vector<mgc::HistPair> acc;
    std::map<uint64_t, uint64_t> ref;
    const Pass p = make_pass({0, 5, KEY_U32_MAX, KEY_PACKED40}, true);
    merge_and_check(acc, ref, p);
    merge_and_check(acc, ref, p);
    for (const mgc::HistPair &h : acc) CHECK(h.n > 0xFFFFFFFFull);
    merge_and_check(acc, ref, Pass());
    n_cases += 3;
  }
  CHECK(over_u32 > 0);
  CHECK(n_cases > 2000);
  printf("ok %llu %llu\n", (unsigned long long)n_cases, (unsigned long long)g_checks);
  return 0;
}
