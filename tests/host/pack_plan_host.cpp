// pack_plan_host.cpp -- the early-packing decision and the capacity of the result (meryl_amd/csrc/mgc_pack_plan.hpp) over their grid,
// on the host (tests/test_pack_plan_host.py builds it with the address and undefined-behaviour sanitizers).
// Prints "ok <eligibility cases> <capacity cases> <chain cases>".
#include "../../meryl_amd/csrc/mgc_pack_plan.hpp"

#include <cstdio>
#include <cstdlib>

using namespace mgc;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

int main() {
  unsigned long long n_elig = 0, n_cap = 0, n_chain = 0;
  const uint64_t CAP = 8192, SMAX = 1ull << 22;

  // ---- eligibility: every file finished by what is queued in one go, some file with k-mers, the switch on ----
  {
    const PackFile empty{0, 0, 0, true, false}, plain{1000, 700, 0, true, false}, at_cap{90000, CAP, 0, false, false},
                   above_cap{90000, CAP + 1, 0, true, false},              // (nothing listed, yet above the capacity: not a count launch's file)
                   streamed{90000, 1946, 615, true, false}, streamed_max{90000, SMAX, 1, true, false},
                   asked{90000, SMAX + 1, 1, true, false},                 // above stream_max: the host asks a probe launch first
                   unstreamed{90000, 5000, 1, false, false},               // an oversized list nothing streams: widened back or sorted
                   sorted{90000, 700, 0, true, true};
    // (an empty file's statistics are not looked at)
    CHECK(pack_file_ok(PackFile{0, SMAX + 5, 3, false, true}, CAP, SMAX));
    CHECK(pack_file_ok(plain, CAP, SMAX) && pack_file_ok(at_cap, CAP, SMAX) && pack_file_ok(streamed, CAP, SMAX) && pack_file_ok(streamed_max, CAP, SMAX));
    CHECK(!pack_file_ok(above_cap, CAP, SMAX) && !pack_file_ok(asked, CAP, SMAX) && !pack_file_ok(unstreamed, CAP, SMAX) && !pack_file_ok(sorted, CAP, SMAX));
    CHECK(!pack_file_ok(streamed, CAP, 1945) && pack_file_ok(streamed, CAP, 1946));       // (MGC_STREAM_MAX moves the line)
    const PackFile kinds[] = {empty, plain, at_cap, streamed, streamed_max, above_cap, asked, unstreamed, sorted};
    const bool ok[] = {true, true, true, true, true, false, false, false, false};
    const int NK = 9;
    // every vector of up to three files over the nine kinds, at every position, with the switch on and off
    for (int a = 0; a < NK; a++) for (int b = -1; b < NK; b++) for (int c = -1; c < NK; c++) for (int sw = 0; sw < 2; sw++) {
      std::vector<PackFile> v{kinds[a]};
      if (b >= 0) v.push_back(kinds[b]);
      if (c >= 0) v.push_back(kinds[c]);
      bool all = ok[a] && (b < 0 || ok[b]) && (c < 0 || ok[c]);
      bool any = kinds[a].size || (b >= 0 && kinds[b].size) || (c >= 0 && kinds[c].size);
      CHECK(pack_overlap_eligible(v, CAP, SMAX, sw != 0) == (all && any && sw != 0));
      n_elig++;
    }
    CHECK(!pack_overlap_eligible({}, CAP, SMAX, true));                    // no file at all
    // 64 files, ten of them with a streamed oversized list (the benchmarked workload's shape); then one nothing streams: off
    std::vector<PackFile> v(64, plain);
    for (int i = 0; i < 10; i++) v[6 * i + 1] = streamed;
    CHECK(pack_overlap_eligible(v, CAP, SMAX, true));
    v[37] = unstreamed;
    CHECK(!pack_overlap_eligible(v, CAP, SMAX, true));
    n_elig += 3;
  }

  // ---- the estimate ----
  {
    const uint64_t inst[] = {0, 1, 4095, 4096, 4097, 100000, 9000000, 9852516073ull, 1ull << 40};
    const double ratios[] = {0.0, -1.0, 1e-9, 0.05, 0.1369, 0.30, 0.99, 1.0, 7.0};
    const int64_t margins[] = {-2000, -1000, -600, -1, 0, 1, PACK_MARGIN_PERMILLE, 1000, 100000};
    for (uint64_t n : inst) for (double r : ratios) for (int64_t mg : margins) {
      const uint64_t e = pack_estimate(r, n, mg);
      CHECK(e <= n);                                                       // never more than one distinct k-mer per instance
      if (!(r > 0.0) || n == 0) CHECK(e == 0);                             // no probe: no estimate
      if (mg <= -1000) CHECK(e == 0);
      if (r > 0.0 && r < 1.0 && mg >= 0) {
        const double exact = r * (double)n;
        CHECK((double)e + 1.0 >= (exact < (double)n ? exact : (double)n));  // a margin of zero or more never falls short of ratio * instances
        if ((double)n >= exact * (1.0 + (double)mg / 1000.0) + PACK_MARGIN_FLOOR + 1) {
          CHECK((double)e + 1.0 >= exact * (1.0 + (double)mg / 1000.0) + PACK_MARGIN_FLOOR);
          CHECK((double)e <= exact * (1.0 + (double)mg / 1000.0) + PACK_MARGIN_FLOOR + 1.0);
        }
      }
      if (r > 0.0 && mg < 0 && mg > -1000 && n) CHECK((double)e <= (r < 1.0 ? r : 1.0) * (double)n);   // a negative margin falls short by construction
      if (r >= 1.0 && mg >= 0) CHECK(e == n);
      // monotone in the margin
      CHECK(pack_estimate(r, n, mg) <= pack_estimate(r, n, mg + 1) || mg == -1);   // (the floor comes in at 0)
      n_cap++;
    }
    // the benchmarked workload's figures: 8.65 G instances at the probe's 0.13655 -> 1.181 G distinct expected, + a sixteenth: room for
    // the 1181289506 there are
    static_assert(PACK_MARGIN_PERMILLE == 64, "the figures below are for a sixteenth");
    const uint64_t e = pack_estimate(0.13654994543564344, 8648488363ull, PACK_MARGIN_PERMILLE);
    CHECK(e > 1256000000ull && e < 1257000000ull && e >= 1181289506ull);
  }

  // ---- what the arena is asked for, and the capacity the gate gets ----
  {
    const uint64_t sizes[] = {0, 1, 32, 1000, 1001, 1ull << 31};
    for (uint64_t est : sizes) for (uint64_t arena : sizes) for (uint64_t out_cap : sizes) for (int caller = 0; caller < 2; caller++) {
      const uint64_t want = pack_arena_want(caller != 0, est, arena);
      if (caller) CHECK(want == 0);                                        // caller buffers are never grown
      else CHECK(want == (est > arena ? est : 0));                         // grown only to a larger estimate; no probe (0): left alone
      // the arena grew, or refused to (it then holds `after`: nothing, or what it held)
      const uint64_t afters[] = {arena, want ? want : arena, 0};
      for (uint64_t after : afters) {
        const uint64_t cap = pack_capacity(caller != 0, out_cap, after);
        CHECK(cap == (caller ? out_cap : after));
        if (!caller && want && after == want) CHECK(cap >= est && cap >= arena);   // the larger of the estimate and what was there
        n_cap++;
      }
    }
    // zero existing capacity and no probe: nowhere to pack into, the serial path
    CHECK(pack_capacity(false, 0, 0) == 0 && pack_arena_want(false, pack_estimate(0.0, 1000000, PACK_MARGIN_PERMILLE), 0) == 0);
    // key / count buffers of different sizes: the smaller decides
    CHECK(pack_buffers_kmers(800, 400, 8) == 100 && pack_buffers_kmers(800, 396, 8) == 99 && pack_buffers_kmers(792, 400, 8) == 99);
    CHECK(pack_buffers_kmers(1600, 400, 16) == 100 && pack_buffers_kmers(0, 400, 8) == 0 && pack_buffers_kmers(256, 256, 8) == 32);
  }

  // ---- the chain: which files ran early for a first deferred file q of m, and where the serial loop starts ----
  for (uint64_t m = 1; m <= 66; m++) for (uint64_t q = 0; q <= m; q++) {
    uint64_t early = 0, first_late = m;
    for (uint64_t i = 0; i < m; i++) {
      const bool e = pack_ran_early(i, q, m);
      // the launch of file i is told a threshold; the device's q is ~0 when nothing was deferred
      const uint64_t dev_q = q == m ? ~0ull : q;
      CHECK(e == (dev_q > pack_gate_threshold(i, m)));
      CHECK(pack_gate_threshold(i, m) < m);
      if (e) { CHECK(first_late == m); early++; }                          // the early files are a prefix
      else if (first_late == m) first_late = i;
      if (i >= q) CHECK(!e);                                               // a deferred file is never packed early
    }
    CHECK(pack_late_from(q, m) == first_late);
    CHECK(early == (q == m ? m : (q ? q - 1 : 0)));                         // one step behind the scans
    n_chain++;
  }
  printf("ok %llu %llu %llu\n", n_elig, n_cap, n_chain);
  return 0;
}
