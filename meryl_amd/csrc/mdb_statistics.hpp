// mdb_statistics.hpp -- the text of `meryl statistics` (merylOperation::reportStatistics, src/meryl/merylOp-histogram.C:65-93) from a
// histogram given as (value, occurrences) pairs ascending by value.  Host only, no dependencies: meryl_db.cpp exports it as
// mdb_format_statistics and tests/host/statistics_host.cpp builds it alone.
#pragma once

#include <algorithm>
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <string>

namespace mdb {

inline std::string format_statistics(uint32_t k, const uint64_t *values, const uint64_t *occurrences, uint64_t n_pairs,
                                     uint64_t num_unique, uint64_t num_distinct, uint64_t num_total) {
  std::string out;
  char line[256];
  auto put = [&](int n) { if (n > 0) out.append(line, (size_t)std::min<int>(n, (int)sizeof(line) - 1)); };
  // nUniverse = buildLowBitMask<uint64>(2k) + 1 in uint64 arithmetic (:65): 4^k while 2k < 64.  From k = 32 on the mask is all
  // ones and the sum WRAPS to 0, so `missing` prints 0 - distinct modulo 2^64.  The wrap is the reference's and is kept.
  const uint64_t mask = (2 * k >= 64) ? ~0ull : ((1ull << (2 * k)) - 1ull);
  const uint64_t n_universe = mask + 1ull;
  put(snprintf(line, sizeof(line), "Number of %u-mers that are:\n", k));
  put(snprintf(line, sizeof(line), "  unique   %20" PRIu64 "  (exactly one instance of the kmer is in the input)\n", num_unique));
  put(snprintf(line, sizeof(line), "  distinct %20" PRIu64 "  (non-redundant kmer sequences in the input)\n", num_distinct));
  put(snprintf(line, sizeof(line), "  present  %20" PRIu64 "  (...)\n", num_total));
  put(snprintf(line, sizeof(line), "  missing  %20" PRIu64 "  (non-redundant kmer sequences not in the input)\n", n_universe - num_distinct));
  out += "\n";
  out += "             number of   cumulative   cumulative     presence\n";
  out += "              distinct     fraction     fraction   in dataset\n";
  out += "frequency        kmers     distinct        total       (1e-6)\n";
  out += "--------- ------------ ------------ ------------ ------------\n";
  uint64_t s_distinct = 0, s_total = 0;
  for (uint64_t i = 0; i < n_pairs; i++) {
    const uint64_t value = values[i], occur = occurrences[i];
    s_distinct += occur;
    s_total += occur * value;
    put(snprintf(line, sizeof(line), "%9" PRIu64 " %12" PRIu64 " %12.4f %12.4f %12.6f\n", value, occur,
                 (double)s_distinct / (double)num_distinct, (double)s_total / (double)num_total,
                 (double)value / (double)num_total * 1000000.0));
  }
  return out;
}

}  // namespace mdb
