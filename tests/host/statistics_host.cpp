// statistics_host.cpp -- the statistics formatter (meryl_amd/csrc/mdb_statistics.hpp) alone, for a sanitizer build on the host.
// stdin: one histogram per line, `k unique distinct total n_pairs value occurrences ...`; stdout: every report followed by a line "==".
#include "../../meryl_amd/csrc/mdb_statistics.hpp"

#include <iostream>
#include <sstream>
#include <vector>

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    uint32_t k = 0;
    uint64_t unique = 0, distinct = 0, total = 0, n = 0;
    if (!(in >> k >> unique >> distinct >> total >> n)) continue;
    std::vector<uint64_t> v(n), o(n);
    for (uint64_t i = 0; i < n; i++) in >> v[i] >> o[i];
    std::cout << mdb::format_statistics(k, v.data(), o.data(), n, unique, distinct, total) << "==\n";
  }
  return 0;
}
