// select_host.cpp -- meryl_amd/csrc/mgc_selector.hpp on the host, for tests/test_select_host.py: the evaluator the kernels run
// (select_keep over mgc_select_term) on cases read from stdin, one per line, all numbers hexadecimal:
//   k hi lo out_value out_label presence  V[0] L[0] ... (one pair per set bit of presence, input order)
//   n_terms  then per term: quantity relation negate ends_product base_mask lhs_index+1 rhs_index+1 lhs_constant rhs_constant
//                           count_mask required_mask
// -> one line per case: 1 (kept) or 0, then what mgc_select_check says for 32 inputs (0 = accepted).
#include "../../meryl_amd/csrc/mgc_selector.hpp"

#include <cinttypes>
#include <cstdio>

struct HostSrc {
  uint32_t presence, out_value;
  uint64_t out_label, lo, hi;
  uint32_t v[32];
  uint64_t l[32];
  uint32_t value(uint32_t i) const { return v[i]; }
  uint64_t label(uint32_t i) const { return l[i]; }
};

int main() {
  unsigned k;
  HostSrc s;
  while (scanf("%x %" SCNx64 " %" SCNx64 " %x %" SCNx64 " %x", &k, &s.hi, &s.lo, &s.out_value, &s.out_label, &s.presence) == 6) {
    for (uint32_t i = 0; i < 32; i++) {
      s.v[i] = 0xdeadbeefu; s.l[i] = 0xdeadbeefdeadbeefull;                    // an absent input's slots must never be read
      if ((s.presence >> i) & 1u)
        if (scanf("%x %" SCNx64, &s.v[i], &s.l[i]) != 2) return 2;
    }
    unsigned n;
    if (scanf("%x", &n) != 1 || n > MGC_SELECT_MAX_TERMS) return 3;
    mgc_select_term t[MGC_SELECT_MAX_TERMS];
    memset(t, 0, sizeof(t));
    for (unsigned i = 0; i < n; i++) {
      unsigned q, r, neg, ends, bm, li, ri, req;
      uint64_t lc, rc, cm;
      if (scanf("%x %x %x %x %x %x %x %" SCNx64 " %" SCNx64 " %" SCNx64 " %x", &q, &r, &neg, &ends, &bm, &li, &ri, &lc, &rc, &cm, &req) != 11) return 4;
      t[i].quantity = (uint8_t)q; t[i].relation = (uint8_t)r; t[i].negate = (uint8_t)neg; t[i].ends_product = (uint8_t)ends;
      t[i].base_mask = (uint8_t)bm; t[i].lhs_index = (int32_t)li - 1; t[i].rhs_index = (int32_t)ri - 1;
      t[i].lhs_constant = lc; t[i].rhs_constant = rc; t[i].count_mask = cm; t[i].required_mask = req;
    }
    static_assert(sizeof(mgc_select_term) == 48, "the term travels in the kernel-argument segment: 16 of them beside the 1 KiB descriptor");
    printf("%d %d\n", mgc::select_keep(t, n, k, s) ? 1 : 0, mgc::select_check(t, n, 32).empty() ? 0 : 1);
  }
  return 0;
}
