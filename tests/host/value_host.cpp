// value_host.cpp -- meryl_amd/csrc/mgc_value.hpp on the host, for tests/test_assign_host.py: the value rules the kernels run
// (value_kernel_op + ValueAcc) over cases read from stdin, one per line:
//   assign constant n  V[0] ... V[n-1]      (decimal)
// -> one line per case: the kernel code and the value, or "refused" for an unknown assignment.  For DIVZ every step is also
// computed the way the reference writes it, round(x / (double)d) (src/meryl2/merylOpCompute.C:227-245), and a case where the two
// forms differ ends the program with status 3.
#include "../../meryl_amd/csrc/mgc_value.hpp"

#include <cmath>
#include <cstdio>

static unsigned int divz_reference(unsigned int x, unsigned int d) {
  if (d == 0) return 0;
  if (x < d) return 1;
  return (unsigned int)round(x / (double)d);
}

int main() {
  int assign, n;
  unsigned long long c;
  while (scanf("%d %llu %d", &assign, &c, &n) == 3) {
    const int vop = mgc::value_kernel_op(assign);
    mgc::ValueAcc va;
    va.begin((unsigned int)c);
    unsigned int ref = 0;
    for (int j = 0; j < n; j++) {
      unsigned int V;
      if (scanf("%u", &V) != 1) return 2;
      if (vop >= 0) va.step(vop, V);
      ref = j == 0 ? V : divz_reference(ref, V);
    }
    if (vop < 0) { printf("refused\n"); continue; }
    const unsigned int v = va.finish(vop, (unsigned int)c, (unsigned int)n);
    if (vop == mgc::VOP_DIVZ && divz_reference(ref, (unsigned int)c) != v) {
      fprintf(stderr, "divzero: the integer form gives %u, round(x / (double)d) gives %u\n", v, divz_reference(ref, (unsigned int)c));
      return 3;
    }
    printf("%d %u\n", vop, v);
  }
  return 0;
}
