// label_host.cpp -- meryl_amd/csrc/mgc_label.hpp on the host, for tests/test_labels_host.py: the label operations the kernels
// run (label_kernel_op + LabelAcc) over cases read from stdin, one per line:
//   is_merge op label_op constant n  L[0] V[0] ... L[n-1] V[n-1]      (hexadecimal labels and constant, decimal otherwise)
// -> one line per case: the kernel code and the label (hexadecimal), or "refused" for an unknown label operation.
#include "../../meryl_amd/csrc/mgc_label.hpp"

#include <cinttypes>
#include <cstdio>

int main() {
  int is_merge, op, label_op, n;
  unsigned long long c;
  while (scanf("%d %d %d %llx %d", &is_merge, &op, &label_op, &c, &n) == 5) {
    const int lop = mgc::label_kernel_op(is_merge != 0, op, label_op);
    mgc::LabelAcc la;
    la.begin(c);
    for (int j = 0; j < n; j++) {
      unsigned long long L;
      unsigned int V;
      if (scanf("%llx %u", &L, &V) != 2) return 2;
      if (lop >= 0) la.step(lop, L, V);
    }
    if (lop < 0) printf("refused\n");
    else printf("%d %llx\n", lop, la.l);
  }
  return 0;
}
