// mgc_label.hpp -- the label of a written k-mer from the labels and values of the inputs that hold it: meryl2's
// merylOpCompute::findOutputLabel (src/meryl2/merylOpCompute.C:286-395); the rules, with the line each comes from, are in
// include/meryl_gpu_count.h (MGC_LABEL_*).  Shared by the kernels (mgc_merge_many.hip, mgc_merge.hip through mgc_common.hpp),
// the host code that resolves an operation's label word (mgc_api.cpp, mgc_eval.cpp) and a stand-alone host program
// (tests/host/label_host.cpp): plain C++, no HIP header needed.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define MGC_LABEL_FN __host__ __device__ __forceinline__
#else
#define MGC_LABEL_FN inline
#endif

namespace mgc {

// kernel codes: the MGC_LABEL_* values once DEFAULT and SELECTED are resolved (label_kernel_op); SELECTED under *-min / *-max
// becomes LOP_SEL_MIN / LOP_SEL_MAX
constexpr int LOP_SET = 1, LOP_FIRST = 2, LOP_MIN = 3, LOP_MAX = 4, LOP_AND = 5, LOP_OR = 6, LOP_XOR = 7, LOP_DIFFERENCE = 8,
              LOP_LIGHTEST = 9, LOP_HEAVIEST = 10, LOP_INVERT = 11, LOP_SEL_MIN = 13, LOP_SEL_MAX = 14;

// MGC_LABEL_* of a merge (is_merge, op = MGC_MERGE_*) or value operation -> the code the kernels take: DEFAULT resolved as
// src/meryl2/merylCommandBuilder-processText.C:384-499 sets it per alias, SELECTED by what the operation selects; -1: unknown
inline int label_kernel_op(bool is_merge, int op, int label_op) {
  if (label_op < 0 || label_op > 12) return -1;
  if (label_op == 0) {
    if (!is_merge) label_op = LOP_FIRST;                                            // value operations
    else if (op == 0 || op == 10) label_op = LOP_OR;                                // union-sum, union
    else if (op == 3 || op == 6) label_op = LOP_AND;                                // intersect-sum, intersect
    else if (op == 1 || op == 2 || op == 4 || op == 5) label_op = 12;               // *-min, *-max: SELECTED
    else if (op == 7) label_op = LOP_DIFFERENCE;                                    // subtract
    else label_op = LOP_FIRST;                                                      // difference, symmetric-difference
  }
  if (label_op == 12) {
    if (is_merge && (op == 1 || op == 4)) return LOP_SEL_MIN;
    if (is_merge && (op == 2 || op == 5)) return LOP_SEL_MAX;
    return LOP_FIRST;
  }
  return label_op;
}

// begin(c), then step(lop, L[j], V[j]) over the active inputs in input order; l is the result
struct LabelAcc {
  unsigned long long l; unsigned int v; bool any;
  MGC_LABEL_FN void begin(unsigned long long c) { l = c; v = 0xFFFFFFFFu; any = false; }
  MGC_LABEL_FN void step(int lop, unsigned long long L, unsigned int V) {
    switch (lop) {
      case LOP_FIRST:      if (!any) l = L; break;
      case LOP_MIN:        if (V < v) { l = L; v = V; } break;                  // strict: a value of 2^32-1 never wins (:309-320)
      case LOP_MAX:        l = L > l ? L : l; break;
      case LOP_AND:        l &= L; break;
      case LOP_OR:         l |= L; break;
      case LOP_XOR:        l ^= L; break;
      case LOP_DIFFERENCE: l = any ? (l & ~L) : (L & ~l); break;                // L[0] & ~c & ~L[1] & ... (:347-352)
      case LOP_LIGHTEST:   if (__builtin_popcountll(L) < __builtin_popcountll(l)) l = L; break;
      case LOP_HEAVIEST:   if (__builtin_popcountll(L) > __builtin_popcountll(l)) l = L; break;
      case LOP_INVERT:     l = ~L; break;
      case LOP_SEL_MIN:    if (!any || V < v) { l = L; v = V; } break;          // the first active input with the smallest value
      case LOP_SEL_MAX:    if (!any || V > v) { l = L; v = V; } break;
      default:             break;                                               // LOP_SET: the constant
    }
    any = true;
  }
};

}  // namespace mgc
