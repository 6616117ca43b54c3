// mgc_route.hpp -- the two decisions of the operation-tree evaluator that pick device code: which pass pair an inner node of
// mgc_db_eval* takes (eval_route; mgc_eval.cpp), and which instantiation of merge_many_kernel / select_kernel a pass of the
// unified launchers runs (pass_inst; mgc_merge_many.hip, mgc_merge.hip).  Shared with a stand-alone host program
// (tests/host/route_host.cpp) that pins both tables: plain C++, no HIP header needed.
#pragma once
#include "../../include/meryl_gpu_count.h"

#include <cstdint>

namespace mgc {

// a merge node takes merge_many (one count pass, one emit pass over all inputs) from this many inputs on; below it the
// two-input merge path kernel.  NOT MEASURED yet: 3 is what the bytes moved suggest; scripts/setops_bench.py leg (a) decides
// (the smallest N at which merge_many is not slower than the fold on both input mixes).
constexpr uint32_t MERGE_MANY_MIN_INPUTS = 3;

// the kernel family is the enumerator's first word; the second says what the pass rule carries
enum Route {
  ROUTE_FOLD,                    // the left fold of the two-input merge (fold_slices)
  ROUTE_SELECT_PLAIN,            // select_kernel, no labels
  ROUTE_SELECT_LABELLED,         //   plain count, labelled emit
  ROUTE_SELECT_SELECTED,         //   with the node's program
  ROUTE_MANY_PLAIN,              // merge_many_kernel, no labels
  ROUTE_MANY_LABELLED,           //   plain count, labelled emit; one input included
  ROUTE_MANY_SELECTED,           //   with the node's program; one input included
  ROUTE_MANY_ASSIGNED,           //   with the node's assignment (and program); both node kinds
};

// value_node: MGC_NODE_VALUE (else MGC_NODE_MERGE); labels: they travel in this evaluation; program / assignment: the node has
// one; many_enabled: MGC_MERGE_MANY is not 0 (it only chooses between the fold and merge_many where neither labels, a program
// nor an assignment needs the latter)
inline Route eval_route(bool value_node, uint32_t n_inputs, bool labels, bool program, bool assignment, bool many_enabled) {
  if (assignment) return ROUTE_MANY_ASSIGNED;
  if (program) return value_node ? ROUTE_SELECT_SELECTED : ROUTE_MANY_SELECTED;
  if (labels) return value_node ? ROUTE_SELECT_LABELLED : ROUTE_MANY_LABELLED;
  if (value_node) return ROUTE_SELECT_PLAIN;
  return (many_enabled && n_inputs >= MERGE_MANY_MIN_INPUTS && n_inputs <= MGC_MERGE_MANY_MAX) ? ROUTE_MANY_PLAIN : ROUTE_FOLD;
}

inline bool route_merges_many(Route r) { return r >= ROUTE_MANY_PLAIN; }

// what a failed pass pair of the route is called in the error text
inline const char *route_context(Route r) {
  switch (r) {
    case ROUTE_SELECT_PLAIN: case ROUTE_SELECT_LABELLED: return "a value operation";
    case ROUTE_SELECT_SELECTED:                          return "a value operation with a selector";
    case ROUTE_MANY_SELECTED:                            return "merging a slice with a selector";
    case ROUTE_MANY_ASSIGNED:                            return "merging a slice with a value assignment";
    default:                                             return "merging a slice";
  }
}

// the template arguments after <K, EMIT> of merge_many_kernel (select_kernel: without ASSIGN)
struct PassInst { bool labels, select, assign; };

// emit: the pass; program: the rule carries a (possibly empty) selector program; program_labels: it holds a LABEL term;
// assignment: a value rule other than VOP_NONE; filter: a value filter on the assigned value; out_labels: the emit pass is given
// somewhere to write labels.  An assignment or a filter always comes with a program.
inline PassInst pass_inst(bool emit, bool program, bool program_labels, bool assignment, bool filter, bool out_labels) {
  PassInst i;
  i.assign = assignment || filter;
  i.select = program || i.assign;
  i.labels = (i.select && program_labels) || (emit && out_labels);   // labels decide what is written only through a program
  return i;
}

}  // namespace mgc
