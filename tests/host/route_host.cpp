// route_host.cpp -- meryl_amd/csrc/mgc_route.hpp on the host, for tests/test_route_host.py: the route an inner node of an
// operation tree takes and the kernel instantiation a pass runs, over cases read from stdin, one per line:
//   R value_node n_inputs labels program assignment many_enabled   -> the route's name, whether it is a merge_many route, and the
//                                                                      context of its error text
//   I emit program program_labels assignment filter out_labels     -> LABELS SELECT ASSIGN (0 / 1)
#include "../../meryl_amd/csrc/mgc_route.hpp"

#include <cstdio>

static const char *route_name(mgc::Route r) {
  switch (r) {
    case mgc::ROUTE_FOLD:            return "fold";
    case mgc::ROUTE_SELECT_PLAIN:    return "select-plain";
    case mgc::ROUTE_SELECT_LABELLED: return "select-labelled";
    case mgc::ROUTE_SELECT_SELECTED: return "select-selected";
    case mgc::ROUTE_MANY_PLAIN:      return "many-plain";
    case mgc::ROUTE_MANY_LABELLED:   return "many-labelled";
    case mgc::ROUTE_MANY_SELECTED:   return "many-selected";
    case mgc::ROUTE_MANY_ASSIGNED:   return "many-assigned";
  }
  return "?";
}

int main() {
  char what;
  int a[6];
  while (scanf(" %c %d %d %d %d %d %d", &what, &a[0], &a[1], &a[2], &a[3], &a[4], &a[5]) == 7) {
    if (what == 'R') {
      const mgc::Route r = mgc::eval_route(a[0] != 0, (uint32_t)a[1], a[2] != 0, a[3] != 0, a[4] != 0, a[5] != 0);
      printf("%s %d %s\n", route_name(r), mgc::route_merges_many(r) ? 1 : 0, mgc::route_context(r));
    } else if (what == 'I') {
      const mgc::PassInst i = mgc::pass_inst(a[0] != 0, a[1] != 0, a[2] != 0, a[3] != 0, a[4] != 0, a[5] != 0);
      printf("%d %d %d\n", i.labels ? 1 : 0, i.select ? 1 : 0, i.assign ? 1 : 0);
    } else {
      return 2;
    }
  }
  return 0;
}
