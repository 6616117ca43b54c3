// group_route_host.cpp -- meryl_amd/csrc/mgc_group_route.hpp on the host, for tests/test_group_route_host.py: the instantiation of
// radix_group_kernel each grouping pass of a file runs, over cases read from stdin, one per line (six numbers; unused ones 0):
//   N msd soa pipe dbg bits_first bits_second -> "refused", or: first | second | keys per tile of the first pass, of the second,
//                                                look-back granules per tile of the second
//   W key hpc bits_lo bits_hi 0 0             -> the same for a whole-key file (key: 0 u64, 2 K128, 3 K96)
//   S key 0 0 0 0 0                           -> the instantiation of both passes of launch_radix_sort's grouping mode
// An instantiation is printed as: key rb kpt dbg narrow hist2 soa pipe hpcd lds_bytes
#include "../../meryl_amd/csrc/mgc_group_route.hpp"

#include <cstdio>

static void print_inst(const mgc::GroupInst &i) {
  static const char *const names[] = {"u64", "u32", "K128", "K96"};
  printf("%s %d %d %d %d %d %d %d %d %zu", names[i.key], i.rb, i.kpt, i.dbg ? 1 : 0, i.narrow ? 1 : 0, i.hist2 ? 1 : 0, i.soa ? 1 : 0,
         i.pipe, i.hpcd, mgc::group_lds_bytes(i));
}

static void print_pair(const mgc::GroupInst &a, const mgc::GroupInst &b) {
  print_inst(a);
  printf(" | ");
  print_inst(b);
  printf(" | %llu %llu %u\n", (unsigned long long)mgc::group_tile(a), (unsigned long long)mgc::group_tile(b), mgc::group_granules(b));
}

int main() {
  char what;
  int a[6];
  while (scanf(" %c %d %d %d %d %d %d", &what, &a[0], &a[1], &a[2], &a[3], &a[4], &a[5]) == 7) {
    mgc::GroupInst first, second;
    if (what == 'N') {
      if (!mgc::group_pick_narrow(a[0] != 0, a[1] != 0, a[2] != 0, a[3] != 0, (uint32_t)a[4], (uint32_t)a[5], &first, &second)) {
        printf("refused\n");
        continue;
      }
      print_pair(first, second);
    } else if (what == 'W') {
      if (a[0] != mgc::GROUP_U64 && a[0] != mgc::GROUP_K128 && a[0] != mgc::GROUP_K96) return 2;
      mgc::group_pick_wide((mgc::GroupKey)a[0], (uint32_t)a[1], (uint32_t)a[2], (uint32_t)a[3], &first, &second);
      print_pair(first, second);
    } else if (what == 'S') {
      if (a[0] != mgc::GROUP_U64 && a[0] != mgc::GROUP_K128) return 2;
      print_inst(mgc::group_pick_sorted((mgc::GroupKey)a[0]));
      printf("\n");
    } else {
      return 2;
    }
  }
  return 0;
}
