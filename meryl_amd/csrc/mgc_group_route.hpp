// mgc_group_route.hpp -- which instantiation of radix_group_kernel<K, RB, 1024, KPT, DBG, NARROW, HIST2, SOA, PIPE, HPCD, BATCH> a grouping
// pass runs (mgc_sort.hip: launch_group_narrow, launch_group_wide, the grouping mode of launch_radix_sort).  The launchers there
// ask these functions and hand the answer to the one table that maps a GroupInst to its template instantiation.  Shared with a
// stand-alone host program (tests/host/group_route_host.cpp) that pins the rules: plain C++, no HIP header needed.
#pragma once
#include <cstddef>
#include <cstdint>

namespace mgc {

enum GroupKey : uint32_t { GROUP_U64, GROUP_U32 /* narrowed words: second pass of a narrowed file */, GROUP_K128, GROUP_K96 };

// the template arguments of one instantiation (BLOCK is 1024 everywhere)
struct GroupInst {
  GroupKey key; int rb, kpt; bool dbg, narrow, hist2, soa; int pipe, hpcd;
  bool batch = false;                                       // one launch over the tiles of many files (radix_group_batch_kernel)
};
inline bool operator==(const GroupInst &a, const GroupInst &b) {
  return a.key == b.key && a.rb == b.rb && a.kpt == b.kpt && a.dbg == b.dbg && a.narrow == b.narrow && a.hist2 == b.hist2 &&
         a.soa == b.soa && a.pipe == b.pipe && a.hpcd == b.hpcd && a.batch == b.batch;
}

// keys per thread of the narrowed passes: the first pass (fetch inside the look-back), the pipelined 5-byte first pass (A/B builds
// give MGC_NARROW_KPT0 on the command line; mgc_sort.hip asserts that both agree), the second pass
constexpr int GROUP_KPT_NARROW0 = 16, GROUP_KPT_NARROW1 = 24;
#ifdef MGC_NARROW_KPT0
constexpr int GROUP_KPT_NARROW0P = MGC_NARROW_KPT0;
#else
constexpr int GROUP_KPT_NARROW0P = 24;
#endif
constexpr int GROUP_BLOCK = 1024;
constexpr size_t GROUP_LDS_MAX = 160 * 1024, GROUP_RANK_TABLE_BYTES = 8192;   // HPCD: 4096 16-bit ranks behind the tile

constexpr int group_key_bytes(GroupKey k) { return k == GROUP_U32 ? 4 : (k == GROUP_U64 ? 8 : (k == GROUP_K96 ? 12 : 16)); }
constexpr int group_kpt_wide(GroupKey k) { return k == GROUP_U64 ? 16 : (k == GROUP_K96 ? 12 : 8); }   // whole keys: 128 / 144 / 128 KiB tiles

// keys per tile, look-back granules per tile, dynamic LDS of an instantiation (GroupSmem<...>::BYTES of mgc_sort.hip, which asserts
// the equality for every row of its table, plus the rank table)
constexpr uint64_t group_tile(const GroupInst &i) { return (uint64_t)GROUP_BLOCK * (uint64_t)i.kpt; }
constexpr uint32_t group_granules(const GroupInst &i) { return (1u << i.rb) / 2u; }
constexpr size_t group_lds_bytes(const GroupInst &i) {
  // a narrowing pass exchanges 32-bit words + the digits (one byte each up to eight bits, else two), any other pass whole keys
  return ((size_t)group_tile(i) * (size_t)(i.narrow ? (i.rb <= 8 ? 5 : 6) : group_key_bytes(i.key)) + 15) / 16 * 16 +
         ((size_t)1 << i.rb) * 20 + 64 * 4 + 4 * 8 + (i.hpcd ? GROUP_RANK_TABLE_BYTES : 0);
}

// ---- a narrowed file: u64 keys (or the 5-byte layout) -> u32 words -> u32 words ----
// msd: high digit first (prepared header + scratch); soa: the 5-byte layout; pipe: Switches::group_pipe; dbg: the instrumented
// instantiations (high digit first only); bits_first / bits_second: digit widths in the order the passes take them.
// false: refused (the 5-byte layout exists only high digit first)
inline bool group_pick_narrow(bool msd, bool soa, bool pipe, bool dbg, uint32_t bits_first, uint32_t bits_second, GroupInst *first,
                              GroupInst *second) {
  if (soa && !msd) return false;
  dbg = dbg && msd;
  const bool ahead = soa && pipe;                           // the fetch a whole tile ahead: 24576-key tiles
  // eight-bit digits take the instantiations with half the counters, walkers and granules (not the instrumented ones)
  const int rb_first = (ahead && !dbg && bits_first <= 8) ? 8 : 9, rb_second = (!dbg && bits_second <= 8) ? 8 : 9;
  *first  = GroupInst{GROUP_U64, rb_first, ahead ? GROUP_KPT_NARROW0P : GROUP_KPT_NARROW0, dbg, true, msd, soa, ahead ? 2 : 0, 0};
  *second = GroupInst{GROUP_U32, rb_second, GROUP_KPT_NARROW1, dbg, false, false, false, 0, 0};
  return true;
}

// ---- many narrowed files in one launch per pass (mgc_group_batch.hpp plans the batches) ----
// Only the judged form is batched: high digit first off the 5-byte layout, fetched a tile ahead, not instrumented, not staggered.
// Every other form keeps its per-file launches.
inline bool group_batch_form(bool msd, bool soa, bool pipe, bool dbg, uint32_t stagger) { return msd && soa && pipe && !dbg && stagger <= 1u; }
inline bool group_pick_narrow_batch(uint32_t bits_first, uint32_t bits_second, GroupInst *first, GroupInst *second) {
  if (!group_pick_narrow(true, true, true, false, bits_first, bits_second, first, second)) return false;
  first->batch = second->batch = true;
  return true;
}

// ---- a whole-key file, high digit first; hpc: SortPlan::hpc; bits_lo / bits_hi: the plan's pass_bits[0] / [1] ----
inline void group_pick_wide(GroupKey key, uint32_t hpc, uint32_t bits_lo, uint32_t bits_hi, GroupInst *first, GroupInst *second) {
  const int kpt = group_kpt_wide(key);
  const int rb = (!hpc && bits_lo <= 8 && bits_hi <= 8) ? 8 : 9;
  const GroupInst plain{key, rb, kpt, false, false, false, false, 0, 0};
  // `compress`: the rank table in LDS where 8 KiB are left behind the tile (not K96)
  const bool tab = rb == 9 && group_lds_bytes(plain) + GROUP_RANK_TABLE_BYTES <= GROUP_LDS_MAX;
  const int hpcd = (tab && hpc == 1) ? 1 : ((tab && hpc == 2 && bits_lo <= 8) ? 2 : 0);
  *first = plain; first->hist2 = true; first->hpcd = hpcd;
  *second = plain;
  if (hpcd == 1) second->hpcd = 1;                          // both digits dense ranks
  if (hpcd == 2) second->rb = 8;                            // the low digit a plain eight-bit field
}

// ---- the grouping mode of launch_radix_sort (low digit first off a histogram read): both passes ----
constexpr GroupInst group_pick_sorted(GroupKey key) { return GroupInst{key, 9, group_kpt_wide(key), false, false, false, false, 0, 0}; }

}  // namespace mgc
