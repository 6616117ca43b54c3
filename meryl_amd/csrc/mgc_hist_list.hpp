// mgc_hist_list.hpp -- the list tier of the tiered histograms (mgc_value_hist.hip, mgc_analyze.cpp): keys that a pass does not count in
// LDS bins are appended to a device list as uint64, the list is sorted and run-length counted on the device, and only the
// (key, occurrences) pairs cross to the host, where they are merged into one sorted vector.  Host code.  The merge needs no HIP: with
// MGC_HIST_LIST_HOST_ONLY the header stops after it.  Internal.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

namespace mgc {
struct HistPair { uint64_t key, n; };

// sorted distinct (keys[i], counts[i]) of one pass -> acc (ascending by key, distinct), the counts of equal keys summed
inline void hist_merge(std::vector<HistPair> &acc, const uint64_t *keys, const uint32_t *counts, size_t n) {
  std::vector<HistPair> out;
  out.reserve(acc.size() + n);
  size_t i = 0, j = 0;
  while (i < acc.size() || j < n) {
    if (j == n || (i < acc.size() && acc[i].key < keys[j])) out.push_back(acc[i++]);
    else if (i == acc.size() || keys[j] < acc[i].key) { out.push_back(HistPair{keys[j], counts[j]}); j++; }
    else { out.push_back(HistPair{keys[j], acc[i].n + counts[j]}); i++; j++; }
  }
  acc.swap(out);
}
}  // namespace mgc

#ifndef MGC_HIST_LIST_HOST_ONLY
#include "mgc_device.h"
#include "mgc_session.hpp"

namespace mgc {
// One histogram's list tier.  A pass: reset, the owner's kernel appends to list() and counts the entries in *list_n() (how the list
// is sized, and what happens when it was too small, is the owner's business), the owner reads *list_n() and drains that many.
struct ListTier {
  const char *who;                          // the owner, in front of every message
  DBuf d_ctr;                               // uint64 list length at 0, uint32 sort-error word at 64
  DBuf d_list[2], d_sws, d_rws, d_uniq, d_ucnt;
  std::vector<HistPair> acc;                // every drained pass, ascending by key

  explicit ListTier(const char *who_) : who(who_) {}

  hipError_t reserve(uint64_t entries) { return d_list[0].ensure(8 * entries); }
  uint64_t   capacity() const { return d_list[0].cap / 8; }
  uint64_t  *list() const { return d_list[0].as<uint64_t>(); }
  uint64_t  *list_n() const { return d_ctr.as<uint64_t>(); }
  hipError_t reset(hipStream_t st) {
    const hipError_t e = d_ctr.ensure(256);
    return e != hipSuccess ? e : hipMemsetAsync(d_ctr.p, 0, 128, st);
  }

  // list()[0, need), keys of key_bits bits -> acc.  Returns with the stream idle; before_sync, if given, is recorded behind the last
  // device work and before the host waits for it (need == 0: it is all that is recorded and waited for).  MGC_* code.
  int drain(uint64_t need, uint32_t key_bits, hipStream_t st, hipEvent_t before_sync = nullptr) {
#define LT_TRY(expr) do { hipError_t e__ = (expr); if (e__ != hipSuccess) {                                         \
    set_err(nullptr, "%s: %s -> %s", who, #expr, hipGetErrorString(e__));                                          \
    return (e__ == hipErrorOutOfMemory) ? MGC_ENOMEM : MGC_EHIP; } } while (0)
    if (need == 0) {
      if (before_sync) { LT_TRY(hipEventRecord(before_sync, st)); LT_TRY(hipEventSynchronize(before_sync)); }
      return MGC_OK;
    }
    uint32_t *d_sort_err = reinterpret_cast<uint32_t *>(d_ctr.as<unsigned char>() + 64);
    LT_TRY(d_list[1].ensure(8 * need));
    LT_TRY(d_sws.ensure(sort_workspace_bytes(need)));
    LT_TRY(d_rws.ensure(rle_workspace_bytes(need)));
    SortPlan plan;
    make_sort_plan(0, key_bits, &plan);
    int in_alt = 0;
    LT_TRY(launch_radix_sort(d_list[0].p, d_list[1].p, need, 1, plan, d_sws.p, d_sws.cap, d_sort_err, &in_alt, st, nullptr));
    const void *sorted = d_list[in_alt ? 1 : 0].p;
    LT_TRY(launch_rle_count(sorted, need, 1, d_rws.p, st));
    uint64_t nd = 0;
    LT_TRY(rle_read_total(d_rws.p, &nd, st));                 // (synchronises)
    uint32_t h_err = 0;
    LT_TRY(hipMemcpyAsync(&h_err, d_sort_err, 4, hipMemcpyDeviceToHost, st));
    LT_TRY(d_uniq.ensure(8 * nd));
    LT_TRY(d_ucnt.ensure(4 * nd));
    LT_TRY(launch_rle_emit(sorted, need, 1, d_rws.p, d_uniq.p, d_ucnt.as<uint32_t>(), st));
    std::vector<uint64_t> hk(nd);
    std::vector<uint32_t> hc(nd);
    LT_TRY(hipMemcpyAsync(hk.data(), d_uniq.p, 8 * nd, hipMemcpyDeviceToHost, st));
    LT_TRY(hipMemcpyAsync(hc.data(), d_ucnt.p, 4 * nd, hipMemcpyDeviceToHost, st));
    if (before_sync) LT_TRY(hipEventRecord(before_sync, st));
    LT_TRY(hipStreamSynchronize(st));
#undef LT_TRY
    if (h_err) { set_err(nullptr, "%s: radix sort look-back timed out", who); return MGC_ETIMEOUT; }
    hist_merge(acc, hk.data(), hc.data(), nd);
    return MGC_OK;
  }
};
}  // namespace mgc
#endif
