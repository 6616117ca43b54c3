// mgc_group_batch.hpp -- which narrowed files share the launches of their grouping passes (mgc_sort.hip, launch_group_narrow_batch) and
// where each file's 4-byte words lie in the pass buffer Y meanwhile.  A pure function of the files' sizes, their launch keys and the
// budget: mgc_count.cpp (Count::group_all) asks it, a stand-alone host program (tests/host/group_batch_host.cpp) pins it.  Plain C++.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace mgc {

// One file as the planner sees it.  key: files may share a launch only if their keys are equal (the first pass's instantiation and the
// plan's digits: shifts and widths are arguments of the launch); eligible: the file takes the batched form at all (a narrowed file,
// high digit first off the 5-byte layout -- group_batch_form -- and not the probe file).
struct BatchFile { uint64_t n; uint32_t key; bool eligible; };
// A file's place in its batch: its slice of Y (byte offset; group_batch_slice_bytes(n) long) and its first tile in the first pass's
// ticket sequence.
struct BatchSlot { uint32_t file; uint64_t y_off, tile0; };
struct Batch { uint32_t key = 0; uint64_t y_bytes = 0, tiles = 0; std::vector<BatchSlot> files; };

constexpr uint64_t GROUP_BATCH_ALIGN = 256;
constexpr uint64_t group_batch_slice_bytes(uint64_t n) { return (4 * n + GROUP_BATCH_ALIGN - 1) / GROUP_BATCH_ALIGN * GROUP_BATCH_ALIGN; }

// Files in index order; a file joins the open batch of its key while the batch stays within budget_bytes of Y and max_files files
// (0: any number), otherwise it opens the next one.  A batch always takes its first file, whatever the budget: a budget below two
// files' slices gives one file per batch, which is the per-file launch sequence.  Empty and ineligible files are in no batch.
// tile_keys: keys per tile of the first pass.
inline std::vector<Batch> group_plan_batches(const std::vector<BatchFile> &files, uint64_t budget_bytes, uint32_t max_files, uint64_t tile_keys) {
  std::vector<Batch> out;
  std::vector<size_t> cur;                                  // per key met so far: its open batch (index into out)
  for (uint32_t i = 0; i < (uint32_t)files.size(); i++) {
    const BatchFile &f = files[i];
    if (!f.eligible || f.n == 0) continue;
    const uint64_t slice = group_batch_slice_bytes(f.n), tiles = (f.n + tile_keys - 1) / tile_keys;
    size_t at = out.size();
    for (size_t o : cur) if (out[o].key == f.key) at = o;
    const bool joins = at < out.size() && out[at].y_bytes + slice <= budget_bytes && (max_files == 0 || out[at].files.size() < max_files);
    if (!joins) {
      bool known = false;
      for (size_t &o : cur) if (out[o].key == f.key) { o = out.size(); known = true; break; }
      if (!known) cur.push_back(out.size());
      at = out.size();
      out.emplace_back();
      out[at].key = f.key;
    }
    Batch &b = out[at];
    b.files.push_back(BatchSlot{i, b.y_bytes, b.tiles});
    b.y_bytes += slice;
    b.tiles += tiles;
  }
  return out;
}

// the largest slice of Y any batch of a plan needs
inline uint64_t group_batches_y_bytes(const std::vector<Batch> &batches) {
  uint64_t m = 0;
  for (const Batch &b : batches) m = b.y_bytes > m ? b.y_bytes : m;
  return m;
}

}  // namespace mgc
