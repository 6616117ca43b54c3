// mgc_pack_plan.hpp -- may the files of a count be packed while later files are still being counted (mgc_count.cpp, Count::pack_plan),
// and how many k-mers the packed result must have room for before the first packing launch is queued.  Pure functions of what the host
// knows once the statistics of all files are back: mgc_count.cpp asks them, a stand-alone host program (tests/host/pack_plan_host.cpp)
// pins them.  Plain C++.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace mgc {

// One file as the decision sees it: its k-mers, its largest sub-bucket, how many sub-buckets are above the count kernels' capacity
// (its oversized list), whether the hash-count kernels take it (finish_uses_hash: only then is an oversized list streamed), and whether
// it was already finished by the stable sort (the probe file can have been).
struct PackFile { uint64_t size, maxsub, nlarge; bool hash, fallback; };

// A file is packed early only if what finishes it is queued in one go, without the host looking at it again: its count launch, and --
// where it has an oversized list -- the streaming launch of that list on the second stream, which the packing chain then waits for as
// well.  Out: a file whose oversized list nothing streams (widened back, or finished by the stable sort: both synchronise and rewrite
// the file), and one with a sub-bucket above stream_max, about which the host asks a probe launch first (Count::oversized_streams).
// What can still change a file's distinct counts afterwards is the retry launch, and that the device decides (the gate,
// mgc_finish.hip: pack_gate_scan_kernel).
inline bool pack_file_ok(const PackFile &f, uint64_t cap, uint64_t stream_max) {
  if (f.size == 0) return true;
  if (f.fallback) return false;
  return f.nlarge == 0 ? f.maxsub <= cap : (f.hash && f.maxsub <= stream_max);
}

// Early packing is on when the switch is (MGC_PACK_OVERLAP=0: off), some file holds k-mers and every file is one of the above.
inline bool pack_overlap_eligible(const std::vector<PackFile> &files, uint64_t cap, uint64_t stream_max, bool switch_on) {
  bool any = false;
  for (const PackFile &f : files) {
    if (!pack_file_ok(f, cap, stream_max)) return false;
    any = any || f.size != 0;
  }
  return switch_on && any;
}

// The margin of the estimate, in thousandths of it.  The estimate takes the probe file's distinct / instances ratio for every file.
// The probe file is the smallest file that is still a fair sample, and on reads of even coverage the smallest file has the lowest
// ratio, so the estimate errs low.  Measured, distinct / instances of the whole count over the probe file's: 1.0003 on the benchmarked
// workload (10 Gbp, k = 21: files 0.1365 .. 0.1368, probe 0.1365), 1.027 / 1.0005 / 0.988 on the tests' 9 Mbase reads (k = 21
// canonical, k = 31 canonical, k = 21 forward: files of 2 K to 240 K k-mers, 0.133 .. 0.147 at the widest).  A sixteenth covers the
// widest of them twice over and costs 0.9 GB of arena at 10 Gbp (12 bytes per k-mer).  Nothing but speed depends on it: an estimate
// that falls short costs the first count of a session part of its overlap (the gate defers, the result grows afterwards); every
// later count of the session finds the arena at the size the one before needed.
constexpr int64_t PACK_MARGIN_PERMILLE = 64;
constexpr uint64_t PACK_MARGIN_FLOOR = 4096;             // k-mers on top of it: tiny inputs, whose files are no sample of each other

// How many distinct k-mers to expect: ratio * instances * (1 + margin), never more than the instances (a k-mer is distinct at most
// once per instance), 0 without a probe ratio.  margin_permille may be negative (tests make the estimate fall short by construction).
inline uint64_t pack_estimate(double probe_ratio, uint64_t instances, int64_t margin_permille) {
  if (!(probe_ratio > 0.0) || instances == 0) return 0;
  const double r = probe_ratio < 1.0 ? probe_ratio : 1.0;
  double e = r * (double)instances * (1.0 + (double)margin_permille / 1000.0);
  if (e < 0.0) e = 0.0;
  const uint64_t est = (e >= (double)instances ? instances : (uint64_t)e) + (margin_permille >= 0 ? PACK_MARGIN_FLOOR : 0);
  return est < instances ? est : instances;
}

// How many k-mers the arena's result buffers should be grown to before anything is queued (0: leave them).  Caller buffers
// (mgc_count_buckets_into) are never grown; nor is an arena that already holds the estimate.
inline uint64_t pack_arena_want(bool caller_buffers, uint64_t estimate, uint64_t arena_kmers) {
  if (caller_buffers || estimate <= arena_kmers) return 0;
  return estimate;
}

// The capacity the gate is given, once the arena has been asked to grow (arena_kmers: what it holds NOW, whether or not it grew).
// 0: nowhere to pack into before the total is known -- the count takes the serial path.
inline uint64_t pack_capacity(bool caller_buffers, uint64_t out_cap, uint64_t arena_kmers) { return caller_buffers ? out_cap : arena_kmers; }

// k-mers a pair of result buffers holds (keys of key_bytes each, 4-byte counts)
inline uint64_t pack_buffers_kmers(size_t key_buf_bytes, size_t count_buf_bytes, size_t key_bytes) {
  const uint64_t a = key_buf_bytes / key_bytes, b = count_buf_bytes / sizeof(uint32_t);
  return a < b ? a : b;
}

// Files are packed in index order, each one step behind its scan (the last sub-bucket of a file ends where the next file's first one
// begins, and that offset is written by the NEXT file's scan).  With q the first deferred file of m (q == m: none), file i was packed
// early iff its successor was scanned: i + 1 < q, or it is the last file and nothing was deferred.
inline bool pack_ran_early(uint64_t i, uint64_t q, uint64_t m) { return i + 1 < q || (i + 1 == m && q == m); }
// ... so the serial loop afterwards starts here
inline uint64_t pack_late_from(uint64_t q, uint64_t m) { return q >= m ? m : (q ? q - 1 : 0); }
// what the packing launch of file i is told: it runs iff the device's q is ABOVE this
inline uint64_t pack_gate_threshold(uint64_t i, uint64_t m) { return i + 1 < m ? i + 1 : i; }

}  // namespace mgc
