// mgc_chunk_ring.hpp -- the chunk ring of the whole-file text readers (mgc_textfile.cpp), host-only: no HIP, no session.
//
// run_chunk_ring pumps chunks 0 .. n_chunks-1 through a ring of caller-owned slots: `n_threads` producer threads fill
// the slots (pread, inflate, ...) and the CALLING thread consumes the chunks in order (upload + parse).  What holds:
//   - chunk c uses slot c mod n_slots;
//   - a producer writes a slot only after the slot's previous chunk was released: `lag` chunks after its consume;
//   - chunks reach `consume` strictly ascending, each at most once;
//   - no chunk reaches `consume` once a failure (alloc, fill, or the consumer's own stop) has been noticed;
//   - on return every thread is joined and no slot is written again.
// tests/host/input_host.cpp runs it under the thread and address sanitizers.
#pragma once

#include "mgc_clock.hpp"

#include <algorithm>
#include <atomic>
#include <cassert>
#include <condition_variable>
#include <cstddef>
#include <cstdint>
#include <mutex>
#include <thread>
#include <vector>

namespace mgc {
// Readers and ring: measured on the 2 x 64-core box (scripts/e2e_cli.py, 20.5 GB FASTQ on tmpfs): 6 readers / 8 slots keep
// the uploader waiting 1.7 s, 16 readers / 24 slots 0.01 s (the loop then runs at the 0.5 s of upload + parse).
// requested <= 0: 16 threads.  The ring has 8 slots more than the threads asked for (threads + 6 chunks of read-ahead at
// lag 2), within max_slots; there are never more threads than chunks.
struct ChunkRingGeometry { int threads, slots; };
inline ChunkRingGeometry chunk_ring_geometry(int requested, uint64_t n_chunks, int max_slots) {
  if (requested <= 0) requested = 16;
  requested = std::max(1, std::min(requested, max_slots - 8));
  return {(int)std::min<uint64_t>((uint64_t)requested, n_chunks ? n_chunks : 1), requested + 8};
}

struct ChunkRingResult {
  enum End { DONE, ALLOC_FAILED, FILL_FAILED, CONSUMER_STOPPED };
  End      end = DONE;        // the FIRST thing that went wrong, if any
  uint64_t chunk = 0;         // ALLOC_FAILED, FILL_FAILED, CONSUMER_STOPPED: the chunk
  int      detail = 0;        // FILL_FAILED: what fill handed back (an errno, a block number); CONSUMER_STOPPED: consume's value
  double   t_wait = 0, t_consume = 0;      // the consumer: waiting for the producers, inside consume
  double   t_fill = 0, t_slot_wait = 0;    // the producers, summed: inside fill, waiting for a free slot (first-use alloc included)
};

//   char   *alloc()                                         a slot, or null; called by the producer that first needs a null
//                                                           slots[i], at most once per slot; the slot stays with the caller
//   int64_t fill(int thread, uint64_t chunk, char *dst, int *detail)   bytes written, or < 0 (*detail says why)
//   int     consume(uint64_t chunk, const char *ptr, size_t len)       non-zero stops the pump
// After consume(c) returns 0 the slot of chunk c - lag goes back to the producers (n_slots > lag).
template <class Alloc, class Fill, class Consume>
ChunkRingResult run_chunk_ring(uint64_t n_chunks, char **slots, int n_slots, int n_threads, int lag, Alloc alloc, Fill fill, Consume consume) {
  ChunkRingResult res;
  if (n_chunks == 0) return res;
  assert(lag >= 0 && n_slots > lag);                               // a ring of lag slots or fewer never frees one: the pump would hang
  const uint64_t R = (uint64_t)n_slots;
  n_threads = (int)std::min<uint64_t>((uint64_t)std::max(1, n_threads), n_chunks);
  std::mutex mu;
  std::condition_variable cv;
  std::vector<uint64_t> free_gen(R, 0), ready_chunk(R, ~0ull);     // slot i may be filled with chunk c iff free_gen[i] == c / R
  std::vector<size_t> ready_len(R, 0);
  std::vector<double> t_fill(n_threads, 0.0), t_slot_wait(n_threads, 0.0);
  std::atomic<uint64_t> next_chunk(0);
  bool stop = false;                                               // under mu, like res.end / chunk / detail until the join
  auto stop_with = [&](ChunkRingResult::End end, uint64_t c, int detail) {       // mu held
    if (!stop) { res.end = end; res.chunk = c; res.detail = detail; }
    stop = true;
    cv.notify_all();
  };
  auto producer = [&](int t) {
    for (;;) {
      const uint64_t c = next_chunk.fetch_add(1);
      if (c >= n_chunks) return;
      const size_t slot = (size_t)(c % R);
      const double w0 = now_s();
      {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return stop || free_gen[slot] == c / R; });
        if (stop) return;
      }
      if (!slots[slot] && !(slots[slot] = alloc())) {              // first use of this slot (exactly one producer gets here per slot)
        std::lock_guard<std::mutex> g(mu);
        stop_with(ChunkRingResult::ALLOC_FAILED, c, 0);
        return;
      }
      const double w1 = now_s();
      t_slot_wait[t] += w1 - w0;
      int detail = 0;
      const int64_t len = fill(t, c, slots[slot], &detail);
      t_fill[t] += now_s() - w1;
      std::lock_guard<std::mutex> g(mu);
      if (len < 0) { stop_with(ChunkRingResult::FILL_FAILED, c, detail); return; }
      ready_chunk[slot] = c; ready_len[slot] = (size_t)len;
      cv.notify_all();
    }
  };
  std::vector<std::thread> producers;
  for (int t = 0; t < n_threads; t++) producers.emplace_back(producer, t);
  for (uint64_t c = 0; c < n_chunks; c++) {
    const size_t slot = (size_t)(c % R);
    size_t len = 0;
    const double t0 = now_s();
    {
      std::unique_lock<std::mutex> lk(mu);
      cv.wait(lk, [&] { return stop || ready_chunk[slot] == c; });
      if (stop) break;
      len = ready_len[slot];
    }
    const double t1 = now_s();
    res.t_wait += t1 - t0;
    const int rc = consume(c, slots[slot], len);
    res.t_consume += now_s() - t1;
    std::lock_guard<std::mutex> g(mu);
    if (rc) { stop_with(ChunkRingResult::CONSUMER_STOPPED, c, rc); break; }
    // The release lags the consume because the consumer reads its slots asynchronously: text_submit(c) first waits for the
    // parse of chunk c-2 (same device buffer) -- after that the pinned slot of chunk c-2 has been read by its upload.
    if (c >= (uint64_t)lag) { free_gen[(size_t)((c - lag) % R)]++; cv.notify_all(); }
  }
  { std::lock_guard<std::mutex> g(mu); stop = true; cv.notify_all(); }
  for (auto &t : producers) t.join();
  for (int t = 0; t < n_threads; t++) { res.t_fill += t_fill[t]; res.t_slot_wait += t_slot_wait[t]; }
  return res;
}
}  // namespace mgc
