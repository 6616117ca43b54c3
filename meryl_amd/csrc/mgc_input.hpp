// mgc_input.hpp -- the state of a session's piece protocol (mgc_input.cpp), held by mgc_session (mgc_session.hpp).  Internal.
//
// Text, BAM and gzip input reach the device in PIECES of at most TEXT_CHUNK bytes of pinned memory.  Piece n goes through slot
// n & 1: it is uploaded on st_up into the slot's device input buffer while piece n - 1 is decoded on st_in, and the slot's done
// event -- recorded behind the last thing piece n queued on st_in -- frees the slot, and the pinned source of the piece, for
// piece n + 2.  The whole-file readers' rings (mgc_chunk_ring.hpp, mgc_gzip_par.hpp: gz_run) count on that lag of two.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

struct mgc_session;

namespace mgc {
// A grow-only table that travels with a piece: a pinned host block and the arena buffer `dev` of the session, of the same size.
struct SideTable {
  int    dev = -1;                       // mgc_session::B_*
  char  *host = nullptr;
  size_t cap = 0;                        // bytes
  // room for `want` bytes in both; a table that has to grow is allocated anew with `grow_to` (>= want) bytes
  hipError_t reserve(mgc_session *s, size_t want, size_t grow_to);
  SideTable() = default;
  SideTable(const SideTable &) = delete;
  SideTable &operator=(const SideTable &) = delete;
  ~SideTable() { if (host) (void)hipHostFree(host); }
};

struct PieceSlot {
  int        dev_in = -1;                // the device input buffer (mgc_session::B_TEXT_IN0 / 1)
  char      *pinned = nullptr;           // TEXT_CHUNK bytes: where mgc_push_text / mgc_push_bam stage the caller's bytes
  hipEvent_t up_ev = nullptr;            // the piece's uploads are done (st_in waits for it)
  hipEvent_t done_ev = nullptr;          // everything the piece queued is done: the slot and the piece's source are free
  bool       used = false;               // done_ev has been recorded
  SideTable  bam_seg;                    // BAM: the piece's segment table (mgc_bam_walk.hpp)
  SideTable  gz_sym;                     // gzip: the symbols of the piece's unresolved prefix (mgc_gzip.hip)
  SideTable  gz_tab;                     // gzip: {begin[n], len[n], crc[n], error}, n = gz_tab_entries(): up, up, down, down
  size_t gz_tab_entries() const { return gz_tab.cap ? (gz_tab.cap - 16) / 16 : 0; }
  static size_t gz_tab_bytes(size_t entries) { return entries * 16 + 16; }
};

struct InputRing {
  static constexpr int FILE_SLOTS_MAX = 64;
  hipStream_t st_up = nullptr;           // pieces are UPLOADED here while the previous piece is decoded on st_in
  uint32_t    next = 0;                  // pieces queued so far
  PieceSlot   slot[2];
  char       *file_slots[FILE_SLOTS_MAX] = {nullptr};    // the whole-file readers' pinned slots (allocated by their producers on first use)
  // the upload stream, the slots' events and their pinned blocks of `chunk` bytes, on first use
  hipError_t setup(size_t chunk);
  // one pinned slot of `chunk` bytes for file_slots, from any thread; nullptr: out of memory
  static char *alloc_file_slot(int device, size_t chunk);
  InputRing();
  InputRing(const InputRing &) = delete;
  InputRing &operator=(const InputRing &) = delete;
  ~InputRing();
};
}  // namespace mgc
