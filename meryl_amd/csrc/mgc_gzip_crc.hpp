// mgc_gzip_crc.hpp -- the CRC ledger of the gzip input route (mgc_input.cpp: gzip_submit), host arithmetic only: no HIP, no session.
//
// The device computes the CRC-32 of every piece of text in ENTRIES of at most 4 KiB that never cross a member's end
// (mgc_gzip.hip: gz_crc32_kernel); the values come back two pieces later.  The ledger builds the table of entries of a piece,
// remembers per device input buffer what the values will mean, folds them into the running member's CRC when they arrive, holds
// CRC and length against the members' trailers, and keeps the first VERDICT (non-empty: the stream is refused).
#pragma once

#include "mgc_gzip_par.hpp"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include <zlib.h>

namespace mgc {
// crc32_combine(crc1, crc2, 4096) without zlib's work: zlib squares a 32 x 32 GF(2) matrix some fifteen times per call (tens of
// microseconds in zlib 1.2), and a 32 MiB piece brings 8192 values.  Nearly every CRC entry is exactly 4096 bytes, so the operator
// "append 4096 zero bytes" is built once -- the one-zero-bit operator squared fifteen times -- and applied in at most 32 steps.
inline uint32_t gf2_times(const uint32_t *mat, uint32_t vec) {
  uint32_t sum = 0;
  for (; vec; vec >>= 1, mat++) if (vec & 1u) sum ^= *mat;
  return sum;
}
inline uint32_t crc32_combine_4096(uint32_t crc1, uint32_t crc2) {
  static const struct Op {
    uint32_t m[32];
    Op() {
      uint32_t a[32], b[32];
      a[0] = 0xedb88320u;                                    // one zero bit
      for (int n = 1; n < 32; n++) a[n] = 1u << (n - 1);
      for (int sq = 0; sq < 15; sq++) {                      // 2^15 bits = 4096 bytes
        for (int n = 0; n < 32; n++) b[n] = gf2_times(a, a[n]);
        memcpy(a, b, sizeof(a));
      }
      memcpy(m, a, sizeof(m));
    }
  } op;
  return gf2_times(op.m, crc1) ^ crc2;
}

struct GzCrcLedger {
  struct Entry { uint32_t len; int32_t end; };            // one entry of a piece's table; end >= 0: a member ends after it (ends[b][end])
  struct End { uint32_t crc, isize; uint64_t comp_off; };
  std::vector<Entry> pending[2];                          // what the values of the piece in device input buffer b will mean
  std::vector<End>   ends[2];
  uint64_t    piece_off[2] = {0, 0};                      // where in the file that piece starts (for the verdict)
  uint32_t    crc = 0;                                    // of the running member, over the entries collected so far
  uint64_t    member_len = 0, members = 0;
  std::string verdict;                                    // non-empty: the stream is refused

  bool refused() const { return !verdict.empty(); }
  void forget_pending() { for (int b = 0; b < 2; b++) { pending[b].clear(); ends[b].clear(); } }
  void reset() { forget_pending(); crc = 0; member_len = 0; members = 0; verdict.clear(); }

  // entries a table of `piece` bytes with n_ends member ends may need room for (the builder makes at most piece / 4096 + n_ends + 1)
  static size_t table_room(uint64_t piece, size_t n_ends) { return (size_t)(piece / 4096) + 2 * n_ends + 2; }

  // The table of the piece that goes through buffer b: begin[i], len[i] tile [0, piece) in order, no entry is longer than 4096
  // bytes or crosses a member's end (member_ends[e].text_off), a member end with no text since the previous boundary gets one
  // entry of 0 bytes.  Returns the number of entries; -1, and nothing remembered, for ends out of order or beyond the piece or
  // more than `room` entries.
  long build_table(int b, uint64_t piece, const GzMemberEnd *member_ends, size_t n_ends, uint64_t comp_off, uint64_t *begin, uint32_t *len,
                   size_t room) {
    uint64_t prev = 0;
    for (size_t e = 0; e < n_ends; e++) {
      if (member_ends[e].text_off < prev || member_ends[e].text_off > piece) return -1;
      prev = member_ends[e].text_off;
    }
    if (table_room(piece, n_ends) > room) return -1;
    piece_off[b] = comp_off;
    size_t n = 0;
    uint64_t at = 0;
    for (size_t e = 0; e <= n_ends; e++) {
      const uint64_t stop = e < n_ends ? member_ends[e].text_off : piece;
      do {                                                  // (a member end with no text before it: one entry of 0 bytes)
        const uint32_t l = (uint32_t)std::min<uint64_t>(4096, stop - at);
        if (e == n_ends && l == 0) break;
        begin[n] = at; len[n] = l;
        at += l;
        pending[b].push_back({l, (e < n_ends && at == stop) ? (int32_t)ends[b].size() : -1});
        n++;
      } while (at < stop);
      if (e < n_ends) ends[b].push_back({member_ends[e].crc, member_ends[e].isize, member_ends[e].comp_off});
    }
    return (long)n;
  }

  // a member's trailer against the running member; the next member begins
  void close_member(const End &e, bool exact_words) {
    if (verdict.empty() && (crc != e.crc || (uint32_t)member_len != e.isize)) {
      char msg[200];
      if (!exact_words) snprintf(msg, sizeof(msg), "CRC32 / ISIZE mismatch (member %llu, trailer at compressed offset %llu)", (unsigned long long)members,
                                 (unsigned long long)e.comp_off);
      else if (crc != e.crc) snprintf(msg, sizeof(msg), "CRC32 mismatch (member %llu, trailer at compressed offset %llu: %08x, text %08x)",
                                      (unsigned long long)members, (unsigned long long)e.comp_off, e.crc, crc);
      else snprintf(msg, sizeof(msg), "ISIZE mismatch (member %llu, trailer at compressed offset %llu: %u, text %llu bytes)",
                    (unsigned long long)members, (unsigned long long)e.comp_off, e.isize, (unsigned long long)member_len);
      verdict = msg;
    }
    crc = 0; member_len = 0; members++;
  }

  // The values of the piece that went through buffer b have arrived -- values[i] of table entry i, and the device's error word:
  // fold them into the running member's CRC and hold every member that ends in the piece against its trailer.
  void collect(int b, const uint32_t *values, uint32_t dev_err) {
    if (pending[b].empty()) return;
    if (dev_err && verdict.empty()) {
      char msg[200];
      snprintf(msg, sizeof(msg), "%s (in the piece that starts at compressed offset %llu)",
               (dev_err & 2u) ? "a back-reference reaches before the start of its gzip member" : "the inflaters produced an invalid symbol",
               (unsigned long long)piece_off[b]);
      verdict = msg;
    }
    for (size_t i = 0; i < pending[b].size(); i++) {
      const Entry &p = pending[b][i];
      crc = p.len == 4096 ? crc32_combine_4096(crc, values[i]) : (uint32_t)crc32_combine(crc, values[i], (z_off_t)p.len);
      member_len += p.len;
      if (p.end >= 0) close_member(ends[b][(size_t)p.end], true);
    }
    pending[b].clear();
    ends[b].clear();
  }

  // member ends that arrive with no text (an empty member, the end of the file), everything before them collected
  void empty_piece(const GzMemberEnd *member_ends, size_t n_ends) {
    for (size_t i = 0; i < n_ends; i++) close_member({member_ends[i].crc, member_ends[i].isize, member_ends[i].comp_off}, false);
  }
};
}  // namespace mgc
