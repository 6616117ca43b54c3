// mgc_gzip_par.hpp -- ONE plain gzip stream inflated by several threads (the two-pass shape of pugz / rapidgzip), host-only:
// no HIP, no session, zlib only for the header's CRC16.  The second pass -- resolving what a thread could not know -- is left
// to whoever receives the pieces in stream order (the device: mgc_gzip.hip; tests/host/gzip_host.cpp does it on the CPU).
//
// The compressed file is cut into SPANS of `span` bytes.  The worker of span c > 0 looks for a deflate block start in its span
// (gz_find_block: a non-final dynamic or stored block whose header holds up and that inflates for a stretch), publishes that
// CANDIDATE and inflates from there with an inflater of its own that writes 16-bit SYMBOLS: 0..255 are bytes, 0x8000 + o is
// "byte o of the 32 KiB before my start" (o = 32767: the byte just before it).  A back-reference that copies a marker copies
// the marker, so every unresolved symbol names a window byte directly.  A worker stops at the first block boundary at or after
// its span's end that IS the next span's candidate; when it passes a candidate without meeting it the candidate was false, the
// worker goes on through that span too and the other worker's output is thrown away.  Nothing is believed: the consumer takes
// the pieces strictly in stream order and takes a worker's output only when the piece before it ended exactly at its start, so
// what is handed on is exact whatever the finder guessed (a file of fixed blocks only inflates serially and is still right).
//
// A PIECE is at most `cap` bytes of text in one slot (a pinned upload buffer), cut at the last block boundary that fit; the
// rest of the worker's output is a continuation in another slot.  Beside the text a piece keeps the symbols of its unresolved
// prefix [0, m_end), m_end one past its last marker: at most 2 bytes per text byte.  Once 32 KiB without a marker lie behind a
// worker it writes bytes straight into the slot.  Slots come from a pool; the last lag + 1 free slots are kept for the task the
// consumer is waiting for, so that workers that ran ahead can never starve it (see where a worker takes its slot).
//
// What holds (tests/host/gzip_host.cpp runs it under the thread and address sanitizers):
//   - pieces reach `consume` in stream order, each at most once, none after a failure was noticed;
//   - a slot is written again only `lag` pieces after its consume returned;
//   - on return every thread is joined and no slot is written again.
#pragma once

#include "mgc_clock.hpp"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <deque>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#include <zlib.h>

namespace mgc {
constexpr uint32_t GZ_WINDOW = 32768;
constexpr uint16_t GZ_MARK   = 0x8000;
constexpr uint64_t GZ_NONE   = ~0ull;

// ---- bits, least significant first, over a mapping that is never read past its end -------------------------------------------
struct GzBits {
  const uint8_t *base = nullptr;
  uint64_t size = 0, ip = 0, bb = 0;      // bytes; next byte to load; the bit buffer
  uint32_t bc = 0;                        // bits in bb
  void seek(uint64_t bit) {
    ip = std::min(bit >> 3, size); bb = 0; bc = 0;
    const uint32_t skip = (uint32_t)(bit & 7);
    if (skip && ip < size) { bb = (uint64_t)base[ip++] >> skip; bc = 8 - skip; }
  }
  uint64_t pos() const { return ip * 8 - bc; }
  void refill() {
    if (ip + 8 <= size) {
      uint64_t w;
      memcpy(&w, base + ip, 8);           // (little-endian hosts)
      bb |= w << bc;
      const uint32_t take = (63 - bc) >> 3;
      ip += take; bc += take * 8;
    } else {
      while (bc <= 56 && ip < size) { bb |= (uint64_t)base[ip++] << bc; bc += 8; }
    }
  }
  // n <= 32 bits; false: the mapping ends first
  bool need(uint32_t n) { if (bc < n) refill(); return bc >= n; }
  uint32_t peek(uint32_t n) const { return (uint32_t)(bb & ((1ull << n) - 1)); }
  void drop(uint32_t n) { bb >>= n; bc -= n; }
  bool take(uint32_t n, uint32_t *v) { if (!need(n)) return false; *v = peek(n); drop(n); return true; }
  void align() { drop(bc & 7); }
};

// ---- a canonical Huffman code: a table for codes of up to FAST bits, counts + sorted symbols for the longer ones ------------------
struct GzCode {
  static constexpr int FAST = 10;
  uint16_t fast[1 << FAST];               // (symbol << 4) | length, 0: longer than FAST bits
  uint16_t count[16], symbol[288];
  int      left = 0;                      // unused code space: 0 complete, < 0 oversubscribed
  // lengths[n]; tables only when `tables`
  void build(const uint8_t *lengths, int n, bool tables) {
    memset(count, 0, sizeof(count));
    for (int i = 0; i < n; i++) count[lengths[i]]++;
    left = 1;
    for (int l = 1; l <= 15; l++) { left <<= 1; left -= count[l]; if (left < 0) return; }
    if (!tables) return;
    uint16_t offs[16], next[16];
    offs[1] = 0;
    for (int l = 1; l < 15; l++) offs[l + 1] = (uint16_t)(offs[l] + count[l]);
    for (int i = 0; i < n; i++) if (lengths[i]) symbol[offs[lengths[i]]++] = (uint16_t)i;
    uint32_t code = 0;
    next[0] = 0;
    for (int l = 1; l <= 15; l++) { code = (code + (l > 1 ? count[l - 1] : 0u)) << 1; next[l] = (uint16_t)code; }
    memset(fast, 0, sizeof(fast));
    for (int i = 0; i < n; i++) {
      const int l = lengths[i];
      if (!l || l > FAST) { if (l) next[l]++; continue; }
      uint32_t c = next[l]++, r = 0;
      for (int b = 0; b < l; b++) r |= ((c >> b) & 1u) << (l - 1 - b);
      for (uint32_t k = r; k < (1u << FAST); k += 1u << l) fast[k] = (uint16_t)((i << 4) | l);
    }
  }
  // the next symbol, or -1 (no such code, or the mapping ends)
  int decode(GzBits &b) const {
    if (b.bc < 15) b.refill();
    const uint16_t e = fast[b.bb & ((1u << FAST) - 1)];
    if (e) { const uint32_t l = e & 15u; if (b.bc < l) return -1; b.drop(l); return e >> 4; }
    int code = 0, first = 0, index = 0;
    uint64_t bits = b.bb;
    for (uint32_t l = 1; l <= 15; l++) {
      if (b.bc < l) return -1;
      code |= (int)(bits & 1); bits >>= 1;
      const int cnt = count[l];
      if (code - cnt < first) { b.drop(l); return symbol[index + (code - first)]; }
      index += cnt; first += cnt; first <<= 1; code <<= 1;
    }
    return -1;
  }
};

enum GzErr { GZ_OK = 0, GZ_E_END /* the mapping ends inside the stream */, GZ_E_BTYPE, GZ_E_STORED, GZ_E_LENGTHS, GZ_E_SYMBOL, GZ_E_DISTANCE,
             GZ_E_FAR /* a reference before the window or the member's start */, GZ_E_HEADER, GZ_E_BIG /* one block that no slot holds */, GZ_E_ORDER /* a piece that does not start where the one before it ended */,
             GZ_OVERFLOW /* not an error: the block does not fit the buffer */ };
inline const char *gz_err_text(int e) {
  static const char *t[] = {"ok", "the file ends inside the stream", "invalid block type", "stored block: LEN != ~NLEN", "invalid code lengths",
                            "invalid literal/length symbol", "invalid distance code", "a back-reference reaches before the start of the member",
                            "invalid gzip header", "one deflate block is larger than a whole upload buffer",
                            "internal: a piece does not start where the piece before it ended", "overflow"};
  return e >= 0 && e <= GZ_OVERFLOW ? t[e] : "?";
}

struct GzTables { GzCode lit, dist; };

// the dynamic block header at b (after its 3 header bits): the two codes, every length checked.  tables: build decode tables too
inline GzErr gz_read_dynamic(GzBits &b, GzTables &t, bool tables) {
  static const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  uint32_t hlit, hdist, hclen, v;
  if (!b.take(5, &hlit) || !b.take(5, &hdist) || !b.take(4, &hclen)) return GZ_E_END;
  const int nlen = (int)hlit + 257, ndist = (int)hdist + 1, ncode = (int)hclen + 4;
  if (nlen > 286 || ndist > 30) return GZ_E_LENGTHS;
  uint8_t lengths[320];
  memset(lengths, 0, 19);
  for (int i = 0; i < ncode; i++) { if (!b.take(3, &v)) return GZ_E_END; lengths[order[i]] = (uint8_t)v; }
  GzCode &cl = t.dist;                                      // (the code-length code borrows the distance code's tables)
  cl.build(lengths, 19, true);
  if (cl.left != 0) return GZ_E_LENGTHS;                    // the code-length code must be complete
  int i = 0;
  while (i < nlen + ndist) {
    const int sym = cl.decode(b);
    if (sym < 0) return b.ip >= b.size ? GZ_E_END : GZ_E_LENGTHS;
    if (sym < 16) { lengths[i++] = (uint8_t)sym; continue; }
    uint32_t rep, prev = 0;
    if (sym == 16) { if (i == 0) return GZ_E_LENGTHS; prev = lengths[i - 1]; if (!b.take(2, &rep)) return GZ_E_END; rep += 3; }
    else if (sym == 17) { if (!b.take(3, &rep)) return GZ_E_END; rep += 3; }
    else { if (!b.take(7, &rep)) return GZ_E_END; rep += 11; }
    if (i + (int)rep > nlen + ndist) return GZ_E_LENGTHS;
    while (rep--) lengths[i++] = (uint8_t)prev;
  }
  if (lengths[256] == 0) return GZ_E_LENGTHS;               // no end-of-block code
  uint8_t dl[32];
  memcpy(dl, lengths + nlen, (size_t)ndist);
  t.lit.build(lengths, nlen, tables);
  // over-subscribed, or incomplete -- but for the single code of one bit, which zlib lets pass here as well (it is code 256: an empty block)
  if (t.lit.left < 0 || (t.lit.left > 0 && !(nlen - t.lit.count[0] == 1 && t.lit.count[1] == 1))) return GZ_E_LENGTHS;
  t.dist.build(dl, ndist, tables);
  // an incomplete distance code is allowed only as the single code of one bit (zlib does the same)
  if (t.dist.left < 0 || (t.dist.left > 0 && !(ndist - t.dist.count[0] == 1 && t.dist.count[1] == 1) && ndist - t.dist.count[0] != 0)) return GZ_E_LENGTHS;
  return GZ_OK;
}

inline const GzTables &gz_fixed_tables() {
  static const GzTables *fixed = [] {
    GzTables *t = new GzTables;
    uint8_t l[288];
    for (int i = 0; i < 288; i++) l[i] = i < 144 ? 8 : (i < 256 ? 9 : (i < 280 ? 7 : 8));
    t->lit.build(l, 288, true);
    for (int i = 0; i < 30; i++) l[i] = 5;
    t->dist.build(l, 30, true);
    return t;
  }();
  return *fixed;
}

// The symbols of one block's codes into out[*pos ...], T = uint16_t (markers allowed) or uint8_t.  mb: where in `out` the current
// member began, -1: before out[0] -- then a reference reaches up to GZ_WINDOW symbols before out[0] and becomes a marker.
template <class T>
inline GzErr gz_inflate_codes(GzBits &b, const GzTables &t, T *out, uint64_t *pos_io, uint64_t cap, int64_t mb) {
  static const uint16_t lbase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
  static const uint8_t  lext[29]  = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
  static const uint16_t dbase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
  static const uint8_t  dext[30]  = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
  uint64_t pos = *pos_io;
  for (;;) {
    int sym = t.lit.decode(b);
    if (sym < 0) { *pos_io = pos; return b.ip >= b.size ? GZ_E_END : GZ_E_SYMBOL; }
    if (sym < 256) {
      if (pos >= cap) return GZ_OVERFLOW;
      out[pos++] = (T)sym;
      continue;
    }
    if (sym == 256) break;
    sym -= 257;
    if (sym >= 29) return GZ_E_SYMBOL;                       // 286, 287
    uint32_t ext = 0, dx = 0;
    if (lext[sym] && !b.take(lext[sym], &ext)) return GZ_E_END;
    const uint32_t len = lbase[sym] + ext;
    const int ds = t.dist.decode(b);
    if (ds < 0) return b.ip >= b.size ? GZ_E_END : GZ_E_DISTANCE;
    if (ds >= 30) return GZ_E_DISTANCE;                      // 30, 31
    if (dext[ds] && !b.take(dext[ds], &dx)) return GZ_E_END;
    const uint64_t d = dbase[ds] + dx;
    if (pos + len > cap) return GZ_OVERFLOW;
    if (mb >= 0 ? d > pos - (uint64_t)mb : d > pos + GZ_WINDOW) return GZ_E_FAR;
    if (d <= pos) {
      const T *src = out + (pos - d);
      T *dst = out + pos;
      if (d >= len) memcpy(dst, src, len * sizeof(T));
      else for (uint32_t k = 0; k < len; k++) dst[k] = src[k];
    } else if (sizeof(T) == 1) {
      return GZ_E_FAR;                                       // (bytes are written only where no marker can arise)
    } else {
      for (uint32_t k = 0; k < len; k++) {
        const uint64_t at = pos + k;
        out[at] = at >= d ? out[at - d] : (T)(GZ_MARK + (GZ_WINDOW - (d - at)));
      }
    }
    pos += len;
  }
  *pos_io = pos;
  return GZ_OK;
}

// One block at b -- b stands at its 3 header bits, or (stored_at_len) at the LEN of a non-final stored block.  *final: BFINAL.
// GZ_OVERFLOW leaves b and *pos_io to the caller to restore.
template <class T>
inline GzErr gz_inflate_block(GzBits &b, GzTables &scratch, bool stored_at_len, T *out, uint64_t *pos_io, uint64_t cap, int64_t mb, bool *final) {
  uint32_t hdr = 0;
  if (!stored_at_len) { if (!b.take(3, &hdr)) return GZ_E_END; }
  *final = (hdr & 1u) != 0;
  const uint32_t type = hdr >> 1;
  if (type == 3) return GZ_E_BTYPE;
  if (type == 0) {
    b.align();
    uint32_t len, nlen;
    if (!b.take(16, &len) || !b.take(16, &nlen)) return GZ_E_END;
    if (len != (~nlen & 0xffffu)) return GZ_E_STORED;
    uint64_t at = b.pos() >> 3;                              // the bit buffer holds whole bytes here: hand them back
    if (at + len > b.size) return GZ_E_END;
    if (*pos_io + len > cap) return GZ_OVERFLOW;
    for (uint32_t k = 0; k < len; k++) out[*pos_io + k] = (T)b.base[at + k];
    *pos_io += len;
    b.seek((at + len) * 8);
    return GZ_OK;
  }
  if (type == 1) return gz_inflate_codes<T>(b, gz_fixed_tables(), out, pos_io, cap, mb);
  const GzErr e = gz_read_dynamic(b, scratch, true);
  if (e != GZ_OK) return e;
  return gz_inflate_codes<T>(b, scratch, out, pos_io, cap, mb);
}

// ---- gzip member header / trailer ---------------------------------------------------------------------------------------------
// the header at byte `at`: *data = where the deflate data starts.  GZ_E_HEADER / GZ_E_END
inline GzErr gz_parse_header(const uint8_t *p, uint64_t size, uint64_t at, uint64_t *data) {
  if (at + 10 > size) return (at + 2 <= size && (p[at] != 0x1f || p[at + 1] != 0x8b)) ? GZ_E_HEADER : GZ_E_END;
  if (p[at] != 0x1f || p[at + 1] != 0x8b || p[at + 2] != 8 || (p[at + 3] & 0xe0)) return GZ_E_HEADER;
  const uint32_t flg = p[at + 3];
  uint64_t o = at + 10;
  if (flg & 4) { if (o + 2 > size) return GZ_E_END; o += 2 + ((uint64_t)p[o] | ((uint64_t)p[o + 1] << 8)); if (o > size) return GZ_E_END; }
  for (int f = 8; f <= 16; f <<= 1)                          // FNAME, FCOMMENT: zero-terminated
    if (flg & f) { while (o < size && p[o]) o++; if (o >= size) return GZ_E_END; o++; }
  if (flg & 2) {                                             // FHCRC: the low 16 bits of the header's CRC-32
    if (o + 2 > size) return GZ_E_END;
    const uint32_t want = (uint32_t)p[o] | ((uint32_t)p[o + 1] << 8);
    if ((crc32(0L, p + at, (uInt)(o - at)) & 0xffffu) != want) return GZ_E_HEADER;
    o += 2;
  }
  *data = o;
  return GZ_OK;
}

// 1: the n bytes at p begin a gzip member
inline bool gz_is_gzip(const uint8_t *p, size_t n) { return n >= 10 && p[0] == 0x1f && p[1] == 0x8b && p[2] == 8 && !(p[3] & 0xe0); }

// ---- where a piece may start ---------------------------------------------------------------------------------------------------
// A block start is known by its KEY: the bit of its header for a coded block, the byte of its LEN for a stored one (whose header
// bits are followed by padding, so the finder cannot tell which bit they began at).  GZ_NONE: no key (a final block never has one).
inline uint64_t gz_key_dynamic(uint64_t bit) { return bit << 1; }
inline uint64_t gz_key_stored(uint64_t len_byte) { return (len_byte << 4) | 1u; }
inline uint64_t gz_key_at(const uint8_t *p, uint64_t size, uint64_t bit) {
  GzBits b; b.base = p; b.size = size; b.seek(bit);
  uint32_t hdr;
  if (!b.take(3, &hdr) || (hdr & 1u)) return GZ_NONE;
  return (hdr >> 1) == 0 ? gz_key_stored((bit + 3 + 7) >> 3) : gz_key_dynamic(bit);
}

// Inflates from a candidate for a stretch -- three blocks, the end of the member or 64 Ki symbols, whichever comes first -- into
// scratch that is thrown away; false: an error turned up
inline bool gz_trial(const uint8_t *p, uint64_t size, uint64_t key, GzTables &tabs, uint16_t *scratch, uint64_t scratch_n) {
  GzBits b; b.base = p; b.size = size;
  bool stored = (key & 1u) != 0;
  b.seek(stored ? (key >> 4) * 8 : key >> 1);
  uint64_t pos = 0;
  for (int blocks = 0; blocks < 3; blocks++) {
    bool final = false;
    const GzErr e = gz_inflate_block<uint16_t>(b, tabs, stored, scratch, &pos, scratch_n, -1, &final);
    stored = false;
    if (e == GZ_OVERFLOW) return true;
    if (e != GZ_OK) return false;
    if (final) return true;
  }
  return true;
}

// The first candidate whose key position lies in bytes [from, to) of the mapping, or GZ_NONE.  Fixed blocks have no header to
// test and are not searched for.
inline uint64_t gz_find_block(const uint8_t *p, uint64_t size, uint64_t from, uint64_t to, GzTables &tabs, uint16_t *scratch, uint64_t scratch_n) {
  to = std::min(to, size);
  GzBits b; b.base = p; b.size = size;
  for (uint64_t byte = from; byte < to; byte++) {
    // a stored block's LEN / NLEN here (its header bits lie in the byte before: that byte's top 3 bits, at the least, are zero)
    if (byte >= 1 && byte + 4 <= size && !(p[byte - 1] & 0xe0)) {
      const uint32_t len = (uint32_t)p[byte] | ((uint32_t)p[byte + 1] << 8), nlen = (uint32_t)p[byte + 2] | ((uint32_t)p[byte + 3] << 8);
      if (len == (~nlen & 0xffffu) && gz_trial(p, size, gz_key_stored(byte), tabs, scratch, scratch_n)) return gz_key_stored(byte);
    }
    uint64_t w = 0;
    if (byte + 8 <= size) memcpy(&w, p + byte, 8); else memcpy(&w, p + byte, (size_t)(size - byte));
    for (uint32_t s = 0; s < 8; s++) {
      const uint32_t h = (uint32_t)(w >> s);
      // BFINAL 0, BTYPE 10, HLIT <= 29, HDIST <= 29
      if ((h & 7u) != 4u || ((h >> 3) & 31u) > 29u || ((h >> 8) & 31u) > 29u) continue;
      const uint64_t bit = byte * 8 + s;
      b.seek(bit + 3);
      if (gz_read_dynamic(b, tabs, false) != GZ_OK) continue;
      if (gz_trial(p, size, gz_key_dynamic(bit), tabs, scratch, scratch_n)) return gz_key_dynamic(bit);
    }
  }
  return GZ_NONE;
}

// ---- pieces ----------------------------------------------------------------------------------------------------------------------
struct GzMemberEnd { uint64_t text_off; uint32_t crc, isize; uint64_t comp_off; };    // the member ends before text_off of the piece
struct GzPiece {
  int       slot = -1;
  uint64_t  start_bit = 0, end_bit = 0;          // compressed position
  bool      at_header = false;                   // it starts at a member's gzip header (no window at all)
  uint64_t  text_len = 0;
  std::vector<uint16_t> symbols;                 // of the unresolved prefix [0, symbols.size())
  std::vector<GzMemberEnd> ends;
  int       err = GZ_OK; uint64_t err_bit = 0;
  bool      last = false;                        // the last piece of its task
  bool      stream_end = false;                  // ... and of the file
  uint64_t  next_span = GZ_NONE;                 // last && !stream_end: the span whose candidate the task stopped at
  uint64_t  end_key = GZ_NONE;                   // ... and the key of the block boundary it stopped at
  bool      end_at_header = false;               // end_bit is a member's gzip header (byte end_bit / 8)
};

struct GzOptions {
  uint64_t span = 4u << 20, cap = 32u << 20;
  int threads = 16, n_slots = 24, lag = 2;
  uint64_t force_span = GZ_NONE, force_bit = 0;  // tests: span force_span's candidate is the coded block "at" this bit, unsearched
  int delay_span0_ms = 0;                        // tests: the worker of span 0 sleeps this long before it takes a slot (a head that falls behind)
};

struct GzInfo { uint64_t members = 0, chunks = 0, confirmed = 0, discarded = 0, text_bytes = 0, symbol_bytes = 0, cuts = 0; };

struct GzResult {
  enum End { DONE, ALLOC_FAILED, FORMAT, CONSUMER_STOPPED };
  End end = DONE;
  int detail = 0;                                // FORMAT: a GzErr; CONSUMER_STOPPED: consume's value
  uint64_t offset = 0;                           // FORMAT: the compressed byte
  GzInfo info;
  double t_wait = 0, t_consume = 0;              // the consumer: waiting for the workers, inside consume
  double t_find = 0, t_inflate = 0, t_confirm = 0, t_slot_wait = 0;   // the workers, summed
};

struct GzPieceView {
  const char *text; uint64_t text_len;
  const uint16_t *symbols; uint64_t n_symbols;
  uint32_t window_valid;                         // bytes of the piece's member that precede it, at most GZ_WINDOW
  const GzMemberEnd *ends; size_t n_ends;
  uint64_t comp_off;                             // where the piece starts in the file (bytes)
};

//   char *alloc()                       a slot of opt.cap bytes, or null; called by the worker that first needs slots[i]
//   int   consume(const GzPieceView &)  non-zero stops the pump
template <class Alloc, class Consume>
GzResult gz_run(const uint8_t *map, uint64_t size, const GzOptions &opt, char **slots, Alloc alloc, Consume consume) {
  GzResult res;
  const uint64_t span = std::max<uint64_t>(opt.span, 1024), cap = opt.cap;
  const uint64_t n_spans = std::max<uint64_t>(1, size / span);           // whole spans: the last one takes the file's tail with it
  const int n_slots = std::max(opt.n_slots, opt.lag + 3);                // the head's lag + 1, and one for a worker that runs ahead
  const int n_threads = (int)std::min<uint64_t>((uint64_t)std::max(1, opt.threads), n_spans);

  struct Task {
    int cand_state = 0;                          // 0: not looked for, 1: someone is looking, 2: known
    uint64_t cand = GZ_NONE;
    std::deque<std::unique_ptr<GzPiece>> pieces; // finished, not yet taken by the consumer
    bool done = false, abandoned = false;
  };
  std::vector<Task> tasks(n_spans);
  std::mutex mu;
  std::condition_variable cv;
  std::vector<int> free_slots;
  for (int i = n_slots - 1; i >= 0; i--) free_slots.push_back(i);
  uint64_t head = 0;                             // the task the consumer waits for
  bool stop = false;
  std::atomic<uint64_t> next_task(0);
  std::vector<double> t_find(n_threads, 0.0), t_inflate(n_threads, 0.0), t_confirm(n_threads, 0.0), t_slot(n_threads, 0.0);

  struct Scratch { GzTables tabs; std::unique_ptr<uint16_t[]> trial, sym; };
  constexpr uint64_t TRIAL_N = 1u << 16;

  // the candidate of span n, found by whoever needs it first
  auto candidate = [&](uint64_t n, Scratch &sc, int t) -> uint64_t {
    {
      std::unique_lock<std::mutex> lk(mu);
      Task &k = tasks[n];
      if (k.cand_state == 1) { const double w0 = now_s(); cv.wait(lk, [&] { return k.cand_state == 2; }); t_confirm[t] += now_s() - w0; }
      if (k.cand_state == 2) return k.cand;
      k.cand_state = 1;
    }
    const double f0 = now_s();
    uint64_t c;
    if (n == opt.force_span) c = gz_key_dynamic(opt.force_bit);
    else c = gz_find_block(map, size, n * span, (n + 1) * span, sc.tabs, sc.trial.get(), TRIAL_N);
    t_find[t] += now_s() - f0;
    std::lock_guard<std::mutex> g(mu);
    tasks[n].cand = c; tasks[n].cand_state = 2;
    cv.notify_all();
    return c;
  };

  auto worker = [&](int t) {
    Scratch sc;
    sc.trial.reset(new uint16_t[TRIAL_N]);
    // Host memory beside the slots: 2 * cap bytes of address space per worker, touched as far as markers reach -- for FASTQ that is the
    // whole piece -- and every finished piece keeps a copy of its prefix (GzPiece::symbols) until it is consumed: with 16 workers and
    // 32 MiB pieces of FASTQ about 1 GiB of pageable memory is written twice.  Symbols written once, into pinned memory, is the remedy.
    sc.sym.reset(new uint16_t[cap]);
    for (;;) {
      const uint64_t c = next_task.fetch_add(1);
      if (c >= n_spans) return;
      Task &task = tasks[c];
      { std::lock_guard<std::mutex> g(mu); if (stop) return; if (task.abandoned) { task.done = true; continue; } }
      // where the task starts
      bool at_header = c == 0, stored_at_len = false;
      uint64_t bit = 0;
      if (c > 0) {
        const uint64_t key = candidate(c, sc, t);
        if (key == GZ_NONE) { std::lock_guard<std::mutex> g(mu); task.done = true; cv.notify_all(); continue; }
        stored_at_len = (key & 1u) != 0;
        bit = stored_at_len ? (key >> 4) * 8 : key >> 1;
      }
      uint64_t n = c + 1;                                              // the next span whose candidate may lie ahead
      bool task_over = false;
      while (!task_over) {
        // ---- one piece ----
        int slot = -1;
        {
          if (c == 0 && opt.delay_span0_ms > 0) std::this_thread::sleep_for(std::chrono::milliseconds(opt.delay_span0_ms));
          const double w0 = now_s();
          std::unique_lock<std::mutex> lk(mu);
          // The last lag + 1 free slots are the head task's.  The consumer gives a slot back only when it holds more than `lag` consumed
          // ones, so a head that waits here with no slot free has all lag + 1 of them in pieces that are queued or consumed: once its queue
          // is drained the consumer holds lag + 1 and frees one.  (With only one slot kept back the head could wait for ever behind
          // workers that ran ahead while the consumer held `lag` slots it would never exceed.)
          cv.wait(lk, [&] { return stop || task.abandoned || (int)free_slots.size() > opt.lag + 1 || (head == c && !free_slots.empty()); });
          t_slot[t] += now_s() - w0;
          if (stop) return;
          if (task.abandoned) { task.done = true; cv.notify_all(); break; }
          slot = free_slots.back(); free_slots.pop_back();
        }
        if (!slots[slot] && !(slots[slot] = alloc())) {
          std::lock_guard<std::mutex> g(mu);
          if (!stop) res.end = GzResult::ALLOC_FAILED;
          stop = true; cv.notify_all();
          return;
        }
        const double i0 = now_s();
        std::unique_ptr<GzPiece> pc(new GzPiece);
        pc->slot = slot; pc->start_bit = bit; pc->at_header = at_header;
        uint8_t *text = reinterpret_cast<uint8_t *>(slots[slot]);
        uint16_t *sym = sc.sym.get();
        bool bytes_mode = false;                                       // true: text[] is written directly
        uint64_t pos = 0, m_end = 0, n_blocks = 0;
        int64_t mb = -1;
        GzBits b; b.base = map; b.size = size;
        if (!at_header) b.seek(bit);
        auto fail = [&](int e, uint64_t where) { pc->err = e; pc->err_bit = where; pc->last = true; task_over = true; };
        for (;;) {
          // -- a block boundary: bit (at_header: a member's header at byte bit / 8) --
          if (at_header) {
            const uint64_t at = bit >> 3;
            uint64_t data = 0;
            // after the last member: the end of the file, or bytes that are no gzip member (ignored, as zlib's gzread does)
            if (at > 0 && (at + 2 > size || map[at] != 0x1f || map[at + 1] != 0x8b)) { pc->last = pc->stream_end = true; task_over = true; break; }
            const GzErr e = gz_parse_header(map, size, at, &data);
            if (e != GZ_OK) { fail(e, bit); break; }
            bit = data * 8; at_header = false; stored_at_len = false;
            b.seek(bit);
            mb = (int64_t)pos;
            if (pos == 0) bytes_mode = true;                           // nothing before it can be referenced: no marker can arise
          }
          const uint64_t reach = (bit + 10) >> 3;                      // (a stored block's key lies up to a byte past its header bits)
          if (!stored_at_len && n < n_spans && reach >= n * span) {
            // confirmation: is this boundary the candidate of a span we have entered?
            const uint64_t here = gz_key_at(map, size, bit);
            bool met = false;
            while (n < n_spans && reach >= n * span) {
              const uint64_t cd = candidate(n, sc, t);
              const uint64_t cd_bit = cd == GZ_NONE ? 0 : ((cd & 1u) ? (cd >> 4) * 8 : cd >> 1);
              if (cd != GZ_NONE && cd == here) { met = true; break; }
              if (cd != GZ_NONE && cd_bit > bit) break;                // still ahead
              n++;                                                     // none, false, or passed: through that span as well
            }
            if (met) { pc->last = true; pc->next_span = n; pc->end_key = here; task_over = true; break; }
          }
          { std::lock_guard<std::mutex> g(mu); if (stop || task.abandoned) { task_over = true; pc->err = -1; break; } }
          // -- the block --
          const GzBits b0 = b;
          const uint64_t pos0 = pos;
          bool final = false;
          GzErr e = bytes_mode ? gz_inflate_block<uint8_t>(b, sc.tabs, stored_at_len, text, &pos, cap, mb, &final)
                               : gz_inflate_block<uint16_t>(b, sc.tabs, stored_at_len, sym, &pos, cap, mb, &final);
          if (e == GZ_OVERFLOW) {
            if (n_blocks == 0) { fail(GZ_E_BIG, bit); break; }
            b = b0; pos = pos0;                                        // cut here: the rest is a continuation with a known start
            break;
          }
          if (e != GZ_OK) { fail(e, b.pos()); break; }
          stored_at_len = false;
          n_blocks++;
          if (!bytes_mode) {
            for (uint64_t i = pos; i > pos0 && i > m_end; i--) if (sym[i - 1] >= GZ_MARK) { m_end = i; break; }
            if (pos - m_end >= GZ_WINDOW || (mb >= 0 && (uint64_t)mb >= m_end)) {
              for (uint64_t i = 0; i < pos; i++) text[i] = (uint8_t)sym[i];
              pc->symbols.assign(sym, sym + m_end);
              bytes_mode = true;
            }
          }
          bit = b.pos();
          if (final) {
            b.align();
            uint32_t crc, isize;
            const uint64_t tr = b.pos() >> 3;
            if (!b.take(32, &crc) || !b.take(32, &isize)) { fail(GZ_E_END, tr * 8); break; }
            pc->ends.push_back({pos, crc, isize, tr});
            bit = (tr + 8) * 8; at_header = true;
          }
        }
        if (!bytes_mode) {
          for (uint64_t i = 0; i < pos; i++) text[i] = (uint8_t)sym[i];
          pc->symbols.assign(sym, sym + m_end);
        }
        pc->text_len = pos;
        pc->end_bit = bit;
        pc->end_at_header = at_header;
        t_inflate[t] += now_s() - i0;
        std::lock_guard<std::mutex> g(mu);
        if (pc->err == -1 || task.abandoned) { free_slots.push_back(slot); task.done = true; cv.notify_all(); break; }
        if (task_over) task.done = true;
        task.pieces.push_back(std::move(pc));
        cv.notify_all();
      }
    }
  };

  std::vector<std::thread> workers;
  for (int t = 0; t < n_threads; t++) workers.emplace_back(worker, t);

  // ---- the consumer: pieces in stream order ----
  std::deque<int> held;                                                // slots consumed, not yet given back
  uint64_t member_bytes = 0;
  bool first_piece_of_task = true, any = false;
  uint64_t prev_end_bit = 0, prev_end_key = GZ_NONE;
  bool prev_end_header = true;                                         // (before the first piece: the header at byte 0)
  res.info.chunks = n_spans;
  for (bool over = false; !over;) {
    std::unique_ptr<GzPiece> pc;
    const double t0 = now_s();
    {
      std::unique_lock<std::mutex> lk(mu);
      cv.wait(lk, [&] { return stop || !tasks[head].pieces.empty(); });
      if (stop) break;
      pc = std::move(tasks[head].pieces.front());
      tasks[head].pieces.pop_front();
      // the acceptance rule: a piece is taken only when the piece before it ended exactly at its start
      const bool follows = (any && first_piece_of_task) ? (prev_end_key != GZ_NONE && tasks[head].cand == prev_end_key)
                                                        : (pc->start_bit == prev_end_bit && pc->at_header == prev_end_header);
      if (!follows && pc->err == GZ_OK) { pc->err = GZ_E_ORDER; pc->err_bit = pc->start_bit; }
    }
    const double t1 = now_s();
    res.t_wait += t1 - t0;
    if (pc->err != GZ_OK) {                                            // damage in a piece whose start is exact: the file's
      std::lock_guard<std::mutex> g(mu);
      res.end = GzResult::FORMAT; res.detail = pc->err; res.offset = pc->err_bit >> 3;
      stop = true; cv.notify_all();
      break;
    }
    if (!first_piece_of_task) { res.info.cuts++; res.info.chunks++; }
    GzPieceView v;
    v.text = slots[pc->slot]; v.text_len = pc->text_len;
    v.symbols = pc->symbols.data(); v.n_symbols = pc->symbols.size();
    v.window_valid = pc->at_header ? 0 : (uint32_t)std::min<uint64_t>(member_bytes, GZ_WINDOW);
    v.ends = pc->ends.data(); v.n_ends = pc->ends.size();
    v.comp_off = pc->start_bit >> 3;
    uint64_t from = 0;
    for (const GzMemberEnd &e : pc->ends) { member_bytes = 0; from = e.text_off; res.info.members++; }
    member_bytes += pc->text_len - from;
    res.info.text_bytes += pc->text_len;
    res.info.symbol_bytes += 2 * (uint64_t)pc->symbols.size();
    const int rc = consume(v);
    res.t_consume += now_s() - t1;
    std::lock_guard<std::mutex> g(mu);
    if (rc) { if (!stop) { res.end = GzResult::CONSUMER_STOPPED; res.detail = rc; } stop = true; cv.notify_all(); break; }
    held.push_back(pc->slot);
    while ((int)held.size() > opt.lag) { free_slots.push_back(held.front()); held.pop_front(); }
    first_piece_of_task = false; any = true;
    prev_end_bit = pc->end_bit; prev_end_header = pc->end_at_header; prev_end_key = pc->end_key;
    if (pc->last) {
      const uint64_t next = pc->stream_end ? n_spans : pc->next_span;
      for (uint64_t k = head + 1; k < next; k++) {                     // their spans were inflated by the task just taken
        Task &d = tasks[k];
        d.abandoned = true;
        if (d.cand_state == 2 && d.cand != GZ_NONE) res.info.discarded++;
        for (auto &q : d.pieces) free_slots.push_back(q->slot);
        d.pieces.clear();
      }
      if (pc->stream_end) { stop = true; over = true; }
      else { head = next; res.info.confirmed++; first_piece_of_task = true; }
    }
    cv.notify_all();
  }
  { std::lock_guard<std::mutex> g(mu); stop = true; cv.notify_all(); }
  for (auto &w : workers) w.join();
  for (int t = 0; t < n_threads; t++) { res.t_find += t_find[t]; res.t_inflate += t_inflate[t]; res.t_confirm += t_confirm[t]; res.t_slot_wait += t_slot[t]; }
  return res;
}
}  // namespace mgc
