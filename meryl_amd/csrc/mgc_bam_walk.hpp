// mgc_bam_walk.hpp -- a resumable walker over the records of an (inflated) BAM byte stream (SAMv1 4.2): it is fed the stream in
// pieces of any size and turns the packed SEQ field of every record into SEGMENTS, the table the device decoder
// (mgc_bam.hip) expands into the base stream: SEQ as stored, '.' after every record, no FLAG filtering.  Host-only, no HIP,
// no zlib; the session (mgc_input.cpp), the whole-file reader (mgc_textfile.cpp) and tests/host/bam_walk_host.cpp use it.
//
// What holds for the segments of a piece of n bytes:
//   - src_off + (n_bases + 1) / 2 <= n: no segment refers to a byte outside its piece;
//   - out_off ascends, the first is 0, every segment produces at least one byte (n_bases + flag >= 1) and the next
//     segment's out_off is this one's plus that many: the table tiles [0, the piece's output bytes);
//   - a SEQ field that runs past the end of the piece gives an unflagged segment for the whole bytes that are there (an even
//     number of bases); its continuation in the next piece starts on a high nibble again.
#pragma once

#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace mgc {
struct BamSegment {
  uint32_t src_off;              // byte offset, within the piece, of the first packed byte
  uint32_t n_bases_and_flag;     // bases (<= 2^31 - 1); bit 31: a '.' follows them
  uint64_t out_off;              // offset of the first output byte, relative to the piece's first output byte
};
static_assert(sizeof(BamSegment) == 16, "the device reads 16-byte segments");
constexpr uint32_t BAM_SEG_DOT = 0x80000000u;
constexpr size_t   BAM_MAX_PIECE = (size_t)1 << 30;

class BamWalker {
 public:
  void reset() { *this = BamWalker(); }

  // One more piece of the stream (n <= 2^30: offsets into it are 32 bits, and an unflagged segment holds two bases per byte of it).  Appends the piece's segments to *segs and adds nothing else to it; *out_bytes
  // is what the segments produce.  false: the stream is damaged (error() says how and where), and stays refused.
  bool walk(const unsigned char *p, size_t n, std::vector<BamSegment> *segs, uint64_t *out_bytes) {
    *out_bytes = 0;
    if (failed_) return false;
    if (n > BAM_MAX_PIECE) return fail("BAM: a piece of %llu bytes at stream offset %llu is more than the walker takes at once", (unsigned long long)n, (unsigned long long)base_);
    uint64_t out = 0;
    size_t pos = 0;
    while (pos < n) {
      if (phase_ == SKIP) {                                   // header text, reference names, what surrounds SEQ
        const uint64_t take = skip_ < (uint64_t)(n - pos) ? skip_ : (uint64_t)(n - pos);
        pos += (size_t)take;
        skip_ -= take;
        if (skip_) break;
        phase_ = after_skip_;
        continue;
      }
      if (phase_ == SEQ) {
        const size_t avail = n - pos;
        if ((uint64_t)avail >= seq_bytes_) {                  // the (rest of the) field lies whole in the piece
          segs->push_back(BamSegment{(uint32_t)pos, seq_bases_ | BAM_SEG_DOT, out});
          out += (uint64_t)seq_bases_ + 1;
          pos += (size_t)seq_bytes_;
          skip_then(rest_, REC_HEAD);
        } else {                                              // it runs past the end: the whole bytes present, no '.'
          segs->push_back(BamSegment{(uint32_t)pos, (uint32_t)(avail * 2), out});
          out += (uint64_t)avail * 2;
          seq_bases_ -= (uint32_t)(avail * 2);
          seq_bytes_ -= avail;
          pos = n;
        }
        continue;
      }
      // a fixed-size field: gathered in carry_ when it straddles two pieces
      const size_t want = need();
      const unsigned char *f;
      if (carried_ == 0 && n - pos >= want) {
        f = p + pos;
        if (phase_ == REC_HEAD) {
          // The walk reads 36 bytes of every record, each in a cache line another thread has just written, and learns where the next
          // one is only from this one: one memory latency per record.  Records of a file are mostly alike, so the line sixteen records
          // ahead at this record's size is asked for now (a hint: a wrong guess costs nothing, the address stays inside the piece).
          const uint64_t ahead = (uint64_t)pos + PREFETCH_RECORDS * (4 + (uint64_t)(uint32_t)i32(f));
          if (ahead + 36 <= (uint64_t)n) { __builtin_prefetch(p + ahead); __builtin_prefetch(p + ahead + 35); }
        }
        pos += want;
      } else {
        const size_t take = (want - carried_) < (n - pos) ? (want - carried_) : (n - pos);
        memcpy(carry_ + carried_, p + pos, take);
        carried_ += take;
        pos += take;
        if (carried_ < want) break;
        f = carry_;
        carried_ = 0;
      }
      const uint64_t at = base_ + pos - want;                 // stream offset of the field
      if (!field(f, at, &pos, n, segs, &out)) return false;
    }
    base_ += n;
    *out_bytes = out;
    return true;
  }

  // the stream has ended: true at a record border (or right after the header), false + error() anywhere else
  bool finish() {
    if (failed_) return false;
    if (phase_ == REC_HEAD && carried_ == 0) return true;
    const bool in_header = phase_ < REC_HEAD || (phase_ == SKIP && after_skip_ < REC_HEAD);
    return fail("truncated BAM %s: the stream ends at offset %llu", in_header ? "header" : "record", (unsigned long long)base_);
  }

  const std::string &error() const { return err_; }
  bool failed() const { return failed_; }
  uint64_t records() const { return records_; }
  uint64_t stream_bytes() const { return base_; }

 private:
  enum Phase { MAGIC, L_TEXT, N_REF, L_NAME, L_REF, REC_HEAD, SEQ, SKIP };
  static constexpr uint64_t PREFETCH_RECORDS = 16;

  size_t need() const { return phase_ == REC_HEAD ? 36 : 4; }
  static int32_t i32(const unsigned char *f) { return (int32_t)((uint32_t)f[0] | ((uint32_t)f[1] << 8) | ((uint32_t)f[2] << 16) | ((uint32_t)f[3] << 24)); }

  bool fail(const char *fmt, ...) __attribute__((format(printf, 2, 3))) {
    char buf[256];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    err_ = buf;
    failed_ = true;
    return false;
  }
  bool fail_field(const char *name, int32_t v, uint64_t at) { return fail("BAM: negative %s (%d) at stream offset %llu", name, v, (unsigned long long)at); }
  void skip_then(uint64_t bytes, Phase next) {
    if (bytes) { phase_ = SKIP; skip_ = bytes; after_skip_ = next; }
    else phase_ = next;
  }
  void next_ref() { phase_ = refs_left_ ? L_NAME : REC_HEAD; }

  // one whole fixed-size field at f (stream offset `at`; *pos: the offset right after it in the piece of n bytes)
  bool field(const unsigned char *f, uint64_t at, size_t *pos, size_t n, std::vector<BamSegment> *segs, uint64_t *out) {
    switch (phase_) {
      case MAGIC:
        if (memcmp(f, "BAM\1", 4) != 0) return fail("BAM: bad magic at stream offset %llu (not a BAM stream)", (unsigned long long)at);
        phase_ = L_TEXT;
        return true;
      case L_TEXT: {
        const int32_t v = i32(f);
        if (v < 0) return fail_field("l_text", v, at);
        skip_then((uint64_t)v, N_REF);
        return true;
      }
      case N_REF: {
        const int32_t v = i32(f);
        if (v < 0) return fail_field("n_ref", v, at);
        refs_left_ = (uint32_t)v;
        next_ref();
        return true;
      }
      case L_NAME: {
        const int32_t v = i32(f);
        if (v < 0) return fail_field("l_name", v, at);
        skip_then((uint64_t)v, L_REF);
        return true;
      }
      case L_REF:
        refs_left_--;
        next_ref();
        return true;
      case REC_HEAD: {
        // block_size, then refID pos l_read_name mapq bin n_cigar_op flag l_seq next_refID next_pos tlen (32 bytes)
        const int32_t block_size = i32(f);
        if (block_size < 32) return fail("BAM record at stream offset %llu: block_size %d < 32", (unsigned long long)at, block_size);
        const uint64_t l_read_name = f[12];
        const uint64_t n_cigar_op = (uint64_t)f[16] | ((uint64_t)f[17] << 8);
        const int32_t l_seq = i32(f + 20);
        if (l_seq < 0) return fail_field("l_seq", l_seq, at + 20);
        const uint64_t before = l_read_name + 4 * n_cigar_op, packed = ((uint64_t)l_seq + 1) / 2;
        if (32 + before + packed > (uint64_t)block_size)
          return fail("BAM record at stream offset %llu: its fields (32 + l_read_name %u + 4 x n_cigar_op %u + (l_seq %d + 1) / 2) are longer than its block_size %d",
                      (unsigned long long)at, (unsigned)l_read_name, (unsigned)n_cigar_op, l_seq, block_size);
        records_++;
        if ((uint64_t)*pos + ((uint64_t)block_size - 32) <= (uint64_t)n) {   // the whole record lies in the piece: no state to keep
          segs->push_back(BamSegment{(uint32_t)(*pos + before), (uint32_t)l_seq | BAM_SEG_DOT, *out});
          *out += (uint64_t)l_seq + 1;
          *pos += (size_t)block_size - 32;
          return true;
        }
        rest_ = (uint64_t)block_size - 32 - before - packed;
        if (l_seq == 0) {                                     // just the '.'
          segs->push_back(BamSegment{(uint32_t)*pos, BAM_SEG_DOT, *out});
          *out += 1;
          skip_then(before + rest_, REC_HEAD);
          return true;
        }
        seq_bases_ = (uint32_t)l_seq;
        seq_bytes_ = packed;
        skip_then(before, SEQ);
        return true;
      }
      default:
        return true;
    }
  }

  Phase         phase_ = MAGIC, after_skip_ = MAGIC;
  uint64_t      skip_ = 0;            // SKIP: bytes still to pass over
  uint64_t      rest_ = 0;            // of the current record: what follows SEQ (qualities, aux)
  uint64_t      seq_bytes_ = 0;       // SEQ: packed bytes still to come
  uint32_t      seq_bases_ = 0;       //      and the bases in them
  uint32_t      refs_left_ = 0;
  unsigned char carry_[36];           // the first bytes of a fixed-size field that straddles two pieces (at most 35)
  size_t        carried_ = 0;
  uint64_t      base_ = 0;            // stream offset of the next piece
  uint64_t      records_ = 0;
  bool          failed_ = false;
  std::string   err_;
};
}  // namespace mgc
