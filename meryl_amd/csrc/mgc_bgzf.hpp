// mgc_bgzf.hpp -- BGZF blocks (gzip members of <= 64 KiB of text, their compressed size in a 'BC' extra subfield, SAMv1 4.1):
// parse one, inflate one, cut a mapped file into chunks of whole blocks.  Host-only, zlib only; shared by the generic reader
// (meryl_seq.cpp) and the whole-file reader (mgc_textfile.cpp).
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>
#include <zlib.h>

namespace mgc {
struct BgzfBlock { uint64_t off; uint32_t csize, hdr, isize; };      // where it starts, total size, header length, bytes of text

enum BgzfParse {
  BGZF_NOT_BLOCK = 0,     // no BGZF header in the n bytes at p (n < 18 included)
  BGZF_BLOCK,             // *b is filled in
  BGZF_TRUNCATED,         // a header, but the block is longer than n: b->csize and b->hdr are set
  BGZF_SHORT,             // the block is too small to hold its header and trailer
  BGZF_BAD_ISIZE          // ISIZE > 64 KiB: b->isize is set
};

// the block at p, of which n bytes are there (b->off is left alone)
inline BgzfParse bgzf_parse_block(const unsigned char *p, size_t n, BgzfBlock *b) {
  if (n < 18 || p[0] != 0x1f || p[1] != 0x8b || p[2] != 8 || !(p[3] & 4)) return BGZF_NOT_BLOCK;
  const size_t hdr = 12 + ((size_t)p[10] | ((size_t)p[11] << 8));
  if (hdr > n) return BGZF_NOT_BLOCK;
  size_t bs = 0;
  for (size_t o = 12; o + 4 <= hdr && !bs;) {
    const size_t slen = (size_t)p[o + 2] | ((size_t)p[o + 3] << 8);
    if (p[o] == 'B' && p[o + 1] == 'C' && slen == 2 && o + 6 <= hdr) bs = ((size_t)p[o + 4] | ((size_t)p[o + 5] << 8)) + 1;
    o += 4 + slen;
  }
  if (!bs) return BGZF_NOT_BLOCK;
  b->csize = (uint32_t)bs; b->hdr = (uint32_t)hdr;
  if (bs > n) return BGZF_TRUNCATED;
  if (bs < hdr + 8) return BGZF_SHORT;
  b->isize = (uint32_t)p[bs - 4] | ((uint32_t)p[bs - 3] << 8) | ((uint32_t)p[bs - 2] << 16) | ((uint32_t)p[bs - 1] << 24);
  return b->isize > 65536 ? BGZF_BAD_ISIZE : BGZF_BLOCK;
}

// Inflates block b, which starts at p, into dst (b.isize bytes) with the caller's raw-deflate stream (inflateInit2(&z, -15));
// false unless the stream ends where it should, gives b.isize bytes and they match the block's CRC.  An empty block (the
// end-of-file marker, and any other) succeeds and produces nothing.
inline bool bgzf_inflate_block(z_stream &z, const unsigned char *p, const BgzfBlock &b, unsigned char *dst) {
  if (b.isize == 0) return true;
  if (inflateReset(&z) != Z_OK) return false;
  z.next_in = const_cast<unsigned char *>(p + b.hdr);
  z.avail_in = b.csize - b.hdr - 8;
  z.next_out = dst;
  z.avail_out = b.isize;
  const int zr = inflate(&z, Z_FINISH);
  const uint32_t want = (uint32_t)p[b.csize - 8] | ((uint32_t)p[b.csize - 7] << 8) | ((uint32_t)p[b.csize - 6] << 16) | ((uint32_t)p[b.csize - 5] << 24);
  return zr == Z_STREAM_END && z.avail_out == 0 && (uint32_t)crc32(0L, dst, b.isize) == want;
}

// A mapped BGZF file as an index of its blocks, cut into chunks [first, last) of whole blocks that hold at most `cap` bytes of
// text each (cap >= 64 KiB).  A trailing chunk of empty blocks only (the end-of-file marker) is kept, with text == 0.
// bad != BGZF_BLOCK: the walk stopped at offset bad_off (blocks and chunks hold what came before it); bad_isize for BGZF_BAD_ISIZE.
struct BgzfChunk { size_t first, last, text; };
struct BgzfPlan {
  std::vector<BgzfBlock> blocks;
  std::vector<BgzfChunk> chunks;
  BgzfParse bad = BGZF_BLOCK; uint64_t bad_off = 0; uint32_t bad_isize = 0;
};
inline BgzfPlan bgzf_plan_chunks(const unsigned char *map, size_t size, size_t cap) {
  BgzfPlan plan;
  size_t text = 0, first = 0;
  for (size_t off = 0; off < size;) {
    BgzfBlock b{(uint64_t)off, 0, 0, 0};
    const BgzfParse r = bgzf_parse_block(map + off, size - off, &b);
    if (r != BGZF_BLOCK) { plan.bad = r; plan.bad_off = off; plan.bad_isize = b.isize; return plan; }
    if (text + b.isize > cap) { plan.chunks.push_back({first, plan.blocks.size(), text}); first = plan.blocks.size(); text = 0; }
    plan.blocks.push_back(b);
    text += b.isize;
    off += b.csize;
  }
  if (plan.blocks.size() > first) plan.chunks.push_back({first, plan.blocks.size(), text});
  return plan;
}
}  // namespace mgc
