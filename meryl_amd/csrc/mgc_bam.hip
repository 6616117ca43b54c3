// mgc_bam.hip -- packed BAM SEQ fields -> base stream, on the device (gfx950).
//
// Replaces, for BAM bytes that are already in HBM, the single host thread that walked the records and expanded their 4-bit
// bases (meryl_seq.cpp: bam_fast_records / bam_load_bases).  The host still walks the records (mgc_bam_walk.hpp: a few
// bytes of every record), and hands over a table of SEGMENTS: {where the packed bytes start in the piece, how many bases,
// whether a '.' follows, where the output starts}.  Output = every record's SEQ as stored, through the nt16 alphabet
// "=ACMGRSVTWYHKDBN" (SAMv1 4.2), high nibble first, and one '.' after every record.
//
// The kernel is output-centric: a thread produces one SPAN of 16 consecutive output bytes, a workgroup a TILE of 256
// spans.  Spans are laid over the 16-byte lines of the destination, not over the output's own offsets -- a file begins
// wherever the stream happens to end -- so every whole span is one 16-byte store; only the first and the last span of
// a piece can be partial and are stored byte by byte.  A thread finds the segment of its first byte by binary search over
// out_off (in the tile's slice of the table, staged in LDS when it holds at most BD_LDS_SEGS segments -- a tile of
// empty records can hold 4096) and walks forward through the segments its span touches.  Every loop is bounded by the
// table; workgroups share nothing; every index taken from the table is checked against the piece and the table sizes.
#include "mgc_device.h"

namespace mgc {

typedef unsigned char      u8;
typedef unsigned int       u32;
typedef unsigned long long u64;

namespace {
constexpr int BD_BLOCK    = 256;
constexpr int BD_SPAN     = 16;                     // output bytes per thread: one 16-byte store
constexpr int BD_TILE     = BD_BLOCK * BD_SPAN;     // 4 KiB of output
constexpr int BD_LDS_SEGS = 512;                    // 8 KiB of LDS

struct Seg { u32 src_off, nbf; u64 out_off; };      // mgc::BamSegment (mgc_bam_walk.hpp)
static_assert(sizeof(Seg) == 16, "segments are 16 bytes");

__device__ __forceinline__ u32 nt16(u32 code) {     // "=ACMGRSV" "TWYHKDBN", little endian
  const u64 half = (code & 8u) ? 0x4e42444b48595754ull : 0x565352474d43413dull;
  return (u32)(half >> ((code & 7u) * 8)) & 0xffu;
}

// the last i in [lo, hi] with tab[i].out_off <= o (lo when there is none)
__device__ __forceinline__ u64 seg_find(const Seg *tab, u64 lo, u64 hi, u64 o) {
  while (lo < hi) {
    const u64 mid = lo + (hi - lo + 1) / 2;
    if (tab[mid].out_off <= o) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// out: where output byte 0 goes; head = out & 15.  Output byte o lies at line coordinate v = o + head of the 16-byte lines
// that start at out - head.
__global__ __launch_bounds__(BD_BLOCK)
void bam_decode_kernel(const u8 *__restrict__ piece, u64 piece_bytes, const Seg *__restrict__ segs, u64 n_segs, u64 out_total,
                       u8 *__restrict__ out, u32 head) {
  __shared__ Seg s_tab[BD_LDS_SEGS];
  const u32 tid = threadIdx.x;
  const u64 v_end = out_total + head;
  const u64 tv0 = (u64)blockIdx.x * BD_TILE;                      // < v_end (the grid)
  const u64 tv1 = tv0 + BD_TILE < v_end ? tv0 + BD_TILE : v_end;
  const u64 to0 = tv0 > head ? tv0 - head : 0;                    // the tile's output bytes [to0, to1)
  const u64 to1 = tv1 - head;

  // the tile's slice of the table: two searches over the whole table, by one thread for all
  __shared__ u64 s_slice[2];
  if (tid == 0) {
    s_slice[0] = seg_find(segs, 0, n_segs - 1, to0);
    s_slice[1] = seg_find(segs, s_slice[0], n_segs - 1, to1 - 1);
  }
  __syncthreads();
  const u64 first = s_slice[0], last = s_slice[1];
  const u64 cnt   = last - first + 1;
  const Seg *tab = segs + first;
  if (cnt <= (u64)BD_LDS_SEGS) {
    for (u32 i = tid; i < (u32)cnt; i += BD_BLOCK) s_tab[i] = segs[first + i];
    __syncthreads();
    tab = s_tab;
  }

  const u64 sv0 = tv0 + (u64)tid * BD_SPAN;                       // the span: lines coordinates [sv0, sv0 + 16)
  if (sv0 >= tv1) return;
  const u64 sv1 = sv0 + BD_SPAN < v_end ? sv0 + BD_SPAN : v_end;
  const u64 o_begin = sv0 > head ? sv0 - head : 0, o_end = sv1 - head;
  const bool whole = sv0 >= head && sv0 + BD_SPAN <= v_end;

  u64 w0 = 0, w1 = 0;                                             // the span's bytes, little endian
  u64 o = o_begin;
  u64 i = seg_find(tab, 0, cnt - 1, o);
  while (o < o_end && i < cnt) {
    const Seg sg = tab[i];
    const u32 nb = sg.nbf & 0x7fffffffu, len = nb + (sg.nbf >> 31);
    const u64 local = o - sg.out_off;                             // (a table that does not ascend: huge, the segment is passed over)
    if (local >= len) { i++; continue; }
    const u32 m = (u32)((u64)(len - local) < o_end - o ? (u64)(len - local) : o_end - o);      // 1 .. 16
    const u32 p = (u32)(o + head - sv0);                          // position in the span
    const u64 src = (u64)sg.src_off + (local >> 1);
    if (m == BD_SPAN && local + BD_SPAN <= nb && src + 9 <= piece_bytes) {
      // the common case: sixteen bases of one record -- eight or nine packed bytes, as sixteen nibbles from the top of `nib`
      u64 be = 0;
#pragma unroll
      for (int j = 0; j < 8; j++) be = (be << 8) | piece[src + j];
      const u64 nib = (local & 1) ? ((be << 4) | (u64)(piece[src + 8] >> 4)) : be;
#pragma unroll
      for (int j = 0; j < 8; j++) {
        w0 |= (u64)nt16((u32)(nib >> (60 - 4 * j)) & 15u) << (8 * j);
        w1 |= (u64)nt16((u32)(nib >> (28 - 4 * j)) & 15u) << (8 * j);
      }
    } else {
      for (u32 j = 0; j < m; j++) {
        const u64 l = local + j;
        u32 c = (u32)'.';
        if (l < nb) {
          const u64 at = (u64)sg.src_off + (l >> 1);
          const u32 b = at < piece_bytes ? piece[at] : 0u;
          c = nt16((l & 1) ? (b & 15u) : (b >> 4));
        }
        const u32 q = p + j;
        if (q < 8) w0 |= (u64)c << (8 * q); else w1 |= (u64)c << (8 * (q - 8));
      }
    }
    o += m;
    if (local + m == len) i++;
  }

  u8 *line = (out - head) + sv0;                                    // 16-byte aligned; only [o_begin, o_end) of it is written
  if (whole) {
    *reinterpret_cast<ulonglong2 *>(line) = make_ulonglong2(w0, w1);
  } else {
    for (u64 q = o_begin + head - sv0; q < o_end + head - sv0; q++)
      line[q] = (u8)((q < 8 ? w0 >> (8 * q) : w1 >> (8 * (q - 8))) & 0xffu);
  }
}
}  // namespace

hipError_t launch_bam_decode(const uint8_t *d_piece, uint64_t piece_bytes, const void *d_segments, uint64_t n_segments, uint64_t out_total,
                             uint8_t *d_out, hipStream_t st) {
  if (out_total == 0 || n_segments == 0) return hipSuccess;
  const u32 head = (u32)(reinterpret_cast<uintptr_t>(d_out) & 15u);
  const u64 tiles = (out_total + head + BD_TILE - 1) / BD_TILE;
  if (tiles > 0x7fffffffull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(bam_decode_kernel, dim3((uint32_t)tiles), dim3(BD_BLOCK), 0, st, d_piece, (u64)piece_bytes,
                     reinterpret_cast<const Seg *>(d_segments), (u64)n_segments, (u64)out_total, d_out, head);
  return hipGetLastError();
}

}  // namespace mgc
