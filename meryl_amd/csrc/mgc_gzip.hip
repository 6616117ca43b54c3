// mgc_gzip.hip -- the second pass of the parallel gzip reader, on the device (gfx950).
//
// The host inflaters (mgc_gzip_par.hpp) start in the middle of a deflate stream and cannot know the 32 KiB before their start:
// where a back-reference reaches into it they write a MARKER, 0x8000 + o for byte o of that window (o = 32767: the byte just
// before the piece).  The pieces arrive here in stream order, each as its text (markers as junk bytes) and the 16-bit symbols
// of its unresolved prefix.  Three kernels per piece, on the text stream:
//   gz_resolve_kernel  text[i] = sym[i] < 256 ? sym[i] : window[sym[i] - 0x8000] for i < n_symbols, in place.  The window is
//                      staged in LDS (32 KiB); output-centric as bam_decode_kernel: a thread owns one 16-byte line of the
//                      destination and stores it whole, only a piece's first and last line are stored byte by byte.  A symbol
//                      in 0x100..0x7FFF, or a marker below 32768 - window_valid (before the start of its gzip member), sets
//                      the error word and writes 0: the index into LDS is always within the window.
//   gz_window_kernel   the next window: the last 32 KiB of (window ++ resolved piece), into the other of two buffers.
//   gz_crc32_kernel    CRC-32 of pieces of at most 4 KiB of the resolved text, one thread per piece, slicing-by-4 with the
//                      tables in LDS; the host combines the values (zlib's crc32_combine) and checks every member's trailer.
// Every index is bounded by the kernel's own arguments; workgroups share nothing but the error word (an atomic OR).
#include "mgc_device.h"

namespace mgc {

typedef unsigned char      u8;
typedef unsigned short     u16;
typedef unsigned int       u32;
typedef unsigned long long u64;

namespace {
constexpr int GR_BLOCK  = 256;
constexpr int GR_SPAN   = 16;                    // output bytes per thread: one 16-byte store
constexpr int GR_TILE   = GR_BLOCK * GR_SPAN;    // 4 KiB of output
constexpr u32 GZ_WIN    = 32768;
constexpr int GR_MAX_BLOCKS = 1024;              // each stages the window once and walks tiles from there

__device__ __forceinline__ u32 resolve_one(u32 s, const u8 *s_win, u32 lowest, u32 *bad) {
  if (s < 256u) return s;
  const u32 o = s - 0x8000u;                     // (s < 0x8000: wraps to >= 0xffff8100, refused below)
  if (s < 0x8000u) { *bad |= 1u; return 0u; }
  if (o < lowest) { *bad |= 2u; return 0u; }
  return s_win[o & (GZ_WIN - 1)];
}

// text: where text byte 0 lies; head = text & 15.  Text byte i lies at line coordinate v = i + head of the 16-byte lines
// that start at text - head.
__global__ __launch_bounds__(GR_BLOCK)
void gz_resolve_kernel(u8 *__restrict__ text, const u16 *__restrict__ sym, u64 n_sym, const u8 *__restrict__ window, u32 window_valid,
                       u32 *__restrict__ error, u32 head, u64 tiles) {
  __shared__ uint4 s_win4[GZ_WIN / 16];
  u8 *s_win = reinterpret_cast<u8 *>(s_win4);
  const u32 tid = threadIdx.x;
  if (window && (reinterpret_cast<uintptr_t>(window) & 15u) == 0) {
    for (u32 i = tid; i < GZ_WIN / 16; i += GR_BLOCK) s_win4[i] = reinterpret_cast<const uint4 *>(window)[i];
  } else {
    for (u32 i = tid; i < GZ_WIN; i += GR_BLOCK) s_win[i] = window ? window[i] : (u8)0;
  }
  __syncthreads();
  const u32 lowest = GZ_WIN - window_valid;      // (window_valid <= GZ_WIN: the launcher)
  const u64 v_end = n_sym + head;
  u32 bad = 0;
  for (u64 tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const u64 sv0 = tile * GR_TILE + (u64)tid * GR_SPAN;
    if (sv0 >= v_end) continue;
    const u64 sv1 = sv0 + GR_SPAN < v_end ? sv0 + GR_SPAN : v_end;
    const u64 o_begin = sv0 > head ? sv0 - head : 0, o_end = sv1 - head;      // o_end <= n_sym
    const bool whole = sv0 >= head && sv0 + GR_SPAN <= v_end;
    u64 w0 = 0, w1 = 0;
    if (whole && (reinterpret_cast<uintptr_t>(sym + o_begin) & 15u) == 0) {
      const uint4 a = reinterpret_cast<const uint4 *>(sym + o_begin)[0], c = reinterpret_cast<const uint4 *>(sym + o_begin)[1];
      const u32 wds[8] = {a.x, a.y, a.z, a.w, c.x, c.y, c.z, c.w};
      if (((a.x | a.y | a.z | a.w | c.x | c.y | c.z | c.w) & 0xff00ff00u) == 0) {          // sixteen plain bytes
#pragma unroll
        for (int j = 0; j < 4; j++) {
          w0 |= (u64)((wds[j] & 0xffu) | ((wds[j] >> 8) & 0xff00u)) << (16 * j);
          w1 |= (u64)((wds[j + 4] & 0xffu) | ((wds[j + 4] >> 8) & 0xff00u)) << (16 * j);
        }
      } else {
#pragma unroll
        for (int j = 0; j < 4; j++) {
          w0 |= (u64)(resolve_one(wds[j] & 0xffffu, s_win, lowest, &bad) | (resolve_one(wds[j] >> 16, s_win, lowest, &bad) << 8)) << (16 * j);
          w1 |= (u64)(resolve_one(wds[j + 4] & 0xffffu, s_win, lowest, &bad) | (resolve_one(wds[j + 4] >> 16, s_win, lowest, &bad) << 8)) << (16 * j);
        }
      }
    } else {
      for (u64 o = o_begin; o < o_end; o++) {
        const u32 c = resolve_one(sym[o], s_win, lowest, &bad);
        const u32 q = (u32)(o + head - sv0);
        if (q < 8) w0 |= (u64)c << (8 * q); else w1 |= (u64)c << (8 * (q - 8));
      }
    }
    u8 *line = (text - head) + sv0;                                           // 16-byte aligned; only [o_begin, o_end) of it is written
    if (whole) {
      *reinterpret_cast<ulonglong2 *>(line) = make_ulonglong2(w0, w1);
    } else {
      for (u64 q = o_begin + head - sv0; q < o_end + head - sv0; q++)
        line[q] = (u8)((q < 8 ? w0 >> (8 * q) : w1 >> (8 * (q - 8))) & 0xffu);
    }
  }
  if (bad) atomicOr(error, bad);
}

// out[j], j < 32768: byte j of the last 32 KiB of (window_in ++ text[0 .. n))
__global__ __launch_bounds__(GR_BLOCK)
void gz_window_kernel(const u8 *__restrict__ text, u64 n, const u8 *__restrict__ window_in, u8 *__restrict__ window_out) {
  const u32 j0 = (blockIdx.x * GR_BLOCK + threadIdx.x) * GR_SPAN;
  if (j0 >= GZ_WIN) return;
  u64 w0 = 0, w1 = 0;
#pragma unroll
  for (u32 q = 0; q < GR_SPAN; q++) {
    const u32 j = j0 + q;
    const u64 back = GZ_WIN - j;                                              // this byte lies `back` bytes before the end
    const u32 c = back <= n ? text[n - back] : (window_in ? window_in[j + n] : 0u);      // (back > n: j + n < 32768)
    if (q < 8) w0 |= (u64)c << (8 * q); else w1 |= (u64)c << (8 * (q - 8));
  }
  if ((reinterpret_cast<uintptr_t>(window_out) & 15u) == 0) {
    *reinterpret_cast<ulonglong2 *>(window_out + j0) = make_ulonglong2(w0, w1);
  } else {
    for (u32 q = 0; q < GR_SPAN; q++) window_out[j0 + q] = (u8)((q < 8 ? w0 >> (8 * q) : w1 >> (8 * (q - 8))) & 0xffu);
  }
}

constexpr int GC_BLOCK = 64;
constexpr u32 GC_MAX_PIECE = 4096;

__global__ __launch_bounds__(GC_BLOCK)
void gz_crc32_kernel(const u8 *__restrict__ text, const u64 *__restrict__ begin, const u32 *__restrict__ len, u64 n_pieces, u32 *__restrict__ crc_out) {
  __shared__ u32 s_t[4][256];
  for (u32 i = threadIdx.x; i < 256; i += GC_BLOCK) {
    u32 c = i;
#pragma unroll
    for (int k = 0; k < 8; k++) c = (c >> 1) ^ ((c & 1u) ? 0xedb88320u : 0u);
    s_t[0][i] = c;
  }
  __syncthreads();
  for (u32 i = threadIdx.x; i < 256; i += GC_BLOCK) {
    u32 c = s_t[0][i];
#pragma unroll
    for (int t = 1; t < 4; t++) { c = s_t[0][c & 0xffu] ^ (c >> 8); s_t[t][i] = c; }
  }
  __syncthreads();
  const u64 p = (u64)blockIdx.x * GC_BLOCK + threadIdx.x;
  if (p >= n_pieces) return;
  const u8 *at = text + begin[p];
  u32 left = len[p] < GC_MAX_PIECE ? len[p] : GC_MAX_PIECE;
  u32 crc = 0xffffffffu;
  auto word = [&](u32 w) {
    crc ^= w;
    crc = s_t[3][crc & 0xffu] ^ s_t[2][(crc >> 8) & 0xffu] ^ s_t[1][(crc >> 16) & 0xffu] ^ s_t[0][crc >> 24];
  };
  while (left && (reinterpret_cast<uintptr_t>(at) & 15u)) { crc = s_t[0][(crc ^ *at++) & 0xffu] ^ (crc >> 8); left--; }
  for (; left >= 16; left -= 16, at += 16) {
    const uint4 v = *reinterpret_cast<const uint4 *>(at);
    word(v.x); word(v.y); word(v.z); word(v.w);
  }
  while (left) { crc = s_t[0][(crc ^ *at++) & 0xffu] ^ (crc >> 8); left--; }
  crc_out[p] = ~crc;
}
}  // namespace

hipError_t launch_gzip_resolve(uint8_t *d_text, uint64_t text_bytes, const uint16_t *d_symbols, uint64_t n_symbols, const uint8_t *d_window_in,
                               uint32_t window_valid, uint8_t *d_window_out, uint32_t *d_error, hipStream_t st) {
  if (n_symbols > text_bytes || window_valid > GZ_WIN) return hipErrorInvalidValue;
  if (n_symbols) {
    const u32 head = (u32)(reinterpret_cast<uintptr_t>(d_text) & 15u);
    const u64 tiles = (n_symbols + head + GR_TILE - 1) / GR_TILE;
    const u32 blocks = (u32)(tiles < (u64)GR_MAX_BLOCKS ? tiles : (u64)GR_MAX_BLOCKS);
    hipLaunchKernelGGL(gz_resolve_kernel, dim3(blocks), dim3(GR_BLOCK), 0, st, d_text, reinterpret_cast<const u16 *>(d_symbols), (u64)n_symbols, d_window_in, window_valid,
                       d_error, head, tiles);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if (d_window_out) {
    hipLaunchKernelGGL(gz_window_kernel, dim3(GZ_WIN / GR_TILE), dim3(GR_BLOCK), 0, st, d_text, (u64)text_bytes, d_window_in, d_window_out);
    return hipGetLastError();
  }
  return hipSuccess;
}

hipError_t launch_gzip_crc32(const uint8_t *d_text, const uint64_t *d_begin, const uint32_t *d_len, uint64_t n_pieces, uint32_t *d_crc, hipStream_t st) {
  if (n_pieces == 0) return hipSuccess;
  const u64 blocks = (n_pieces + GC_BLOCK - 1) / GC_BLOCK;
  if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gz_crc32_kernel, dim3((uint32_t)blocks), dim3(GC_BLOCK), 0, st, d_text, reinterpret_cast<const u64 *>(d_begin), d_len, (u64)n_pieces, d_crc);
  return hipGetLastError();
}

}  // namespace mgc
