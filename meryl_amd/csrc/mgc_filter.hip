// mgc_filter.hip -- meryl-lookup -include / -exclude (src/meryl-lookup/include-exclude.C) on the device, gfx950.
//
// One step takes a piece of RAW FASTA/FASTQ text per input (already in HBM, beginning at a record start) and leaves the text
// of the kept records per input, in input order, in HBM: the host looks at counts and sizes only, never at a byte of text.
//   index  : line starts (newlines per 4 KiB tile -> scan -> emit), then records -- FASTQ: line number modulo 4, every '@' and
//            '+' line start checked; FASTA: the lines that start with '>' compacted (tile count -> scan -> emit);
//            per record the spans of its identifier, bases and qualities
//   bases  : four-line FASTQ is walked in place; FASTA goes through a de-lined copy (header lines, \r \n blank tab dropped)
//   found  : per record (pair) the windows with value(fmer) > 0 || value(rmer) > 0 (include-exclude.C:64-78) through
//            lk_roll / lk_find; counts are summed per wave by record before one atomic per record and wave
//   emit   : keep = (found > 0) == include (:124-125); sizes -> scan -> a wave (a workgroup for long records) per kept record
//            writes ">"/"@" ident " nKmers=" found, the bases on one line, ("+", qualities) (:107-108) with 16-byte stores
#include "mgc_lookup_dev.hpp"
#include "mgc_compact.hpp"
#include "../../include/meryl_gpu_count.h"
#include "../../include/meryl_seq.h"

#include <algorithm>
#include <vector>

namespace mgc {

constexpr int FI_TILE = 256 * 16;                   // bytes of text per workgroup
constexpr u64 FI_LONG = 32768;                      // output bytes from which a record is written by a workgroup, not a wave

__device__ __forceinline__ bool fi_ws(u32 c) { return c == '\n' || c == '\r' || c == ' ' || c == '\t'; }
__device__ __forceinline__ u32 fi_byte(const uint4 &v, int q) {
  const u32 w = (q >> 2) == 0 ? v.x : (q >> 2) == 1 ? v.y : (q >> 2) == 2 ? v.z : v.w;
  return (w >> (8 * (q & 3))) & 0xFFu;
}
// the 16 bytes at text[base ..] ('.' past the end)
__device__ __forceinline__ uint4 fi_load(const uint8_t *__restrict__ text, u64 base, u64 n) {
  return load16(text, base, n, ((size_t)(text + base) & 15u) == 0);
}
// last i in [lo, hi) with a[i] <= pos (lo when there is none)
__device__ __forceinline__ u64 fi_last_le(const u64 *__restrict__ a, u64 lo, u64 hi, u64 pos) {
  while (hi - lo > 1) { const u64 mid = lo + ((hi - lo) >> 1); if (a[mid] <= pos) lo = mid; else hi = mid; }
  return lo;
}
// the same for one position per thread of a workgroup whose positions lie in [tile_b, tile_e]: two lanes search the whole
// array, the others only between their results.  Every thread of the workgroup must call it; cnt >= 1.
__device__ __forceinline__ u64 fi_block_rec(const u64 *__restrict__ a, u64 cnt, u64 tile_b, u64 tile_e, u64 pos, u64 *s_rng) {
  if (threadIdx.x < 2) s_rng[threadIdx.x] = fi_last_le(a, 0, cnt, threadIdx.x ? tile_e : tile_b);
  __syncthreads();
  return fi_last_le(a, s_rng[0], s_rng[1] + 1, pos);
}

// ---- line starts -------------------------------------------------------------------------------------------------------
// ls[0] = 0, ls[j] = the position after the j-th newline; an unterminated last line ends at the sentinel ls[nl + 1] = n + 1,
// so that line j is always [ls[j], ls[j + 1] - 1)
template <bool EMIT>
__global__ __launch_bounds__(256)
void filter_nl_kernel(const uint8_t *__restrict__ text, u64 n, u64 *__restrict__ tiles /*EMIT: exclusive bases*/, u64 nl, u32 open_tail,
                      u64 *__restrict__ ls) {
  const u64 base = (u64)blockIdx.x * FI_TILE + (u64)threadIdx.x * 16;
  u32 c = 0;
  uint4 v = make_uint4(0, 0, 0, 0);
  if (base < n) {
    v = fi_load(text, base, n);
#pragma unroll
    for (int q = 0; q < 16; q++) c += fi_byte(v, q) == '\n';
  }
  u64 o;
  if (!compact_slot<256, EMIT>(c, tiles, &o)) return;
  if (blockIdx.x == 0 && threadIdx.x == 0) { ls[0] = 0; if (open_tail) ls[nl + 1] = n + 1; }
  if (c) {
#pragma unroll
    for (int q = 0; q < 16; q++) if (fi_byte(v, q) == '\n') ls[++o] = base + q + 1;
  }
}
// first / last byte of a piece: the format and whether the last line is terminated -- misc[1] = MGC_TEXT_* or 0,
// misc[2] = 1 when the text does not end with a newline, misc[3] = the first byte
__global__ void filter_meta_kernel(const uint8_t *__restrict__ text, u64 n, u64 *__restrict__ misc) {
  const u32 c = text[0];
  misc[1] = c == '>' ? MGC_TEXT_FASTA : c == '@' ? MGC_TEXT_FASTQ : 0;
  misc[2] = text[n - 1] != '\n';
  misc[3] = c;
}

// ---- FASTA: the header lines, compacted in order -------------------------------------------------------------------------
constexpr int FI_LTILE = 256 * 8;                   // lines per workgroup
template <bool EMIT>
__global__ __launch_bounds__(256)
void filter_hdr_kernel(const uint8_t *__restrict__ text, const u64 *__restrict__ ls, u64 n_lines, u64 *__restrict__ tiles /*EMIT: exclusive bases*/,
                       u64 n_rec, u64 *__restrict__ rl) {
  const u64 base = (u64)blockIdx.x * FI_LTILE + (u64)threadIdx.x * 8;
  u32 hdr = 0;
  for (int q = 0; q < 8; q++) { const u64 i = base + q; if (i < n_lines) hdr |= (u32)(text[ls[i]] == '>') << q; }
  u64 o;
  if (!compact_slot<256, EMIT>(__popc(hdr), tiles, &o)) return;
  if (blockIdx.x == 0 && threadIdx.x == 0) rl[n_rec] = n_lines;
  for (int q = 0; q < 8; q++) if ((hdr >> q) & 1u) rl[o++] = base + q;
}

// ---- spans of a record ------------------------------------------------------------------------------------------------
struct FiRec { u64 id_b, q_b, q_len; u32 id_len, reserved; };

// FASTA (rl != null): record r is the lines rl[r] .. rl[r + 1] - 1; its header line is [hb, he) with the line end.
// FASTQ: record r is the lines 4r .. 4r + 3; a first line that does not start with '@' or a third that does not start with
// '+' raises *err (multi-line FASTQ ends here); bases and qualities are their lines without the terminator.
__global__ __launch_bounds__(256)
void filter_spans_kernel(const uint8_t *__restrict__ text, u64 n, const u64 *__restrict__ ls, const u64 *__restrict__ rl, u64 n_rec,
                         FiRec *__restrict__ rec, u64 *__restrict__ hb, u64 *__restrict__ he, u64 *__restrict__ bb, u64 *__restrict__ be,
                         u32 *__restrict__ err) {
  const u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_rec) return;
  const u64 h = rl ? rl[r] : 4 * r;
  const u64 a = ls[h];
  u64 e = ls[h + 1] - 1;
  if (e > a && text[e - 1] == '\r') e--;
  u64 i = a + 1;
  while (i < e && text[i] != ' ' && text[i] != '\t') i++;       // ident(): up to the first blank or tab
  FiRec x;
  x.id_b = a + 1; x.id_len = (u32)(i - (a + 1)); x.q_b = 0; x.q_len = 0; x.reserved = 0;
  if (rl) {
    hb[r] = a;
    he[r] = ls[h + 1] < n ? ls[h + 1] : n;
  } else {
    if (text[a] != '@') *err = 1u;
    if (text[ls[h + 2]] != '+') *err = 2u;
    u64 sa = ls[h + 1], se = ls[h + 2] - 1;
    if (se > sa && text[se - 1] == '\r') se--;
    bb[r] = sa; be[r] = se;
    u64 qa = ls[h + 3], qe = ls[h + 4] - 1;
    if (qe > qa && text[qe - 1] == '\r') qe--;
    x.q_b = qa; x.q_len = qe - qa;
  }
  rec[r] = x;
}

// ---- FASTA: the de-lined copy --------------------------------------------------------------------------------------------
// kept: every byte outside the header lines that is not \r \n blank tab.  bb[r] = kept bytes before record r's header.
// One record walk counts, one writes (it also leaves bb[r] where a header begins).
template <bool EMIT>
__global__ __launch_bounds__(256)
void filter_flat_kernel(const uint8_t *__restrict__ text, u64 n, const u64 *__restrict__ hb, const u64 *__restrict__ he, u64 n_rec,
                        u64 *__restrict__ tiles /*EMIT: exclusive bases*/, uint8_t *__restrict__ flat, u64 *__restrict__ bb) {
  __shared__ u64 s_rng[2];
  const u64 tile_b = (u64)blockIdx.x * FI_TILE, base = tile_b + (u64)threadIdx.x * 16;
  const u64 tile_e = tile_b + FI_TILE - 1 < n ? tile_b + FI_TILE - 1 : n - 1;
  const u64 r0 = fi_block_rec(hb, n_rec, tile_b, tile_e, base < n ? base : n - 1, s_rng);
  u32 c = 0;
  uint4 v = make_uint4(0, 0, 0, 0);
  if (base < n) {
    v = fi_load(text, base, n);
    u64 r = r0, cur_he = he[r], nxt = r + 1 < n_rec ? hb[r + 1] : ~0ull;
#pragma unroll
    for (int q = 0; q < 16; q++) {
      const u64 p = base + q;
      if (p >= nxt) { r++; cur_he = he[r]; nxt = r + 1 < n_rec ? hb[r + 1] : ~0ull; }
      c += (p < n && p >= cur_he && !fi_ws(fi_byte(v, q)));
    }
  }
  u64 o;
  if (!compact_slot<256, EMIT>(c, tiles, &o)) return;
  if (base < n) {
    u64 r = r0, cur_hb = hb[r], cur_he = he[r], nxt = r + 1 < n_rec ? hb[r + 1] : ~0ull;
#pragma unroll
    for (int q = 0; q < 16; q++) {
      const u64 p = base + q;
      if (p < n) {
        if (p >= nxt) { r++; cur_hb = nxt; cur_he = he[r]; nxt = r + 1 < n_rec ? hb[r + 1] : ~0ull; }
        if (p == cur_hb) bb[r] = o;
        const u32 ch = fi_byte(v, q);
        if (p >= cur_he && !fi_ws(ch)) flat[o++] = (uint8_t)ch;
      }
    }
  }
}

// ---- found count per record ------------------------------------------------------------------------------------------
// Record r's bases are stream[bb[r], end(r)), end(r) = be[r] (FASTQ, in place) or bb[r + 1] (the de-lined copy); a window
// counts when it starts at or after base `skip` of its record (-10x, include-exclude.C:71) and ends inside it.  A thread rolls
// the windows starting in its 16 bytes; the counts of a wave are summed by record (records ascend with the lanes) and added
// with one atomic per record and wave -- a long record costs one atomic per wave, a short one a handful.
template <typename K>
__global__ __launch_bounds__(256)
void filter_found_kernel(const LkTable tab, u32 k, const uint8_t *__restrict__ stream, u64 n_stream, const u64 *__restrict__ bb,
                         const u64 *__restrict__ be, u64 n_rec, u32 skip, u64 *__restrict__ found) {
  __shared__ u64 s_rng[2];
  const K *keys = reinterpret_cast<const K *>(tab.keys);
  const u64 tile_b = (u64)blockIdx.x * (256 * LK_RUN), i0 = tile_b + (u64)threadIdx.x * LK_RUN;
  const u64 tile_e = tile_b + 256 * LK_RUN - 1 < n_stream ? tile_b + 256 * LK_RUN - 1 : n_stream - 1;
  u64 r = fi_block_rec(bb, n_rec, tile_b, tile_e, i0 < n_stream ? i0 : n_stream - 1, s_rng);
  const bool active = i0 < n_stream;
  u32 cnt = 0;
  if (active) {
    u64 rb = bb[r], re = be ? be[r] : bb[r + 1], nb = r + 1 < n_rec ? bb[r + 1] : ~0ull;
    const bool none = i0 + k > re && i0 + LK_RUN <= nb;        // no window of this record or the next starts here
    if (!none)
      lk_roll<K>(stream, n_stream, k, i0, [&](u64 s, K f, K rc, bool pal) {
        while (s >= nb) {
          if (cnt) atomicAdd(reinterpret_cast<unsigned long long *>(found + r), (unsigned long long)cnt);
          cnt = 0;
          r++; rb = nb; re = be ? be[r] : bb[r + 1]; nb = r + 1 < n_rec ? bb[r + 1] : ~0ull;
        }
        if (s >= rb + skip && s + k <= re) {
          u32 v = lk_find<K>(keys, tab.vals, tab.index, tab.shift, f, tab.n_index);
          if (v == 0 && !pal) v = lk_find<K>(keys, tab.vals, tab.index, tab.shift, rc, tab.n_index);
          cnt += v != 0;
        }
      });
  }
  const u32 lane = lane_id();
  u32 key = active ? (u32)r : 0xFFFFFFFFu, val = cnt;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const u32 k2 = __shfl_up(key, d), v2 = __shfl_up(val, d);
    if ((int)lane >= d && k2 == key) val += v2;
  }
  const u32 knext = __shfl_down(key, 1);
  if ((lane == 63 || knext != key) && val && key != 0xFFFFFFFFu)
    atomicAdd(reinterpret_cast<unsigned long long *>(found + key), (unsigned long long)val);
}

// ---- keep, sizes, gather -------------------------------------------------------------------------------------------------
struct FiSide {
  const uint8_t *text, *stream;      // raw text; where the bases are (the text itself, or the de-lined copy)
  const FiRec *rec;
  const u64 *bb, *be;                // be == null: bb[r + 1]
  u64 *off;                          // n_rec + 1: size, then offset of record r's output
  uint8_t *out;
};

__global__ __launch_bounds__(256)
void filter_size_kernel(const u64 *__restrict__ found, u64 n_rec, u32 include, u32 n_inputs, const FiSide s0, const FiSide s1,
                        u64 *__restrict__ n_kept) {
  const u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  bool keep = false;
  if (r < n_rec) {
    const u64 f = found[r];
    keep = (f > 0) == (include != 0);                             // include-exclude.C:124-125
    for (u32 i = 0; i < n_inputs; i++) {
      const FiSide &s = i ? s1 : s0;
      const FiRec x = s.rec[r];
      const u64 nb = (s.be ? s.be[r] : s.bb[r + 1]) - s.bb[r];
      // ">ident nKmers=N\n" bases "\n" [ "+\n" quals "\n" ]
      s.off[r] = keep ? 1 + (u64)x.id_len + 8 + rp_dec_len(f) + 1 + nb + 1 + (x.q_len ? 2 + x.q_len + 1 : 0) : 0;
    }
  }
  const int c = __syncthreads_count(keep);
  if (threadIdx.x == 0 && c) atomicAdd(reinterpret_cast<unsigned long long *>(n_kept), (unsigned long long)c);
}

// n bytes by `nl` lanes: 16-byte stores to the aligned part of dst; 16-byte loads when src is aligned with it
__device__ __forceinline__ void fi_copy(uint8_t *dst, const uint8_t *src, u64 n, u32 lane, u32 nl) {
  u64 head = (16 - ((size_t)dst & 15u)) & 15u;
  if (head > n) head = n;
  for (u64 i = lane; i < head; i += nl) dst[i] = src[i];
  dst += head; src += head; n -= head;
  const u64 nv = n >> 4;
  if (((size_t)src & 15u) == 0) {
    for (u64 i = lane; i < nv; i += nl) reinterpret_cast<uint4 *>(dst)[i] = reinterpret_cast<const uint4 *>(src)[i];
  } else {
    for (u64 i = lane; i < nv; i += nl) { uint4 v; __builtin_memcpy(&v, src + 16 * i, 16); reinterpret_cast<uint4 *>(dst)[i] = v; }
  }
  for (u64 i = (nv << 4) + lane; i < n; i += nl) dst[i] = src[i];
}

// outputFASTA / outputFASTQ with the header "%s nKmers=%lu" (include-exclude.C:107-108): FASTQ when the record has qualities
__device__ __forceinline__ void fi_emit_record(const FiSide &s, u64 r, u64 f, u32 lane, u32 nl) {
  const FiRec x = s.rec[r];
  const u64 b0 = s.bb[r], nb = (s.be ? s.be[r] : s.bb[r + 1]) - b0;
  uint8_t *o = s.out + s.off[r];
  if (lane == 0) o[0] = x.q_len ? '@' : '>';
  fi_copy(o + 1, s.text + x.id_b, x.id_len, lane, nl);
  o += 1 + x.id_len;
  if (lane < 8) o[lane] = (uint8_t)" nKmers="[lane];
  o += 8;
  const u32 dl = rp_dec_len(f);
  if (lane < dl) { u64 y = f; for (u32 j = dl - 1; j > lane; j--) y /= 10; o[lane] = (uint8_t)('0' + y % 10); }
  o += dl;
  if (lane == 0) o[0] = '\n';
  o++;
  fi_copy(o, s.stream + b0, nb, lane, nl);
  o += nb;
  if (lane == 0) o[0] = '\n';
  o++;
  if (x.q_len) {
    if (lane == 0) { o[0] = '+'; o[1] = '\n'; }
    o += 2;
    fi_copy(o, s.text + x.q_b, x.q_len, lane, nl);
    o += x.q_len;
    if (lane == 0) o[0] = '\n';
  }
}

// a wave per kept record (the records of FI_LONG output bytes and more are left to the kernel below)
__global__ __launch_bounds__(256)
void filter_gather_kernel(const FiSide s, const u64 *__restrict__ found, u64 n_rec) {
  const u64 nw = (u64)gridDim.x * 4;
  for (u64 r = (u64)blockIdx.x * 4 + wave_id(); r < n_rec; r += nw) {
    const u64 sz = s.off[r + 1] - s.off[r];
    if (sz == 0 || sz >= FI_LONG) continue;
    fi_emit_record(s, r, found[r], lane_id(), 64);
  }
}
// a workgroup per long record
__global__ __launch_bounds__(256)
void filter_gather_long_kernel(const FiSide s, const u64 *__restrict__ found, u64 n_rec) {
  for (u64 r = blockIdx.x; r < n_rec; r += gridDim.x) {
    if (s.off[r + 1] - s.off[r] < FI_LONG) continue;
    fi_emit_record(s, r, found[r], threadIdx.x, 256);
  }
}

}  // namespace mgc

// ================================================================================================
//  C ABI
// ================================================================================================
namespace {
using mgc::DBuf;
using mgc::u32;
using mgc::u64;

int fi_fail(int rc, const std::string &m) { mgc::lk_set_error(m); return rc; }
#define FI_HIP(expr) do { hipError_t e__ = (expr); if (e__ != hipSuccess) return fi_fail(MGC_EHIP, std::string("mgc_lookup_filter: " #expr ": ") + hipGetErrorString(e__)); } while (0)

struct FiInput {
  DBuf tiles, scr, ls, rl, rec, hb, he, bb, be, flat, off;
  u64 n = 0, n_lines = 0, nr_all = 0, nr = 0;   // nr: complete records of this piece; nr_all: record starts (FASTA)
  int fmt = 0;
};
struct FiWork { FiInput in[2]; DBuf found, misc; };
// the filter's buffers grow with a quarter of headroom (one workspace serves every piece of a file)
hipError_t fi_need(DBuf &b, size_t bytes) { return bytes <= b.cap ? hipSuccess : b.ensure(bytes + bytes / 4 + 256); }

// the compaction workspace of `tiles` tiles over an input's grow-only buffers; the total goes where the caller reads it
hipError_t fi_compact_ws(FiInput &S, u64 tiles, u64 *d_total, mgc::CompactWs *w) {
  MGC_CHECK(fi_need(S.tiles, 8 * (tiles + 2)));
  MGC_CHECK(fi_need(S.scr, 8 * mgc::compact_scratch_elems(tiles)));
  *w = {d_total, S.tiles.as<u64>(), S.scr.as<u64>(), tiles};
  return hipSuccess;
}

uint32_t fi_grid(u64 items, u64 per_block) { const u64 g = (items + per_block - 1) / per_block; return (uint32_t)(g ? g : 1); }

// lines and records of one piece
int fi_index(FiInput &S, const uint8_t *d_text, u64 n, bool final, u64 *d_misc, hipStream_t st) {
  S.n = n; S.n_lines = S.nr_all = S.nr = 0; S.fmt = 0;
  if (n == 0) return MGC_OK;
  const u64 tiles = (n + mgc::FI_TILE - 1) / mgc::FI_TILE;
  mgc::CompactWs w;
  FI_HIP(fi_compact_ws(S, tiles, d_misc + 0, &w));
  hipLaunchKernelGGL(mgc::filter_nl_kernel<false>, dim3((uint32_t)tiles), dim3(256), 0, st, d_text, n, w.tiles, (u64)0, 0u, (u64 *)nullptr);
  FI_HIP(mgc::compact_scan(w, st));
  hipLaunchKernelGGL(mgc::filter_meta_kernel, dim3(1), dim3(1), 0, st, d_text, n, d_misc);
  FI_HIP(hipGetLastError());
  u64 m[4];
  FI_HIP(hipMemcpyAsync(m, d_misc, sizeof(m), hipMemcpyDeviceToHost, st));
  FI_HIP(hipStreamSynchronize(st));
  const u64 nl = m[0];
  const bool open_tail = m[2] != 0;
  S.fmt = (int)m[1];
  if (!S.fmt) return fi_fail(MGC_EFORMAT, std::string("mgc_lookup_filter: a record starts with '") + (char)m[3] + "', neither '>' nor '@'");
  S.n_lines = nl + (open_tail ? 1 : 0);
  FI_HIP(fi_need(S.ls, 8 * (nl + 2)));
  hipLaunchKernelGGL(mgc::filter_nl_kernel<true>, dim3((uint32_t)tiles), dim3(256), 0, st, d_text, n, w.tiles, nl, open_tail ? 1u : 0u, S.ls.as<u64>());
  FI_HIP(hipGetLastError());
  if (S.fmt == MGC_TEXT_FASTQ) {
    if (final && S.n_lines % 4)
      return fi_fail(MGC_EFORMAT, "mgc_lookup_filter: the FASTQ text ends inside a record (" + std::to_string(S.n_lines) + " lines; four-line FASTQ only)");
    S.nr = final ? S.n_lines / 4 : (S.n_lines - 1) / 4;           // not final: a record is complete when another line start follows
    S.nr_all = S.nr;
    return MGC_OK;
  }
  const u64 ltiles = (S.n_lines + mgc::FI_LTILE - 1) / mgc::FI_LTILE;
  FI_HIP(fi_compact_ws(S, ltiles, d_misc + 4, &w));
  hipLaunchKernelGGL(mgc::filter_hdr_kernel<false>, dim3((uint32_t)ltiles), dim3(256), 0, st, d_text, S.ls.as<u64>(), S.n_lines, w.tiles, (u64)0,
                     (u64 *)nullptr);
  FI_HIP(mgc::compact_scan(w, st));
  FI_HIP(hipMemcpyAsync(&S.nr_all, d_misc + 4, 8, hipMemcpyDeviceToHost, st));
  FI_HIP(hipStreamSynchronize(st));
  FI_HIP(fi_need(S.rl, 8 * (S.nr_all + 1)));
  hipLaunchKernelGGL(mgc::filter_hdr_kernel<true>, dim3((uint32_t)ltiles), dim3(256), 0, st, d_text, S.ls.as<u64>(), S.n_lines, w.tiles, S.nr_all,
                     S.rl.as<u64>());
  FI_HIP(hipGetLastError());
  S.nr = final ? S.nr_all : S.nr_all - 1;                           // the last record is complete only when the input ends here
  return MGC_OK;
}

// where record `r` of a piece begins (n when the piece has no such record)
int fi_record_start(FiInput &S, u64 r, uint64_t *pos, hipStream_t st) {
  *pos = S.n;
  if (S.n == 0) return MGC_OK;
  u64 line = 0;
  if (S.fmt == MGC_TEXT_FASTQ) line = 4 * r;
  else if (r < S.nr_all) { FI_HIP(hipMemcpyAsync(&line, S.rl.as<u64>() + r, 8, hipMemcpyDeviceToHost, st)); FI_HIP(hipStreamSynchronize(st)); }
  else return MGC_OK;
  if (line >= S.n_lines) return MGC_OK;
  FI_HIP(hipMemcpyAsync(pos, S.ls.as<u64>() + line, 8, hipMemcpyDeviceToHost, st));
  FI_HIP(hipStreamSynchronize(st));
  return MGC_OK;
}

// One step.  final[i]: input i ends with its piece.  nr_piece[i] (may be null): the complete records each piece held.
int fi_step(FiWork &W, const mgc_lookup *t, int mode, uint32_t skip_first, uint32_t n_inputs, const uint8_t *const d_text[2],
            const uint64_t n_text[2], const bool final[2], bool equal_counts, uint8_t *const d_out[2], const uint64_t out_cap[2],
            mgc_filter_result *res, uint64_t nr_piece[2], hipStream_t st) {
  memset(res, 0, sizeof(*res));
  FI_HIP(hipSetDevice(t->device));
  FI_HIP(fi_need(W.misc, 8 * 16));
  u64 *d_misc = W.misc.as<u64>();
  FI_HIP(hipMemsetAsync(d_misc, 0, 8 * 16, st));
  for (uint32_t i = 0; i < n_inputs; i++) {
    const int rc = fi_index(W.in[i], d_text[i], n_text[i], final[i], d_misc, st);
    if (rc != MGC_OK) return rc;
    res->format[i] = (uint32_t)W.in[i].fmt;
    if (nr_piece) nr_piece[i] = W.in[i].nr;
  }
  const u64 NR = n_inputs == 2 ? std::min(W.in[0].nr, W.in[1].nr) : W.in[0].nr;
  if (equal_counts && n_inputs == 2 && W.in[0].nr != W.in[1].nr)
    return fi_fail(MGC_EINVAL, "mgc_lookup_filter: the inputs hold different numbers of records: " + std::to_string(W.in[0].nr) + " in the first, " +
                                   std::to_string(W.in[1].nr) + " in the second");
  if (NR >= 0xFFFFFFFFull) return fi_fail(MGC_EINVAL, "mgc_lookup_filter: more than 2^32 - 2 records in one piece");
  res->n_records = NR;
  for (uint32_t i = 0; i < n_inputs; i++) {
    const int rc = fi_record_start(W.in[i], NR, &res->consumed[i], st);
    if (rc != MGC_OK) return rc;
  }
  if (NR == 0) return MGC_OK;

  mgc::LkTable tab;
  tab.keys = t->d_keys.p; tab.vals = t->d_vals.as<u32>(); tab.index = t->d_index.as<const u64>();
  tab.n_index = 1ull << t->index_bits; tab.shift = t->shift; tab.reserved = 0;
  FI_HIP(fi_need(W.found, 8 * NR));
  u64 *d_found = W.found.as<u64>();
  FI_HIP(hipMemsetAsync(d_found, 0, 8 * NR, st));
  uint32_t *d_err = reinterpret_cast<uint32_t *>(d_misc + 9);
  mgc::FiSide side[2];
  memset(side, 0, sizeof(side));
  for (uint32_t i = 0; i < n_inputs; i++) {
    FiInput &S = W.in[i];
    const bool fasta = S.fmt == MGC_TEXT_FASTA;
    const u64 n = S.n, nspan = fasta ? S.nr_all : NR;
    FI_HIP(fi_need(S.rec, sizeof(mgc::FiRec) * nspan));
    if (fasta) { FI_HIP(fi_need(S.hb, 8 * nspan)); FI_HIP(fi_need(S.he, 8 * nspan)); FI_HIP(fi_need(S.bb, 8 * (nspan + 1))); FI_HIP(fi_need(S.flat, n)); }
    else       { FI_HIP(fi_need(S.bb, 8 * nspan)); FI_HIP(fi_need(S.be, 8 * nspan)); }
    hipLaunchKernelGGL(mgc::filter_spans_kernel, dim3(fi_grid(nspan, 256)), dim3(256), 0, st, d_text[i], n, S.ls.as<u64>(),
                       fasta ? S.rl.as<u64>() : (const u64 *)nullptr, nspan, S.rec.as<mgc::FiRec>(), S.hb.as<u64>(), S.he.as<u64>(),
                       S.bb.as<u64>(), S.be.as<u64>(), d_err);
    FI_HIP(hipGetLastError());
    const uint8_t *stream = d_text[i];
    if (fasta) {
      const u64 tiles = (n + mgc::FI_TILE - 1) / mgc::FI_TILE;
      mgc::CompactWs w;                                               // the total is bb[nspan]: where the last record's bases end
      FI_HIP(fi_compact_ws(S, tiles, S.bb.as<u64>() + nspan, &w));
      hipLaunchKernelGGL(mgc::filter_flat_kernel<false>, dim3((uint32_t)tiles), dim3(256), 0, st, d_text[i], n, S.hb.as<u64>(), S.he.as<u64>(), nspan,
                         w.tiles, (uint8_t *)nullptr, (u64 *)nullptr);
      FI_HIP(mgc::compact_scan(w, st));
      hipLaunchKernelGGL(mgc::filter_flat_kernel<true>, dim3((uint32_t)tiles), dim3(256), 0, st, d_text[i], n, S.hb.as<u64>(), S.he.as<u64>(), nspan,
                         w.tiles, S.flat.as<uint8_t>(), S.bb.as<u64>());
      FI_HIP(hipGetLastError());
      stream = S.flat.as<uint8_t>();
    }
    const u64 *d_be = fasta ? (const u64 *)nullptr : S.be.as<u64>();
    const uint32_t skip = i == 0 ? skip_first : 0u;                 // -10x: the first input only (include-exclude.C:92-93)
    const uint32_t g = fi_grid(n, 256 * mgc::LK_RUN);
    if (t->kw == 2)
      hipLaunchKernelGGL(mgc::filter_found_kernel<mgc::K128>, dim3(g), dim3(256), 0, st, tab, t->k, stream, n, S.bb.as<u64>(), d_be, NR, skip, d_found);
    else
      hipLaunchKernelGGL(mgc::filter_found_kernel<mgc::u64>, dim3(g), dim3(256), 0, st, tab, t->k, stream, n, S.bb.as<u64>(), d_be, NR, skip, d_found);
    FI_HIP(hipGetLastError());
    FI_HIP(fi_need(S.off, 8 * (NR + 1)));
    side[i].text = d_text[i]; side[i].stream = stream; side[i].rec = S.rec.as<mgc::FiRec>();
    side[i].bb = S.bb.as<u64>(); side[i].be = d_be; side[i].off = S.off.as<u64>(); side[i].out = d_out ? d_out[i] : nullptr;
  }
  hipLaunchKernelGGL(mgc::filter_size_kernel, dim3(fi_grid(NR, 256)), dim3(256), 0, st, d_found, NR, mode == MGC_FILTER_INCLUDE ? 1u : 0u, n_inputs,
                     side[0], side[1], d_misc + 8);
  FI_HIP(hipGetLastError());
  u64 totals[2] = {0, 0}, kept_err[2] = {0, 0};
  for (uint32_t i = 0; i < n_inputs; i++) {
    FiInput &S = W.in[i];
    FI_HIP(fi_need(S.scr, 8 * mgc::scan_scratch_elems(NR + 1)));
    FI_HIP(mgc::scan_u64_exclusive(S.off.as<u64>(), NR, S.scr.as<u64>(), S.off.as<u64>() + NR, st));
    FI_HIP(hipMemcpyAsync(&totals[i], S.off.as<u64>() + NR, 8, hipMemcpyDeviceToHost, st));
  }
  FI_HIP(hipMemcpyAsync(kept_err, d_misc + 8, 16, hipMemcpyDeviceToHost, st));
  FI_HIP(hipStreamSynchronize(st));
  if ((uint32_t)kept_err[1])
    return fi_fail(MGC_EFORMAT, (uint32_t)kept_err[1] == 1u ? "mgc_lookup_filter: a FASTQ record does not start with '@' (four-line FASTQ only; multi-line FASTQ is refused)"
                                                            : "mgc_lookup_filter: the third line of a FASTQ record does not start with '+' (four-line FASTQ only; multi-line FASTQ is refused)");
  res->n_kept = kept_err[0];
  bool fits = true;
  for (uint32_t i = 0; i < n_inputs; i++) {
    res->out_bytes[i] = totals[i];
    if (totals[i] && (!d_out || !d_out[i] || !out_cap || out_cap[i] < totals[i])) fits = false;
  }
  if (!fits)                                                        // nothing is written; out_bytes holds what is needed
    return fi_fail(MGC_EINVAL, "mgc_lookup_filter: an output buffer is too small (" + std::to_string(totals[0]) + " and " + std::to_string(totals[1]) + " bytes are needed)");
  for (uint32_t i = 0; i < n_inputs; i++) {
    if (!totals[i]) continue;
    hipLaunchKernelGGL(mgc::filter_gather_kernel, dim3(fi_grid(std::min<u64>(NR, 1u << 18), 4)), dim3(256), 0, st, side[i], d_found, NR);
    FI_HIP(hipGetLastError());
    hipLaunchKernelGGL(mgc::filter_gather_long_kernel, dim3((uint32_t)std::min<u64>(NR, 4096)), dim3(256), 0, st, side[i], d_found, NR);
    FI_HIP(hipGetLastError());
  }
  return MGC_OK;
}
}  // namespace

extern "C" int mgc_lookup_filter_text(const mgc_lookup *t, int mode, uint32_t skip_first, uint32_t n_inputs, const uint8_t *const d_text[2],
                                      const uint64_t n_text[2], int final, uint8_t *const d_out[2], const uint64_t out_cap[2],
                                      mgc_filter_result *res, void *stream) {
  if (!t || !res || !d_text || !n_text || n_inputs < 1 || n_inputs > 2 || (mode != MGC_FILTER_INCLUDE && mode != MGC_FILTER_EXCLUDE))
    return fi_fail(MGC_EINVAL, "mgc_lookup_filter_text: bad arguments");
  for (uint32_t i = 0; i < n_inputs; i++)
    if (n_text[i] && !d_text[i]) return fi_fail(MGC_EINVAL, "mgc_lookup_filter_text: no text");
  FiWork W;
  const bool fin[2] = {final != 0, final != 0};
  const int rc = fi_step(W, t, mode, skip_first, n_inputs, d_text, n_text, fin, final != 0, d_out, out_cap, res, nullptr, (hipStream_t)stream);
  (void)hipStreamSynchronize((hipStream_t)stream);                  // the workspace is released on return
  return rc;
}

// ---- whole files ----------------------------------------------------------------------------------------------------------
namespace {
struct FiFile {
  msr_reader *r = nullptr;
  char *h = nullptr;                  // pinned: what is left of the last piece, then what was read since
  uint64_t cap = 0, have = 0;
  bool eof = false;
  DBuf d_in, d_out;
  char *h_out = nullptr;
  uint64_t h_out_cap = 0;
  ~FiFile() { if (r) msr_close(r); if (h) (void)hipHostFree(h); if (h_out) (void)hipHostFree(h_out); }
  int grow(uint64_t c) {
    char *p = nullptr;
    FI_HIP(hipHostMalloc(reinterpret_cast<void **>(&p), c, hipHostMallocDefault));
    if (have) memcpy(p, h, have);
    if (h) (void)hipHostFree(h);
    h = p; cap = c;
    return MGC_OK;
  }
  int fill() {
    while (!eof && have < cap) {
      const int64_t got = msr_read_text(r, h + have, cap - have);
      if (got < 0) return fi_fail(MGC_EINVAL, std::string("mgc_lookup_filter_files: ") + msr_last_error());
      if (got == 0) eof = true; else have += (uint64_t)got;
    }
    return MGC_OK;
  }
  void consume(uint64_t c) { if (c > have) c = have; if (c < have) memmove(h, h + c, have - c); have -= c; }
};
}  // namespace

extern "C" int mgc_lookup_filter_files(const mgc_lookup *t, int mode, uint32_t skip_first, const char *path1, const char *path2,
                                       uint64_t batch_bytes, mgc_lookup_write_cb out1, void *user1, mgc_lookup_write_cb out2, void *user2,
                                       mgc_filter_result *totals) {
  if (!t || !path1 || !out1 || !totals || (path2 && !out2) || (mode != MGC_FILTER_INCLUDE && mode != MGC_FILTER_EXCLUDE))
    return fi_fail(MGC_EINVAL, "mgc_lookup_filter_files: bad arguments");
  memset(totals, 0, sizeof(*totals));
  if (batch_bytes == 0) batch_bytes = 64ull << 20;
  if (batch_bytes < 256) batch_bytes = 256;
  const uint32_t n_inputs = path2 ? 2u : 1u;
  const char *paths[2] = {path1, path2};
  mgc_lookup_write_cb cbs[2] = {out1, out2};
  void *users[2] = {user1, user2};
  FI_HIP(hipSetDevice(t->device));
  FiFile F[2];
  FiWork W;
  hipStream_t st = nullptr;
  for (uint32_t i = 0; i < n_inputs; i++) {
    F[i].r = msr_open(paths[i]);
    if (!F[i].r) return fi_fail(MGC_EINVAL, std::string("mgc_lookup_filter_files: ") + msr_last_error());
    if (msr_format(F[i].r) != MSR_FORMAT_FASTX) return fi_fail(MGC_EFORMAT, std::string("mgc_lookup_filter_files: '") + paths[i] + "' is not FASTA/FASTQ text");
    const int rc = F[i].grow(batch_bytes);
    if (rc != MGC_OK) return rc;
  }
  // the records an input still holds (the other one has ended): indexed, not looked up
  auto count_rest = [&](FiFile &f, FiInput &S, uint64_t *n) -> int {
    for (;;) {
      int rc = f.fill();
      if (rc != MGC_OK) return rc;
      if (f.have == 0) return MGC_OK;
      FI_HIP(fi_need(f.d_in, f.have));
      FI_HIP(fi_need(W.misc, 8 * 16));
      FI_HIP(hipMemcpyAsync(f.d_in.p, f.h, f.have, hipMemcpyHostToDevice, st));
      if ((rc = fi_index(S, f.d_in.as<uint8_t>(), f.have, f.eof, W.misc.as<u64>(), st)) != MGC_OK) return rc;
      uint64_t pos = 0;
      if ((rc = fi_record_start(S, S.nr, &pos, st)) != MGC_OK) return rc;
      *n += S.nr;
      if (f.eof) return MGC_OK;
      if (S.nr == 0 && (rc = f.grow(f.cap * 2)) != MGC_OK) return rc;
      f.consume(pos);
    }
  };
  for (;;) {
    const uint8_t *d_text[2] = {nullptr, nullptr};
    uint8_t *d_out[2] = {nullptr, nullptr};
    uint64_t n_text[2] = {0, 0}, out_cap[2] = {0, 0}, nr_piece[2] = {0, 0};
    bool fin[2] = {true, true};
    for (uint32_t i = 0; i < n_inputs; i++) {
      const int rc = F[i].fill();
      if (rc != MGC_OK) return rc;
      FI_HIP(fi_need(F[i].d_in, F[i].have));
      FI_HIP(fi_need(F[i].d_out, F[i].have + F[i].have / 4 + 4096));
      if (F[i].have) FI_HIP(hipMemcpyAsync(F[i].d_in.p, F[i].h, F[i].have, hipMemcpyHostToDevice, st));
      d_text[i] = F[i].d_in.as<uint8_t>(); n_text[i] = F[i].have; fin[i] = F[i].eof;
      d_out[i] = F[i].d_out.as<uint8_t>(); out_cap[i] = F[i].d_out.cap;
    }
    mgc_filter_result res;
    int rc = fi_step(W, t, mode, skip_first, n_inputs, d_text, n_text, fin, false, d_out, out_cap, &res, nr_piece, st);
    if (rc == MGC_EINVAL && (res.out_bytes[0] > out_cap[0] || res.out_bytes[1] > out_cap[1])) {   // a piece of many short records
      for (uint32_t i = 0; i < n_inputs; i++) { FI_HIP(fi_need(F[i].d_out, res.out_bytes[i])); d_out[i] = F[i].d_out.as<uint8_t>(); out_cap[i] = F[i].d_out.cap; }
      rc = fi_step(W, t, mode, skip_first, n_inputs, d_text, n_text, fin, false, d_out, out_cap, &res, nr_piece, st);
    }
    if (rc != MGC_OK) return rc;
    for (uint32_t i = 0; i < n_inputs; i++) {
      const uint64_t m = res.out_bytes[i];
      totals->format[i] = totals->format[i] ? totals->format[i] : res.format[i];
      if (!m) continue;
      if (F[i].h_out_cap < m) {
        if (F[i].h_out) (void)hipHostFree(F[i].h_out);
        F[i].h_out = nullptr; F[i].h_out_cap = 0;
        FI_HIP(hipHostMalloc(reinterpret_cast<void **>(&F[i].h_out), m + m / 4, hipHostMallocDefault));
        F[i].h_out_cap = m + m / 4;
      }
      FI_HIP(hipMemcpyAsync(F[i].h_out, d_out[i], m, hipMemcpyDeviceToHost, st));
    }
    FI_HIP(hipStreamSynchronize(st));
    for (uint32_t i = 0; i < n_inputs; i++) {
      if (!res.out_bytes[i]) continue;
      const int r = cbs[i](F[i].h_out, res.out_bytes[i], users[i]);
      if (r != 0) return fi_fail(MGC_ESTATE, "mgc_lookup_filter_files: the write callback returned " + std::to_string(r));
      totals->out_bytes[i] += res.out_bytes[i];
    }
    totals->n_records += res.n_records;
    totals->n_kept += res.n_kept;
    bool all_eof = true, some_done = false, all_done = true;
    for (uint32_t i = 0; i < n_inputs; i++) {
      totals->consumed[i] += res.consumed[i];
      F[i].consume(res.consumed[i]);
      all_eof = all_eof && F[i].eof;
      const bool done = F[i].eof && F[i].have == 0;
      some_done = some_done || done;
      all_done = all_done && done;
    }
    if (some_done && !all_done) {
      // one input has ended and the other has not: include-exclude.C:48-55 would go on with an empty sequence; here it is an error
      uint64_t cnt[2] = {totals->n_records, totals->n_records};
      for (uint32_t i = 0; i < 2; i++) { const int rc2 = count_rest(F[i], W.in[i], &cnt[i]); if (rc2 != MGC_OK) return rc2; }
      return fi_fail(MGC_EINVAL, "mgc_lookup_filter_files: the inputs hold different numbers of records: " + std::to_string(cnt[0]) + " in '" + paths[0] +
                                     "', " + std::to_string(cnt[1]) + " in '" + paths[1] + "'");
    }
    if (all_eof) break;
    if (res.n_records == 0)                                         // a record longer than its piece: a larger piece
      for (uint32_t i = 0; i < n_inputs; i++)
        if (!F[i].eof && nr_piece[i] == 0) { const int rc2 = F[i].grow(F[i].cap * 2); if (rc2 != MGC_OK) return rc2; }
  }
  return MGC_OK;
}
