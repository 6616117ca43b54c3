// mgc_list.hip -- k-mer text lists formatted on the device (gfx950): include/meryl_list.h.
//
// What the kernel replaces in the reference (paths relative to the reference root):
//   list_kernel<IPT, false> / <IPT, true>
//       printKmer: toString + toDec + toBin into a 256-byte line, then fputs under a lock
//                                              src/meryl2/merylOp-nextMer.C:24-50 (v1: src/meryl/merylOp-nextMer.C:673-676)
//       called once per k-mer by every action with a list
//                                              src/meryl2/merylOpTemplate.C:76-163
//
// A line is k letters + TAB + 1..10 digits [+ TAB + label_size bits] + NL: everything but the digits has one length per call.  The
// length pass (EMIT = false) sums the line lengths of a tile of k-mers and leaves one total per tile; the library's scan
// (compact_scan) turns the totals into the byte offset of every tile.  The format pass (EMIT = true) scans the line lengths
// inside the tile again (compact_slot, the same helper in both passes), writes every line into an LDS image of the tile's text and
// copies the image out in whole 16-byte words; the image is laid out at the misalignment of its destination, so an LDS word IS a
// destination word, and only the bytes before the first and after the last whole word are stored one by one (the neighbouring
// tiles own the rest of those two words).  HBM sees lines, not characters.
//
// Tile size.  The longest line has k + 1 + 10 + (label_size ? 1 + label_size : 0) + 1 bytes; max_line = mgc_list_max_line =
// k + 13 + label_size <= 141 bounds it (exactly with a label, by one byte without).  A tile is 256 threads x IPT k-mers with
// IPT = 4, 2 or 1, the largest for which 256 * IPT * max_line <= LS_IMG_BYTES = 36864: max_line <= 36 (k <= 23 without labels)
// takes 1024 k-mers, <= 72 takes 512, and the longest (141 * 256 = 36096) 256.  The image is
// LS_IMG_BYTES + 16 bytes for the misalignment = 36880 bytes of static LDS (limit 65536), beside the 20 bytes of the scan: four
// workgroups per CU.
#include "../../include/meryl_db.h"
#include "mgc_compact.hpp"
#include "mgc_list.hpp"
#include "mgc_session.hpp"

#include <algorithm>
#include <string>
#include <vector>

namespace mgc {

constexpr int LS_BLOCK = 256;
constexpr u32 LS_IMG_BYTES = 36864;                      // the text of one tile, at most
constexpr u32 LS_IMG_WORDS = LS_IMG_BYTES / 16 + 1;      // + the word the misalignment spills into

// the bytes of a line without its digits
__host__ __device__ inline u32 list_fixed_bytes(u32 k, u32 label_size) { return k + 1 + (label_size ? 1 + label_size : 0) + 1; }
inline u32 list_ipt(u32 max_line) { return max_line * 4 * LS_BLOCK <= LS_IMG_BYTES ? 4u : max_line * 2 * LS_BLOCK <= LS_IMG_BYTES ? 2u : 1u; }

__device__ __forceinline__ u32 dec_len(u32 v) {
  return 1u + (v >= 10u) + (v >= 100u) + (v >= 1000u) + (v >= 10000u) + (v >= 100000u) + (v >= 1000000u) + (v >= 10000000u) +
         (v >= 100000000u) + (v >= 1000000000u);
}

struct ListArgs {
  const void *keys; const u32 *vals; const u64 *labs;    // labs null: zeros
  u64 a, b;                                              // the k-mers [a, b) of the stream are listed
  u32 k, label_size, wide;
};

// Workgroup x takes tile tile0 + x of the stream (tiles is already moved up by tile0).
//   EMIT = false: tiles[x] <- the bytes of the tile's lines.
//   EMIT = true : tiles[x] is the byte offset of the tile's first line in the whole text, base_off that of k-mer a (the first tile
//                 of a piece may begin inside a tile: its clipped lines count nothing, and its text begins at base_off); the text
//                 goes to out + (offset - base_off).  piece_bytes (may be null; one-workgroup launches only) <- the tile's bytes.
template <int IPT, bool EMIT>
__global__ __launch_bounds__(LS_BLOCK)
void list_kernel(ListArgs A, u64 tile0, u64 *__restrict__ tiles, u64 base_off, uint8_t *__restrict__ out, u64 *__restrict__ piece_bytes) {
  const u64 first = (tile0 + blockIdx.x) * (u64)(LS_BLOCK * IPT) + (u64)threadIdx.x * IPT;
  const u32 fixed = list_fixed_bytes(A.k, A.label_size);
  u32 v[IPT], len[IPT], sum = 0;
#pragma unroll
  for (int q = 0; q < IPT; q++) {
    const u64 i = first + q;
    const bool in = i >= A.a && i < A.b;
    v[q] = in ? A.vals[i] : 0u;
    len[q] = in ? fixed + dec_len(v[q]) : 0u;
    sum += len[q];
  }
  u64 o = 0;
  u32 tot = 0;
  if (!compact_slot<LS_BLOCK, EMIT>(sum, tiles, &o, &tot)) return;
  if constexpr (EMIT) {
    __shared__ uint4 s_img[LS_IMG_WORDS];
    unsigned char *img = reinterpret_cast<unsigned char *>(s_img);
    const u64 tile_off = tiles[blockIdx.x];
    const u64 rel0 = (blockIdx.x == 0 ? base_off : tile_off) - base_off;     // where the tile's text begins in the piece
    const u32 mis = (u32)(rel0 & 15u);
    u32 p = mis + (u32)(o - tile_off);
#pragma unroll
    for (int q = 0; q < IPT; q++) {
      if (!len[q]) continue;
      const u64 i = first + q;
      u64 lo, hi = 0;
      if (A.wide) { const K128 kk = reinterpret_cast<const K128 *>(A.keys)[i]; lo = kk.lo; hi = kk.hi; }
      else lo = reinterpret_cast<const u64 *>(A.keys)[i];
      for (u32 b = 0; b < A.k; b++) {                          // A C T G = codes 0 1 2 3, most significant base first
        const u32 sh = 2 * (A.k - 1 - b);
        const u32 c = (u32)((sh >= 64 ? hi >> (sh - 64) : lo >> sh) & 3ull);
        img[p++] = (unsigned char)(0x47544341u >> (8 * c));
      }
      img[p++] = '\t';
      const u32 nd = len[q] - fixed;
      u32 x = v[q];
      for (u32 d = nd; d-- > 0;) {                             // x / 10 = (x * 0xCCCCCCCD) >> 35, exact for every uint32
        const u32 t = __umulhi(x, 0xCCCCCCCDu) >> 3;
        img[p + d] = (unsigned char)('0' + (x - t * 10u));
        x = t;
      }
      p += nd;
      if (A.label_size) {
        img[p++] = '\t';
        const u64 lab = A.labs ? A.labs[i] : 0ull;
        for (u32 b = 0; b < A.label_size; b++) img[p++] = (unsigned char)('0' + (u32)((lab >> (A.label_size - 1 - b)) & 1ull));
      }
      img[p++] = '\n';
    }
    __syncthreads();
    // image bytes [mis, end) -> out + rel0 - mis + the same index: whole words [w0, w1), the bytes around them singly
    const u32 end = mis + tot, w0 = (mis + 15u) >> 4, w1 = end >> 4;
    uint8_t *dst = out + (rel0 - mis);
    for (u32 w = w0 + threadIdx.x; w < w1; w += LS_BLOCK) reinterpret_cast<uint4 *>(dst)[w] = s_img[w];
    const u32 head_end = min(16u * w0, end), tail = max(16u * w1, head_end);
    if (threadIdx.x < 16) {
      const u32 b = mis + threadIdx.x;
      if (b < head_end) dst[b] = img[b];
    } else if (threadIdx.x < 32) {
      const u32 b = tail + threadIdx.x - 16;
      if (b < end) dst[b] = img[b];
    }
    if (piece_bytes && threadIdx.x == 0) *piece_bytes = tot;
  }
}

template <bool EMIT>
static hipError_t launch_list(u32 ipt, const ListArgs &A, u64 tile0, u64 n_tiles, u64 *tiles, u64 base_off, uint8_t *out, u64 *piece_bytes, hipStream_t st) {
  const dim3 g((uint32_t)n_tiles), b(LS_BLOCK);
  if (ipt == 4)      hipLaunchKernelGGL((list_kernel<4, EMIT>), g, b, 0, st, A, tile0, tiles + tile0, base_off, out, piece_bytes);
  else if (ipt == 2) hipLaunchKernelGGL((list_kernel<2, EMIT>), g, b, 0, st, A, tile0, tiles + tile0, base_off, out, piece_bytes);
  else               hipLaunchKernelGGL((list_kernel<1, EMIT>), g, b, 0, st, A, tile0, tiles + tile0, base_off, out, piece_bytes);
  return hipGetLastError();
}

struct ListStage {
  DBuf d_stage[2], ws;
  void *h_stage[2] = {nullptr, nullptr};
  size_t cap = 0;
  hipStream_t xs = nullptr;
  hipEvent_t ev_fmt[2] = {nullptr, nullptr}, ev_cp[2] = {nullptr, nullptr};
  std::vector<u64> h_tiles;
  hipError_t init() {
    if (xs) return hipSuccess;
    MGC_CHECK(hipStreamCreateWithFlags(&xs, hipStreamNonBlocking));
    for (int i = 0; i < 2; i++) {
      MGC_CHECK(hipEventCreateWithFlags(&ev_fmt[i], hipEventDisableTiming));
      MGC_CHECK(hipEventCreateWithFlags(&ev_cp[i], hipEventDisableTiming));
    }
    return hipSuccess;
  }
  // grow-only, in steps of at least a doubling so that 64 slices of growing size do not pin 64 times; nothing is in flight between listings
  hipError_t ensure(size_t bytes, size_t most) {
    if (bytes <= cap) return hipSuccess;
    bytes = std::min(most, std::max(bytes, 2 * cap));
    for (int i = 0; i < 2; i++) {
      if (h_stage[i]) { (void)hipHostFree(h_stage[i]); h_stage[i] = nullptr; }
      cap = 0;
      MGC_CHECK(d_stage[i].ensure(bytes));
      MGC_CHECK(hipHostMalloc(&h_stage[i], bytes, hipHostMallocDefault));
    }
    cap = bytes;
    return hipSuccess;
  }
  ~ListStage() {
    if (xs) (void)hipStreamSynchronize(xs);
    for (int i = 0; i < 2; i++) {
      if (h_stage[i]) (void)hipHostFree(h_stage[i]);
      if (ev_fmt[i]) (void)hipEventDestroy(ev_fmt[i]);
      if (ev_cp[i]) (void)hipEventDestroy(ev_cp[i]);
    }
    if (xs) (void)hipStreamDestroy(xs);
  }
};

ListStage *list_stage_open() { return new ListStage; }
void list_stage_close(ListStage *s) { delete s; }

#define LS_HIP(expr)                                                                              \
  do {                                                                                            \
    hipError_t e__ = (expr);                                                                      \
    if (e__ != hipSuccess) {                                                                      \
      mgc::set_err(nullptr, "%s: %s -> %s", who, #expr, hipGetErrorString(e__));                  \
      return (e__ == hipErrorOutOfMemory) ? MGC_ENOMEM : MGC_EHIP;                                \
    }                                                                                             \
  } while (0)

static int list_check(uint64_t n, const void *d_keys, const uint32_t *d_values, uint32_t k, uint32_t label_size, uint64_t chunk_bytes,
                      mgc_list_write_cb cb, const char *who) {
  if (k < 1 || k > 64) { set_err(nullptr, "%s: k = %u is outside 1..64", who, k); return MGC_EINVAL; }
  if (label_size > 64) { set_err(nullptr, "%s: a label has at most 64 bits, not %u", who, label_size); return MGC_EINVAL; }
  if (chunk_bytes < mgc_list_max_line(k, label_size)) {
    set_err(nullptr, "%s: chunk_bytes %llu is shorter than the longest line (%u bytes)", who, (unsigned long long)chunk_bytes, mgc_list_max_line(k, label_size));
    return MGC_EINVAL;
  }
  if (!cb) { set_err(nullptr, "%s: no callback", who); return MGC_EINVAL; }
  if (n && (!d_keys || !d_values)) { set_err(nullptr, "%s: a NULL array of %llu k-mers", who, (unsigned long long)n); return MGC_EINVAL; }
  return MGC_OK;
}

// the pieces of one listing: piece j is formatted into d_stage[j & 1] on st, copied to h_stage[j & 1] on xs, and handed to the
// callback while piece j + 1 is formatted
static int list_pieces(ListStage *s, const void *d_keys, const uint32_t *d_values, const uint64_t *d_labels, uint64_t n, uint32_t k,
                       uint32_t label_size, uint64_t chunk_bytes, mgc_list_write_cb cb, void *user, hipStream_t st, const char *who) {
  const u32 max_line = mgc_list_max_line(k, label_size), ipt = list_ipt(max_line);
  chunk_bytes = std::min<uint64_t>(chunk_bytes, 1ull << 40);   // (sums of offsets and chunk_bytes stay far from 2^64)
  const u64 T = (u64)LS_BLOCK * ipt, nt = (n + T - 1) / T;
  LS_HIP(s->init());
  LS_HIP(s->ws.ensure(8 * compact_ws_elems(nt)));
  const CompactWs w = compact_ws_at(s->ws.p, nt);
  ListArgs A{d_keys, d_values, reinterpret_cast<const u64 *>(d_labels), 0, n, k, label_size, k > 32 ? 1u : 0u};
  // the length pass, the scan, and the tile offsets on the host: h_tiles[t] = the byte offset of tile t, h_tiles[nt] = the bytes of all
  LS_HIP(launch_list<false>(ipt, A, 0, nt, w.tiles, 0, nullptr, nullptr, st));
  LS_HIP(compact_scan(w, st));
  s->h_tiles.resize(nt + 1);
  LS_HIP(hipMemcpyAsync(s->h_tiles.data(), w.tiles, 8 * nt, hipMemcpyDeviceToHost, st));
  LS_HIP(hipMemcpyAsync(s->h_tiles.data() + nt, w.total, 8, hipMemcpyDeviceToHost, st));
  LS_HIP(hipStreamSynchronize(st));
  const std::vector<u64> &off = s->h_tiles;
  const u64 total = off[nt];
  LS_HIP(s->ensure((size_t)std::min<u64>(chunk_bytes, total), (size_t)chunk_bytes));
  u64 *d_piece_bytes = w.total + 1;                          // (the workspace's first eight words are the total's)
  u64 a = 0, off_a = 0, piece = 0, pending_bytes = 0;
  bool pending = false;
  auto deliver = [&](int slot) -> int {
    LS_HIP(hipEventSynchronize(s->ev_cp[slot]));
    const int r = cb(s->h_stage[slot], pending_bytes, user);
    if (r != 0) { set_err(nullptr, "%s: the write callback returned %d", who, r); return MGC_ESTATE; }
    return MGC_OK;
  };
  while (a < n) {
    // the k-mers of the piece by a search over the tile offsets: up to the last tile boundary the piece can reach; where it
    // reaches none (a piece smaller than the rest of its tile), as many k-mers of the tile as fit whatever their values, and the
    // kernel says how many bytes they were.  That second form waits for the stream and reads 8 bytes back per piece, so piece j + 1 is not
    // formatted while piece j is copied: the double buffering degenerates there.  Only a chunk_bytes below a tile's text reaches it (tests).
    const u64 ta = a / T;
    const u64 e = (u64)(std::upper_bound(off.begin() + ta + 1, off.end(), off_a + chunk_bytes) - off.begin()) - 1;
    const bool whole_tiles = e > ta;
    const u64 b = whole_tiles ? std::min<u64>(e * T, n) : std::min<u64>(std::min<u64>(a + chunk_bytes / max_line, (ta + 1) * T), n);
    u64 bytes = whole_tiles ? off[e] - off_a : 0;
    const int slot = (int)(piece & 1);
    if (piece >= 2) LS_HIP(hipStreamWaitEvent(st, s->ev_cp[slot], 0));     // piece - 2 has left d_stage[slot]
    A.a = a; A.b = b;
    LS_HIP(launch_list<true>(ipt, A, ta, (b + T - 1) / T - ta, w.tiles, off_a, s->d_stage[slot].as<uint8_t>(), whole_tiles ? nullptr : d_piece_bytes, st));
    if (!whole_tiles) {
      LS_HIP(hipMemcpyAsync(&bytes, d_piece_bytes, 8, hipMemcpyDeviceToHost, st));
      LS_HIP(hipStreamSynchronize(st));
      if (bytes == 0 || bytes > chunk_bytes) { set_err(nullptr, "%s: a piece of %llu bytes", who, (unsigned long long)bytes); return MGC_ESTATE; }
    }
    LS_HIP(hipEventRecord(s->ev_fmt[slot], st));
    LS_HIP(hipStreamWaitEvent(s->xs, s->ev_fmt[slot], 0));
    LS_HIP(hipMemcpyAsync(s->h_stage[slot], s->d_stage[slot].p, bytes, hipMemcpyDeviceToHost, s->xs));
    LS_HIP(hipEventRecord(s->ev_cp[slot], s->xs));
    if (pending) { const int rc = deliver(slot ^ 1); if (rc != MGC_OK) return rc; }
    pending = true;
    pending_bytes = bytes;
    a = b; off_a += bytes; piece++;
  }
  if (pending) return deliver((int)((piece - 1) & 1));
  return MGC_OK;
}

int list_kmers(ListStage *s, const void *d_keys, const uint32_t *d_values, const uint64_t *d_labels, uint64_t n, uint32_t k, uint32_t label_size,
               uint64_t chunk_bytes, mgc_list_write_cb cb, void *user, hipStream_t st, const char *who) {
  int rc = list_check(n, d_keys, d_values, k, label_size, chunk_bytes, cb, who);
  if (rc != MGC_OK || n == 0) return rc;
  rc = list_pieces(s, d_keys, d_values, d_labels, n, k, label_size, chunk_bytes, cb, user, st, who);
  if (rc != MGC_OK) {                                        // a piece may still be on its way: the buffers are reused or freed next
    (void)hipStreamSynchronize(st);
    if (s->xs) (void)hipStreamSynchronize(s->xs);
  }
  return rc;
}

}  // namespace mgc

// k letters, TAB, ten digits, TAB, label_size bits, NL: exact with a label; a list without labels has no second TAB and its longest
// line is one byte shorter than this bound
extern "C" uint32_t mgc_list_max_line(uint32_t k, uint32_t label_size) { return k + 1 + 10 + 1 + label_size + 1; }

extern "C" uint32_t mgc_list_tile_kmers(uint32_t k, uint32_t label_size) {
  if (k < 1 || k > 64 || label_size > 64) return 0;
  return mgc::LS_BLOCK * mgc::list_ipt(mgc_list_max_line(k, label_size));
}

extern "C" size_t mgc_list_slice_name(const char *name, uint32_t file, char *buf, size_t buf_size) {
  const char *h = name ? strchr(name, '#') : nullptr;
  if (!h) return 0;
  size_t run = 0;
  while (h[run] == '#') run++;
  char digits[72];
  const int nd = snprintf(digits, sizeof(digits), "%0*u", (int)std::min<size_t>(std::max<size_t>(run, 2), 64), file);
  const size_t head = (size_t)(h - name), tail = strlen(h + run), len = head + (size_t)nd + tail;
  if (!buf || buf_size < len + 1) return 0;
  memcpy(buf, name, head);
  memcpy(buf + head, digits, (size_t)nd);
  memcpy(buf + head + nd, h + run, tail + 1);
  return len;
}

// ---- the two passes on their own, device to device ----
extern "C" size_t mgc_dev_list_workspace_bytes(uint64_t n, uint32_t k, uint32_t label_size) {
  const uint32_t T = mgc_list_tile_kmers(k, label_size);
  return T ? 8 * mgc::compact_ws_elems((n + T - 1) / T) : 0;
}

static int dev_list_check(const char *who, const uint32_t *d_values, uint64_t n, uint32_t k, uint32_t label_size, void *d_ws, size_t ws_bytes) {
  if (k < 1 || k > 64 || label_size > 64) { mgc::set_err(nullptr, "%s: k outside 1..64, or a label of more than 64 bits", who); return MGC_EINVAL; }
  if (!d_ws || ws_bytes < mgc_dev_list_workspace_bytes(n, k, label_size) || (n && !d_values)) { mgc::set_err(nullptr, "%s: bad arguments", who); return MGC_EINVAL; }
  return MGC_OK;
}

extern "C" int mgc_dev_list_lengths(const uint32_t *d_values, uint64_t n, uint32_t k, uint32_t label_size, void *d_ws, size_t ws_bytes,
                                    uint64_t *n_bytes, void *stream) {
  const char *who = "mgc_dev_list_lengths";
  const int rc = dev_list_check(who, d_values, n, k, label_size, d_ws, ws_bytes);
  if (rc != MGC_OK) return rc;
  const mgc::u64 T = mgc_list_tile_kmers(k, label_size), nt = (n + T - 1) / T;
  const mgc::CompactWs w = mgc::compact_ws_at(d_ws, nt);
  hipStream_t st = (hipStream_t)stream;
  const mgc::ListArgs A{nullptr, d_values, nullptr, 0, n, k, label_size, k > 32 ? 1u : 0u};
  if (nt) LS_HIP(mgc::launch_list<false>((mgc::u32)(T / mgc::LS_BLOCK), A, 0, nt, w.tiles, 0, nullptr, nullptr, st));
  LS_HIP(mgc::compact_scan(w, st));
  if (n_bytes) {
    mgc::u64 total = 0;
    LS_HIP(hipMemcpyAsync(&total, w.total, 8, hipMemcpyDeviceToHost, st));
    LS_HIP(hipStreamSynchronize(st));
    *n_bytes = total;
  }
  return MGC_OK;
}

extern "C" int mgc_dev_list_format(const void *d_keys, const uint32_t *d_values, const uint64_t *d_labels_or_null, uint64_t n, uint32_t k,
                                   uint32_t label_size, void *d_ws, size_t ws_bytes, void *d_text, void *stream) {
  const char *who = "mgc_dev_list_format";
  const int rc = dev_list_check(who, d_values, n, k, label_size, d_ws, ws_bytes);
  if (rc != MGC_OK) return rc;
  if (n == 0) return MGC_OK;
  if (!d_keys || !d_text || (reinterpret_cast<uintptr_t>(d_text) & 15u)) { mgc::set_err(nullptr, "%s: no k-mers, or no 16-byte aligned text buffer", who); return MGC_EINVAL; }
  const mgc::u64 T = mgc_list_tile_kmers(k, label_size), nt = (n + T - 1) / T;
  const mgc::CompactWs w = mgc::compact_ws_at(d_ws, nt);
  const mgc::ListArgs A{d_keys, d_values, reinterpret_cast<const mgc::u64 *>(d_labels_or_null), 0, n, k, label_size, k > 32 ? 1u : 0u};
  LS_HIP(mgc::launch_list<true>((mgc::u32)(T / mgc::LS_BLOCK), A, 0, nt, w.tiles, 0, reinterpret_cast<uint8_t *>(d_text), nullptr, (hipStream_t)stream));
  return MGC_OK;
}

extern "C" int mgc_list_kmers(const void *d_keys, const uint32_t *d_values, const uint64_t *d_labels_or_null, uint64_t n, uint32_t k,
                              uint32_t label_size, uint64_t chunk_bytes, mgc_list_write_cb cb, void *user, void *stream) {
  const int rc = mgc::list_check(n, d_keys, d_values, k, label_size, chunk_bytes, cb, "mgc_list_kmers");
  if (rc != MGC_OK || n == 0) return rc;
  mgc::ListStage stage;
  return mgc::list_kmers(&stage, d_keys, d_values, d_labels_or_null, n, k, label_size, chunk_bytes, cb, user, (hipStream_t)stream, "mgc_list_kmers");
}
