// mgc_lookup.hip -- the exact k-mer lookup table (include/meryl_lookup.h), gfx950.
//
// Replaces merylExactLookup [meryl-utility, not in tree] as meryl-lookup uses it: load(db, ..., minValue, maxValue)
// (src/meryl-lookup/meryl-lookup.C:36-100), value(kmer) / nKmers() per k-mer of a sequence
// (src/meryl-lookup/existence.C:63-82).  The table is the sorted (k-mer, value) stream itself plus a direct index over
// the top bits: index read -> binary search among the few k-mers sharing those bits.  Integer work bound by HBM/L2
// latency, not bandwidth: queries are batched so that thousands of searches are in flight per CU.
#include "mgc_lookup_dev.hpp"
#include "mgc_compact.hpp"
#include "mgc_dbfile.hpp"

#include <algorithm>
#include <atomic>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

namespace mgc {

template <typename K>
__global__ __launch_bounds__(256)
void lookup_values_kernel(const K *__restrict__ keys, const u32 *__restrict__ vals, const u64 *__restrict__ index, u32 shift,
                          const K *__restrict__ q, u64 n, u32 *__restrict__ out, u64 n_index) {
  const u64 stride = (u64)gridDim.x * blockDim.x;
  // queries come from the caller as they are: one with bits above 2k must not index past the table
  for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = lk_find<K>(keys, vals, index, shift, q[i], n_index);
}

template <typename K>
__global__ __launch_bounds__(256)
void lookup_stream_kernel(const K *__restrict__ keys, const u32 *__restrict__ vals, const u64 *__restrict__ index, u32 shift,
                          const uint8_t *__restrict__ bases, u64 n_bases, u32 k, u32 *__restrict__ out) {
  const u64 i0 = ((u64)blockIdx.x * blockDim.x + threadIdx.x) * LK_RUN;
  if (i0 >= n_bases) return;
  for (int q = 0; q < LK_RUN; q++) if (i0 + q < n_bases) out[i0 + q] = 0;
  lk_walk<K>(keys, vals, index, shift, bases, n_bases, k, i0, [&](u64 s, u32 v) { out[s] = v; });
}

template <typename K>
__global__ __launch_bounds__(256)
void lookup_existence_kernel(const K *__restrict__ keys, const u32 *__restrict__ vals, const u64 *__restrict__ index, u32 shift,
                             const uint8_t *__restrict__ bases, u64 n_bases, u32 k, const u64 *__restrict__ seq_start, u64 n_seq,
                             u64 *__restrict__ total, u64 *__restrict__ found) {
  const u64 i0 = ((u64)blockIdx.x * blockDim.x + threadIdx.x) * LK_RUN;
  if (i0 >= n_bases || n_seq == 0) return;
  u64 cur = ~0ull, tot = 0, fnd = 0;
  auto flush = [&]() {
    if (cur != ~0ull && tot) {
      atomicAdd(reinterpret_cast<unsigned long long *>(total + cur), (unsigned long long)tot);
      if (fnd) atomicAdd(reinterpret_cast<unsigned long long *>(found + cur), (unsigned long long)fnd);
    }
    tot = 0; fnd = 0;
  };
  lk_walk<K>(keys, vals, index, shift, bases, n_bases, k, i0, [&](u64 s, u32 v) {
    if (cur == ~0ull || s >= seq_start[cur + 1]) {   // the window's sequence: last start <= s
      flush();
      u64 lo = 0, hi = n_seq;
      while (hi - lo > 1) { const u64 mid = lo + ((hi - lo) >> 1); if (seq_start[mid] <= s) lo = mid; else hi = mid; }
      cur = lo;
    }
    if (s + k <= seq_start[cur + 1]) { tot++; fnd += (v != 0); }     // a window must lie inside its sequence
  });
  flush();
}

// ---- value filter (minValue <= v <= maxValue), order-preserving: count per tile, scan, emit ----------------------
constexpr int FL_TILE = 256 * 8;
// (the count pass reads no key: it is instantiated for u64 alone and launched without keys or outputs)
template <typename K, bool EMIT>
__global__ __launch_bounds__(256)
void filter_kernel(const K *__restrict__ keys, const u32 *__restrict__ vals, u64 n, u64 vmin, u64 vmax,
                   u64 *__restrict__ tiles /*EMIT: exclusive bases*/, K *__restrict__ out_k, u32 *__restrict__ out_v) {
  const u64 base = (u64)blockIdx.x * FL_TILE + (u64)threadIdx.x * 8;
  u32 keep = 0;
  for (int q = 0; q < 8; q++) { const u64 i = base + q; if (i < n) { const u64 v = vals[i]; keep |= (u32)(v >= vmin && v <= vmax) << q; } }
  u64 o;
  if (!compact_slot<256, EMIT>(__popc(keep), tiles, &o)) return;
  for (int q = 0; q < 8; q++)
    if ((keep >> q) & 1u) { out_k[o] = keys[base + q]; out_v[o] = vals[base + q]; o++; }
}


// ================================================================================================
//  Position reports of meryl-lookup: -bed, -bed-runs, -wig-count, -wig-depth (src/meryl-lookup/dump.C)
// ================================================================================================
// dump.C:109-135 (presence: bit t = table t holds fmer or rmer), :146-164 (count: value(f) + value(r), value(f) alone for a
// palindrome, summed over the tables in uint32 -- it wraps), :222-233 (depth: presence in table 0 only)
template <typename K, int WHAT>
__device__ __forceinline__ u32 lk_probe(const LkSet &set, K f, K r, bool pal) {
  u32 acc = 0;
  const u32 nt = WHAT == MGC_LOOKUP_DEPTH ? 1u : set.n;
  for (u32 t = 0; t < nt; t++) {
    const LkTable &d = set.t[t];
    const K *keys = reinterpret_cast<const K *>(d.keys);
    const u32 fv = lk_find<K>(keys, d.vals, d.index, d.shift, f, d.n_index);
    if (WHAT == MGC_LOOKUP_COUNT) {
      acc += fv;
      if (!pal) acc += lk_find<K>(keys, d.vals, d.index, d.shift, r, d.n_index);
    } else {
      const bool hit = fv != 0 || (!pal && lk_find<K>(keys, d.vals, d.index, d.shift, r, d.n_index) != 0);
      acc |= (u32)hit << t;
    }
  }
  return acc;
}

template <typename K, int WHAT>
__global__ __launch_bounds__(256)
void lookup_positions_kernel(const LkSet set, const uint8_t *__restrict__ bases, u64 n_bases, u32 *__restrict__ out) {
  const u64 i0 = ((u64)blockIdx.x * blockDim.x + threadIdx.x) * LK_RUN;
  if (i0 >= n_bases) return;
  for (int q = 0; q < LK_RUN; q++) if (i0 + q < n_bases) out[i0 + q] = 0;
  lk_roll<K>(bases, n_bases, set.k, i0, [&](u64 s, K f, K r, bool pal) { out[s] = lk_probe<K, WHAT>(set, f, r, pal); });
}

// depth[i] = number of table-0 windows starting in i-k+1 .. i (dump.C:222-241 builds it as +1 / -1 at each found window's
// begin / end and a prefix sum).  One workgroup = 4096 bases: waves 0-3 flag the windows starting in the tile, four lanes of
// wave 4 the (k-1 <= 63)-window halo before it, into LDS; then every base sums its k flags (sliding over its 16 bases).  Windows
// never cross a non-ACGT byte, so a sequence boundary needs no special case.
constexpr int LK_DEPTH_TILE = 256 * LK_RUN;
constexpr int LK_HALO = 64;
template <typename K>
__global__ __launch_bounds__(320)
void lookup_depth_kernel(const LkSet set, const uint8_t *__restrict__ bases, u64 n_bases, u32 *__restrict__ out) {
  __shared__ uint8_t s_hit[LK_HALO + LK_DEPTH_TILE];
  const u64 b0 = (u64)blockIdx.x * LK_DEPTH_TILE;
  const u32 tid = threadIdx.x;
  const bool main = tid < 256;
  const u32 h = tid - 256;                                    // halo lane (wave 4)
  const bool halo = !main && h < (u32)(LK_HALO / LK_RUN);
  const u32 slot = main ? LK_HALO + tid * LK_RUN : h * LK_RUN;
  if (main || halo) {
    for (int q = 0; q < LK_RUN; q++) s_hit[slot + q] = 0;
    const u64 i0 = main ? b0 + (u64)tid * LK_RUN : b0 - LK_HALO + (u64)h * LK_RUN;
    if ((main || b0 >= (u64)LK_HALO) && i0 < n_bases)
      lk_roll<K>(bases, n_bases, set.k, i0, [&](u64 s, K f, K r, bool pal) {
        s_hit[slot + (u32)(s - i0)] = (uint8_t)lk_probe<K, MGC_LOOKUP_DEPTH>(set, f, r, pal);
      });
  }
  __syncthreads();
  if (!main) return;
  const u64 i_first = b0 + (u64)tid * LK_RUN;
  if (i_first >= n_bases) return;
  const u32 k = set.k;                                        // 1..64: slot - (k - 1) >= 0
  u32 d = 0;
  for (u32 j = 0; j < k; j++) d += s_hit[slot - j];
  for (int q = 0; q < LK_RUN; q++) {
    if (i_first + q >= n_bases) break;
    if (q) d += (u32)s_hit[slot + q] - (u32)s_hit[slot + q - k];
    out[i_first + q] = d;
  }
}

// ---- text (dump.C:251-298 outputBED, :302-364 outputBEDruns, :368-405 outputWIG) ----------------------------------------
// Without labels only one flag is kept, "found in any table" (dump.C:127-131).
__device__ __forceinline__ u32 rp_eff(u32 m, u32 any_only) { return any_only ? (u32)(m != 0) : m; }
// tables whose run of flags ends just before p: p is the run's E, the first position after it (dump.C:329-350).  The base
// before a sequence's first one is its predecessor's trailing breaker, whose flags are 0.
__device__ __forceinline__ u32 rp_fall(const u32 *__restrict__ val, u64 p, u32 any_only) {
  const u32 prev = p ? rp_eff(val[p - 1], any_only) : 0u;
  return prev & ~rp_eff(val[p], any_only);
}
__device__ __forceinline__ u32 rp_edge(const u32 *__restrict__ val, u64 p, u32 t, u32 any_only) {
  const u32 cur = (rp_eff(val[p], any_only) >> t) & 1u;
  const u32 prev = p ? (rp_eff(val[p - 1], any_only) >> t) & 1u : 0u;
  return cur ^ prev;
}

__global__ __launch_bounds__(256)
void runs_lines_kernel(const u32 *__restrict__ val, u64 n, u32 any_only, u64 *__restrict__ lines) {
  const u64 stride = (u64)gridDim.x * blockDim.x;
  for (u64 p = (u64)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += stride) lines[p] = (u64)__popc(rp_fall(val, p, any_only));
}
// rising and falling edges of table t's flags, compacted in order (count per tile, scan, emit): they alternate, so the j-th
// run of the table is [edges[2j], edges[2j+1]) -- no thread walks a run
template <bool EMIT>
__global__ __launch_bounds__(256)
void runs_edge_kernel(const u32 *__restrict__ val, u64 n, u32 t, u32 any_only, u64 *__restrict__ tiles /*EMIT: exclusive bases*/,
                      u64 *__restrict__ edges) {
  const u64 base = (u64)blockIdx.x * FL_TILE + (u64)threadIdx.x * 8;
  u32 edge = 0;
  for (int q = 0; q < 8; q++) { const u64 i = base + q; if (i < n) edge |= rp_edge(val, i, t, any_only) << q; }
  u64 o;
  if (!compact_slot<256, EMIT>(__popc(edge), tiles, &o)) return;
  for (int q = 0; q < 8; q++) if ((edge >> q) & 1u) edges[o++] = base + q;
}
// run j of table t -> its line: lines[E] (exclusive scan of the lines per position) + the tables before t that also end at E
__global__ __launch_bounds__(256)
void runs_pair_kernel(const u64 *__restrict__ edges, u64 n_runs, const u32 *__restrict__ val, u64 n, const u64 *__restrict__ lines,
                      u32 t, u32 any_only, u64 *__restrict__ run_bgn) {
  const u64 stride = (u64)gridDim.x * blockDim.x;
  for (u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x; j < n_runs; j += stride) {
    const u64 e = edges[2 * j + 1];
    if (e >= n) continue;                                     // cannot happen: every sequence ends with a breaker
    const u32 below = rp_fall(val, e, any_only) & ((1u << t) - 1u);
    run_bgn[lines[e] + __popc(below)] = edges[2 * j];
  }
}

struct RpCtx {
  const u32 *val;                    // per position: presence mask / count / depth
  const u64 *seq_start;              // n_seq + 1: seq_start[0] = 0, seq_start[n_seq] = n_bases
  u64 n_seq;
  const char *names; const u64 *name_off;
  const char *labels; const u64 *label_off;
  const u64 *lines, *run_bgn;        // -bed-runs: first line of each position, begin of each line
  u32 n_labels, k, mode, any_only;
};

struct RpCount {                     // bytes only
  u64 o = 0;
  __device__ void put(char) { o++; }
  __device__ void put_str(const char *, u64 n) { o += n; }
  __device__ void put_dec(u64 x) { o += rp_dec_len(x); }
};
struct RpWrite {                     // the bytes [lo, hi) of the range's text land in buf[0, hi - lo)
  char *buf;
  u64 o, lo, hi;
  __device__ void at(u64 i, char c) { if (i >= lo && i < hi) buf[i - lo] = c; }
  __device__ void put(char c) { at(o++, c); }
  __device__ void put_str(const char *s, u64 n) { for (u64 i = 0; i < n; i++) at(o + i, s[i]); o += n; }
  __device__ void put_dec(u64 x) {   // toDec()
    const u32 l = rp_dec_len(x);
    if (x >> 32) { for (u32 j = l; j-- > 0;) { at(o + j, (char)('0' + x % 10)); x /= 10; } }
    else { u32 y = (u32)x; for (u32 j = l; j-- > 0;) { at(o + j, (char)('0' + y % 10u)); y /= 10u; } }
    o += l;
  }
};

// last sequence starting at or before p: the non-empty one that holds it
__device__ __forceinline__ u64 rp_seq(const u64 *__restrict__ ss, u64 n_seq, u64 p) {
  u64 lo = 0, hi = n_seq;
  while (hi - lo > 1) { const u64 mid = lo + ((hi - lo) >> 1); if (ss[mid] <= p) lo = mid; else hi = mid; }
  return lo;
}

// all lines of position p (sequence s)
template <typename O>
__device__ void rp_emit(const RpCtx &c, u64 p, u64 s, O &out) {
  const u64 ss = c.seq_start[s], loc = p - ss;
  if (c.mode == MGC_REPORT_WIG_COUNT || c.mode == MGC_REPORT_WIG_DEPTH) {
    if (loc == 0) {                                           // dump.C:377, for this sequence and the empty ones just before it
      u64 a = 0, b = s;
      while (a < b) { const u64 mid = a + ((b - a) >> 1); if (c.seq_start[mid] < p) a = mid + 1; else b = mid; }
      for (u64 q = a; q <= s; q++) {
        out.put_str("variableStep chrom=", 19);
        out.put_str(c.names + c.name_off[q], c.name_off[q + 1] - c.name_off[q]);
        out.put('\n');
      }
    }
    const u32 v = c.val[p];                                   // dump.C:387-401: zero prints nothing
    if (v) { out.put_dec(loc + 1); out.put('\t'); out.put_dec(v); out.put('\n'); }
    return;
  }
  const bool runs = c.mode == MGC_REPORT_BED_RUNS;
  u32 m = runs ? rp_fall(c.val, p, c.any_only) : rp_eff(c.val[p], c.any_only);
  if (!m) return;
  const char *nm = c.names + c.name_off[s];
  const u64 nl = c.name_off[s + 1] - c.name_off[s];
  u64 li = runs ? c.lines[p] : 0;
  while (m) {                                                 // table order (dump.C:275, :330)
    const u32 t = __ffs(m) - 1;
    m &= m - 1;
    out.put_str(nm, nl);
    out.put('\t');
    out.put_dec(runs ? c.run_bgn[li++] - ss : loc);
    out.put('\t');
    out.put_dec(loc + c.k);                                   // -bed: p + k; -bed-runs: E + k (dump.C:350)
    if (t < c.n_labels) { out.put('\t'); out.put_str(c.labels + c.label_off[t], c.label_off[t + 1] - c.label_off[t]); }
    out.put('\n');
  }
}

// bytes of every position of [a, b) -> len[p - a]
__global__ __launch_bounds__(256)
void report_len_kernel(const RpCtx c, u64 a, u64 b, u64 *__restrict__ len) {
  const u64 i0 = a + ((u64)blockIdx.x * blockDim.x + threadIdx.x) * LK_RUN;
  if (i0 >= b) return;
  u64 s = rp_seq(c.seq_start, c.n_seq, i0);
  for (int q = 0; q < LK_RUN; q++) {
    const u64 p = i0 + q;
    if (p >= b) break;
    while (c.seq_start[s + 1] <= p) s++;
    RpCount o;
    rp_emit(c, p, s, o);
    len[p - a] = o.o;
  }
}

// the bytes [lo, hi) of the text of positions [a, b): off = exclusive scan of len, off[b - a] = the range's total
__global__ __launch_bounds__(256)
void report_format_kernel(const RpCtx c, u64 a, u64 b, const u64 *__restrict__ off, u64 lo, u64 hi, char *__restrict__ buf) {
  u64 x = 0, y = b - a;                                       // the position whose text holds byte lo: last off <= lo
  while (y - x > 1) { const u64 mid = x + ((y - x) >> 1); if (off[mid] <= lo) x = mid; else y = mid; }
  const u64 stride = (u64)gridDim.x * blockDim.x * LK_RUN;
  for (u64 i0 = a + x + ((u64)blockIdx.x * blockDim.x + threadIdx.x) * LK_RUN; i0 < b && off[i0 - a] < hi; i0 += stride) {
    u64 s = rp_seq(c.seq_start, c.n_seq, i0);
    for (int q = 0; q < LK_RUN; q++) {
      const u64 p = i0 + q;
      if (p >= b) break;
      const u64 o0 = off[p - a];
      if (o0 >= hi) break;
      if (off[p - a + 1] <= lo) continue;
      while (c.seq_start[s + 1] <= p) s++;
      RpWrite w{buf, o0, lo, hi};
      rp_emit(c, p, s, w);
    }
  }
}

// every non-empty sequence must end with a byte that is not ACGT, so that no window crosses into the next one
__global__ __launch_bounds__(256)
void report_check_kernel(const uint8_t *__restrict__ bases, const u64 *__restrict__ ss, u64 n_seq, u32 *__restrict__ bad) {
  const u64 stride = (u64)gridDim.x * blockDim.x;
  for (u64 s = (u64)blockIdx.x * blockDim.x + threadIdx.x; s < n_seq; s += stride)
    if (ss[s + 1] > ss[s] && lk_code(bases[ss[s + 1] - 1]) >= 0) *bad = 1u;
}

}  // namespace mgc

// ================================================================================================
//  C ABI
// ================================================================================================
namespace {
thread_local std::string g_lk_error;
void lk_err(const std::string &m) { g_lk_error = m; }
}  // namespace

namespace mgc { void lk_set_error(const std::string &m) { g_lk_error = m; } }

extern "C" const char *mgc_lookup_error(void) { return g_lk_error.c_str(); }

extern "C" void mgc_lookup_free(mgc_lookup *t) {
  if (!t) return;
  (void)hipSetDevice(t->device);
  delete t;
}

#define LK_TRY(expr) do { hipError_t e__ = (expr); if (e__ != hipSuccess) { lk_err(std::string(#expr) + ": " + hipGetErrorString(e__)); mgc_lookup_free(t); return nullptr; } } while (0)

// keys/values already on the device (filtered, owned by the table): build the index
static uint32_t lookup_index_bits(uint32_t k, uint64_t n) {
  uint32_t bits = 0;
  while (bits < 2 * k && bits < 28 && (n >> (bits + 2)) > 0) bits++;             // ~4 k-mers per index entry
  return bits;
}

extern "C" int mgc_lookup_estimate(const char *db_path, uint64_t min_value, uint64_t max_value, mgc_lookup_info *info) {
  if (!db_path || !info) { lk_err("mgc_lookup_estimate: bad arguments"); return MGC_EINVAL; }
  mdb_reader *r = mdb_reader_open(db_path);
  if (!r) { lk_err(std::string("mgc_lookup_estimate: ") + mdb_last_error()); return MGC_EINVAL; }
  mdb_info di;
  mdb_reader_info(r, &di);
  std::vector<uint64_t> values(di.hist_len ? di.hist_len : 1), occ(di.hist_len ? di.hist_len : 1);
  if (di.hist_len && mdb_reader_histogram(r, values.data(), occ.data()) != 0) {
    lk_err(std::string("mgc_lookup_estimate: ") + mdb_last_error());
    mdb_reader_close(r);
    return MGC_EINVAL;
  }
  mdb_reader_close(r);
  uint64_t n_db = 0, n = 0;
  for (uint64_t i = 0; i < di.hist_len; i++) {
    n_db += occ[i];
    if (values[i] >= min_value && values[i] <= max_value) n += occ[i];
  }
  memset(info, 0, sizeof(*info));
  info->k = di.k; info->key_words = di.k > 32 ? 2u : 1u;
  info->index_bits = lookup_index_bits(di.k, n);
  info->n_kmers = n; info->n_kmers_in_db = n_db;
  info->device_bytes = (sizeof(uint64_t) * info->key_words + sizeof(uint32_t)) * n + sizeof(uint64_t) * ((1ull << info->index_bits) + 1);
  return MGC_OK;
}

static mgc_lookup *lookup_finish(mgc_lookup *t) {
  const uint32_t bits = lookup_index_bits(t->k, t->n);
  t->index_bits = bits;
  t->shift = 2 * t->k - bits;
  const uint64_t entries = (1ull << bits) + 1;
  LK_TRY(t->d_index.ensure(sizeof(uint64_t) * entries));
  if (bits == 0) {                                          // a handful of k-mers: one bucket
    const uint64_t two[2] = {0, t->n};
    LK_TRY(hipMemcpy(t->d_index.p, two, sizeof(two), hipMemcpyHostToDevice));
  } else {
    LK_TRY(mgc::launch_block_offsets(t->d_keys.p, t->n, t->kw, t->shift, 1ull << bits, t->d_index.as<uint64_t>(), nullptr));
    LK_TRY(hipStreamSynchronize(nullptr));
  }
  return t;
}

extern "C" mgc_lookup *mgc_lookup_from_device(const void *d_keys, const uint32_t *d_values, uint64_t n, uint32_t k,
                                              uint64_t min_value, uint64_t max_value, int device) {
  if (k == 0 || k > 64 || (n && (!d_keys || !d_values))) { lk_err("mgc_lookup_from_device: bad arguments"); return nullptr; }
  mgc_lookup *t = new mgc_lookup();
  if (device < 0) (void)hipGetDevice(&device);
  t->device = device; t->k = k; t->kw = k > 32 ? 2u : 1u; t->n_db = n;
  LK_TRY(hipSetDevice(device));
  const size_t kbytes = sizeof(uint64_t) * t->kw;
  if (min_value <= 1 && max_value >= 0xFFFFFFFFull) {       // nothing to filter (stored values are >= 1)
    t->n = n;
    LK_TRY(t->d_keys.ensure(kbytes * n));
    LK_TRY(t->d_vals.ensure(sizeof(uint32_t) * n));
    if (n) {
      LK_TRY(hipMemcpy(t->d_keys.p, d_keys, kbytes * n, hipMemcpyDeviceToDevice));
      LK_TRY(hipMemcpy(t->d_vals.p, d_values, sizeof(uint32_t) * n, hipMemcpyDeviceToDevice));
    }
    return lookup_finish(t);
  }
  const uint64_t tiles = (n + mgc::FL_TILE - 1) / mgc::FL_TILE;
  mgc::DBuf d_ws;
  mgc::CompactWs w = {};
  uint64_t kept = 0;
  if (tiles) {
    LK_TRY(d_ws.ensure(sizeof(uint64_t) * mgc::compact_ws_elems(tiles)));
    w = mgc::compact_ws_at(d_ws.p, tiles);
    hipLaunchKernelGGL((mgc::filter_kernel<mgc::u64, false>), dim3((uint32_t)tiles), dim3(256), 0, nullptr, (const mgc::u64 *)nullptr, d_values,
                       (mgc::u64)n, (mgc::u64)min_value, (mgc::u64)max_value, w.tiles, (mgc::u64 *)nullptr, (uint32_t *)nullptr);
    hipError_t e = mgc::compact_scan(w, nullptr);
    if (e == hipSuccess) e = hipMemcpy(&kept, w.total, sizeof(uint64_t), hipMemcpyDeviceToHost);
    if (e != hipSuccess) { lk_err(std::string("value filter: ") + hipGetErrorString(e)); mgc_lookup_free(t); return nullptr; }
  }
  t->n = kept;
  hipError_t e = t->d_keys.ensure(kbytes * kept);
  if (e == hipSuccess) e = t->d_vals.ensure(sizeof(uint32_t) * kept);
  if (e == hipSuccess && tiles) {
    if (t->kw == 2)
      hipLaunchKernelGGL((mgc::filter_kernel<mgc::K128, true>), dim3((uint32_t)tiles), dim3(256), 0, nullptr, reinterpret_cast<const mgc::K128 *>(d_keys),
                         d_values, (mgc::u64)n, (mgc::u64)min_value, (mgc::u64)max_value, w.tiles, t->d_keys.as<mgc::K128>(), t->d_vals.as<uint32_t>());
    else
      hipLaunchKernelGGL((mgc::filter_kernel<mgc::u64, true>), dim3((uint32_t)tiles), dim3(256), 0, nullptr, reinterpret_cast<const mgc::u64 *>(d_keys),
                         d_values, (mgc::u64)n, (mgc::u64)min_value, (mgc::u64)max_value, w.tiles, t->d_keys.as<mgc::u64>(), t->d_vals.as<uint32_t>());
    e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
  }
  if (e != hipSuccess) { lk_err(std::string("value filter: ") + hipGetErrorString(e)); mgc_lookup_free(t); return nullptr; }
  return lookup_finish(t);
}

extern "C" mgc_lookup *mgc_lookup_load(const char *db_path, uint64_t min_value, uint64_t max_value, int device, int host_threads) {
  if (!db_path) { lk_err("mgc_lookup_load: no database"); return nullptr; }
  mdb_reader *r = mdb_reader_open(db_path);
  if (!r) { lk_err(std::string("mgc_lookup_load: ") + mdb_last_error()); return nullptr; }
  mdb_info info;
  mdb_reader_info(r, &info);
  mdb_reader_close(r);
  const uint32_t kw = info.k > 32 ? 2u : 1u;
  if (host_threads <= 0) host_threads = (int)std::thread::hardware_concurrency();
  host_threads = std::max(1, std::min(host_threads, MGC_NUM_FILES));
  // Host threads only READ the 64 data files (mgc_dbfile.hpp); every file then goes to HBM at its running offset in the unfiltered
  // arrays -- its bytes as they are, decoded there (mgc_decode.hip), or as arrays where only the host decoder follows it -- and the
  // value filter is the device compaction of mgc_lookup_from_device.
  const bool host_decode = mgc::decode_on_host();           // once per table load (tests switch it between loads)
  if (device < 0) (void)hipGetDevice(&device);
  if (hipSetDevice(device) != hipSuccess) { lk_err("mgc_lookup_load: hipSetDevice failed"); return nullptr; }
  std::vector<mgc::DbFile> file(MGC_NUM_FILES);
  std::atomic<uint32_t> nextf(0);
  std::mutex mu;
  std::string open_msg;
  auto reader = [&]() {
    mdb_reader *rr = mdb_reader_open(db_path);
    if (!rr) { std::lock_guard<std::mutex> g(mu); open_msg = mdb_last_error(); return; }
    for (;;) {
      const uint32_t ff = nextf.fetch_add(1);
      if (ff >= MGC_NUM_FILES) break;
      mgc::dbfile_read(rr, ff, kw, host_decode, false, &file[ff]);
    }
    mdb_reader_close(rr);
  };
  {
    std::vector<std::thread> pool;
    for (int i = 1; i < host_threads; i++) pool.emplace_back(reader);
    reader();
    for (auto &th : pool) th.join();
  }
  if (nextf.load() < MGC_NUM_FILES) { lk_err("mgc_lookup_load: " + open_msg); return nullptr; }     // no thread could open the database
  uint64_t total = 0, max_size = 0, max_nb = 0;
  for (const mgc::DbFile &f : file) {
    if (f.rc != MGC_OK) { lk_err("mgc_lookup_load: " + f.msg); return nullptr; }
    total += f.n; max_size = std::max(max_size, f.size); max_nb = std::max(max_nb, f.nb);
  }
  const size_t kbytes = sizeof(uint64_t) * kw;
  mgc::DBuf dk, dv;
  mgc::DbFileScratch scratch;
  hipError_t e = dk.ensure(kbytes * total);
  if (e == hipSuccess) e = dv.ensure(sizeof(uint32_t) * total);
  if (e == hipSuccess) e = scratch.file.ensure(max_size + 16);          // all files are read: the scratch never grows between them
  if (e == hipSuccess) e = scratch.blocks.ensure(sizeof(mdb_raw_block) * max_nb);
  std::string msg;
  uint64_t o = 0;
  for (uint32_t ff = 0; ff < MGC_NUM_FILES && e == hipSuccess; ff++) {
    mgc::DbFile &f = file[ff];
    uint32_t h_err = 0;
    e = mgc::dbfile_upload(f, info, kw, scratch, dk.as<unsigned char>() + kbytes * o, dv.as<uint32_t>() + o, nullptr, &h_err, nullptr);
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);                  // the scratch is the next file's
    if (e == hipSuccess && mgc::dbfile_decode_rc(h_err, &msg) != MGC_OK) { lk_err("mgc_lookup_load: " + msg); return nullptr; }
    o += f.n;
  }
  file.clear();                                             // the host copies and the scratch go before the filter allocates
  scratch = mgc::DbFileScratch();
  if (e != hipSuccess) { lk_err(std::string("mgc_lookup_load: ") + hipGetErrorString(e)); return nullptr; }
  return mgc_lookup_from_device(dk.p, dv.as<uint32_t>(), total, info.k, min_value, max_value, device);
}

extern "C" int mgc_lookup_get_info(const mgc_lookup *t, mgc_lookup_info *info) {
  if (!t || !info) return MGC_EINVAL;
  info->k = t->k; info->key_words = t->kw; info->index_bits = t->index_bits; info->reserved = 0;
  info->n_kmers = t->n; info->n_kmers_in_db = t->n_db;
  info->device_bytes = (sizeof(uint64_t) * t->kw + sizeof(uint32_t)) * t->n + sizeof(uint64_t) * ((1ull << t->index_bits) + 1);
  return MGC_OK;
}

namespace {
int lk_rc(hipError_t e, const char *what) {
  if (e == hipSuccess) return MGC_OK;
  lk_err(std::string(what) + ": " + hipGetErrorString(e));
  return MGC_EHIP;
}
uint32_t lk_grid(uint64_t threads) { const uint64_t g = (threads + 255) / 256; return (uint32_t)(g ? g : 1); }
}  // namespace

extern "C" int mgc_lookup_values(const mgc_lookup *t, const void *d_kmers, uint64_t n, uint32_t *d_out, void *stream) {
  if (!t || (n && (!d_kmers || !d_out))) return MGC_EINVAL;
  if (n == 0) return MGC_OK;
  uint64_t g = (n + 255) / 256;
  if (g > 65536) g = 65536;
  if (t->kw == 2)
    hipLaunchKernelGGL((mgc::lookup_values_kernel<mgc::K128>), dim3((uint32_t)g), dim3(256), 0, (hipStream_t)stream, t->d_keys.as<const mgc::K128>(),
                       t->d_vals.as<uint32_t>(), t->d_index.as<const mgc::u64>(), t->shift, reinterpret_cast<const mgc::K128 *>(d_kmers), (mgc::u64)n, d_out, (mgc::u64)1 << t->index_bits);
  else
    hipLaunchKernelGGL((mgc::lookup_values_kernel<mgc::u64>), dim3((uint32_t)g), dim3(256), 0, (hipStream_t)stream, t->d_keys.as<const mgc::u64>(),
                       t->d_vals.as<uint32_t>(), t->d_index.as<const mgc::u64>(), t->shift, reinterpret_cast<const mgc::u64 *>(d_kmers), (mgc::u64)n, d_out, (mgc::u64)1 << t->index_bits);
  return lk_rc(hipGetLastError(), "lookup_values");
}

extern "C" int mgc_lookup_stream(const mgc_lookup *t, const uint8_t *d_bases, uint64_t n_bases, uint32_t *d_out, void *stream) {
  if (!t || (n_bases && (!d_bases || !d_out))) return MGC_EINVAL;
  if (n_bases == 0) return MGC_OK;
  const uint32_t g = lk_grid((n_bases + mgc::LK_RUN - 1) / mgc::LK_RUN);
  if (t->kw == 2)
    hipLaunchKernelGGL((mgc::lookup_stream_kernel<mgc::K128>), dim3(g), dim3(256), 0, (hipStream_t)stream, t->d_keys.as<const mgc::K128>(),
                       t->d_vals.as<uint32_t>(), t->d_index.as<const mgc::u64>(), t->shift, d_bases, (mgc::u64)n_bases, t->k, d_out);
  else
    hipLaunchKernelGGL((mgc::lookup_stream_kernel<mgc::u64>), dim3(g), dim3(256), 0, (hipStream_t)stream, t->d_keys.as<const mgc::u64>(),
                       t->d_vals.as<uint32_t>(), t->d_index.as<const mgc::u64>(), t->shift, d_bases, (mgc::u64)n_bases, t->k, d_out);
  return lk_rc(hipGetLastError(), "lookup_stream");
}

extern "C" int mgc_lookup_existence(const mgc_lookup *t, const uint8_t *d_bases, uint64_t n_bases, const uint64_t *d_seq_start,
                                    uint64_t n_seq, uint64_t *d_total, uint64_t *d_found, void *stream) {
  if (!t || (n_seq && (!d_seq_start || !d_total || !d_found)) || (n_bases && !d_bases)) return MGC_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (n_seq) {
    hipError_t e = hipMemsetAsync(d_total, 0, sizeof(uint64_t) * n_seq, st);
    if (e == hipSuccess) e = hipMemsetAsync(d_found, 0, sizeof(uint64_t) * n_seq, st);
    if (e != hipSuccess) return lk_rc(e, "lookup_existence");
  }
  if (n_bases == 0 || n_seq == 0) return MGC_OK;
  const uint32_t g = lk_grid((n_bases + mgc::LK_RUN - 1) / mgc::LK_RUN);
  if (t->kw == 2)
    hipLaunchKernelGGL((mgc::lookup_existence_kernel<mgc::K128>), dim3(g), dim3(256), 0, st, t->d_keys.as<const mgc::K128>(), t->d_vals.as<uint32_t>(),
                       t->d_index.as<const mgc::u64>(), t->shift, d_bases, (mgc::u64)n_bases, t->k,
                       reinterpret_cast<const mgc::u64 *>(d_seq_start), (mgc::u64)n_seq, reinterpret_cast<mgc::u64 *>(d_total), reinterpret_cast<mgc::u64 *>(d_found));
  else
    hipLaunchKernelGGL((mgc::lookup_existence_kernel<mgc::u64>), dim3(g), dim3(256), 0, st, t->d_keys.as<const mgc::u64>(), t->d_vals.as<uint32_t>(),
                       t->d_index.as<const mgc::u64>(), t->shift, d_bases, (mgc::u64)n_bases, t->k,
                       reinterpret_cast<const mgc::u64 *>(d_seq_start), (mgc::u64)n_seq, reinterpret_cast<mgc::u64 *>(d_total), reinterpret_cast<mgc::u64 *>(d_found));
  return lk_rc(hipGetLastError(), "lookup_existence");
}

// ---- position reports (src/meryl-lookup/dump.C) ------------------------------------------------------------------------------
namespace {
int lk_set(const mgc_lookup *const *tables, uint32_t n_tables, mgc::LkSet &set, const char *who) {
  if (!tables || n_tables == 0 || n_tables > mgc::LK_MAX_TABLES) {
    lk_err(std::string(who) + ": between 1 and " + std::to_string(mgc::LK_MAX_TABLES) + " tables");
    return MGC_EINVAL;
  }
  memset(&set, 0, sizeof(set));
  for (uint32_t t = 0; t < n_tables; t++) {
    const mgc_lookup *L = tables[t];
    if (!L) { lk_err(std::string(who) + ": no table"); return MGC_EINVAL; }
    if (L->k != tables[0]->k) { lk_err(std::string(who) + ": the tables have different k-mer sizes"); return MGC_EINVAL; }
    set.t[t].keys = L->d_keys.p; set.t[t].vals = L->d_vals.as<uint32_t>(); set.t[t].index = L->d_index.as<const mgc::u64>();
    set.t[t].n_index = 1ull << L->index_bits; set.t[t].shift = L->shift;
  }
  set.n = n_tables; set.k = tables[0]->k;
  return MGC_OK;
}

hipError_t lk_launch_positions(const mgc::LkSet &set, bool wide, int what, const uint8_t *d_bases, uint64_t n_bases, uint32_t *d_out,
                               hipStream_t st) {
  if (n_bases == 0) return hipSuccess;
  if (what == MGC_LOOKUP_DEPTH) {
    const uint32_t g = (uint32_t)((n_bases + mgc::LK_DEPTH_TILE - 1) / mgc::LK_DEPTH_TILE);
    if (wide) hipLaunchKernelGGL(mgc::lookup_depth_kernel<mgc::K128>, dim3(g), dim3(320), 0, st, set, d_bases, (mgc::u64)n_bases, d_out);
    else      hipLaunchKernelGGL(mgc::lookup_depth_kernel<mgc::u64>, dim3(g), dim3(320), 0, st, set, d_bases, (mgc::u64)n_bases, d_out);
    return hipGetLastError();
  }
  const uint32_t g = lk_grid((n_bases + mgc::LK_RUN - 1) / mgc::LK_RUN);
  if (what == MGC_LOOKUP_COUNT) {
    if (wide) hipLaunchKernelGGL((mgc::lookup_positions_kernel<mgc::K128, MGC_LOOKUP_COUNT>), dim3(g), dim3(256), 0, st, set, d_bases, (mgc::u64)n_bases, d_out);
    else      hipLaunchKernelGGL((mgc::lookup_positions_kernel<mgc::u64, MGC_LOOKUP_COUNT>), dim3(g), dim3(256), 0, st, set, d_bases, (mgc::u64)n_bases, d_out);
  } else {
    if (wide) hipLaunchKernelGGL((mgc::lookup_positions_kernel<mgc::K128, MGC_LOOKUP_PRESENCE>), dim3(g), dim3(256), 0, st, set, d_bases, (mgc::u64)n_bases, d_out);
    else      hipLaunchKernelGGL((mgc::lookup_positions_kernel<mgc::u64, MGC_LOOKUP_PRESENCE>), dim3(g), dim3(256), 0, st, set, d_bases, (mgc::u64)n_bases, d_out);
  }
  return hipGetLastError();
}
}  // namespace

extern "C" int mgc_lookup_positions(const mgc_lookup *const *tables, uint32_t n_tables, int what, const uint8_t *d_bases, uint64_t n_bases,
                                    uint32_t *d_out, void *stream) {
  mgc::LkSet set;
  const int rc = lk_set(tables, n_tables, set, "mgc_lookup_positions");
  if (rc != MGC_OK) return rc;
  if (what < MGC_LOOKUP_PRESENCE || what > MGC_LOOKUP_DEPTH) { lk_err("mgc_lookup_positions: unknown 'what'"); return MGC_EINVAL; }
  if (n_bases && (!d_bases || !d_out)) { lk_err("mgc_lookup_positions: no bases or no output"); return MGC_EINVAL; }
  return lk_rc(lk_launch_positions(set, tables[0]->kw == 2, what, d_bases, n_bases, d_out, (hipStream_t)stream), "lookup_positions");
}

namespace {
// device and pinned buffers of one report, released on every way out
struct RpBuffers {
  std::vector<void *> dev, pinned;
  hipStream_t cs = nullptr, xs = nullptr;
  hipEvent_t ev_fmt[2] = {nullptr, nullptr}, ev_cp[2] = {nullptr, nullptr};
  hipError_t alloc(void **p, size_t bytes) { hipError_t e = hipMalloc(p, bytes ? bytes : 8); if (e == hipSuccess) dev.push_back(*p); return e; }
  hipError_t host(void **p, size_t bytes) { hipError_t e = hipHostMalloc(p, bytes ? bytes : 8, hipHostMallocDefault); if (e == hipSuccess) pinned.push_back(*p); return e; }
  ~RpBuffers() {
    if (cs) (void)hipStreamSynchronize(cs);
    if (xs) (void)hipStreamSynchronize(xs);
    for (void *p : dev) (void)hipFree(p);
    for (void *p : pinned) (void)hipHostFree(p);
    for (int i = 0; i < 2; i++) { if (ev_fmt[i]) (void)hipEventDestroy(ev_fmt[i]); if (ev_cp[i]) (void)hipEventDestroy(ev_cp[i]); }
    if (cs) (void)hipStreamDestroy(cs);
    if (xs) (void)hipStreamDestroy(xs);
  }
};
}  // namespace

#define RP_HIP(expr) do { hipError_t e__ = (expr); if (e__ != hipSuccess) return lk_rc(e__, #expr); } while (0)

extern "C" int mgc_lookup_report(const mgc_lookup *const *tables, uint32_t n_tables, int mode, const char *const *labels, uint32_t n_labels,
                                 const uint8_t *d_bases, uint64_t n_bases, const uint64_t *seq_start, const char *const *names, uint64_t n_seq,
                                 uint64_t chunk_bytes, mgc_lookup_write_cb write_cb, void *user) {
  mgc::LkSet set;
  int rc = lk_set(tables, n_tables, set, "mgc_lookup_report");
  if (rc != MGC_OK) return rc;
  const bool wig = mode == MGC_REPORT_WIG_COUNT || mode == MGC_REPORT_WIG_DEPTH;
  if (mode < MGC_REPORT_BED || mode > MGC_REPORT_WIG_DEPTH) { lk_err("mgc_lookup_report: unknown mode"); return MGC_EINVAL; }
  if (!write_cb || !seq_start || (n_seq && !names) || (n_labels && !labels) || (n_bases && !d_bases)) {
    lk_err("mgc_lookup_report: bad arguments");
    return MGC_EINVAL;
  }
  if (wig && n_labels) { lk_err("mgc_lookup_report: labels are not supported for the WIG reports"); return MGC_EINVAL; }
  if (seq_start[0] != 0 || seq_start[n_seq] != n_bases) { lk_err("mgc_lookup_report: seq_start must run from 0 to n_bases"); return MGC_EINVAL; }
  // names and labels: one blob + offsets each; the longest line decides the smallest piece
  std::string name_blob, label_blob;
  std::vector<uint64_t> name_off(n_seq + 1, 0), label_off((size_t)n_labels + 1, 0);
  uint64_t max_name = 0, max_label = 0;
  for (uint64_t s = 0; s < n_seq; s++) {
    if (seq_start[s + 1] < seq_start[s]) { lk_err("mgc_lookup_report: seq_start decreases"); return MGC_EINVAL; }
    if (!names[s]) { lk_err("mgc_lookup_report: a sequence without a name"); return MGC_EINVAL; }
    const size_t l = strlen(names[s]);
    name_blob.append(names[s], l);
    name_off[s + 1] = name_blob.size();
    max_name = std::max<uint64_t>(max_name, l);
  }
  bool labels_present = false;                                                    // meryl-lookup.C:27-31
  for (uint32_t t = 0; t < n_labels; t++) {
    const size_t l = labels[t] ? strlen(labels[t]) : 0;
    if (l) label_blob.append(labels[t], l);
    label_off[t + 1] = label_blob.size();
    max_label = std::max<uint64_t>(max_label, l);
    labels_present = labels_present || l > 0;
  }
  const uint64_t longest = wig ? std::max<uint64_t>(19 + max_name + 1, 20 + 1 + 10 + 1)
                               : max_name + 1 + 20 + 1 + 20 + (n_labels ? 1 + max_label : 0) + 1;
  if (chunk_bytes < longest) {
    lk_err("mgc_lookup_report: chunk_bytes " + std::to_string(chunk_bytes) + " is shorter than the longest line (" + std::to_string(longest) + " bytes)");
    return MGC_EINVAL;
  }
  RP_HIP(hipSetDevice(tables[0]->device));
  RpBuffers B;
  RP_HIP(hipStreamCreate(&B.cs));
  RP_HIP(hipStreamCreate(&B.xs));
  for (int i = 0; i < 2; i++) { RP_HIP(hipEventCreateWithFlags(&B.ev_fmt[i], hipEventDisableTiming)); RP_HIP(hipEventCreateWithFlags(&B.ev_cp[i], hipEventDisableTiming)); }
  hipStream_t cs = B.cs;

  // ranges of positions: a range's byte offsets are one scan; its text leaves in pieces of chunk_bytes
  const uint64_t R = std::max<uint64_t>(4096, std::min<uint64_t>(1ull << 24, chunk_bytes / 4));
  const uint64_t R_eff = std::max<uint64_t>(1, std::min<uint64_t>(R, n_bases));
  mgc::u64 *d_ss = nullptr, *d_noff = nullptr, *d_loff = nullptr, *d_off = nullptr, *d_scr = nullptr, *d_lines = nullptr, *d_bgn = nullptr;
  char *d_names = nullptr, *d_labels = nullptr, *d_stage[2] = {nullptr, nullptr}, *h_stage[2] = {nullptr, nullptr};
  uint32_t *d_val = nullptr, *d_bad = nullptr;
  RP_HIP(B.alloc(reinterpret_cast<void **>(&d_ss), 8 * (n_seq + 1)));
  RP_HIP(B.alloc(reinterpret_cast<void **>(&d_noff), 8 * (n_seq + 1)));
  RP_HIP(B.alloc(reinterpret_cast<void **>(&d_loff), 8 * ((uint64_t)n_labels + 1)));
  RP_HIP(B.alloc(reinterpret_cast<void **>(&d_names), name_blob.size()));
  RP_HIP(B.alloc(reinterpret_cast<void **>(&d_labels), label_blob.size()));
  RP_HIP(B.alloc(reinterpret_cast<void **>(&d_val), 4 * n_bases));
  RP_HIP(B.alloc(reinterpret_cast<void **>(&d_bad), 8));
  const size_t scr_elems = mgc::scan_scratch_elems(R_eff + 1) + 8;
  RP_HIP(B.alloc(reinterpret_cast<void **>(&d_off), 8 * (R_eff + 1 + 8)));
  RP_HIP(B.alloc(reinterpret_cast<void **>(&d_scr), 8 * scr_elems));
  for (int i = 0; i < 2; i++) {
    RP_HIP(B.alloc(reinterpret_cast<void **>(&d_stage[i]), chunk_bytes));
    RP_HIP(B.host(reinterpret_cast<void **>(&h_stage[i]), chunk_bytes));
  }
  RP_HIP(hipMemcpyAsync(d_ss, seq_start, 8 * (n_seq + 1), hipMemcpyHostToDevice, cs));
  RP_HIP(hipMemcpyAsync(d_noff, name_off.data(), 8 * (n_seq + 1), hipMemcpyHostToDevice, cs));
  RP_HIP(hipMemcpyAsync(d_loff, label_off.data(), 8 * ((uint64_t)n_labels + 1), hipMemcpyHostToDevice, cs));
  if (!name_blob.empty()) RP_HIP(hipMemcpyAsync(d_names, name_blob.data(), name_blob.size(), hipMemcpyHostToDevice, cs));
  if (!label_blob.empty()) RP_HIP(hipMemcpyAsync(d_labels, label_blob.data(), label_blob.size(), hipMemcpyHostToDevice, cs));
  RP_HIP(hipMemsetAsync(d_bad, 0, 8, cs));
  if (n_seq) {
    hipLaunchKernelGGL(mgc::report_check_kernel, dim3(lk_grid(std::min<uint64_t>(n_seq, 1u << 20))), dim3(256), 0, cs, d_bases, d_ss, (mgc::u64)n_seq, d_bad);
    RP_HIP(hipGetLastError());
  }
  uint32_t h_bad = 0;
  RP_HIP(hipMemcpyAsync(&h_bad, d_bad, 4, hipMemcpyDeviceToHost, cs));
  RP_HIP(hipStreamSynchronize(cs));                       // (the pageable uploads above are done too)
  if (h_bad) { lk_err("mgc_lookup_report: a non-empty sequence does not end with a non-ACGT byte"); return MGC_EINVAL; }

  // per position: presence mask, count or depth
  const int what = mode == MGC_REPORT_WIG_COUNT ? MGC_LOOKUP_COUNT : mode == MGC_REPORT_WIG_DEPTH ? MGC_LOOKUP_DEPTH : MGC_LOOKUP_PRESENCE;
  RP_HIP(lk_launch_positions(set, tables[0]->kw == 2, what, d_bases, n_bases, d_val, cs));
  const uint32_t any_only = labels_present ? 0u : 1u;

  // -bed-runs: the line of every run, and its begin
  if (mode == MGC_REPORT_BED_RUNS && n_bases) {
    RP_HIP(B.alloc(reinterpret_cast<void **>(&d_lines), 8 * (n_bases + 1)));
    const uint64_t tiles = (n_bases + mgc::FL_TILE - 1) / mgc::FL_TILE;
    mgc::u64 *d_s2 = nullptr, *d_edges = nullptr;
    void *d_ews = nullptr;
    RP_HIP(B.alloc(reinterpret_cast<void **>(&d_s2), 8 * (mgc::scan_scratch_elems(n_bases + 1) + 8)));   // the scan of the lines per position
    RP_HIP(B.alloc(&d_ews, 8 * mgc::compact_ws_elems(tiles)));                                           // the compaction of a table's edges
    const mgc::CompactWs ew = mgc::compact_ws_at(d_ews, tiles);
    hipLaunchKernelGGL(mgc::runs_lines_kernel, dim3(lk_grid(std::min<uint64_t>(n_bases, 1u << 24))), dim3(256), 0, cs, d_val, (mgc::u64)n_bases, any_only, d_lines);
    RP_HIP(hipGetLastError());
    RP_HIP(mgc::scan_u64_exclusive(d_lines, n_bases, d_s2, ew.total, cs));
    uint64_t n_lines = 0;
    RP_HIP(hipMemcpyAsync(&n_lines, ew.total, 8, hipMemcpyDeviceToHost, cs));
    RP_HIP(hipStreamSynchronize(cs));
    RP_HIP(B.alloc(reinterpret_cast<void **>(&d_bgn), 8 * n_lines));
    const uint32_t n_flag = any_only ? 1u : n_tables;
    for (uint32_t t = 0; t < n_flag && n_lines; t++) {
      hipLaunchKernelGGL(mgc::runs_edge_kernel<false>, dim3((uint32_t)tiles), dim3(256), 0, cs, d_val, (mgc::u64)n_bases, t, any_only, ew.tiles, (mgc::u64 *)nullptr);
      RP_HIP(mgc::compact_scan(ew, cs));
      uint64_t n_edges = 0;
      RP_HIP(hipMemcpyAsync(&n_edges, ew.total, 8, hipMemcpyDeviceToHost, cs));
      RP_HIP(hipStreamSynchronize(cs));
      if (!n_edges) continue;
      if (n_edges > 2 * n_lines) { lk_err("mgc_lookup_report: a run of flags does not end inside the stream"); return MGC_EINVAL; }
      if (!d_edges) RP_HIP(B.alloc(reinterpret_cast<void **>(&d_edges), 8 * 2 * n_lines));   // every run is a line: enough for any table
      hipLaunchKernelGGL(mgc::runs_edge_kernel<true>, dim3((uint32_t)tiles), dim3(256), 0, cs, d_val, (mgc::u64)n_bases, t, any_only, ew.tiles, d_edges);
      RP_HIP(hipGetLastError());
      hipLaunchKernelGGL(mgc::runs_pair_kernel, dim3(lk_grid(std::min<uint64_t>(n_edges / 2, 1u << 24))), dim3(256), 0, cs, d_edges, (mgc::u64)(n_edges / 2),
                         d_val, (mgc::u64)n_bases, d_lines, t, any_only, d_bgn);
      RP_HIP(hipGetLastError());
    }
  }

  mgc::RpCtx ctx;
  ctx.val = d_val; ctx.seq_start = d_ss; ctx.n_seq = n_seq; ctx.names = d_names; ctx.name_off = d_noff;
  ctx.labels = d_labels; ctx.label_off = d_loff; ctx.lines = d_lines; ctx.run_bgn = d_bgn;
  ctx.n_labels = n_labels; ctx.k = set.k; ctx.mode = (uint32_t)mode; ctx.any_only = any_only;

  // pieces: piece j is formatted into d_stage[j & 1] on cs, copied to h_stage[j & 1] on xs, and handed to the callback while
  // piece j + 1 is formatted
  uint64_t piece = 0, pending_bytes = 0;
  bool pending = false;
  auto deliver = [&](int slot) -> int {
    hipError_t e = hipEventSynchronize(B.ev_cp[slot]);
    if (e != hipSuccess) return lk_rc(e, "report copy");
    const int r = write_cb(h_stage[slot], pending_bytes, user);
    if (r != 0) { lk_err("mgc_lookup_report: the write callback returned " + std::to_string(r)); return MGC_ESTATE; }
    return MGC_OK;
  };
  for (uint64_t a = 0; a < n_bases; a += R_eff) {
    const uint64_t b = std::min<uint64_t>(n_bases, a + R_eff), np = b - a;
    RP_HIP(hipMemsetAsync(d_off + np, 0, 8, cs));
    hipLaunchKernelGGL(mgc::report_len_kernel, dim3(lk_grid((np + mgc::LK_RUN - 1) / mgc::LK_RUN)), dim3(256), 0, cs, ctx, (mgc::u64)a, (mgc::u64)b, d_off);
    RP_HIP(hipGetLastError());
    RP_HIP(mgc::scan_u64_exclusive(d_off, np + 1, d_scr, d_off + np + 1, cs));
    uint64_t total = 0;
    RP_HIP(hipMemcpyAsync(&total, d_off + np, 8, hipMemcpyDeviceToHost, cs));
    RP_HIP(hipStreamSynchronize(cs));
    const uint32_t g = lk_grid(std::min<uint64_t>((np + mgc::LK_RUN - 1) / mgc::LK_RUN, 256u * 1024u));
    for (uint64_t lo = 0; lo < total; lo += chunk_bytes, piece++) {
      const uint64_t hi = std::min<uint64_t>(total, lo + chunk_bytes);
      const int slot = (int)(piece & 1);
      if (piece >= 2) RP_HIP(hipStreamWaitEvent(cs, B.ev_cp[slot], 0));        // piece - 2 has left d_stage[slot]
      hipLaunchKernelGGL(mgc::report_format_kernel, dim3(g), dim3(256), 0, cs, ctx, (mgc::u64)a, (mgc::u64)b, d_off, (mgc::u64)lo, (mgc::u64)hi, d_stage[slot]);
      RP_HIP(hipGetLastError());
      RP_HIP(hipEventRecord(B.ev_fmt[slot], cs));
      RP_HIP(hipStreamWaitEvent(B.xs, B.ev_fmt[slot], 0));
      RP_HIP(hipMemcpyAsync(h_stage[slot], d_stage[slot], hi - lo, hipMemcpyDeviceToHost, B.xs));
      RP_HIP(hipEventRecord(B.ev_cp[slot], B.xs));
      if (pending && (rc = deliver(slot ^ 1)) != MGC_OK) return rc;
      pending = true;
      pending_bytes = hi - lo;
    }
  }
  if (pending && (rc = deliver((int)((piece - 1) & 1))) != MGC_OK) return rc;
  // WIG headers of the empty sequences at the very end of the stream (the device writes the others before their successor)
  if (wig) {
    std::string tail;
    for (uint64_t s = 0; s < n_seq; s++)
      if (seq_start[s] == n_bases) tail += "variableStep chrom=" + std::string(names[s]) + "\n";
    for (uint64_t o = 0; o < tail.size(); o += chunk_bytes) {
      const uint64_t m = std::min<uint64_t>(chunk_bytes, tail.size() - o);
      memcpy(h_stage[0], tail.data() + o, m);
      const int r = write_cb(h_stage[0], m, user);
      if (r != 0) { lk_err("mgc_lookup_report: the write callback returned " + std::to_string(r)); return MGC_ESTATE; }
    }
  }
  return MGC_OK;
}
