// mgc_merge_many.hip -- up to 32 sorted (k-mer, value) streams -> one, in one count pass and one emit pass (gfx950).
//
// What it replaces in the reference (paths relative to the reference root): the k-way streaming merge of
// merylOperation::nextMer (src/meryl/merylOp-nextMer.C:418-683): the smallest k-mer over the inputs and the inputs that hold
// it, _actLen / _actCount[] / _actIndex[] in input order (:478-523), combined by the operation (:559-612 with
// findMin/Max/SumCount and subtractCount, :23-62).  mgc_merge.hip does this for two inputs per launch and more inputs fold
// from the left; here every input is read once per pass.
//
// The merged-with-duplicates order is (key, input index).
//   1. partition (one wave per tile border): border t is the largest key x with #{elements < x} <= t*TILE, found by bisecting
//      the key space; lane i keeps input i's lower bound and narrows its own range with the key interval, the wave sums the
//      lanes.  At most N elements are equal to x, so a tile holds fewer than TILE + N elements, and since every input is cut
//      at the same key a group of equal keys never straddles a border.
//   2. tile kernel (count and emit): the N runs of a tile are staged in LDS side by side with a tag (input << 16 | index in
//      the run), then merged pairwise in ceil(log2 N) rounds between two LDS images: every element finds its place by one
//      binary search in its partner run (left run first on ties, so equal keys end up in input order).  The first element
//      of each group of equal keys walks the group, combines the values (read from global memory through the tag) and
//      decides whether the k-mer is written; block scan of the heads, tile bases from scan_u64_exclusive.
// LDS: 2 images x CAP x (key + 4 B tag) + a 32-entry table per input property: 48 KiB for 8-byte keys (CAP 2048), 40 KiB for
// 16-byte keys (CAP 1024) whatever N is -- three workgroups per CU.  Per element and pass: (8|16) + 4 B read from HBM (the
// values only where the pass needs them), and in LDS one write to stage, then per round one read, one write and
// log2(run length) probes: about sum_{r < log2 N} log2(CAP * 2^r / N) key probes, 21 for N = 3 and 40 for N = 32 at CAP 2048.
// No global atomics.
//
// Labels (meryl2; merylOpCompute::findOutputLabel, src/meryl2/merylOpCompute.C:286-395): the LABELS instantiation of the emit
// pass reaches an element's label through the same tag as its value -- 8 B more read per element, 8 B more written per kept
// k-mer, never staged in LDS (only a 32-entry table of the inputs' label pointers joins the value pointers') -- and the head
// thread folds them with LabelAcc (mgc_label.hpp) in input order.  Labels do not decide what is written: the count pass is
// the unlabelled one.
//
// Selectors (meryl2; merylSelector::isTrue, src/meryl2/merylSelector.C:72-156): the SELECT instantiations AND a program of
// value: / label: / bases: / input: tests (mgc_selector.hpp) onto the operation's rule.  Then labels and values can decide what is
// written, and the count pass reads what the program needs.
//
// Value assignment (meryl2; merylOpCompute::findOutputValue, src/meryl2/merylOpCompute.C:136-282): the ASSIGN instantiations
// (always with SELECT) keep the operation's presence rule only and let the head thread fold the group's values with ValueAcc
// (mgc_value.hpp) in place of the operation's value chain; a k-mer whose assigned value is 0 is not written, so the count pass
// reads the values unless the rule is #c or count.  The program, the labels and a value filter see the assigned value.
#include "mgc_common.hpp"
#include "mgc_route.hpp"
#include "mgc_selector.hpp"
#include "mgc_value.hpp"

namespace mgc {

constexpr int MM_BLOCK = 256;
constexpr int MM_MAX   = 32;                       // MGC_MERGE_MANY_MAX
template <typename K> struct MMGeom;
template <> struct MMGeom<u64>  { static constexpr int ITEMS = 8; typedef u64  Int; };
template <> struct MMGeom<K128> { static constexpr int ITEMS = 4; typedef u128 Int; };
// a tile holds the elements between two borders: at most TILE + N - 1 <= CAP
template <typename K> constexpr int mm_cap()  { return MM_BLOCK * MMGeom<K>::ITEMS; }
template <typename K> constexpr int mm_tile() { return mm_cap<K>() - MM_MAX; }

__device__ __forceinline__ u64  mm_int(u64 k)  { return k; }
__device__ __forceinline__ u128 mm_int(K128 k) { return KeyOps<K128>::v(k); }

// the inputs travel in the kernel-argument segment (like the tables of the position reports)
struct MergeManyDesc {
  const void *keys[MM_MAX];
  const u32  *vals[MM_MAX];
  u64         n[MM_MAX];
  const u64  *labs[MM_MAX];                       // LABELS: input i's labels, null = all zeros
  u32         count;
};

// splits[b * 32 + i] = number of elements of input i before border b (b in [0, tiles])
template <typename K>
__global__ __launch_bounds__(MM_BLOCK)
void merge_many_partition_kernel(MergeManyDesc d, u64 total, u64 tiles, u64 *__restrict__ splits) {
  typedef typename MMGeom<K>::Int KI;
  const u64 b = (u64)blockIdx.x * (MM_BLOCK / 64) + wave_id();
  if (b > tiles) return;                                     // (wave-uniform)
  const u32 lane = lane_id();
  const K *A = nullptr;
  u64 n = 0;
#pragma unroll
  for (int i = 0; i < MM_MAX; i++)
    if (lane == (u32)i && (u32)i < d.count) { A = reinterpret_cast<const K *>(d.keys[i]); n = d.n[i]; }
  const u64 r = b * (u64)mm_tile<K>();
  u64 L = 0, H = n;                                          // elements < lo, elements <= hi
  if (r >= total) L = n;
  else if (b > 0) {
    KI lo = 0, hi = ~(KI)0;
    while (lo < hi) {                                        // (wave-uniform: lo and hi are)
      const KI span = hi - lo, mid = lo + (span >> 1) + (span & 1);
      u64 l = L, h = H;
      while (l < h) {
        const u64 m = l + ((h - l) >> 1);
        if (mm_int(A[m]) < mid) l = m + 1; else h = m;
      }
      u64 sum = l;
#pragma unroll
      for (int s = 32; s > 0; s >>= 1) sum += __shfl_xor(sum, s);
      if (sum <= r) { lo = mid; L = l; } else { hi = mid - 1; H = l; }
    }
  }
  if (lane < MM_MAX) splits[b * MM_MAX + lane] = L;
}

// what a selector term sees of one group of equal keys (Src of mgc_selector.hpp).  The group is stored in input order from
// position p on, so input i's element is at p + popcount(presence below bit i): one LDS tag read and one global read.
template <typename K> struct MMSelectSrc {
  u32 presence, out_value;
  u64 out_label, lo, hi;
  const u32 *sg;                                             // the merged image's tags
  u32 p;                                                     // where the group begins
  const u32 *const *vp;
  const u64 *const *lp;                                      // null: no LABEL term asks
  __device__ __forceinline__ u32 tag(u32 i) const { return sg[p + __builtin_popcount(presence & ((1u << i) - 1u))]; }
  __device__ __forceinline__ u32 value(u32 i) const { const u32 t = tag(i); return vp[t >> 16][t & 0xFFFFu]; }
  __device__ __forceinline__ u64 label(u32 i) const {
    if (!lp) return 0ull;
    const u32 t = tag(i);
    const u64 *q = lp[t >> 16];
    return q ? q[t & 0xFFFFu] : 0ull;
  }
};
__device__ __forceinline__ void mm_key_words(u64 k, u64 *lo, u64 *hi)  { *lo = k; *hi = 0; }
__device__ __forceinline__ void mm_key_words(K128 k, u64 *lo, u64 *hi) { *lo = k.lo; *hi = k.hi; }

// SELECT: a selector program (mgc_selector.hpp) is ANDed onto the operation's keep rule by the head thread of every group; it
// travels in the kernel-argument segment beside the descriptor and every read of it is wave-uniform.  The count pass then reads
// what the program needs (SELF_*): values for VALUE terms, labels -- the LABELS instantiation, LabelAcc included -- for LABEL
// terms, so that it decides exactly what the emit pass decides.  Without SELECT the argument is an empty struct.
// ASSIGN: the value rule (a kernel code of mgc_value.hpp), its constant and the value filter of a filter node travel as one more
// argument, wave-uniform like the program; without ASSIGN it is an empty struct and the kernel is the one it was.
struct AssignRule { int vop; u32 vc; int fop; u32 reserved; u64 fc; };   // fop < 0: no filter; fc: the filter's threshold
struct AssignNone {};
template <bool ASSIGN> struct AssignArg { typedef AssignNone type; };
template <> struct AssignArg<true> { typedef AssignRule type; };

template <typename K, bool EMIT, bool LABELS = false, bool SELECT = false, bool ASSIGN = false>
__global__ __launch_bounds__(MM_BLOCK)
void merge_many_kernel(MergeManyDesc d, typename SelectArg<SELECT>::type prog, int op, const u64 *__restrict__ splits,
                       u64 *__restrict__ tile_cnt /*EMIT: exclusive bases*/, K *__restrict__ outK, u32 *__restrict__ outC, int lop = 0, u64 lc = 0,
                       u64 *__restrict__ outL = nullptr, typename AssignArg<ASSIGN>::type asg = {}) {
  static_assert(EMIT || !LABELS || SELECT, "labels do not change what is written: without a selector there is no labelled count pass");
  static_assert(SELECT || !ASSIGN, "an assignment comes with a (possibly empty) program");
  constexpr int CAP = mm_cap<K>(), ITEMS = MMGeom<K>::ITEMS;
  __shared__ K         s_key[2][CAP];
  __shared__ u32       s_tag[2][CAP];
  __shared__ const K  *s_kp[MM_MAX];                         // input i's first element of this tile
  __shared__ const u32 *s_vp[MM_MAX];
  __shared__ const u64 *s_lp[LABELS ? MM_MAX : 1];           // LABELS: input i's first label of this tile, null = all zeros
  __shared__ u32       s_off[MM_MAX + 1];                    // where run i begins in the staged image; [i >= N] = nt
  __shared__ u32       s_tmp[MM_BLOCK / 64 + 1];
  const u32 N = d.count;
  if (threadIdx.x < 64) {
    const u32 i = threadIdx.x;
    u64 beg = 0, end = 0;
    if (i < N) { beg = splits[(u64)blockIdx.x * MM_MAX + i]; end = splits[((u64)blockIdx.x + 1) * MM_MAX + i]; }
    const u32 len = (u32)(end - beg);
    u32 x = len;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) { const u32 y = __shfl_up(x, s); if ((int)i >= s) x += y; }
    if (i <= MM_MAX) s_off[i] = x - len;
#pragma unroll
    for (int j = 0; j < MM_MAX; j++)
      if (i == (u32)j) {
        s_kp[j] = reinterpret_cast<const K *>(d.keys[j]) + beg; s_vp[j] = d.vals[j] + beg;
        if constexpr (LABELS) s_lp[j] = d.labs[j] ? d.labs[j] + beg : nullptr;
      }
  }
  __syncthreads();
  const u32 nt = s_off[MM_MAX];
  if (nt > (u32)CAP) {                                       // cannot happen (fewer than TILE + N elements between two borders)
    if (!EMIT && threadIdx.x == 0) tile_cnt[blockIdx.x] = 0;
    return;
  }
  // stage: element j of the image belongs to the last run that begins at or before j
  for (u32 j = threadIdx.x; j < nt; j += MM_BLOCK) {
    u32 run = 0;
#pragma unroll
    for (int s = MM_MAX / 2; s > 0; s >>= 1) if (s_off[run + s] <= j) run += s;
    const u32 local = j - s_off[run];
    s_key[0][j] = s_kp[run][local];
    s_tag[0][j] = (run << 16) | local;
  }
  __syncthreads();
  // pairwise rounds: at width w the runs are groups of w inputs; group m merges with group m ^ 1
  int cur = 0;
  for (u32 w = 1; w < N; w <<= 1) {
    const K *sk = s_key[cur];
    for (u32 j = threadIdx.x; j < nt; j += MM_BLOCK) {
      const K   key = sk[j];
      const u32 tag = s_tag[cur][j];
      const u32 m = (tag >> 16) / w;
      const u32 a0 = s_off[(m & ~1u) * w], a1 = s_off[(m | 1u) * w], b1 = s_off[((m | 1u) + 1) * w];
      u32 dest;
      if (!(m & 1u)) {                                       // left run: the right run's elements below the key come first
        u32 l = a1, h = b1;
        while (l < h) { const u32 mid = (l + h) >> 1; if (KeyOps<K>::lt(sk[mid], key)) l = mid + 1; else h = mid; }
        dest = j + (l - a1);
      } else {                                               // right run: the left run's elements up to the key come first
        u32 l = a0, h = a1;
        while (l < h) { const u32 mid = (l + h) >> 1; if (!KeyOps<K>::lt(key, sk[mid])) l = mid + 1; else h = mid; }
        dest = a0 + (j - a1) + (l - a0);
      }
      s_key[cur ^ 1][dest] = key;
      s_tag[cur ^ 1][dest] = tag;
    }
    __syncthreads();
    cur ^= 1;
  }
  const K   *sk = s_key[cur];
  const u32 *sg = s_tag[cur];
  bool need_v = EMIT || op == 7;
  if constexpr (SELECT) need_v = need_v || (prog.flags & SELF_VALUES);
  if constexpr (ASSIGN) need_v = EMIT || value_needs_values(asg.vop) || (prog.flags & SELF_VALUES);
  const u32 l0 = threadIdx.x * ITEMS;
  u32 heads = 0, head_mask = 0, vreg[ITEMS];
  u64 lreg[LABELS ? ITEMS : 1];
#pragma unroll
  for (int q = 0; q < ITEMS; q++) {
    vreg[q] = 0;
    if constexpr (LABELS) lreg[q] = 0;
    const u32 p = l0 + q;
    if (p >= nt) continue;
    const K key = sk[p];
    if (p > 0 && !KeyOps<K>::ne(sk[p - 1], key)) continue;   // not the first of its group
    // the group, in input order: _actLen = cnt, _actIndex[0] = first, _actCount[] = the values
    const u32 first = sg[p] >> 16;
    u32 cnt = 0, v = 0, presence = 0;                        // SELECT: bit i = input i holds the k-mer
    bool alive = true;                                       // subtract: the running difference stayed positive
    LabelAcc la;
    if constexpr (LABELS) la.begin(lc);
    ValueAcc va;
    if constexpr (ASSIGN) va.begin(asg.vc);
    for (u32 g = p; g < nt && !KeyOps<K>::ne(sk[g], key); g++) {
      u32 c = 0;
      if (need_v) { const u32 tag = sg[g]; c = s_vp[tag >> 16][tag & 0xFFFFu]; }
      if constexpr (SELECT) presence |= 1u << (sg[g] >> 16);
      if constexpr (LABELS) {                                // _acta[ll]._lab / ._val in input order
        const u32 tag = sg[g];
        const u64 *lp = s_lp[tag >> 16];
        la.step(lop, lp ? lp[tag & 0xFFFFu] : 0ull, c);
      }
      if constexpr (ASSIGN) va.step(asg.vop, c);            // _acta[ii]._val in input order
      else if (cnt == 0) v = c;
      else if (op == 7) { if (v > c) v -= c; else alive = false; }
      else if (op == 0 || op == 3) v += c;                   // the sum wraps mod 2^32 like kmvalu arithmetic
      else if (op == 1 || op == 4) v = c < v ? c : v;
      else if (op == 2 || op == 5) v = c > v ? c : v;
      cnt++;
    }
    bool keep;
    if (op <= 2 || op == 10) keep = true;
    else if (op <= 6) keep = cnt == N;
    else if (op == 7) keep = first == 0 && alive;
    else if (op == 8) keep = first == 0 && cnt == 1;
    else keep = cnt == 1;
    if constexpr (ASSIGN) {                                  // so far the presence rule alone (`alive` was never cleared); now the value
      v = va.finish(asg.vop, asg.vc, cnt);
      keep = keep && v != 0 && value_filter_keeps(asg.fop, v, asg.fc);
    }
    if constexpr (SELECT) {
      if (keep) {
        MMSelectSrc<K> src;
        src.presence = presence; src.out_value = (!ASSIGN && op == 10) ? cnt : v; src.out_label = 0;
        if constexpr (LABELS) src.out_label = la.l;
        mm_key_words(key, &src.lo, &src.hi);
        src.sg = sg; src.p = p; src.vp = s_vp; src.lp = LABELS ? s_lp : nullptr;
        keep = select_keep(prog.t, prog.n, prog.k, src);
      }
    }
    if (keep) {
      head_mask |= 1u << q; heads++; vreg[q] = (!ASSIGN && op == 10) ? cnt : v;
      if constexpr (LABELS) lreg[q] = la.l;
    }
  }
  u32 tot;
  const u32 base = block_excl_scan<MM_BLOCK, u32>(heads, s_tmp, &tot);
  if (!EMIT) {
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = tot;
    return;
  }
  u64 o = tile_cnt[blockIdx.x] + base;
#pragma unroll
  for (int q = 0; q < ITEMS; q++)
    if (head_mask & (1u << q)) {
      outK[o] = sk[l0 + q]; outC[o] = vreg[q];
      if constexpr (LABELS) { if (!SELECT || outL) outL[o] = lreg[q]; }
      o++;
    }
}

uint32_t merge_many_tile(uint32_t key_words) { return key_words == 2 ? (uint32_t)mm_tile<K128>() : (uint32_t)mm_tile<u64>(); }

static inline uint64_t mm_total(const uint64_t *n, uint32_t n_inputs) {
  uint64_t t = 0;
  for (uint32_t i = 0; i < n_inputs; i++) t += n[i];
  return t;
}
static inline uint64_t mm_tiles(uint64_t total, uint32_t key_words) {
  const uint64_t T = merge_many_tile(key_words);
  return (total + T - 1) / T;
}
// workspace: the contiguous CompactWs (mgc_common.hpp), then the borders (u64 x 32 x (tiles + 1))
static inline size_t mm_splits_at(uint64_t t) { return compact_ws_elems(t); }

size_t merge_many_workspace_bytes(const uint64_t *n, uint32_t n_inputs, uint32_t key_words) {
  const uint64_t t = mm_tiles(mm_total(n, n_inputs), key_words);
  return (mm_splits_at(t) + (size_t)(t + 1) * MM_MAX) * sizeof(u64) + 256;
}

static bool mm_desc(MergeManyDesc *d, const MergeManyInputs &in, int op) {
  if (!in.keys || !in.vals || !in.n || in.count < 1 || in.count > (uint32_t)MM_MAX || op < 0 || op > 10) return false;
  memset(d, 0, sizeof(*d));
  d->count = in.count;
  for (uint32_t i = 0; i < in.count; i++) {
    if (in.n[i] && (!in.keys[i] || !in.vals[i])) return false;
    if (in.n[i] >> 32) return false;                         // a run's index inside a tile and the tile sizes are 32-bit; inputs are file slices
    d->keys[i] = in.keys[i]; d->vals[i] = in.vals[i]; d->n[i] = in.n[i];
    d->labs[i] = in.labs ? reinterpret_cast<const u64 *>(in.labs[i]) : nullptr;
  }
  return true;
}

// vop: a kernel code (value_kernel_op, mgc_value.hpp).  fop >= 0: the value filter of a filter node (MGC_VALUE_LESS_THAN ..
// NOT_EQUAL_TO) with threshold fc, tested on the assigned value.
static bool mm_assign_rule(AssignRule *r, int vop, uint64_t vc, int fop, uint64_t fc) {
  if (vop < VOP_SET || vop > VOP_COUNT || vop == 3 || fop > 5) return false;
  r->vop = vop; r->vc = (u32)vc; r->fop = fop < 0 ? -1 : fop; r->reserved = 0; r->fc = fc;
  return true;
}

// the one place that names the instantiations: <K, false>, <K, true>, <K, true, true>, and every <K, EMIT, LABELS, true[, true]>
template <typename K, bool EMIT>
static void mm_launch(PassInst pi, const MergeManyDesc &d, const SelectProgram &pg, const AssignRule &asg, int op, uint64_t t, const u64 *splits,
                      u64 *tiles, void *outK, u32 *outC, int lop, u64 lc, u64 *outL, hipStream_t st) {
#define MM_GO(LABELS, SELECT, ASSIGN, ...) \
  hipLaunchKernelGGL((merge_many_kernel<K, EMIT, LABELS, SELECT, ASSIGN>), dim3((uint32_t)t), dim3(MM_BLOCK), 0, st, d, __VA_ARGS__)
#define MM_ARGS op, splits, tiles, reinterpret_cast<K *>(outK), outC, lop, lc, outL
  if (pi.assign) {
    if (pi.labels) MM_GO(true, true, true, pg, MM_ARGS, asg);
    else MM_GO(false, true, true, pg, MM_ARGS, asg);
  } else if (pi.select) {
    if (pi.labels) MM_GO(true, true, false, pg, MM_ARGS);
    else MM_GO(false, true, false, pg, MM_ARGS);
  } else if constexpr (EMIT) {
    if (pi.labels) MM_GO(true, false, false, SelectNone{}, MM_ARGS);
    else MM_GO(false, false, false, SelectNone{}, MM_ARGS);
  } else {
    MM_GO(false, false, false, SelectNone{}, MM_ARGS);
  }
#undef MM_ARGS
#undef MM_GO
}

// count (emit false): cuts the inputs into tiles and leaves the output length at ws[0] (merge_read_total reads it); emit: the same
// inputs, operation and rule over the workspace the count pass left, writes the merged stream.  One to MM_MAX inputs.
hipError_t launch_merge_many(bool emit, const MergeManyInputs &in, int op, const PassRule &r, void *d_ws, void *d_out_keys,
                             uint32_t *d_out_vals, hipStream_t st) {
  MergeManyDesc d;
  SelectProgram pg;
  AssignRule asg = {};
  const bool assignment = r.vop != VOP_NONE, filter = r.fop >= 0, select = r.select || assignment || filter;
  u64 *outL = emit ? reinterpret_cast<u64 *>(r.out_labs) : nullptr;
  if (!mm_desc(&d, in, op) || (in.key_words != 1 && in.key_words != 2)) return hipErrorInvalidValue;
  if ((select || outL) && (r.lop < LOP_SET || r.lop > LOP_SEL_MAX || r.lop == 12 || (r.lop == LOP_INVERT && in.count > 1))) return hipErrorInvalidValue;
  if (!select_program(&pg, select ? r.terms : nullptr, select ? r.n_terms : 0, select ? r.k : 1)) return hipErrorInvalidValue;
  if ((assignment || filter) && !mm_assign_rule(&asg, r.vop, r.vc, r.fop, r.fc)) return hipErrorInvalidValue;
  const PassInst pi = pass_inst(emit, select, (pg.flags & SELF_LABELS) != 0, assignment, filter, outL != nullptr);
  u64 *ws = reinterpret_cast<u64 *>(d_ws);
  const uint64_t total = mm_total(in.n, in.count), t = mm_tiles(total, in.key_words);
  if (t == 0) return emit ? hipSuccess : hipMemsetAsync(ws, 0, 8, st);
  const CompactWs w = compact_ws_at(d_ws, t);
  u64 *tiles = w.tiles, *splits = ws + mm_splits_at(t);
  if (emit) {
    if (in.key_words == 2) mm_launch<K128, true>(pi, d, pg, asg, op, t, splits, tiles, d_out_keys, d_out_vals, r.lop, (u64)r.lc, outL, st);
    else mm_launch<u64, true>(pi, d, pg, asg, op, t, splits, tiles, d_out_keys, d_out_vals, r.lop, (u64)r.lc, outL, st);
    return hipGetLastError();
  }
  const uint32_t pgrid = (uint32_t)((t + 1 + MM_BLOCK / 64 - 1) / (MM_BLOCK / 64));
  if (in.key_words == 2) {
    hipLaunchKernelGGL((merge_many_partition_kernel<K128>), dim3(pgrid), dim3(MM_BLOCK), 0, st, d, (u64)total, (u64)t, splits);
    mm_launch<K128, false>(pi, d, pg, asg, op, t, splits, tiles, nullptr, nullptr, r.lop, (u64)r.lc, nullptr, st);
  } else {
    hipLaunchKernelGGL((merge_many_partition_kernel<u64>), dim3(pgrid), dim3(MM_BLOCK), 0, st, d, (u64)total, (u64)t, splits);
    mm_launch<u64, false>(pi, d, pg, asg, op, t, splits, tiles, nullptr, nullptr, r.lop, (u64)r.lc, nullptr, st);
  }
  return compact_scan(w, st);
}

}  // namespace mgc
