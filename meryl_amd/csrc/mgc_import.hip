// mgc_import.hip -- `kmer value` and `kmer value label` text -> sorted distinct (k-mer, summed value[, summed label]) records, on
// the device (gfx950).
//
// What it replaces in the reference (paths relative to the reference root):
//   parse_*          the line loop of src/meryl-import/meryl-import.C:177-219: readLine + splitToWords, `#<value>` lines
//                    setting the persistent value (:175, :188-191), addR of every base of the first word (:196-197: a word
//                    longer than k keeps its LAST k bases), reverseComplement and the canonical / forward / reverse pick
//                    (:199-211), the optional second word as the value (:193-194); and that of the meryl 2 dialect,
//                    src/meryl2-import/meryl-import.C:199-264, with `value=` / `label=` lines and a third word
//   pair_*           the std::sort of (suffix, value) records in countSingleKmersWithValues, src/meryl/merylCountArray.C:387
//   triple_*         the same sort with a label beside the value, src/meryl2/merylCountArray.C:381
//   reduce_*         the summing loop over equal suffixes, :393-408 (uint32 sums wrap, :403); labels, meryl2 :400
//
// Two things are sequential in the text: the output slot of a record (records before it) and the persistent words (the
// last setter line before it).  Both are one scan with the operator of PAgg / P2Agg below: tiles of 4096 bytes summarise
// themselves, one workgroup composes the summaries, a second pass over the text writes.  That skeleton (parse_count_kernel,
// parse_total_kernel, parse_emit_kernel, parse_state_kernel) is written once; a dialect (Meryl1, Meryl2) gives it an aggregate,
// a state, a line grammar and the hooks fold / setter / seed / store and begin / chunk / commit.  Meryl1 carries one 32-bit
// persistent word through LDS, the tiles and the state; Meryl2 a value and a 64-bit label.
// The same shape -- per-tile aggregate, one composing workgroup, emit -- sums the values of equal keys: the aggregate carries
// "sum of the segment still open at the end", so a key repeated over any number of tiles and workgroups is summed across
// them (RAgg; with LABELS the label sum rides beside the value sum).
// No kernel here waits for another workgroup of its launch; every index is checked against n before it is used.
#include "mgc_common.hpp"
#include "mgc_import_dev.hpp"
#include "../../include/meryl_import_labelled.h"

namespace mgc {

// Exclusive scan of one aggregate per thread with A::combine (associative, not commutative), through LDS.
// s: BLOCK entries.  Every thread of the block must call it.
template <int BLOCK, typename A>
__device__ __forceinline__ A block_scan_excl(A v, A *s, A *total) {
  const u32 t = threadIdx.x;
  __syncthreads();                        // s may still be read from a previous call
  s[t] = v;
  __syncthreads();
  for (u32 d = 1; d < (u32)BLOCK; d <<= 1) {
    A x = s[t];
    if (t >= d) x = A::combine(s[t - d], x);
    __syncthreads();
    s[t] = x;
    __syncthreads();
  }
  *total = s[BLOCK - 1];
  return t ? s[t - 1] : A::identity();
}

// One workgroup turns T per-tile aggregates into their exclusive scan, in place; the total goes to *total.
constexpr int CP_BLOCK = 1024;
template <typename A>
__global__ __launch_bounds__(CP_BLOCK)
void compose_tiles_kernel(A *__restrict__ tiles, u64 T, A *__restrict__ total) {
  __shared__ A s[CP_BLOCK];
  const u64 per = (T + CP_BLOCK - 1) / CP_BLOCK;
  const u64 a = (u64)threadIdx.x * per < T ? (u64)threadIdx.x * per : T;
  const u64 b = a + per < T ? a + per : T;
  A agg = A::identity();
  for (u64 i = a; i < b; i++) agg = A::combine(agg, tiles[i]);
  A tot;
  A run = block_scan_excl<CP_BLOCK, A>(agg, s, &tot);
  for (u64 i = a; i < b; i++) {
    const A x = tiles[i];
    tiles[i] = run;
    run = A::combine(run, x);
  }
  if (threadIdx.x == 0) *total = tot;
}

// ============================================================================
//  Text parser
// ============================================================================
constexpr int PR_BLOCK = 256;
constexpr int PR_BYTES = 16;                       // text bytes per thread
constexpr int PR_TILE  = PR_BLOCK * PR_BYTES;      // 4096

// records / lines that start in a range, and the number of the last `#` line in it
struct PAgg {
  u32 rec, lines, has, val;
  static __device__ __forceinline__ PAgg identity() { PAgg a; a.rec = a.lines = a.has = a.val = 0; return a; }
  static __device__ __forceinline__ PAgg combine(PAgg a, PAgg b) {
    PAgg r; r.rec = a.rec + b.rec; r.lines = a.lines + b.lines; r.has = a.has | b.has; r.val = b.has ? b.val : a.val; return r;
  }
};
// the meryl 2 dialect: the numbers of the last `value=` and of the last `label=` line
struct P2Agg {
  u32 rec, lines, vhas, val, lhas, pad;
  u64 lab;
  static __device__ __forceinline__ P2Agg identity() { P2Agg a; a.rec = a.lines = a.vhas = a.val = a.lhas = a.pad = 0; a.lab = 0; return a; }
  static __device__ __forceinline__ P2Agg combine(P2Agg a, P2Agg b) {
    P2Agg r; r.rec = a.rec + b.rec; r.lines = a.lines + b.lines; r.pad = 0;
    r.vhas = a.vhas | b.vhas; r.val = b.vhas ? b.val : a.val;
    r.lhas = a.lhas | b.lhas; r.lab = b.lhas ? b.lab : a.lab;
    return r;
  }
};

// what a line is in either dialect.  LN_VALUE: `#<n>` / `value=<n>`; LN_LABEL: `label=<n>`
enum { LN_BLANK = 0, LN_RECORD = 1, LN_BAD = 2, LN_VALUE = 3, LN_LABEL = 4 };
struct Line  { u32 kind, bad, value, has_value; u64 lo, hi; };
struct Line2 { u32 kind, bad, value, has_value, has_label; u64 label, lo, hi; };

__device__ __forceinline__ bool pr_is_space(u32 c) { return c == ' ' || c == '\t' || c == '\r'; }

// a decimal word at t[j...]: ends at white space, '\n' or n.  false: no digit, a byte that is not a digit, or above 2^32 - 1
__device__ __forceinline__ bool pr_number(const uint8_t *__restrict__ t, u64 n, u64 &j, u32 *out) {
  u64 v = 0;
  u32 nd = 0;
  bool ok = true;
  while (j < n) {
    const u32 c = t[j];
    if (c == '\n' || pr_is_space(c)) break;
    if (c < '0' || c > '9') ok = false;
    else { v = v * 10ull + (u64)(c - '0'); if (v > 0xFFFFFFFFull) { ok = false; v = 0; } nd++; }
    j++;
  }
  *out = (u32)v;
  return ok && nd > 0;
}

// first byte of the line's first word (n: none)
__device__ __forceinline__ u64 pr_first_word(const uint8_t *__restrict__ t, u64 n, u64 p) {
  while (p < n && pr_is_space(t[p])) p++;
  return (p < n && t[p] != '\n') ? p : n;
}

// the k-mer word at t[j...] (ends at white space, '\n' or n; j is left behind it): its last k bases packed into *f -- A0 C1 T2 G3,
// either case (mgc_kmer.hip).  -> 0, or MGC_IMPORT_BAD_BASE / MGC_IMPORT_BAD_SHORT.  KT: u64 (k <= 32) or u128
template <typename KT>
__device__ __forceinline__ u32 pr_kmer_word(const uint8_t *__restrict__ t, u64 n, u64 &j, u32 k, KT *f_out) {
  const KT mask = (2 * k == 8 * sizeof(KT)) ? ~(KT)0 : (((KT)1 << (2 * k)) - 1);
  KT f = 0;
  u32 len = 0;
  bool bases_ok = true;
  while (j < n) {
    const u32 c = t[j];
    if (c == '\n' || pr_is_space(c)) break;
    const u32 up = c & 0xDFu;
    if (up != 'A' && up != 'C' && up != 'G' && up != 'T') bases_ok = false;
    f = ((f << 2) | (KT)((c >> 1) & 3u)) & mask;
    if (len < 0xFFFFFFFFu) len++;
    j++;
  }
  *f_out = f;
  return !bases_ok ? (u32)MGC_IMPORT_BAD_BASE : len < k ? (u32)MGC_IMPORT_BAD_SHORT : 0u;
}

// min(forward, reverse complement) / forward / reverse complement of the k bases in f -> {lo, hi}
template <typename KT>
__device__ __forceinline__ void pr_pick(KT f, u32 k, int mode, u64 *lo, u64 *hi) {
  KT key = f;
  if (mode != MGC_MODE_FORWARD) {
    KT r = 0, x = f;
    for (u32 i = 0; i < k; i++) { r = (r << 2) | ((x & 3) ^ 2); x >>= 2; }   // base i -> base k-1-i, complemented
    key = (mode == MGC_MODE_REVERSE) ? r : (f < r ? f : r);
  }
  *lo = (u64)key;
  if (sizeof(KT) > 8) *hi = (u64)((u128)key >> 64);
}

// the line that starts at byte p.  KT: u64 (k <= 32) or u128
template <typename KT>
__device__ Line parse_line(const uint8_t *__restrict__ t, u64 n, u64 p, u32 k, int mode, bool want_key) {
  Line L;
  L.kind = LN_BLANK; L.bad = 0; L.value = 0; L.has_value = 0; L.lo = L.hi = 0;
  u64 j = pr_first_word(t, n, p);
  if (j >= n) return L;
  if (t[j] == '#') {                                                     // meryl-import.C:188-191
    j++;
    if (pr_number(t, n, j, &L.value)) L.kind = LN_VALUE;
    else { L.kind = LN_BAD; L.bad = MGC_IMPORT_BAD_HASH; }
    return L;
  }
  KT f = 0;
  if (const u32 bad = pr_kmer_word<KT>(t, n, j, k, &f)) { L.kind = LN_BAD; L.bad = bad; return L; }
  while (j < n && pr_is_space(t[j])) j++;
  if (j < n && t[j] != '\n') {                                           // :193-194; words after it are ignored
    if (!pr_number(t, n, j, &L.value)) { L.kind = LN_BAD; L.bad = MGC_IMPORT_BAD_VALUE; return L; }
    L.has_value = 1;
  }
  L.kind = LN_RECORD;
  if (want_key) pr_pick<KT>(f, k, mode, &L.lo, &L.hi);
  return L;
}

// bit q: a line starts at byte p0 + q (a line starts at byte 0 and after every '\n')
__device__ __forceinline__ u32 pr_line_starts(const uint8_t *__restrict__ t, u64 n, u64 p0, bool aligned) {
  if (p0 >= n) return 0;
  const uint4 w = load16(t, p0, n, aligned);             // bytes at and beyond n read as '.'
  const u32 ww[4] = {w.x, w.y, w.z, w.w};
  u32 prev = p0 ? (u32)t[p0 - 1] : (u32)'\n';
  u32 starts = 0;
#pragma unroll
  for (int q = 0; q < PR_BYTES; q++) {
    if (p0 + q < n && prev == '\n') starts |= 1u << q;
    prev = (ww[q >> 2] >> (8 * (q & 3))) & 0xFFu;
  }
  return starts;
}

// ---- the meryl 2 grammar (include/meryl_import_labelled.h): `kmer [value [label]]` records, `value=<n>` and `label=<n>` lines
//      (src/meryl2-import/meryl-import.C:199-233) ----
__device__ __forceinline__ u64 pr_word_end(const uint8_t *__restrict__ t, u64 n, u64 j) {
  while (j < n && t[j] != '\n' && !pr_is_space(t[j])) j++;
  return j;
}

// decodeInteger over the word t[a, e): `123` / `123d`, `<hex>h` (digits in either case), `<octal>o`, `<binary>b`
// (documentation/source/reference.rst:615-617); the word's last byte decides the base.  false: no digit, a digit the base
// does not have, any other byte (SI suffixes, an upper-case suffix letter, a sign), or a number above `limit`
__device__ __forceinline__ bool pr2_number(const uint8_t *__restrict__ t, u64 a, u64 e, u64 limit, u64 *out) {
  *out = 0;
  if (a >= e) return false;
  const u32 last = t[e - 1];
  u32 base = 10;
  if (last == 'h') base = 16;
  else if (last == 'o') base = 8;
  else if (last == 'b') base = 2;
  if (last == 'h' || last == 'o' || last == 'b' || last == 'd') e--;
  if (a >= e) return false;
  u64 v = 0;
  for (u64 j = a; j < e; j++) {
    const u32 c = t[j], lc = c | 0x20u;
    u32 d;
    if (c >= '0' && c <= '9') d = c - '0';
    else if (lc >= 'a' && lc <= 'f') d = lc - 'a' + 10u;
    else return false;
    if (d >= base || (u64)d > limit || v > (limit - (u64)d) / (u64)base) return false;
    v = v * (u64)base + (u64)d;
  }
  *out = v;
  return true;
}

// 1: the word at j starts with `value=`, 2: with `label=` (strncmp(word, ..., 6), meryl-import.C:210, :215), 0: neither
__device__ __forceinline__ u32 pr2_assign(const uint8_t *__restrict__ t, u64 n, u64 j) {
  if (j + 6 > n || t[j + 5] != '=') return 0;
  if (t[j] == 'v' && t[j + 1] == 'a' && t[j + 2] == 'l' && t[j + 3] == 'u' && t[j + 4] == 'e') return 1;
  if (t[j] == 'l' && t[j + 1] == 'a' && t[j + 2] == 'b' && t[j + 3] == 'e' && t[j + 4] == 'l') return 2;
  return 0;
}

// the number of a `value=` / `label=` line whose first word starts at j (which = pr2_assign)
__device__ __forceinline__ bool pr2_assign_number(const uint8_t *__restrict__ t, u64 n, u64 j, u32 which, u64 lmask, u64 *out) {
  return pr2_number(t, j + 6, pr_word_end(t, n, j), which == 1 ? 0xFFFFFFFFull : lmask, out);
}

// the line that starts at byte p.  lmask: the bits a label may hold
template <typename KT>
__device__ Line2 parse_line2(const uint8_t *__restrict__ t, u64 n, u64 p, u32 k, int mode, u64 lmask, bool want_key) {
  Line2 L;
  L.kind = LN_BLANK; L.bad = 0; L.value = 0; L.has_value = 0; L.has_label = 0; L.label = 0; L.lo = L.hi = 0;
  u64 j = pr_first_word(t, n, p);
  if (j >= n) return L;
  if (const u32 which = pr2_assign(t, n, j)) {                           // :210-218; words after it are ignored
    u64 v = 0;
    if (!pr2_assign_number(t, n, j, which, lmask, &v)) { L.kind = LN_BAD; L.bad = MGC_IMPORT_BAD_ASSIGN; return L; }
    if (which == 1) { L.kind = LN_VALUE; L.value = (u32)v; } else { L.kind = LN_LABEL; L.label = v; }
    return L;
  }
  KT f = 0;                                                              // :222-223, as parse_line reads it
  if (const u32 bad = pr_kmer_word<KT>(t, n, j, k, &f)) { L.kind = LN_BAD; L.bad = bad; return L; }
  while (j < n && pr_is_space(t[j])) j++;
  if (j < n && t[j] != '\n') {                                           // :225-226
    const u64 e = pr_word_end(t, n, j);
    u64 v = 0;
    if (!pr2_number(t, j, e, 0xFFFFFFFFull, &v)) { L.kind = LN_BAD; L.bad = MGC_IMPORT_BAD_VALUE; return L; }
    L.value = (u32)v; L.has_value = 1;
    j = e;
    while (j < n && pr_is_space(t[j])) j++;
    if (j < n && t[j] != '\n') {                                         // :230-231; words after it are ignored
      if (!pr2_number(t, j, pr_word_end(t, n, j), lmask, &L.label)) { L.kind = LN_BAD; L.bad = MGC_IMPORT_BAD_LABEL; return L; }
      L.has_label = 1;
    }
  }
  L.kind = LN_RECORD;
  if (want_key) pr_pick<KT>(f, k, mode, &L.lo, &L.hi);                   // :235-246
  return L;
}

// ---- the two dialects ----
// A dialect names its aggregate, its state and its grammar, and the places where the parse skeleton below meets the
// persistent words.  On the scan side: fold (count pass: a line the grammar read, when it is a setter line, into the aggregate),
// setter (emit pass: is the line whose first word starts at j a setter line?  A well-formed one is applied to the aggregate;
// a malformed one is still no record), seed (the words that hold before a thread's first line: the scan's where it saw a
// setter, else the state's) and store (value and label of one record).  On the state side: begin (the words before any
// line), chunk (those of the chunk the count pass saw) and commit (they become the persistent ones).
struct Meryl1 {
  typedef PAgg Agg;
  typedef ImportState State;
  template <typename KT>
  static __device__ __forceinline__ Line parse(const uint8_t *__restrict__ t, u64 n, u64 p, u32 k, int mode, u64, bool want_key) {
    return parse_line<KT>(t, n, p, k, mode, want_key);
  }
  static __device__ __forceinline__ void fold(PAgg &a, const Line &L) { if (L.kind == LN_VALUE) { a.has = 1; a.val = L.value; } }
  static __device__ __forceinline__ bool setter(const uint8_t *__restrict__ t, u64 n, u64 j, u64, PAgg &a) {
    if (t[j] != '#') return false;
    j++;
    u32 v = 0;
    if (pr_number(t, n, j, &v)) { a.has = 1; a.val = v; }
    return true;
  }
  static __device__ __forceinline__ void seed(PAgg &a, const ImportState *__restrict__ s) { if (!a.has) a.val = s->persistent; }
  static __device__ __forceinline__ void store(const Line &L, const PAgg &a, u64 slot, u32 *__restrict__ vals, u64 *) {
    vals[slot] = L.has_value ? L.value : a.val;
  }
  static __device__ __forceinline__ void begin(ImportState *s) { s->persistent = 1; s->pad0 = 0; }
  static __device__ __forceinline__ void chunk(ImportState *s, const PAgg &a) { s->chunk_has = a.has; s->chunk_val = a.val; }
  static __device__ __forceinline__ void commit(ImportState *s) { if (s->chunk_has) s->persistent = s->chunk_val; }
};

struct Meryl2 {
  typedef P2Agg Agg;
  typedef Import2State State;
  template <typename KT>
  static __device__ __forceinline__ Line2 parse(const uint8_t *__restrict__ t, u64 n, u64 p, u32 k, int mode, u64 lmask, bool want_key) {
    return parse_line2<KT>(t, n, p, k, mode, lmask, want_key);
  }
  static __device__ __forceinline__ void fold(P2Agg &a, const Line2 &L) {
    if (L.kind == LN_VALUE) { a.vhas = 1; a.val = L.value; }
    else if (L.kind == LN_LABEL) { a.lhas = 1; a.lab = L.label; }
  }
  static __device__ __forceinline__ bool setter(const uint8_t *__restrict__ t, u64 n, u64 j, u64 lmask, P2Agg &a) {
    const u32 which = pr2_assign(t, n, j);
    if (!which) return false;
    u64 v = 0;
    if (pr2_assign_number(t, n, j, which, lmask, &v)) {
      if (which == 1) { a.vhas = 1; a.val = (u32)v; } else { a.lhas = 1; a.lab = v; }
    }
    return true;
  }
  static __device__ __forceinline__ void seed(P2Agg &a, const Import2State *__restrict__ s) {
    if (!a.vhas) a.val = s->persistent_value;
    if (!a.lhas) a.lab = s->persistent_label;
  }
  static __device__ __forceinline__ void store(const Line2 &L, const P2Agg &a, u64 slot, u32 *__restrict__ vals, u64 *__restrict__ labs) {
    vals[slot] = L.has_value ? L.value : a.val;                           // :225-233
    labs[slot] = L.has_label ? L.label : a.lab;
  }
  static __device__ __forceinline__ void begin(Import2State *s) {         // (the reference leaves both unset, :176-177)
    s->persistent_label = 0; s->persistent_value = 1; s->pad0 = 0;
  }
  static __device__ __forceinline__ void chunk(Import2State *s, const P2Agg &a) {
    s->chunk_vhas = a.vhas; s->chunk_val = a.val; s->chunk_lhas = a.lhas; s->chunk_lab = a.lab; s->pad1 = 0;
  }
  static __device__ __forceinline__ void commit(Import2State *s) {
    if (s->chunk_vhas) s->persistent_value = s->chunk_val;
    if (s->chunk_lhas) s->persistent_label = s->chunk_lab;
  }
};

// ---- the parse skeleton: everything but the grammar and the persistent words, once for both dialects ----
// lines that start in the tile of byte `pos` before it, summed over the block into *s_cnt (LDS); every thread must call it
__device__ __forceinline__ void pr_lines_before(const uint8_t *__restrict__ t, u64 n, u64 pos, bool count, u32 *s_cnt) {
  if (threadIdx.x == 0) *s_cnt = 0;
  __syncthreads();
  if (count) {
    const u64 tile0 = (pos / PR_TILE) * PR_TILE;
    u32 c = 0;
    for (u64 q = tile0 + threadIdx.x; q < pos && q < n; q += PR_BLOCK) c += (q == 0 || t[q - 1] == '\n') ? 1u : 0u;
    if (c) atomicAdd(s_cnt, c);
  }
  __syncthreads();
}

// Pass 1: every line validated, the tile's aggregate written; the first refused line of the chunk by its byte offset.
// KT: u64 (k <= 32) or u128; lmask: the bits a label may hold (meryl 2)
template <typename KT, typename D>
__global__ __launch_bounds__(PR_BLOCK)
void parse_count_kernel(const uint8_t *__restrict__ t, u64 n, u32 k, u64 lmask, typename D::State *__restrict__ state,
                        typename D::Agg *__restrict__ tiles) {
  typedef typename D::Agg A;
  __shared__ A s[PR_BLOCK];
  const bool aligned = (reinterpret_cast<uintptr_t>(t) & 15u) == 0;
  const u64 p0 = (u64)blockIdx.x * PR_TILE + (u64)threadIdx.x * PR_BYTES;
  u32 starts = pr_line_starts(t, n, p0, aligned);
  A agg = A::identity();
  u64 bad = ~0ull;
  while (starts) {
    const u32 q = (u32)__builtin_ctz(starts);
    starts &= starts - 1;
    const auto L = D::template parse<KT>(t, n, p0 + q, k, MGC_MODE_FORWARD, lmask, false);
    agg.lines++;
    if (L.kind == LN_RECORD) agg.rec++;
    else if (L.kind == LN_BAD) { if (bad == ~0ull) bad = ((p0 + q) << 3) | (u64)L.bad; }
    else D::fold(agg, L);
  }
  if (bad != ~0ull) atomicMin(reinterpret_cast<unsigned long long *>(&state->chunk_bad), (unsigned long long)bad);   // refused input only
  A tot;
  (void)block_scan_excl<PR_BLOCK, A>(agg, s, &tot);
  if (threadIdx.x == 0) tiles[blockIdx.x] = tot;
}

// after the composing step: the chunk's totals into the state; a refused line's byte offset -> its line number
template <typename D>
__global__ __launch_bounds__(PR_BLOCK)
void parse_total_kernel(const uint8_t *__restrict__ t, u64 n, typename D::State *__restrict__ state,
                        const typename D::Agg *__restrict__ tiles, const typename D::Agg *__restrict__ total) {
  __shared__ u32 s_cnt;
  const u64 bad = state->chunk_bad;
  pr_lines_before(t, n, bad >> 3, bad != ~0ull, &s_cnt);
  if (threadIdx.x == 0) {
    state->chunk_lines = total->lines;
    state->chunk_records = total->rec;
    D::chunk(state, *total);
    if (bad != ~0ull && state->first_bad == ~0ull) {
      const u64 line = state->lines_seen + (u64)tiles[(bad >> 3) / PR_TILE].lines + (u64)s_cnt + 1ull;
      state->first_bad = (line << 3) | (bad & 7ull);
    }
  }
}

// Pass 2: the records of the chunk in input order.
template <typename KT, typename D>
__global__ __launch_bounds__(PR_BLOCK)
void parse_emit_kernel(const uint8_t *__restrict__ t, u64 n, u32 k, int mode, u64 lmask, const typename D::State *__restrict__ state,
                       const typename D::Agg *__restrict__ tiles, u64 n_records, void *__restrict__ keys, u32 *__restrict__ vals,
                       u64 *__restrict__ labs) {
  typedef typename D::Agg A;
  __shared__ A s[PR_BLOCK];
  const bool aligned = (reinterpret_cast<uintptr_t>(t) & 15u) == 0;
  const u64 p0 = (u64)blockIdx.x * PR_TILE + (u64)threadIdx.x * PR_BYTES;
  const u32 starts0 = pr_line_starts(t, n, p0, aligned);
  // what this thread's lines are: only a setter line is read beyond the head of its first word
  A agg = A::identity();
  u32 recs = 0;                                                           // bit q: the line at p0 + q is a record
  for (u32 starts = starts0; starts;) {
    const u32 q = (u32)__builtin_ctz(starts);
    starts &= starts - 1;
    const u64 j = pr_first_word(t, n, p0 + q);
    if (j >= n) continue;
    if (!D::setter(t, n, j, lmask, agg)) { agg.rec++; recs |= 1u << q; }
  }
  A tot;
  A cur = A::combine(tiles[blockIdx.x], block_scan_excl<PR_BLOCK, A>(agg, s, &tot));   // the lines before this thread's
  u64 slot = (u64)cur.rec;
  D::seed(cur, state);
  for (u32 starts = starts0; starts;) {
    const u32 q = (u32)__builtin_ctz(starts);
    starts &= starts - 1;
    if (recs & (1u << q)) {
      const auto L = D::template parse<KT>(t, n, p0 + q, k, mode, lmask, true);
      if (slot < n_records) {                                             // (always, for text the count pass accepted)
        if (sizeof(KT) > 8) { K128 kk; kk.lo = L.lo; kk.hi = L.hi; reinterpret_cast<K128 *>(keys)[slot] = kk; }
        else reinterpret_cast<u64 *>(keys)[slot] = L.lo;
        D::store(L, cur, slot, vals, labs);
      }
      slot++;
    } else {
      const u64 j = pr_first_word(t, n, p0 + q);
      if (j < n) (void)D::setter(t, n, j, lmask, cur);                    // the later of two setters on one thread wins
    }
  }
}

// the state between chunks.  ST_BEGIN: before the first line; ST_RESET: before a count pass; ST_COMMIT: after an emit pass
enum { ST_BEGIN = 0, ST_RESET = 1, ST_COMMIT = 2 };
template <typename D>
__global__ void parse_state_kernel(typename D::State *state, int op) {
  if (op == ST_BEGIN) { state->lines_seen = 0; state->records_seen = 0; state->first_bad = ~0ull; D::begin(state); }
  if (op == ST_COMMIT) {
    state->lines_seen += state->chunk_lines;
    state->records_seen += state->chunk_records;
    D::commit(state);
  }
  state->chunk_lines = 0; state->chunk_records = 0; state->chunk_bad = ~0ull;
  D::chunk(state, D::Agg::identity());
}

template <typename State> struct DialectOf;
template <> struct DialectOf<ImportState>  { typedef Meryl1 D; };
template <> struct DialectOf<Import2State> { typedef Meryl2 D; };

static inline uint64_t parse_tiles(uint64_t n) { return (n + PR_TILE - 1) / PR_TILE; }
static inline u64 label_mask(uint32_t label_width) { return label_width >= 64 ? ~0ull : ((1ull << label_width) - 1ull); }

// workspace: [0, 64): the total; then one aggregate per tile
template <typename State>
size_t parse_workspace_bytes(uint64_t n_text) { return 64 + sizeof(typename DialectOf<State>::D::Agg) * (size_t)(parse_tiles(n_text) + 1); }

template <typename State>
hipError_t launch_parse_begin(State *d_state, hipStream_t st) {
  hipLaunchKernelGGL(parse_state_kernel<typename DialectOf<State>::D>, dim3(1), dim3(1), 0, st, d_state, (int)ST_BEGIN);
  return hipGetLastError();
}

template <typename State>
hipError_t launch_parse_count(const uint8_t *d_text, uint64_t n, uint32_t k, uint32_t label_width, State *d_state, void *d_ws, hipStream_t st) {
  typedef typename DialectOf<State>::D D;
  typedef typename D::Agg A;
  hipLaunchKernelGGL(parse_state_kernel<D>, dim3(1), dim3(1), 0, st, d_state, (int)ST_RESET);
  MGC_CHECK(hipGetLastError());
  const uint64_t T = parse_tiles(n);
  if (T == 0) return hipSuccess;
  A *total = reinterpret_cast<A *>(d_ws);
  A *tiles = reinterpret_cast<A *>(reinterpret_cast<unsigned char *>(d_ws) + 64);
  const u64 lmask = label_mask(label_width);
  if (k > 32) hipLaunchKernelGGL((parse_count_kernel<u128, D>), dim3((uint32_t)T), dim3(PR_BLOCK), 0, st, d_text, (u64)n, k, lmask, d_state, tiles);
  else        hipLaunchKernelGGL((parse_count_kernel<u64, D>), dim3((uint32_t)T), dim3(PR_BLOCK), 0, st, d_text, (u64)n, k, lmask, d_state, tiles);
  MGC_CHECK(hipGetLastError());
  hipLaunchKernelGGL(compose_tiles_kernel<A>, dim3(1), dim3(CP_BLOCK), 0, st, tiles, (u64)T, total);
  MGC_CHECK(hipGetLastError());
  hipLaunchKernelGGL(parse_total_kernel<D>, dim3(1), dim3(PR_BLOCK), 0, st, d_text, (u64)n, d_state, (const A *)tiles, (const A *)total);
  return hipGetLastError();
}

template <typename State>
hipError_t launch_parse_emit(const uint8_t *d_text, uint64_t n, uint32_t k, int mode, uint32_t label_width, State *d_state, void *d_ws,
                             void *d_keys, uint32_t *d_values, uint64_t *d_labels, hipStream_t st) {
  typedef typename DialectOf<State>::D D;
  typedef typename D::Agg A;
  const uint64_t T = parse_tiles(n);
  if (T) {
    const A *tiles = reinterpret_cast<const A *>(reinterpret_cast<const unsigned char *>(d_ws) + 64);
    // the number of records the count pass found bounds every store (the host allocated that many)
    uint64_t n_records = 0;
    MGC_CHECK(hipMemcpyAsync(&n_records, &d_state->chunk_records, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    MGC_CHECK(hipStreamSynchronize(st));
    if (n_records) {
      const u64 lmask = label_mask(label_width);
      if (k > 32) hipLaunchKernelGGL((parse_emit_kernel<u128, D>), dim3((uint32_t)T), dim3(PR_BLOCK), 0, st, d_text, (u64)n, k, mode, lmask,
                                     (const State *)d_state, tiles, (u64)n_records, d_keys, d_values, (u64 *)d_labels);
      else        hipLaunchKernelGGL((parse_emit_kernel<u64, D>), dim3((uint32_t)T), dim3(PR_BLOCK), 0, st, d_text, (u64)n, k, mode, lmask,
                                     (const State *)d_state, tiles, (u64)n_records, d_keys, d_values, (u64 *)d_labels);
      MGC_CHECK(hipGetLastError());
    }
  }
  hipLaunchKernelGGL(parse_state_kernel<D>, dim3(1), dim3(1), 0, st, d_state, (int)ST_COMMIT);
  return hipGetLastError();
}

#define MGC_PARSE_FOR(State)                                                                                                              \
  template size_t     parse_workspace_bytes<State>(uint64_t);                                                                             \
  template hipError_t launch_parse_begin<State>(State *, hipStream_t);                                                                    \
  template hipError_t launch_parse_count<State>(const uint8_t *, uint64_t, uint32_t, uint32_t, State *, void *, hipStream_t);             \
  template hipError_t launch_parse_emit<State>(const uint8_t *, uint64_t, uint32_t, int, uint32_t, State *, void *, void *, uint32_t *,   \
                                               uint64_t *, hipStream_t);
MGC_PARSE_FOR(ImportState)
MGC_PARSE_FOR(Import2State)
#undef MGC_PARSE_FOR

// ============================================================================
//  Pair sort: stable, low digit first, 8 bits per pass.
//  Per pass: digit counts per (digit, tile) -> exclusive scan over the whole table -> scatter, every pair ranked inside its
//  tile by 64-lane ballots (per-wave counters in LDS, no atomics on them: a wave's leaders hold distinct digits).
//  Traffic per pass: keys read twice, values once, both written once: 2 x (8|16) + 4 + (8|16) + 4 bytes per pair.
// ============================================================================
constexpr int SP_BLOCK = 256;
constexpr int SP_WAVES = SP_BLOCK / 64;
constexpr int SP_BITS  = 8;
constexpr int SP_BINS  = 1 << SP_BITS;
template <typename K> struct SpItems;
template <> struct SpItems<u64>  { static constexpr int N = 16; };
template <> struct SpItems<K128> { static constexpr int N = 8; };

template <typename K>
__global__ __launch_bounds__(SP_BLOCK)
void pair_hist_kernel(const K *__restrict__ keys, u64 n, u32 shift, u32 mask, u64 *__restrict__ table, u32 nblk) {
  constexpr int ITEMS = SpItems<K>::N;
  __shared__ u32 s_h[SP_BINS];
  s_h[threadIdx.x] = 0;
  __syncthreads();
  const u64 tile0 = (u64)blockIdx.x * (SP_BLOCK * ITEMS);
#pragma unroll
  for (int it = 0; it < ITEMS; it++) {
    const u64 pos = tile0 + (u64)it * SP_BLOCK + threadIdx.x;
    if (pos < n) atomicAdd(&s_h[KeyOps<K>::digit(keys[pos], shift, mask)], 1u);
  }
  __syncthreads();
  table[(u64)threadIdx.x * nblk + blockIdx.x] = s_h[threadIdx.x];
}

template <typename K>
__global__ __launch_bounds__(SP_BLOCK)
void pair_scatter_kernel(const K *__restrict__ kin, const u32 *__restrict__ vin, K *__restrict__ kout, u32 *__restrict__ vout, u64 n,
                         u32 shift, u32 mask, const u64 *__restrict__ table /*scanned*/, u32 nblk) {
  constexpr int ITEMS = SpItems<K>::N;
  __shared__ u32 s_cnt[SP_WAVES][SP_BINS];
  __shared__ u64 s_base[SP_BINS];
  const u32 lane = lane_id(), w = wave_id();
#pragma unroll
  for (int i = 0; i < SP_WAVES; i++) s_cnt[i][threadIdx.x] = 0;
  __syncthreads();
  const u64 wave0 = (u64)blockIdx.x * (SP_BLOCK * ITEMS) + (u64)w * (64 * ITEMS);
  const u64 lt = (1ull << lane) - 1ull;
  K   key[ITEMS];
  u32 val[ITEMS], dig[ITEMS], rk[ITEMS];
#pragma unroll
  for (int it = 0; it < ITEMS; it++) {
    const u64 pos = wave0 + (u64)it * 64 + lane;
    const bool valid = pos < n;
    key[it] = KeyOps<K>::zero(); val[it] = 0;
    if (valid) { key[it] = kin[pos]; val[it] = vin[pos]; }
    const u32 d = valid ? KeyOps<K>::digit(key[it], shift, mask) : 0u;
    u64 peers = __ballot(valid);
#pragma unroll
    for (int b = 0; b < SP_BITS; b++) {
      const bool bit = (d >> b) & 1u;
      const u64 bal = __ballot(bit);
      peers &= bit ? bal : ~bal;
    }
    const u32 leader = peers ? (u32)__builtin_ctzll(peers) : 0u;
    u32 pre = 0;
    if (valid && lane == leader) { pre = s_cnt[w][d]; s_cnt[w][d] = pre + (u32)__popcll(peers); }
    __builtin_amdgcn_wave_barrier();
    pre = __shfl(pre, (int)leader);
    dig[it] = d;
    rk[it] = pre + (u32)__popcll(peers & lt);
  }
  __syncthreads();
  {
    const u32 d = threadIdx.x;
    u32 run = 0;
#pragma unroll
    for (int i = 0; i < SP_WAVES; i++) { const u32 c = s_cnt[i][d]; s_cnt[i][d] = run; run += c; }
    s_base[d] = table[(u64)d * nblk + blockIdx.x];
  }
  __syncthreads();
#pragma unroll
  for (int it = 0; it < ITEMS; it++) {
    const u64 pos = wave0 + (u64)it * 64 + lane;
    if (pos < n) {
      const u64 dst = s_base[dig[it]] + (u64)s_cnt[w][dig[it]] + (u64)rk[it];
      if (dst < n) { kout[dst] = key[it]; vout[dst] = val[it]; }         // (always: the table counts exactly these pairs)
    }
  }
}

static inline uint64_t sp_tiles(uint64_t n, uint32_t key_words) {
  const uint64_t tile = (uint64_t)SP_BLOCK * (key_words == 2 ? SpItems<K128>::N : SpItems<u64>::N);
  return (n + tile - 1) / tile;
}
size_t sort_pairs_workspace_bytes(uint64_t n) {
  const uint64_t e = (uint64_t)SP_BINS * sp_tiles(n, 2);                 // (the smaller tile: enough for either key width)
  return (size_t)(e + scan_scratch_elems(e) + 8) * sizeof(u64);
}

template <typename K>
static hipError_t sort_pairs_t(K *keys, u32 *vals, K *akeys, u32 *avals, uint64_t n, uint32_t begin_bit, uint32_t end_bit, void *d_ws,
                               int *result_in_alt, hipStream_t st) {
  const uint32_t nblk = (uint32_t)sp_tiles(n, KeyOps<K>::WORDS);
  const uint64_t e = (uint64_t)SP_BINS * nblk;
  u64 *table = reinterpret_cast<u64 *>(d_ws), *scratch = table + e;
  int in_alt = 0;
  for (uint32_t shift = begin_bit; shift < end_bit; shift += SP_BITS) {
    const uint32_t bits = end_bit - shift < (uint32_t)SP_BITS ? end_bit - shift : (uint32_t)SP_BITS;
    const uint32_t mask = (1u << bits) - 1u;
    K *src = in_alt ? akeys : keys, *dst = in_alt ? keys : akeys;
    u32 *vsrc = in_alt ? avals : vals, *vdst = in_alt ? vals : avals;
    hipLaunchKernelGGL(pair_hist_kernel<K>, dim3(nblk), dim3(SP_BLOCK), 0, st, (const K *)src, (u64)n, shift, mask, table, nblk);
    MGC_CHECK(hipGetLastError());
    MGC_CHECK(scan_u64_exclusive(table, e, scratch, nullptr, st));
    hipLaunchKernelGGL(pair_scatter_kernel<K>, dim3(nblk), dim3(SP_BLOCK), 0, st, (const K *)src, (const u32 *)vsrc, dst, vdst, (u64)n,
                       shift, mask, (const u64 *)table, nblk);
    MGC_CHECK(hipGetLastError());
    in_alt ^= 1;
  }
  *result_in_alt = in_alt;
  return hipSuccess;
}

hipError_t launch_sort_pairs(void *d_keys, uint32_t *d_vals, void *d_alt_keys, uint32_t *d_alt_vals, uint64_t n, uint32_t key_words,
                             uint32_t begin_bit, uint32_t end_bit, void *d_ws, int *result_in_alt, hipStream_t st) {
  *result_in_alt = 0;
  if (n == 0 || begin_bit >= end_bit) return hipSuccess;
  if (n > (1ull << 40)) return hipErrorInvalidValue;                     // (the tile count is a 32-bit grid dimension)
  if (key_words == 2)
    return sort_pairs_t<K128>(reinterpret_cast<K128 *>(d_keys), d_vals, reinterpret_cast<K128 *>(d_alt_keys), d_alt_vals, n, begin_bit,
                              end_bit, d_ws, result_in_alt, st);
  return sort_pairs_t<u64>(reinterpret_cast<u64 *>(d_keys), d_vals, reinterpret_cast<u64 *>(d_alt_keys), d_alt_vals, n, begin_bit, end_bit,
                           d_ws, result_in_alt, st);
}

// ============================================================================
//  Triple sort: the pair sort over (key, record number), then one gather of values and labels.  Per pass that moves 4 bytes
//  of payload per record instead of 12; the price is one pass of scattered 4- and 8-byte reads at the end.
// ============================================================================
constexpr int TG_BLOCK = 256;
__global__ __launch_bounds__(TG_BLOCK)
void triple_number_kernel(u32 *__restrict__ idx, u64 n) {
  const u64 i = (u64)blockIdx.x * TG_BLOCK + threadIdx.x;
  if (i < n) idx[i] = (u32)i;
}
__global__ __launch_bounds__(TG_BLOCK)
void triple_gather_kernel(const u32 *__restrict__ idx, const u32 *__restrict__ vin, const u64 *__restrict__ lin, u32 *__restrict__ vout,
                          u64 *__restrict__ lout, u64 n) {
  const u64 i = (u64)blockIdx.x * TG_BLOCK + threadIdx.x;
  if (i < n) {
    const u64 j = idx[i];
    if (j < n) { vout[i] = vin[j]; lout[i] = lin[j]; }                   // (always: idx is a permutation of 0 .. n-1)
  }
}

static inline size_t tg_index_bytes(uint64_t n) { return (size_t)((n * sizeof(u32) + 255) & ~255ull); }
static inline size_t tg_pair_bytes(uint64_t n) { return (sort_pairs_workspace_bytes(n) + 255) & ~(size_t)255; }
// workspace: the pair sort's, then two arrays of record numbers
size_t sort_triples_workspace_bytes(uint64_t n) { return tg_pair_bytes(n) + 2 * tg_index_bytes(n); }

hipError_t launch_sort_triples(void *d_keys, uint32_t *d_vals, uint64_t *d_labs, void *d_alt_keys, uint32_t *d_alt_vals, uint64_t *d_alt_labs,
                               uint64_t n, uint32_t key_words, uint32_t begin_bit, uint32_t end_bit, void *d_ws, int *result_in_alt,
                               hipStream_t st) {
  *result_in_alt = 0;
  if (n == 0 || begin_bit >= end_bit) return hipSuccess;
  if (n > MGC_SORT_TRIPLES_MAX_N) return hipErrorInvalidValue;           // (a record number is 32 bits; the C layer says so in words)
  unsigned char *ws = reinterpret_cast<unsigned char *>(d_ws);
  u32 *idx0 = reinterpret_cast<u32 *>(ws + tg_pair_bytes(n)), *idx1 = reinterpret_cast<u32 *>(ws + tg_pair_bytes(n) + tg_index_bytes(n));
  const uint32_t grid = (uint32_t)((n + TG_BLOCK - 1) / TG_BLOCK);
  hipLaunchKernelGGL(triple_number_kernel, dim3(grid), dim3(TG_BLOCK), 0, st, idx0, (u64)n);
  MGC_CHECK(hipGetLastError());
  int in_alt = 0;
  MGC_CHECK(launch_sort_pairs(d_keys, idx0, d_alt_keys, idx1, n, key_words, begin_bit, end_bit, d_ws, &in_alt, st));
  hipLaunchKernelGGL(triple_gather_kernel, dim3(grid), dim3(TG_BLOCK), 0, st, (const u32 *)(in_alt ? idx1 : idx0), (const u32 *)d_vals,
                     (const u64 *)d_labs, d_alt_vals, (u64 *)d_alt_labs, (u64)n);
  MGC_CHECK(hipGetLastError());
  // values and labels are in the alternates now: the keys join them there
  if (!in_alt) MGC_CHECK(hipMemcpyAsync(d_alt_keys, d_keys, (size_t)n * sizeof(u64) * key_words, hipMemcpyDeviceToDevice, st));
  *result_in_alt = 1;
  return hipSuccess;
}

// ============================================================================
//  Reduce by key over sorted pairs, or over sorted triples (LABELS): the labels of a segment are summed beside its values
//  (_labels[...] += getLabel(), src/meryl2/merylCountArray.C:400; the low label_width bits are what the writer stores)
// ============================================================================
constexpr int RD_BLOCK = 256;
constexpr int RD_ITEMS = 8;
constexpr int RD_TILE  = RD_BLOCK * RD_ITEMS;

// segment heads of a range, and the (wrapped) sum of the values from its last head to its end -- of ALL its values when it
// holds no head: the part of a segment that is still open where the range ends.  LABELS: the label sum of that part too
struct RNoLabels {};
struct RLabels { u64 lsum; };
template <bool LABELS>
struct RAgg : std::conditional<LABELS, RLabels, RNoLabels>::type {      // (16 bytes without labels: the empty base takes none)
  u64 heads; u32 has, sum;
  static __device__ __forceinline__ RAgg identity() {
    RAgg a; a.heads = 0; a.has = 0; a.sum = 0;
    if constexpr (LABELS) a.lsum = 0;
    return a;
  }
  static __device__ __forceinline__ RAgg combine(RAgg a, RAgg b) {
    RAgg r; r.heads = a.heads + b.heads; r.has = a.has | b.has; r.sum = b.has ? b.sum : a.sum + b.sum;
    if constexpr (LABELS) r.lsum = b.has ? b.lsum : a.lsum + b.lsum;
    return r;
  }
};
static_assert(sizeof(RAgg<false>) == 16 && sizeof(RAgg<true>) == 24, "the reduce workspaces are sized by these");

// labs, lmask, out_labs: read only with LABELS
template <typename K, bool LABELS, bool EMIT>
__global__ __launch_bounds__(RD_BLOCK)
void reduce_kernel(const K *__restrict__ keys, const u32 *__restrict__ vals, const u64 *__restrict__ labs, u64 n,
                   RAgg<LABELS> *__restrict__ tiles /*EMIT: scanned*/, u64 n_out, u64 lmask, K *__restrict__ out_keys,
                   u32 *__restrict__ out_vals, u64 *__restrict__ out_labs) {
  typedef RAgg<LABELS> A;
  __shared__ A s[RD_BLOCK];
  const u64 i0 = (u64)blockIdx.x * RD_TILE + (u64)threadIdx.x * RD_ITEMS;
  K   kreg[RD_ITEMS];
  u32 vreg[RD_ITEMS];
  u64 lreg[RD_ITEMS];
  u32 head = 0;                                          // bit q: element i0 + q starts a segment
  K prev = KeyOps<K>::zero();
  if (i0 > 0 && i0 < n) prev = keys[i0 - 1];
  A agg = A::identity();
#pragma unroll
  for (int q = 0; q < RD_ITEMS; q++) {
    const u64 i = i0 + q;
    kreg[q] = KeyOps<K>::zero(); vreg[q] = 0; lreg[q] = 0;
    if (i < n) {
      kreg[q] = keys[i]; vreg[q] = vals[i];
      if constexpr (LABELS) lreg[q] = labs[i];
      const bool h = (i == 0) || KeyOps<K>::ne(prev, kreg[q]);
      if (h) {
        head |= 1u << q; agg.heads++; agg.has = 1; agg.sum = 0;
        if constexpr (LABELS) agg.lsum = 0;
      }
      agg.sum += vreg[q];
      if constexpr (LABELS) agg.lsum += lreg[q];
      prev = kreg[q];
    }
  }
  A tot;
  const A excl = block_scan_excl<RD_BLOCK, A>(agg, s, &tot);
  if (!EMIT) {
    if (threadIdx.x == 0) tiles[blockIdx.x] = tot;
    return;
  }
  const A before = A::combine(tiles[blockIdx.x], excl);
  u64 hc = before.heads;
  u32 run = before.sum;
  u64 lrun = 0;
  if constexpr (LABELS) lrun = before.lsum;
  K next = KeyOps<K>::zero();
  if (i0 + RD_ITEMS < n) next = keys[i0 + RD_ITEMS];
#pragma unroll
  for (int q = 0; q < RD_ITEMS; q++) {
    const u64 i = i0 + q;
    if (i < n) {
      if (head & (1u << q)) { hc++; run = 0; lrun = 0; }
      run += vreg[q];
      if constexpr (LABELS) lrun += lreg[q];
      const K nx = (q + 1 < RD_ITEMS) ? kreg[(q + 1 < RD_ITEMS) ? q + 1 : q] : next;
      const bool last = (i + 1 == n) || KeyOps<K>::ne(kreg[q], nx);      // the segment ends here: its sums are complete
      if (last && hc >= 1 && hc - 1 < n_out) {
        out_keys[hc - 1] = kreg[q]; out_vals[hc - 1] = run;
        if constexpr (LABELS) out_labs[hc - 1] = lrun & lmask;
      }
    }
  }
}

__global__ void reduce_total_kernel(const u64 *heads, u64 *out) { *out = *heads; }

static inline uint64_t rd_tiles(uint64_t n) { return (n + RD_TILE - 1) / RD_TILE; }
// workspace: [0] distinct keys (u64), [64, 128): the composed total, then one RAgg per tile
size_t reduce_pairs_workspace_bytes(uint64_t n) { return 128 + sizeof(RAgg<false>) * (size_t)(rd_tiles(n) + 1); }
size_t reduce_triples_workspace_bytes(uint64_t n) { return 128 + sizeof(RAgg<true>) * (size_t)(rd_tiles(n) + 1); }

// one pass of the reduction.  !EMIT: the tiles' aggregates, composed, and the number of distinct keys into the workspace
template <typename K, bool LABELS, bool EMIT>
static hipError_t reduce_pass(const void *d_keys, const uint32_t *d_vals, const uint64_t *d_labs, uint64_t n, uint64_t T, void *d_ws,
                              uint64_t n_out, u64 lmask, void *d_out_keys, uint32_t *d_out_vals, uint64_t *d_out_labs, hipStream_t st) {
  typedef RAgg<LABELS> A;
  A *total = reinterpret_cast<A *>(reinterpret_cast<unsigned char *>(d_ws) + 64);
  A *tiles = reinterpret_cast<A *>(reinterpret_cast<unsigned char *>(d_ws) + 128);
  hipLaunchKernelGGL((reduce_kernel<K, LABELS, EMIT>), dim3((uint32_t)T), dim3(RD_BLOCK), 0, st, reinterpret_cast<const K *>(d_keys), d_vals,
                     (const u64 *)d_labs, (u64)n, tiles, (u64)n_out, lmask, reinterpret_cast<K *>(d_out_keys), d_out_vals, (u64 *)d_out_labs);
  if (EMIT) return hipGetLastError();
  MGC_CHECK(hipGetLastError());
  hipLaunchKernelGGL(compose_tiles_kernel<A>, dim3(1), dim3(CP_BLOCK), 0, st, tiles, (u64)T, total);
  MGC_CHECK(hipGetLastError());
  hipLaunchKernelGGL(reduce_total_kernel, dim3(1), dim3(1), 0, st, (const u64 *)&total->heads, reinterpret_cast<u64 *>(d_ws));
  return hipGetLastError();
}

// d_labs: NULL for pairs
template <bool EMIT>
static hipError_t reduce_pass_for(const void *d_keys, const uint32_t *d_vals, const uint64_t *d_labs, uint64_t n, uint32_t key_words, uint64_t T,
                                  void *d_ws, uint64_t n_out, u64 lmask, void *d_out_keys, uint32_t *d_out_vals, uint64_t *d_out_labs,
                                  hipStream_t st) {
  if (d_labs)
    return key_words == 2 ? reduce_pass<K128, true, EMIT>(d_keys, d_vals, d_labs, n, T, d_ws, n_out, lmask, d_out_keys, d_out_vals, d_out_labs, st)
                          : reduce_pass<u64, true, EMIT>(d_keys, d_vals, d_labs, n, T, d_ws, n_out, lmask, d_out_keys, d_out_vals, d_out_labs, st);
  return key_words == 2 ? reduce_pass<K128, false, EMIT>(d_keys, d_vals, d_labs, n, T, d_ws, n_out, lmask, d_out_keys, d_out_vals, d_out_labs, st)
                        : reduce_pass<u64, false, EMIT>(d_keys, d_vals, d_labs, n, T, d_ws, n_out, lmask, d_out_keys, d_out_vals, d_out_labs, st);
}

hipError_t launch_reduce_count(const void *d_keys, const uint32_t *d_vals, const uint64_t *d_labs, uint64_t n, uint32_t key_words, void *d_ws,
                               hipStream_t st) {
  const uint64_t T = rd_tiles(n);
  if (T == 0) return hipMemsetAsync(d_ws, 0, 8, st);
  if (T > 0xFFFFFFFFull) return hipErrorInvalidValue;
  return reduce_pass_for<false>(d_keys, d_vals, d_labs, n, key_words, T, d_ws, 0, 0, nullptr, nullptr, nullptr, st);
}

hipError_t launch_reduce_emit(const void *d_keys, const uint32_t *d_vals, const uint64_t *d_labs, uint64_t n, uint32_t key_words,
                              uint32_t label_width, void *d_ws, void *d_out_keys, uint32_t *d_out_vals, uint64_t *d_out_labs, hipStream_t st) {
  const uint64_t T = rd_tiles(n);
  if (T == 0) return hipSuccess;
  if (T > 0xFFFFFFFFull) return hipErrorInvalidValue;
  // the count pass's total bounds every store (the caller allocated that many)
  uint64_t n_out = 0;
  MGC_CHECK(hipMemcpyAsync(&n_out, d_ws, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  MGC_CHECK(hipStreamSynchronize(st));
  return reduce_pass_for<true>(d_keys, d_vals, d_labs, n, key_words, T, d_ws, n_out, label_mask(label_width), d_out_keys, d_out_vals, d_out_labs, st);
}

}  // namespace mgc
