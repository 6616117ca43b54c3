// mgc_sam_fsm.hpp -- the SEQ column of SAM text as a finite-state parse that can be cut anywhere: the summary of a run of bytes as a
// function of the state the run is entered in, the composition of two summaries, and what a run emits for a given entry state.  The
// parse kernels (mgc_parse.hip: a thread's 16 bytes, a tile, a piece) and a plain host program (tests/host/sam_fsm_host.cpp) take all
// of it from here.  No dependency but <cstdint>.
//
// The contract (include/meryl_gpu_count.h, MGC_TEXT_SAM): a LINE START begins the file or follows '\n'.  A line whose start is '\n'
// is empty, one whose start is '@' is a header line; neither emits anything.  A line start of '\r' refuses the file.  Every other
// line is an alignment line: a byte's column is the number of tabs before it in the line, the bytes of column 9 that are not '\t'
// '\n' '\r' '*' are emitted as they are, the line's '\n' emits one '.', and a '\n' with fewer than 9 tabs before it refuses the file.
//
// The state of the byte after a run is one of twelve: column 0 .. 9, SAM_PAST (a column above 9), SAM_HEADER.  Only the bytes of a
// run before its first line start -- its HEAD -- depend on the state it is entered in, and of that state they need the column only:
// the head's bytes after i tabs are emitted iff column + i == 9.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MGC_SAM_FN __host__ __device__ __forceinline__
#else
#define MGC_SAM_FN inline
#endif

namespace mgc {

constexpr uint32_t SAM_SEQ_COLUMN = 9u, SAM_PAST = 10u, SAM_HEADER = 11u;
constexpr uint32_t SAM_ERR_FEW_COLUMNS = 1u, SAM_ERR_CR_LINE_START = 2u;    // why a file is refused
constexpr uint32_t SAM_OUT_NONE = 0u, SAM_OUT_BYTE = 1u, SAM_OUT_DOT = 2u;

// One byte met in a known state: what it emits, what it finds wrong (ORed into *err), and the state of the next byte.  After a '\n'
// the next byte is a line start, which takes no state: 0 stands for it.
MGC_SAM_FN uint32_t sam_step(uint32_t state, uint8_t c, bool line_start, uint32_t *out, uint32_t *err) {
  *out = SAM_OUT_NONE;
  if (line_start) {
    if (c == '\n') return 0u;                                // an empty line
    if (c == '@') return SAM_HEADER;
    if (c == '\r') *err |= SAM_ERR_CR_LINE_START;
    return c == '\t' ? 1u : 0u;
  }
  if (c == '\n') {
    if (state != SAM_HEADER) { if (state >= SAM_SEQ_COLUMN) *out = SAM_OUT_DOT; else *err |= SAM_ERR_FEW_COLUMNS; }
    return 0u;
  }
  if (state == SAM_HEADER) return state;
  if (c == '\t') return state < SAM_PAST ? state + 1u : SAM_PAST;
  if (state == SAM_SEQ_COLUMN && c != '\r' && c != '*') *out = SAM_OUT_BYTE;
  return state;
}

// ---- exit state as a function of the entry state ----------------------------------------------------------------------------------
// Either "x, whatever the entry state" (the run holds a line start or a '\n'): SAM_FN_CONST | x; or "the entry column and t tabs": t.
// 0 is the identity.
constexpr uint32_t SAM_FN_CONST = 16u;
MGC_SAM_FN uint32_t sam_tabs_on(uint32_t state, uint32_t tabs) { return state >= SAM_PAST ? state : (state + tabs > SAM_PAST ? SAM_PAST : state + tabs); }
MGC_SAM_FN uint32_t sam_fn_apply(uint32_t fn, uint32_t state) { return (fn & SAM_FN_CONST) ? (fn & 15u) : sam_tabs_on(state, fn); }
// f, then g.  Associative: a segmented scan -- the state at the last line start plus the tabs since
MGC_SAM_FN uint32_t sam_fn_then(uint32_t f, uint32_t g) {
  if (g & SAM_FN_CONST) return g;
  if (f & SAM_FN_CONST) return SAM_FN_CONST | sam_tabs_on(f & 15u, g);
  return f + g > SAM_PAST ? SAM_PAST : f + g;
}

// ---- the emit-eligible bytes of a head by the tabs before them: ten counters ---------------------------------------------------
struct SamSegWide {                                          // any run below 4 GiB: a tile, a piece, a file
  uint32_t c[10];
  MGC_SAM_FN void clear() { for (int i = 0; i < 10; i++) c[i] = 0u; }
  MGC_SAM_FN void add(uint32_t i, uint32_t n) { c[i] += n; }
  MGC_SAM_FN uint32_t get(uint32_t i) const { return c[i]; }
};
struct SamSegPacked {                                        // a run of at most 31 bytes (a thread's 16), in registers: 5 bits each
  uint64_t p;
  MGC_SAM_FN void clear() { p = 0ull; }
  MGC_SAM_FN void add(uint32_t i, uint32_t n) { p += (uint64_t)n << (5u * i); }
  MGC_SAM_FN uint32_t get(uint32_t i) const { return (uint32_t)(p >> (5u * i)) & 31u; }
};

constexpr uint32_t SAM_S_NONEMPTY = 1u;                      // the run holds a byte
constexpr uint32_t SAM_S_HEAD_NL = 2u;                       // the head ends with a '\n' (whose verdict depends on the entry state)
constexpr uint32_t SAM_S_LAST_NL = 4u;                       // the run's last byte is '\n': the next run begins with a line start
constexpr uint32_t SAM_S_ERR_SHIFT = 4u;                     // SAM_ERR_* found after the head, whatever the entry state

template <class Seg>
struct SamSummary {
  Seg      seg;                                              // head: emit-eligible bytes after i tabs of the head, i = 0 .. 9
  uint32_t tabs;                                             // head: its tabs (before its '\n'), saturating at 10
  uint32_t rest;                                             // bytes emitted after the head
  uint32_t fn;                                               // exit state as a function of the entry state
  uint32_t flags;
};
typedef SamSummary<SamSegWide> SamTileSummary;               // 56 bytes: fits the text parser's 64-byte tile summary

MGC_SAM_FN bool sam_emit_eligible(uint8_t c) { return c != '\t' && c != '\n' && c != '\r' && c != '*'; }

// The summary of a run, a byte at a time: begin(whether the first byte is a line start), feed(every byte), finish().
template <class Seg>
struct SamSummariser {
  SamSummary<Seg> S;
  bool     head, ls;
  uint32_t tabs, state, err;
  MGC_SAM_FN void begin(bool first_is_line_start) {
    S.seg.clear(); S.tabs = 0u; S.rest = 0u; S.fn = 0u; S.flags = 0u;
    head = !first_is_line_start; ls = first_is_line_start;
    tabs = 0u; state = 0u; err = 0u;
  }
  MGC_SAM_FN void feed(uint8_t c) {
    S.flags |= SAM_S_NONEMPTY;
    if (head) {
      if (c == '\n') { S.flags |= SAM_S_HEAD_NL; head = false; S.tabs = tabs; state = 0u; }
      else if (c == '\t') tabs = tabs < SAM_PAST ? tabs + 1u : SAM_PAST;
      else if (tabs <= SAM_SEQ_COLUMN && sam_emit_eligible(c)) S.seg.add(tabs, 1u);
    } else {
      uint32_t out;
      state = sam_step(state, c, ls, &out, &err);
      if (out != SAM_OUT_NONE) S.rest++;
    }
    ls = c == '\n';
  }
  MGC_SAM_FN void finish() {
    if (!(S.flags & SAM_S_NONEMPTY)) return;
    if (head) { S.tabs = tabs; S.fn = tabs; }
    else S.fn = SAM_FN_CONST | state;
    if (ls) S.flags |= SAM_S_LAST_NL;
    S.flags |= err << SAM_S_ERR_SHIFT;
  }
};

// The summary of n bytes whose first byte is (not) a line start.
template <class Seg>
MGC_SAM_FN void sam_summarise(const uint8_t *b, uint64_t n, bool first_is_line_start, SamSummary<Seg> *S) {
  SamSummariser<Seg> r;
  r.begin(first_is_line_start);
  for (uint64_t i = 0; i < n; i++) r.feed(b[i]);
  r.finish();
  *S = r.S;
}

// What a summarised run emits when it is entered in `state`; what is wrong with it then is ORed into *err.
template <class Seg>
MGC_SAM_FN uint32_t sam_emit_for_entry(const SamSummary<Seg> &S, uint32_t state, uint32_t *err) {
  uint32_t e = S.rest;
  *err |= S.flags >> SAM_S_ERR_SHIFT;
  if (state == SAM_HEADER) return e;
  if (state <= SAM_SEQ_COLUMN) e += S.seg.get(SAM_SEQ_COLUMN - state);
  if (S.flags & SAM_S_HEAD_NL) {
    if (sam_tabs_on(state, S.tabs) >= SAM_SEQ_COLUMN) e += 1u;
    else *err |= SAM_ERR_FEW_COLUMNS;
  }
  return e;
}

// The summary of run a followed by run b (b summarised with first_is_line_start = a's SAM_S_LAST_NL).
template <class SegA, class SegB>
MGC_SAM_FN void sam_compose(SamSummary<SegA> *a, const SamSummary<SegB> &b) {
  if (!(b.flags & SAM_S_NONEMPTY)) return;
  if (!(a->flags & SAM_S_NONEMPTY)) {
    a->seg.clear();
    for (uint32_t i = 0; i < 10u; i++) a->seg.add(i, b.seg.get(i));
    a->tabs = b.tabs; a->rest = b.rest; a->fn = b.fn; a->flags = b.flags;
    return;
  }
  uint32_t flags = a->flags & ~SAM_S_LAST_NL;
  if (a->fn & SAM_FN_CONST) {                                // a's head is closed: b is entered in a known state
    uint32_t err = 0u;
    a->rest += sam_emit_for_entry(b, a->fn & 15u, &err);
    flags |= err << SAM_S_ERR_SHIFT;
  } else {                                                   // b's head goes on with a's
    for (uint32_t i = 0; i + a->tabs <= SAM_SEQ_COLUMN; i++) a->seg.add(a->tabs + i, b.seg.get(i));
    a->tabs = a->tabs + b.tabs > SAM_PAST ? SAM_PAST : a->tabs + b.tabs;
    a->rest += b.rest;
    flags |= b.flags & (SAM_S_HEAD_NL | (~0u << SAM_S_ERR_SHIFT));
  }
  a->fn = sam_fn_then(a->fn, b.fn);
  a->flags = flags | (b.flags & SAM_S_LAST_NL);
}

}  // namespace mgc
