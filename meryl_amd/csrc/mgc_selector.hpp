// mgc_selector.hpp -- whether a k-mer an operation is about to write passes the operation's selector program: meryl2's
// merylSelector::isTrue (src/meryl2/merylSelector.C:72-156) over a sum of products (merylOp-nextMer.C:58-192); the rules, with the
// line each comes from, are in include/meryl_gpu_count.h (mgc_select_term).  Shared by the kernels (mgc_merge_many.hip,
// mgc_merge.hip), the host code that checks and parses programs (mgc_api.cpp, mgc_eval.cpp) and a stand-alone host program
// (tests/host/select_host.cpp): plain C++, no HIP header needed.
#pragma once
#include "../../include/meryl_gpu_count.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#if defined(__HIPCC__)
#define MGC_SEL_FN __host__ __device__ __forceinline__
#else
#define MGC_SEL_FN inline
#endif

namespace mgc {

// what a program needs read per element (SelectProgram::flags)
constexpr uint32_t SELF_VALUES = 1u, SELF_LABELS = 2u, SELF_KEYS = 4u;

// a program as the kernels take it, in the kernel-argument segment (784 bytes)
struct SelectProgram {
  mgc_select_term t[MGC_SELECT_MAX_TERMS];
  uint32_t n, flags;                 // terms, SELF_*
  uint32_t k, reserved;              // k-mer size (BASES)
};

// the kernel argument of an instantiation: the program with SELECT, an empty struct without
struct SelectNone {};
template <bool SELECT> struct SelectArg { typedef SelectNone type; };
template <> struct SelectArg<true> { typedef SelectProgram type; };

// the same for a kernel that stages the program in LDS word by word (select_kernel): plain 64-bit words, so that the staging
// loop indexes the argument with constants only
struct SelectWords { unsigned long long w[sizeof(SelectProgram) / 8]; };
static_assert(sizeof(SelectProgram) % 8 == 0 && sizeof(SelectWords) == sizeof(SelectProgram), "the program as whole words");
template <bool SELECT> struct SelectWordsArg { typedef SelectNone type; };
template <> struct SelectWordsArg<true> { typedef SelectWords type; };

template <typename T>
MGC_SEL_FN bool sel_compare(int rel, T x, T y) {
  switch (rel) {
    case MGC_REL_EQ:  return x == y;
    case MGC_REL_NEQ: return x != y;
    case MGC_REL_LEQ: return x <= y;
    case MGC_REL_GEQ: return x >= y;
    case MGC_REL_LT:  return x < y;
    case MGC_REL_GT:  return x > y;
    default:          return false;
  }
}

// bases of one key word that are NOT letter `code`: XOR the letter to A (00), squash a base's two bits into the upper one and
// count (countNonZeroBases, merylSelector.H:123-139); `valid` keeps the bits that hold bases -- the zeros above 2k are no A's
MGC_SEL_FN uint32_t sel_not_letter(uint64_t w, uint32_t code, uint64_t valid) {
  w ^= 0x5555555555555555ull * code;
  w |= w << 1;
  w &= 0xaaaaaaaaaaaaaaaaull & valid;
  return (uint32_t)__builtin_popcountll(w);
}
// how many bases of the k-mer (lo: bases 0..31 from the right, hi: the rest) are one of the letters of base_mask
MGC_SEL_FN uint32_t sel_count_bases(uint64_t lo, uint64_t hi, uint32_t k, uint32_t base_mask) {
  const uint32_t kl = k < 32 ? k : 32, kh = k > 32 ? (k > 64 ? 32 : k - 32) : 0;
  const uint64_t vl = kl == 32 ? ~0ull : ((1ull << (2 * kl)) - 1), vh = kh == 32 ? ~0ull : ((1ull << (2 * kh)) - 1);
  uint32_t c = 0;
  for (uint32_t code = 0; code < 4; code++)
    if (base_mask & (1u << code)) c += (kl + kh) - sel_not_letter(lo, code, vl) - sel_not_letter(hi, code, vh);
  return c;
}

// Src: what a term may look at --
//   uint32_t presence      bit i: input i + 1 holds the k-mer
//   uint32_t out_value; uint64_t out_label; uint64_t lo, hi     the k-mer as it would be written
//   uint32_t value(i); uint64_t label(i)                        of input i + 1, which holds the k-mer
template <typename T> struct SelSide { bool ok; T v; };         // ok false: the side names an input that does not hold the k-mer
template <typename Src>
MGC_SEL_FN SelSide<uint32_t> sel_side_value(const Src &s, int32_t index, uint64_t constant) {
  if (index < 0) return {true, (uint32_t)constant};
  if (index == 0) return {true, s.out_value};
  const uint32_t i = (uint32_t)index - 1;
  if (i >= 32 || !((s.presence >> i) & 1u)) return {false, 0u};
  return {true, s.value(i)};
}
template <typename Src>
MGC_SEL_FN SelSide<uint64_t> sel_side_label(const Src &s, int32_t index, uint64_t constant) {
  if (index < 0) return {true, constant};
  if (index == 0) return {true, s.out_label};
  const uint32_t i = (uint32_t)index - 1;
  if (i >= 32 || !((s.presence >> i) & 1u)) return {false, 0ull};
  return {true, s.label(i)};
}

template <typename Src>
MGC_SEL_FN bool select_term(const mgc_select_term &t, uint32_t k, const Src &s) {
  bool r = false;
  switch (t.quantity) {
    case MGC_SEL_VALUE: {
      const SelSide<uint32_t> a = sel_side_value(s, t.lhs_index, t.lhs_constant), b = sel_side_value(s, t.rhs_index, t.rhs_constant);
      if (!a.ok || !b.ok) return false;
      r = sel_compare<uint32_t>(t.relation, a.v, b.v);
      break;
    }
    case MGC_SEL_LABEL: {
      const SelSide<uint64_t> a = sel_side_label(s, t.lhs_index, t.lhs_constant), b = sel_side_label(s, t.rhs_index, t.rhs_constant);
      if (!a.ok || !b.ok) return false;
      r = sel_compare<uint64_t>(t.relation, a.v, b.v);
      break;
    }
    case MGC_SEL_BASES: {
      const uint64_t c = sel_count_bases(s.lo, s.hi, k, t.base_mask);
      r = t.lhs_index == 0 ? sel_compare<uint64_t>(t.relation, c, t.rhs_constant) : sel_compare<uint64_t>(t.relation, t.lhs_constant, c);
      break;
    }
    case MGC_SEL_INPUT:
      r = ((t.count_mask >> __builtin_popcount(s.presence)) & 1ull) && (t.required_mask & ~s.presence) == 0;
      break;
    default:
      return false;
  }
  return r != (t.negate != 0);
}

// the sum of products: kept when every term of some product holds; no terms: kept
template <typename Src>
MGC_SEL_FN bool select_keep(const mgc_select_term *t, uint32_t n, uint32_t k, const Src &s) {
  if (n == 0) return true;
  bool product = true;
  for (uint32_t i = 0; i < n; i++) {
    if (product) product = select_term(t[i], k, s);
    if (t[i].ends_product || i + 1 == n) {
      if (product) return true;
      product = true;
    }
  }
  return false;
}

// ---- host side: checking and parsing programs ---------------------------------------------------------------------------
inline uint32_t select_flags(const mgc_select_term *t, uint32_t n) {
  uint32_t f = 0;
  for (uint32_t i = 0; i < n; i++) {
    if (t[i].quantity == MGC_SEL_VALUE) f |= SELF_VALUES;
    if (t[i].quantity == MGC_SEL_LABEL) f |= SELF_VALUES | SELF_LABELS;      // LabelAcc's MIN / SELECTED look at the values
    if (t[i].quantity == MGC_SEL_BASES) f |= SELF_KEYS;
  }
  return f;
}

// checked terms (select_check) -> the program a launch passes; false: more terms than a program holds, or a k no key holds
inline bool select_program(SelectProgram *pg, const mgc_select_term *t, uint32_t n, uint32_t k) {
  if (n > MGC_SELECT_MAX_TERMS || (n && !t) || k < 1 || k > 64) return false;
  memset(pg, 0, sizeof(*pg));
  for (uint32_t i = 0; i < n; i++) pg->t[i] = t[i];
  pg->n = n; pg->flags = select_flags(t, n); pg->k = k;
  return true;
}

// mgc_select_check: empty string = a program every kernel may take for a node of n_inputs inputs
inline std::string select_check(const mgc_select_term *t, uint32_t n, uint32_t n_inputs) {
  if (n > MGC_SELECT_MAX_TERMS) return "a selector has at most " + std::to_string(MGC_SELECT_MAX_TERMS) + " terms, this one " + std::to_string(n);
  if (n && !t) return "no terms";
  const uint32_t N = n_inputs > 32 ? 32 : n_inputs;
  for (uint32_t i = 0; i < n; i++) {
    const mgc_select_term &e = t[i];
    const std::string id = "term " + std::to_string(i + 1) + ": ";
    if (e.quantity < MGC_SEL_VALUE || e.quantity > MGC_SEL_INPUT) return id + "unknown quantity " + std::to_string(e.quantity);
    if (e.quantity == MGC_SEL_INPUT) {
      const uint64_t allowed = N >= 63 ? ~0ull : ((1ull << (N + 1)) - 1);
      if (e.count_mask & ~allowed) return id + "a k-mer cannot be in more than " + std::to_string(n_inputs) + " inputs; there are only that many";
      if (N < 32 && (e.required_mask >> N)) return id + "a required input does not exist; there are only " + std::to_string(n_inputs) + " inputs";
      continue;
    }
    if (e.relation < MGC_REL_EQ || e.relation > MGC_REL_GT) return id + "unknown relation " + std::to_string(e.relation);
    if (e.lhs_index < -1 || e.rhs_index < -1) return id + "an index below -1";
    if (e.lhs_index > (int32_t)N || e.rhs_index > (int32_t)N)
      return id + "input " + std::to_string(e.lhs_index > e.rhs_index ? e.lhs_index : e.rhs_index) + " does not exist; there are only " +
             std::to_string(n_inputs) + " inputs";
    if (e.lhs_index == e.rhs_index) return id + "both sides are the same source: always true (or false)";
    if (e.quantity == MGC_SEL_BASES) {
      if (e.lhs_index > 0 || e.rhs_index > 0) return id + "a bases: selector cannot name an input (the k-mer is the same in all of them)";
      if (!(e.base_mask & 15u) || (e.base_mask & ~15u)) return id + "a bases: selector needs letters of acgt";
    }
  }
  return "";
}

inline bool sel_is_relation(const char *s, uint32_t *len, int *rel) {
  static const struct { const char *w; int r; } two[] = {{"==", MGC_REL_EQ}, {"eq", MGC_REL_EQ}, {"!=", MGC_REL_NEQ}, {"<>", MGC_REL_NEQ},
      {"ne", MGC_REL_NEQ}, {"<=", MGC_REL_LEQ}, {"le", MGC_REL_LEQ}, {">=", MGC_REL_GEQ}, {"ge", MGC_REL_GEQ}, {"lt", MGC_REL_LT}, {"gt", MGC_REL_GT}};
  for (const auto &e : two)
    if (s[0] == e.w[0] && s[0] && s[1] == e.w[1]) { *len = 2; *rel = e.r; return true; }
  if (s[0] == '=') { *len = 1; *rel = MGC_REL_EQ; return true; }
  if (s[0] == '<') { *len = 1; *rel = MGC_REL_LT; return true; }
  if (s[0] == '>') { *len = 1; *rel = MGC_REL_GT; return true; }
  return false;
}
// an unsigned integer: decimal, 0x hexadecimal, 0b binary; the whole string
inline bool sel_integer(const std::string &s, uint64_t *v) {
  if (s.empty()) return false;
  int base = 10;
  size_t at = 0;
  if (s.size() > 2 && s[0] == '0' && (s[1] == 'x' || s[1] == 'X')) { base = 16; at = 2; }
  else if (s.size() > 2 && s[0] == '0' && (s[1] == 'b' || s[1] == 'B')) { base = 2; at = 2; }
  uint64_t x = 0;
  for (; at < s.size(); at++) {
    const char c = s[at];
    int d = (c >= '0' && c <= '9') ? c - '0' : (c >= 'a' && c <= 'f') ? c - 'a' + 10 : (c >= 'A' && c <= 'F') ? c - 'A' + 10 : 99;
    if (d >= base) return false;
    if (x > (~0ull - (uint64_t)d) / (uint64_t)base) return false;
    x = x * (uint64_t)base + (uint64_t)d;
  }
  *v = x;
  return true;
}
// one side of a comparison (decodeSelector, merylCommandBuilder-isSelect.C:141-158)
inline std::string sel_side(const std::string &s, int32_t *index, uint64_t *constant) {
  for (const char *w : {"distinct=", "word-freq=", "word-frequency=", "threshold="})
    if (s.compare(0, strlen(w), w) == 0)
      return std::string("'") + w + "' inside a selector is not offered here: it stays on the value operations";
  uint64_t v = 0;
  if (s[0] == '@') {
    if (!sel_integer(s.substr(1), &v) || v > 0x7fffffffull) return "'" + s + "' is not an input index";
    *index = (int32_t)v; *constant = 0;
    return "";
  }
  if (!sel_integer(s[0] == '#' ? s.substr(1) : s, &v)) return "'" + s + "' is not an integer";
  *index = -1; *constant = v;
  return "";
}
// "[lhs]REL rhs" -> the term's relation and sides
inline std::string sel_comparison(const std::string &s, mgc_select_term *t) {
  size_t rb = 0;
  uint32_t rl = 0;
  int rel = 0;
  while (rb < s.size() && !sel_is_relation(s.c_str() + rb, &rl, &rel)) rb++;
  if (rb >= s.size()) return "no comparison operator found, expecting one of '==', 'eq', '!=', 'ge', '<', etc.";
  t->relation = (uint8_t)rel;
  const std::string lhs = s.substr(0, rb), rhs = s.substr(rb + rl);
  if (rhs.empty()) return "no second argument to the comparison operator";
  std::string m;
  if (lhs.empty()) { t->lhs_index = 0; t->lhs_constant = 0; }
  else if (!(m = sel_side(lhs, &t->lhs_index, &t->lhs_constant)).empty()) return m;
  return sel_side(rhs, &t->rhs_index, &t->rhs_constant);
}
// the list of an input: selector (isInputSelector, merylCommandBuilder-isSelect.C:357-477; finalizeSelectorInputs, merylSelector.C:189-246)
inline std::string sel_input_list(const std::string &s, uint32_t n_inputs, mgc_select_term *t) {
  const uint32_t N = n_inputs > 32 ? 32 : n_inputs;
  uint64_t counts = 0;
  bool any = false, some_count = false;
  size_t at = 0;
  while (at <= s.size()) {
    size_t end = s.find_first_of(":,", at);
    if (end == std::string::npos) end = s.size();
    const std::string w = s.substr(at, end - at);
    at = end + 1;
    if (w.empty()) continue;
    const size_t dash = w.find('-');
    const std::string a = w.substr(0, dash), b = dash == std::string::npos ? "" : w.substr(dash + 1);
    uint64_t x = 0, y = 0;
    auto count_range = [&](uint64_t lo, uint64_t hi) -> std::string {
      if (lo == 0) return "there is no 0th input";
      if (hi > N) return "cannot occur in " + std::to_string(hi) + " inputs; there are only " + std::to_string(n_inputs) + " inputs";
      for (uint64_t c = lo; c <= hi; c++) counts |= 1ull << c;
      some_count = true;
      return "";
    };
    auto index_range = [&](uint64_t lo, uint64_t hi) -> std::string {
      if (lo == 0) return "there is no 0th input";
      if (hi > N) return "input " + std::to_string(hi) + " does not exist; there are only " + std::to_string(n_inputs) + " inputs";
      for (uint64_t i = lo; i <= hi; i++) t->required_mask |= 1u << (i - 1);
      return "";
    };
    std::string m;
    if (w == "all") m = count_range(N, N);
    else if (w == "any") any = true;
    else if (w == "first") m = index_range(1, 1);
    else if (dash == std::string::npos && a[0] == '@' && sel_integer(a.substr(1), &x)) m = index_range(x, x);
    else if (a[0] == '@' && !b.empty() && b[0] == '@' && sel_integer(a.substr(1), &x) && sel_integer(b.substr(1), &y)) m = index_range(x, y);
    else if (dash == std::string::npos && sel_integer(a, &x)) m = count_range(x, x);
    else if (sel_integer(a, &x) && b == "all") m = count_range(x, x > N ? x : N);      // in at least x inputs
    else if (sel_integer(a, &x) && sel_integer(b, &y)) m = count_range(x, y);
    else m = "unknown word '" + w + "'";
    if (!m.empty()) return m;
  }
  if (any || !some_count) counts |= (N >= 63 ? ~0ull : ((1ull << (N + 1)) - 1)) & ~1ull;   // 'any' == '1-all', the default
  t->count_mask = counts;
  return "";
}

// mgc_select_parse: empty string = parsed, *n_terms terms written (at most cap)
inline std::string select_parse(const char *const *words, uint32_t n_words, uint32_t n_inputs, mgc_select_term *terms, uint32_t cap,
                                uint32_t *n_terms) {
  uint32_t n = 0;
  bool negate = false, product_empty = true;
  for (uint32_t i = 0; i < n_words; i++) {
    if (!words[i]) return "a null word";
    const std::string w(words[i]);
    if (w == "not") { negate = !negate; continue; }
    if (w == "and") continue;
    if (w == "or") {
      if (negate) return "'not' before 'or': nothing to negate";
      if (product_empty) return "'or' after an empty product: a term must come first";
      terms[n - 1].ends_product = 1;
      product_empty = true;
      continue;
    }
    mgc_select_term t;
    memset(&t, 0, sizeof(t));
    t.lhs_index = t.rhs_index = -1;
    t.negate = negate ? 1 : 0;
    std::string m;
    if (w.compare(0, 6, "value:") == 0) { t.quantity = MGC_SEL_VALUE; m = sel_comparison(w.substr(6), &t); }
    else if (w.compare(0, 6, "label:") == 0) { t.quantity = MGC_SEL_LABEL; m = sel_comparison(w.substr(6), &t); }
    else if (w.compare(0, 6, "bases:") == 0) {
      t.quantity = MGC_SEL_BASES;
      const size_t colon = w.find(':', 6);
      if (colon == std::string::npos) m = "expecting bases:<letters>:<comparison>";
      else {
        for (size_t j = 6; j < colon && m.empty(); j++)
          switch (w[j]) {
            case 'a': case 'A': t.base_mask |= MGC_SEL_BASE_A; break;
            case 'c': case 'C': t.base_mask |= MGC_SEL_BASE_C; break;
            case 't': case 'T': t.base_mask |= MGC_SEL_BASE_T; break;
            case 'g': case 'G': t.base_mask |= MGC_SEL_BASE_G; break;
            default: m = std::string("invalid 'bases' letter '") + w[j] + "'";
          }
        if (m.empty()) m = sel_comparison(w.substr(colon + 1), &t);
      }
    } else if (w.compare(0, 6, "input:") == 0) {
      t.quantity = MGC_SEL_INPUT;
      t.lhs_index = t.rhs_index = 0;
      m = sel_input_list(w.substr(6), n_inputs, &t);
    } else m = "not a selector word";
    if (!m.empty()) return "selector '" + w + "': " + m;
    if (n >= MGC_SELECT_MAX_TERMS) return "a selector has at most " + std::to_string(MGC_SELECT_MAX_TERMS) + " terms";
    if (n >= cap) return "room for " + std::to_string(cap) + " terms only";
    m = select_check(&t, 1, n_inputs);
    if (!m.empty()) return "selector '" + w + "': " + m.substr(m.find(": ") + 2);
    terms[n++] = t;
    negate = false;
    product_empty = false;
  }
  if (negate) return "a dangling 'not': no selector follows it";
  if (n && product_empty) return "a dangling 'or': no selector follows it";
  *n_terms = n;
  return "";
}

}  // namespace mgc
