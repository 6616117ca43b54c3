// mgc_value.hpp -- the value of a written k-mer from the values of the inputs that hold it: meryl2's
// merylOpCompute::findOutputValue (src/meryl2/merylOpCompute.C:136-282), named on the command line by value=<word>[#c]
// (merylCommandBuilder::isAssignValue, src/meryl2/merylCommandBuilder-isAssign.C:44-103); the rules, with the line each comes
// from, are in include/meryl_gpu_count.h (MGC_ASSIGN_*).  Shared by the kernels (mgc_merge_many.hip), the host code that parses
// and checks an assignment (mgc_api.cpp, mgc_eval.cpp) and a stand-alone host program (tests/host/value_host.cpp): plain C++,
// no HIP header needed.
#pragma once
#include "mgc_label.hpp"

#include <cstdint>
#include <string>

#if defined(__HIPCC__)
#define MGC_VALUE_FN __host__ __device__ __forceinline__
#else
#define MGC_VALUE_FN inline
#endif

namespace mgc {

// kernel codes: the MGC_ASSIGN_* values once SELECTED is resolved (value_kernel_op)
constexpr int VOP_NONE = 0, VOP_SET = 1, VOP_FIRST = 2, VOP_MIN = 4, VOP_MAX = 5, VOP_ADD = 6, VOP_SUB = 7, VOP_MUL = 8, VOP_DIV = 9,
              VOP_DIVZ = 10, VOP_MOD = 11, VOP_COUNT = 12;
constexpr uint32_t VALUE_MAX = 0xFFFFFFFFu;                 // kmvalumax

// MGC_ASSIGN_* -> the code the kernels take; SELECTED is FIRST: the reference's valueSelected takes _acta[0] under a
// `#warning wrong` (:149-152), and the input an assignment "selects" is the first active one; -1: unknown
inline int value_kernel_op(int assign) {
  if (assign < 0 || assign > 12) return -1;
  return assign == 3 ? VOP_FIRST : assign;
}
// the constant isAssignValue gives a word that names none (merylCommandBuilder-isAssign.C:78-91)
inline uint64_t value_default_constant(int assign) {
  const int vop = value_kernel_op(assign);
  if (vop == VOP_MIN) return VALUE_MAX;
  if (vop == VOP_MUL || vop == VOP_DIV || vop == VOP_DIVZ) return 1;
  return 0;
}
// whether a pass needs the inputs' values to know what the rule gives (a zero result is not written)
MGC_VALUE_FN bool value_needs_values(int vop) { return vop != VOP_SET && vop != VOP_COUNT; }

// label_kernel_op (mgc_label.hpp) on a node with an assignment: SELECTED -- named, or what DEFAULT means under *-min / *-max --
// follows the assignment instead of the operation: min -> LOP_SEL_MIN, max -> LOP_SEL_MAX, anything else -> LOP_FIRST
inline int label_kernel_op_assigned(bool is_merge, int op, int label_op, int assign) {
  const int lop = label_kernel_op(is_merge, op, label_op);
  const int vop = value_kernel_op(assign);
  if (lop < 0 || vop <= VOP_NONE) return lop;
  const bool selected = label_op == 12 || (label_op == 0 && is_merge && (op == 1 || op == 2 || op == 4 || op == 5));
  if (!selected) return lop;
  return vop == VOP_MIN ? LOP_SEL_MIN : vop == VOP_MAX ? LOP_SEL_MAX : LOP_FIRST;
}

// one step of valueDivZ (:227-245): d == 0 -> 0; x < d -> 1 (also when x is 0, as there); otherwise round(x / (double)d), which
// for 32-bit operands is (2x + d) / 2d in integers (the quotient is at least 1 / 2d away from a half, far more than a double's
// rounding error; tests/host/value_host.cpp compares the two forms)
MGC_VALUE_FN uint32_t value_divz(uint32_t x, uint32_t d) {
  if (d == 0) return 0;
  if (x < d) return 1;
  return (uint32_t)((2ull * x + d) / (2ull * d));
}

// a value filter node (MGC_VALUE_LESS_THAN .. MGC_VALUE_NOT_EQUAL_TO) under an assignment tests the assigned value: the
// reference's filter is a value: term on the output k-mer (merylCommandBuilder-processText.C:466-468); fop < 0: no filter
MGC_VALUE_FN bool value_filter_keeps(int fop, uint32_t v, uint64_t c) {
  switch (fop) {
    case 0:  return (uint64_t)v <  c;
    case 1:  return (uint64_t)v >  c;
    case 2:  return (uint64_t)v >= c;
    case 3:  return (uint64_t)v <= c;
    case 4:  return (uint64_t)v == c;
    case 5:  return (uint64_t)v != c;
    default: return true;
  }
}

// begin(c), then step(vop, V[j]) over the active inputs in input order, then finish(vop, c, number of active inputs) is the
// value; all arithmetic on 32-bit kmvalu
struct ValueAcc {
  unsigned int v, r; bool any;
  MGC_VALUE_FN void begin(unsigned int c) { v = c; r = 0; any = false; }
  // the remainder chain of valueMod (:248-275): v is q, r accumulates mod 2^32
  MGC_VALUE_FN void mod_step(unsigned int d) {
    if (d > 0) { const unsigned int qt = v / d; r += v - qt * d; v = qt; }
    else { r += v; v = 0; }
  }
  MGC_VALUE_FN void step(int vop, unsigned int V) {
    switch (vop) {
      case VOP_FIRST: if (!any) v = V; break;                                                   // :154-157
      case VOP_MIN:   v = V < v ? V : v; break;                                                 // :159-163
      case VOP_MAX:   v = V > v ? V : v; break;                                                 // :165-169
      case VOP_ADD:   v = (VALUE_MAX - v < V) ? VALUE_MAX : v + V; break;                       // :171-178
      case VOP_SUB:   if (!any) v = V; else v = v > V ? v - V : 0u; break;                      // :180-187
      // the reference divides kmvalumax by the running value (:199), zero included; here a running value of 0 stays 0
      case VOP_MUL:   v = (v == 0) ? 0u : (VALUE_MAX / v < V) ? VALUE_MAX : v * V; break;
      case VOP_DIV:   if (!any) v = V; else v = V > 0 ? v / V : 0u; break;                      // :206-213
      case VOP_DIVZ:  if (!any) v = V; else v = value_divz(v, V); break;                        // :227-236
      case VOP_MOD:   if (!any) v = V; else mod_step(V); break;                                 // :248-261
      default:        break;                                                                    // SET, COUNT
    }
    any = true;
  }
  MGC_VALUE_FN unsigned int finish(int vop, unsigned int c, unsigned int n_active) {
    switch (vop) {
      case VOP_SET:   return c;                                                                 // :145-147
      case VOP_SUB:   return v > c ? v - c : 0u;                                                // :189-192
      case VOP_DIV:   return c > 0 ? v / c : 0u;                                                // :215-218
      case VOP_DIVZ:  return value_divz(v, c);                                                  // :238-243
      case VOP_MOD:   mod_step(c); return r;                                                    // :263-273
      case VOP_COUNT: return n_active;                                                          // :278-280
      default:        return v;
    }
  }
};

// ---- host side: the text after value= ------------------------------------------------------------------------------------
// an unsigned integer: decimal, 0x hexadecimal, 0b binary; the whole string (what the selector parser takes)
inline bool value_integer(const std::string &s, uint64_t *v) {
  if (s.empty()) return false;
  int base = 10;
  size_t at = 0;
  if (s.size() > 2 && s[0] == '0' && (s[1] == 'x' || s[1] == 'X')) { base = 16; at = 2; }
  else if (s.size() > 2 && s[0] == '0' && (s[1] == 'b' || s[1] == 'B')) { base = 2; at = 2; }
  uint64_t x = 0;
  for (; at < s.size(); at++) {
    const char c = s[at];
    const int d = (c >= '0' && c <= '9') ? c - '0' : (c >= 'a' && c <= 'f') ? c - 'a' + 10 : (c >= 'A' && c <= 'F') ? c - 'A' + 10 : 99;
    if (d >= base) return false;
    if (x > (~0ull - (uint64_t)d) / (uint64_t)base) return false;
    x = x * (uint64_t)base + (uint64_t)d;
  }
  *v = x;
  return true;
}

// mgc_value_assign_parse: `word`, `word#c` or `#c` -> the MGC_ASSIGN_* code and the constant (the word's default when it names
// none); empty string = parsed
inline std::string value_assign_parse(const char *text, int *assign, uint64_t *constant) {
  static const struct { const char *word; int code; bool takes_constant; } words[] = {
    {"first", 2, false}, {"selected", 3, false}, {"min", 4, true}, {"max", 5, true}, {"add", 6, true}, {"sum", 6, true}, {"sub", 7, true},
    {"dif", 7, true}, {"mul", 8, true}, {"div", 9, true}, {"divzero", 10, true}, {"mod", 11, true}, {"rem", 11, true}, {"count", 12, false}};
  if (!text || !text[0]) return "expecting value=<word>, value=<word>#<constant> or value=#<constant>";
  const std::string s(text);
  const size_t hash = s.find('#');
  const std::string word = s.substr(0, hash);
  int code = -1;
  bool takes = true;
  if (word.empty()) code = 1;
  for (const auto &e : words) if (word == e.word) { code = e.code; takes = e.takes_constant; }
  if (code < 0) return "Unknown assign:value=<parameter> in 'value=" + s + "'.";
  uint64_t c = value_default_constant(code);
  if (hash != std::string::npos) {
    if (!takes) return "'value=" + word + "' takes no constant";
    if (!value_integer(s.substr(hash + 1), &c)) return "'" + s.substr(hash + 1) + "' in 'value=" + s + "' is not an integer";
    if (c > VALUE_MAX) return "the constant of 'value=" + s + "' does not fit a 32-bit value";
  }
  *assign = code;
  *constant = c;
  return "";
}

}  // namespace mgc
