"""Shared by test_select.py and test_select_host.py: meryl2's selectors (include/meryl_gpu_count.h: mgc_select_term;
src/meryl2/merylSelector.C:72-156, merylCommandBuilder-isSelect.C) as a short Python statement -- what a term decides for one
k-mer, the sum of products, the words of the command line -> terms -- and the merge / value operations with a program applied
to lists of (keys, values, labels)."""
import re

import label_helpers as LH

M32 = 0xFFFFFFFF
M64 = 0xFFFFFFFFFFFFFFFF
VALUE, LABEL, BASES, INPUT = 1, 2, 3, 4
EQ, NEQ, LEQ, GEQ, LT, GT = 1, 2, 3, 4, 5, 6
MAX_TERMS = 16
LETTER_BIT = {"a": 1, "c": 2, "t": 4, "g": 8}            # bit = the 2-bit code of the letter: A 0, C 1, T 2, G 3
RELATIONS = {"==": EQ, "=": EQ, "eq": EQ, "!=": NEQ, "<>": NEQ, "ne": NEQ, "<=": LEQ, "le": LEQ, ">=": GEQ, "ge": GEQ,
             "<": LT, "lt": LT, ">": GT, "gt": GT}
FIELDS = ("quantity", "relation", "negate", "ends_product", "base_mask", "lhs_index", "rhs_index", "lhs_constant", "rhs_constant",
          "count_mask", "required_mask")


def term(quantity, relation=0, negate=0, ends_product=0, base_mask=0, lhs_index=-1, rhs_index=-1, lhs_constant=0, rhs_constant=0,
         count_mask=0, required_mask=0):
    return dict(zip(FIELDS, (quantity, relation, negate, ends_product, base_mask, lhs_index, rhs_index, lhs_constant, rhs_constant,
                             count_mask, required_mask)))


def compare(rel, x, y):
    return {EQ: x == y, NEQ: x != y, LEQ: x <= y, GEQ: x >= y, LT: x < y, GT: x > y}[rel]


def count_bases(key, k, base_mask):
    """bases of the k-mer `key` (an int, 2 bits per base, the last base in the low bits) that are a letter of base_mask"""
    return sum(1 for i in range(k) if base_mask & (1 << ((key >> (2 * i)) & 3)))


def term_true(t, k, key, out_value, out_label, present):
    """present: {input index (1-based): (value, label)} of the inputs that hold the k-mer"""
    q = t["quantity"]
    if q in (VALUE, LABEL):
        sides = []
        for idx, c in ((t["lhs_index"], t["lhs_constant"]), (t["rhs_index"], t["rhs_constant"])):
            if idx < 0:
                sides.append(c & M32 if q == VALUE else c & M64)
            elif idx == 0:
                sides.append(out_value if q == VALUE else out_label)
            elif idx in present:
                sides.append(present[idx][0 if q == VALUE else 1])
            else:
                return False                                         # an absent input: false, also under `not`
        r = compare(t["relation"], sides[0], sides[1])
    elif q == BASES:
        c = count_bases(key, k, t["base_mask"])
        r = compare(t["relation"], c, t["rhs_constant"]) if t["lhs_index"] == 0 else compare(t["relation"], t["lhs_constant"], c)
    elif q == INPUT:
        mask = sum(1 << (i - 1) for i in present)
        r = bool((t["count_mask"] >> len(present)) & 1) and (t["required_mask"] & ~mask) == 0
    else:
        return False
    return r != bool(t["negate"])


def keep(terms, k, key, out_value, out_label, present):
    if not terms:
        return True
    product = True
    for i, t in enumerate(terms):
        product = product and term_true(t, k, key, out_value, out_label, present)
        if t["ends_product"] or i + 1 == len(terms):
            if product:
                return True
            product = True
    return False


# ---- words -> terms ------------------------------------------------------------------------------------------------------
def _integer(s):
    if re.fullmatch(r"0[xX][0-9a-fA-F]+", s):
        return int(s, 16)
    if re.fullmatch(r"0[bB][01]+", s):
        return int(s[2:], 2)
    if re.fullmatch(r"[0-9]+", s):
        return int(s)
    raise ValueError("'%s' is not an integer" % s)


def _side(s):
    for w in ("distinct=", "word-freq=", "word-frequency=", "threshold="):
        if s.startswith(w):
            raise ValueError("'%s' inside a selector is not offered" % w)
    if s.startswith("@"):
        return _integer(s[1:]), 0
    v = _integer(s[1:] if s.startswith("#") else s)
    if v > M64:
        raise ValueError("too large")
    return -1, v


def _comparison(s, t):
    at = next((i for i in range(len(s)) if s[i:i + 2] in RELATIONS or s[i] in "=<>"), None)
    if at is None:
        raise ValueError("no comparison operator")
    rel = s[at:at + 2] if s[at:at + 2] in RELATIONS else s[at]
    lhs, rhs = s[:at], s[at + len(rel):]
    if not rhs:
        raise ValueError("no second argument")
    t["relation"] = RELATIONS[rel]
    t["lhs_index"], t["lhs_constant"] = (0, 0) if not lhs else _side(lhs)
    t["rhs_index"], t["rhs_constant"] = _side(rhs)


def parse(words, n_inputs):
    """-> list of terms; ValueError for what mgc_select_parse refuses"""
    N = n_inputs
    terms, negate, empty = [], False, True
    for w in words:
        if w == "not":
            negate = not negate
            continue
        if w == "and":
            continue
        if w == "or":
            if negate or empty:
                raise ValueError("'or' after nothing")
            terms[-1]["ends_product"] = 1
            empty = True
            continue
        t = term(0, negate=int(negate))
        if w.startswith("value:") or w.startswith("label:"):
            t["quantity"] = VALUE if w[0] == "v" else LABEL
            _comparison(w[6:], t)
        elif w.startswith("bases:"):
            t["quantity"] = BASES
            letters, colon, rest = w[6:].partition(":")
            if not colon or not letters or any(c not in "acgt" for c in letters.lower()):
                raise ValueError("bases:<letters>:<comparison>")
            t["base_mask"] = 0
            for c in letters.lower():
                t["base_mask"] |= LETTER_BIT[c]
            _comparison(rest, t)
            if t["lhs_index"] > 0 or t["rhs_index"] > 0:
                raise ValueError("a bases: selector cannot name an input")
        elif w.startswith("input:"):
            t["quantity"] = INPUT
            counts, any_, some = 0, False, False
            for x in [x for x in re.split("[:,]", w[6:]) if x]:
                m = None
                if x == "all":
                    lo = hi = N
                elif x == "any":
                    any_ = True
                    continue
                elif x == "first" or (m := re.fullmatch(r"@(\d+)(?:-@(\d+))?", x)):
                    a, b = (1, 1) if x == "first" else (int(m.group(1)), int(m.group(2) or m.group(1)))
                    if a == 0 or b > N:
                        raise ValueError("no such input")
                    for i in range(a, b + 1):
                        t["required_mask"] |= 1 << (i - 1)
                    continue
                elif m := re.fullmatch(r"(\d+)-all", x):
                    lo, hi = int(m.group(1)), max(int(m.group(1)), N)          # in at least n inputs
                elif m := re.fullmatch(r"(\d+)(?:-(\d+))?", x):
                    lo, hi = int(m.group(1)), int(m.group(2) or m.group(1))
                else:
                    raise ValueError("unknown word '%s'" % x)
                if lo == 0 or hi > N:
                    raise ValueError("no such count")
                some = True
                for c in range(lo, hi + 1):
                    counts |= 1 << c
            if any_ or not some:
                counts |= ((1 << (N + 1)) - 1) & ~1
            t["count_mask"] = counts
        else:
            raise ValueError("not a selector word: '%s'" % w)
        if t["quantity"] != INPUT:
            if max(t["lhs_index"], t["rhs_index"]) > N:
                raise ValueError("no such input")
            if t["lhs_index"] == t["rhs_index"]:
                raise ValueError("both sides are the same source")
        if len(terms) >= MAX_TERMS:
            raise ValueError("too many terms")
        terms.append(t)
        negate, empty = False, False
    if negate or (terms and empty):
        raise ValueError("a dangling connective")
    return terms


def same_term(t, c):
    """a model term against a capi.SelectTerm, over the fields its quantity uses"""
    names = {VALUE: FIELDS[:4] + FIELDS[5:9], LABEL: FIELDS[:4] + FIELDS[5:9], BASES: FIELDS[:9], INPUT: ("quantity", "negate", "ends_product",
             "count_mask", "required_mask")}[t["quantity"]]
    return all(int(getattr(c, n)) == int(t[n]) for n in names)


def to_ctypes(terms):
    from meryl_amd import capi
    arr = (capi.SelectTerm * max(len(terms), 1))()
    for e, t in zip(arr, terms):
        for n in FIELDS:
            setattr(e, n, t[n])
    return arr


# ---- the operations with a program -----------------------------------------------------------------------------------------
def merge_selected(inputs, op, label_word, label_constant, terms, k):
    """inputs: [(keys as ints, values, labels)] with ascending distinct keys -> (keys, values, labels) of MGC_MERGE_* `op` with the
    label operation and the program: merylOp-nextMer.C:559-612, findOutputLabel, then the selector"""
    N = len(inputs)
    act = {}
    for i, (keys, vals, labs) in enumerate(inputs):
        for key, v, l in zip(keys, vals, labs):
            act.setdefault(key, []).append((i, v, l))
    out = ([], [], [])
    for key in sorted(act):
        a = act[key]
        idx0, vals, n = a[0][0], [v for _, v, _ in a], len(a)
        v = n if op == 10 else sum(vals) & M32 if op in (0, 3) else min(vals) if op in (1, 4) else max(vals) if op in (2, 5) else vals[0]
        if op in (3, 4, 5, 6) and n != N:
            continue
        if op == 7:
            if idx0 != 0:
                continue
            alive = True
            for c in vals[1:]:
                if v > c:
                    v -= c
                else:
                    alive = False
                    break
            if not alive:
                continue
        if (op == 8 and not (n == 1 and idx0 == 0)) or (op == 9 and n != 1):
            continue
        lab = LH.label_of(label_word, label_constant, [l for _, _, l in a], vals, merge_op=op)
        if keep(terms, k, key, v, lab, {i + 1: (vv, ll) for i, vv, ll in a}):
            for col, x in zip(out, (key, v, lab)):
                col.append(x)
    return out


def value_selected(keys, vals, labs, fop, constant, label_word, label_constant, terms, k):
    out = ([], [], [])
    for key, v, l in zip(keys, vals, labs):
        nv = LH.sel_value(fop, v, constant)
        if nv == 0:
            continue
        lab = LH.label_of(label_word, label_constant, [l], [v])
        if keep(terms, k, key, nv, lab, {1: (v, l)}):
            for col, x in zip(out, (key, nv, lab)):
                col.append(x)
    return out
