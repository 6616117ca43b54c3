"""Shared by test_assign.py and test_assign_host.py: meryl2's value assignment (include/meryl_gpu_count.h: MGC_ASSIGN_*;
merylOpCompute::findOutputValue, src/meryl2/merylOpCompute.C:136-282; merylCommandBuilder-isAssign.C:44-103) as a short Python
statement in exact integer arithmetic -- the value a rule gives, the text after value= -> (code, constant) -- and the merge
operations with an assignment, a label operation and a program applied to lists of (keys, values, labels)."""
import re

import label_helpers as LH
import select_helpers as S

M32 = 0xFFFFFFFF
NONE, SET, FIRST, SELECTED, MIN, MAX, ADD, SUB, MUL, DIV, DIVZ, MOD, COUNT = range(13)
WORDS = {"first": FIRST, "selected": SELECTED, "min": MIN, "max": MAX, "add": ADD, "sum": ADD, "sub": SUB, "dif": SUB, "mul": MUL,
         "div": DIV, "divzero": DIVZ, "mod": MOD, "rem": MOD, "count": COUNT}
NO_CONSTANT = ("first", "selected", "count")
DEFAULT_CONSTANT = {MIN: M32, MUL: 1, DIV: 1, DIVZ: 1}                # every other code: 0
CODE_WORD = {SET: "set", FIRST: "first", SELECTED: "selected", MIN: "min", MAX: "max", ADD: "add", SUB: "sub", MUL: "mul", DIV: "div",
             DIVZ: "divzero", MOD: "mod", COUNT: "count"}


def divz(x, d):
    """one step of divzero: round half up of x / d in exact arithmetic"""
    if d == 0:
        return 0
    if x < d:
        return 1
    return (2 * x + d) // (2 * d)


def value_of(word, c, vals):
    """the value of a written k-mer: vals = the values of the active inputs in input order, c = the constant (cut to 32 bits);
    word: a word of WORDS, "set" or an MGC_ASSIGN_* code"""
    code = word if isinstance(word, int) else SET if word == "set" else WORDS[word]
    c &= M32
    if code == SET:
        return c
    if code in (FIRST, SELECTED):
        return vals[0]
    if code == MIN:
        return min([c] + list(vals))
    if code == MAX:
        return max([c] + list(vals))
    if code == ADD:
        return min(c + sum(vals), M32)
    if code == SUB:
        v = vals[0]
        for x in list(vals[1:]) + [c]:
            v = v - x if v > x else 0
        return v
    if code == MUL:
        v = c
        for x in vals:
            v = min(v * x, M32)                                      # 0 stays 0
        return v
    if code == DIV:
        v = vals[0]
        for x in list(vals[1:]) + [c]:
            v = v // x if x else 0
        return v
    if code == DIVZ:
        v = vals[0]
        for x in list(vals[1:]) + [c]:
            v = divz(v, x)
        return v
    if code == MOD:
        q, r = vals[0], 0
        for x in list(vals[1:]) + [c]:
            if x:
                r, q = r + q % x, q // x
            else:
                r, q = r + q, 0
        return r & M32
    if code == COUNT:
        return len(vals)
    raise ValueError(word)


def _integer(s):
    if re.fullmatch(r"0[xX][0-9a-fA-F]+", s):
        return int(s, 16)
    if re.fullmatch(r"0[bB][01]+", s):
        return int(s[2:], 2)
    if re.fullmatch(r"[0-9]+", s):
        return int(s)
    raise ValueError("'%s' is not an integer" % s)


def parse_value(text):
    """what follows value= -> (MGC_ASSIGN_* code, constant); ValueError for what mgc_value_assign_parse refuses"""
    if not text:
        raise ValueError("nothing after value=")
    word, hash_, const = text.partition("#")
    if word == "":
        code = SET
    elif word in WORDS:
        code = WORDS[word]
    else:
        raise ValueError("unknown word '%s'" % word)
    if not hash_:
        return code, DEFAULT_CONSTANT.get(code, 0)
    if word in NO_CONSTANT:
        raise ValueError("'%s' takes no constant" % word)
    c = _integer(const)
    if c > M32:
        raise ValueError("a constant above 2^32-1")
    return code, c


def present(op, idx0, n, N):
    """the presence rule an operation keeps under an assignment (merylCommandBuilder-processText.C:384-442)"""
    if op in (0, 1, 2, 10):
        return True
    if op in (3, 4, 5, 6):
        return n == N
    if op == 7:
        return idx0 == 0
    if op == 8:
        return idx0 == 0 and n == 1
    return n == 1


def label_under(value, label_word, label_constant, L, V, merge_op):
    """findOutputLabel on a node with an assignment: SELECTED (named, or the default of *-min / *-max) follows the assignment"""
    code = value[0] if isinstance(value[0], int) else SET if value[0] == "set" else WORDS[value[0]]
    word = label_word
    if word == "default":
        word = LH.DEFAULT_OF_MERGE[merge_op] if merge_op is not None else "first"
    if word == "selected":
        return LH.label_of("selected", label_constant, L, V, merge_op=1 if code == MIN else 2 if code == MAX else 0)
    return LH.label_of(word, label_constant, L, V, merge_op=merge_op)


def groups_of(inputs):
    """[(keys as ints, values, labels)] -> [(key, [(input index, value, label)] in input order)], keys ascending"""
    act = {}
    for i, (keys, vals, labs) in enumerate(inputs):
        for key, v, l in zip(keys, vals, labs):
            act.setdefault(key, []).append((i, v, l))
    return [(key, act[key]) for key in sorted(act)]


def merge_assigned(inputs, op, value, label, terms, k, value_filter=None, groups=None, stats=None):
    """inputs: [(keys as ints, values, labels)] with ascending distinct keys; value: (word or code, constant) or None (the
    operation's own rule: select_helpers.merge_selected); label: (word, constant); value_filter: (MGC_VALUE_* 0..5, threshold) of a
    value filter node, whose one input `op` is then ignored for; groups: groups_of(inputs), when the caller keeps it; stats: a dict
    that counts the k-mers the presence rule passed ("present"), of those the ones dropped for a zero value ("zero"), the ones
    whose value is 2^32-1 ("saturated") and the ones written ("kept") -> (keys, values, labels)"""
    if value is None or value[0] in (NONE, "none"):
        assert value_filter is None
        return S.merge_selected(inputs, op, label[0], label[1], terms, k)
    N = len(inputs)
    out = ([], [], [])
    stats = stats if stats is not None else {}
    for key, a in groups if groups is not None else groups_of(inputs):
        vals = [v for _, v, _ in a]
        if value_filter is None and not present(op, a[0][0], len(a), N):
            continue
        stats["present"] = stats.get("present", 0) + 1
        v = value_of(value[0], value[1], vals)
        if v == 0:                                                   # merylOp-nextMer.C:119
            stats["zero"] = stats.get("zero", 0) + 1
            continue
        if v == M32:
            stats["saturated"] = stats.get("saturated", 0) + 1
        if value_filter is not None and LH.sel_value(value_filter[0], v, value_filter[1]) == 0:
            continue
        lab = label_under(value, label[0], label[1], [l for _, _, l in a], vals, None if value_filter is not None else op)
        if S.keep(terms, k, key, v, lab, {i + 1: (vv, ll) for i, vv, ll in a}):
            stats["kept"] = stats.get("kept", 0) + 1
            for col, x in zip(out, (key, v, lab)):
                col.append(x)
    return out
