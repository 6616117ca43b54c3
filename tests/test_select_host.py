"""Selectors on a machine without a GPU: the new symbols are exported and declared; the evaluator the kernels run
(meryl_amd/csrc/mgc_selector.hpp) agrees with the Python statement of it (select_helpers) in a stand-alone host program built with
the address and undefined-behaviour sanitizers; mgc_select_parse agrees with the model's parser on a table of words and refuses
what it must; the device entry points and mgc_db_eval_selected refuse every violation before any device call and before any
output directory exists; the command line refuses malformed selectors and the words it does not offer."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import select_helpers as S
from test_db_eval_host import tiny_db

NEW_SYMBOLS = ("mgc_select_parse", "mgc_select_check", "mgc_dev_merge_many_count_selected", "mgc_dev_merge_many_emit_selected",
               "mgc_dev_select_count_selected", "mgc_dev_select_emit_selected", "mgc_db_eval_selected")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = S.M64


def test_new_symbols_are_exported_and_declared(native_lib):
    from meryl_amd import capi
    headers = open(os.path.join(ROOT, "include", "meryl_gpu_count.h")).read() + open(os.path.join(ROOT, "include", "meryl_db.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(native_lib, name), name
        assert name in capi.SYMBOLS, name
        assert re.search(r"\b%s\(" % name, headers), name
    assert "mgc_select_term" in headers
    for word, code in (("SEL_VALUE", 1), ("SEL_LABEL", 2), ("SEL_BASES", 3), ("SEL_INPUT", 4), ("REL_EQ", 1), ("REL_NEQ", 2), ("REL_LEQ", 3),
                       ("REL_GEQ", 4), ("REL_LT", 5), ("REL_GT", 6), ("SELECT_MAX_TERMS", 16)):
        assert re.search(r"#define MGC_%s\s+%d\b" % (word, code), headers), word
        assert getattr(capi, word) == code
    assert (S.VALUE, S.LABEL, S.BASES, S.INPUT, S.MAX_TERMS) == (capi.SEL_VALUE, capi.SEL_LABEL, capi.SEL_BASES, capi.SEL_INPUT, capi.SELECT_MAX_TERMS)
    assert ctypes.sizeof(capi.SelectTerm) == 48                          # 16 of them beside the 1 KiB descriptor: inside the 4 KiB argument segment
    assert ctypes.sizeof(capi.EvalNodeSelected) == ctypes.sizeof(capi.EvalNodeLabelled) + 8


# ---- the evaluator ----------------------------------------------------------------------------------------------------------
def kmer_of(bases):
    """A 0, C 1, T 2, G 3; the first base most significant"""
    x = 0
    for b in bases:
        x = (x << 2) | "ACTG".index(b)
    return x


def grid():
    """[(k, key, out_value, out_label, present {index: (value, label)}, terms)]"""
    rng = np.random.default_rng(72)
    cases = []
    big = lambda: int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(0, 2))           # noqa: E731
    T = S.term
    # every VALUE / LABEL relation x negate x sides from constant, output and input, present or absent
    worlds = [(7, 0b101, {1: (3, 0b001), 2: (7, 0b101), 4: (9, M64)}),
              (0xFFFFFFFF, M64, {2: (0xFFFFFFFF, 1 << 63), 3: (1, 0), 32: (5, 5)}),
              (1, 0, {1: (1, 0)})]
    sides = [(-1, 7), (-1, 0), (-1, (1 << 32) + 7), (-1, M64), (0, 0), (1, 0), (2, 0), (3, 0), (4, 0), (32, 0)]
    for q in (S.VALUE, S.LABEL):
        for rel in range(1, 7):
            for neg in (0, 1):
                for li, lc in sides:
                    for ri, rc in sides:
                        if li == ri and li >= 0:
                            continue
                        for ov, ol, present in worlds:
                            cases.append((21, 12345, ov, ol, present, [T(q, rel, neg, 0, 0, li, ri, lc, rc)]))
    # BASES: k = 15, 32, 33, 64; all-A, all-G, all-C, all-T and random k-mers; every letter mask, relation, negate, side order
    for k in (15, 32, 33, 64):
        kmers = [kmer_of("A" * k), kmer_of("G" * k), kmer_of("C" * k), kmer_of("T" * k), kmer_of(("ACGT" * 16)[:k])]
        kmers += [int.from_bytes(rng.bytes(16), "little") & ((1 << (2 * k)) - 1) for _ in range(3)]
        for key in kmers:
            for mask in range(1, 16):
                want = S.count_bases(key, k, mask)
                for rel in range(1, 7):
                    for neg in (0, 1):
                        c = [want, max(want - 1, 0), want + 1, 0, k][(rel + neg + mask) % 5]
                        cases.append((k, key, 1, 0, {1: (1, 0)}, [T(S.BASES, rel, neg, 0, mask, 0, -1, 0, c)]))
                        cases.append((k, key, 1, 0, {1: (1, 0)}, [T(S.BASES, rel, neg, 0, mask, -1, 0, c, 0)]))
    # INPUT: count masks with bit 0, bit N and bit 32; required masks inside and outside the presence
    presences = [{}, {1: (1, 1)}, {2: (1, 1), 3: (1, 1)}, {i: (i, i) for i in range(1, 33)}, {i: (i, i) for i in range(1, 33) if i != 17}, {32: (1, 1)}]
    for present in presences:
        n = len(present)
        for cm in (1, 1 << n, 1 << 32, (1 << 33) - 1, ((1 << 33) - 1) & ~(1 << n), 0, 0b110, 1 << 31):
            for req in (0, 1, 0b110, 1 << 31, 1 << 16, 0xFFFFFFFF):
                for neg in (0, 1):
                    cases.append((21, 99, n, 0, present, [T(S.INPUT, 0, neg, 0, 0, -1, -1, 0, 0, cm, req)]))
    # sums of products: random programs of up to 16 terms
    for _ in range(600):
        n = int(rng.integers(0, 17))
        present = {i: (int(rng.integers(1, 6)), int(rng.integers(0, 8))) for i in range(1, 6) if rng.integers(0, 2)}
        terms = []
        for j in range(n):
            q = int(rng.integers(1, 5))
            neg, ends = int(rng.integers(0, 2)), int(rng.integers(0, 3) == 0)
            if q in (S.VALUE, S.LABEL):
                li, ri = [int(x) for x in rng.choice([-1, 0, 1, 2, 3, 4, 5], 2, replace=False)]
                terms.append(T(q, int(rng.integers(1, 7)), neg, ends, 0, li, ri, int(rng.integers(0, 8)), int(rng.integers(0, 8))))
            elif q == S.BASES:
                terms.append(T(q, int(rng.integers(1, 7)), neg, ends, int(rng.integers(1, 16)), 0, -1, 0, int(rng.integers(0, 22))))
            else:
                terms.append(T(q, 0, neg, ends, 0, -1, -1, 0, 0, int(rng.integers(0, 64)), int(rng.integers(0, 32))))
        cases.append((21, big() & ((1 << 42) - 1), int(rng.integers(1, 6)), int(rng.integers(0, 8)), present, terms))
    return cases


def test_evaluator_on_the_host_against_the_model(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "select_host")
    c = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        os.path.join(ROOT, "tests", "host", "select_host.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert c.returncode == 0, c.stderr
    cases = grid()
    lines, want = [], []
    for k, key, ov, ol, present, terms in cases:
        mask = sum(1 << (i - 1) for i in present)
        f = ["%x %x %x %x %x %x" % (k, key >> 64, key & M64, ov, ol, mask)]
        f += ["%x %x" % present[i] for i in sorted(present)]
        f.append("%x" % len(terms))
        for t in terms:
            f.append("%x %x %x %x %x %x %x %x %x %x %x" % (t["quantity"], t["relation"], t["negate"], t["ends_product"], t["base_mask"], t["lhs_index"] + 1,
                                                          t["rhs_index"] + 1, t["lhs_constant"], t["rhs_constant"], t["count_mask"], t["required_mask"]))
        lines.append(" ".join(f))
        want.append(int(S.keep(terms, k, key, ov, ol, present)))
    p = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    got = p.stdout.split("\n")[:-1]
    assert len(got) == len(want) > 10000
    for line, g, w in zip(lines, got, want):
        assert int(g.split()[0]) == w, (line, g, w)
    assert 0.2 < sum(want) / len(want) < 0.8                             # the grid decides both ways
    # the absent-input rule itself: false with and without `not`
    for neg in (0, 1):
        assert not S.keep([S.term(S.VALUE, S.GT, neg, 0, 0, 2, 1)], 21, 5, 1, 0, {1: (5, 0)})
    assert S.keep([S.term(S.VALUE, S.GT, 1, 0, 0, 2, 1)], 21, 5, 1, 0, {1: (5, 0), 2: (5, 0)})


# ---- the parser -------------------------------------------------------------------------------------------------------------
GOOD_WORDS = [
    (["value:ge5"], 1), (["value:>=5"], 3), (["value:@2>@1"], 2), (["value:@2gt@1"], 2), (["value:#7<@3"], 3), (["value:7lt@3"], 3),
    (["value:==0x10"], 1), (["value:=3"], 1), (["value:eq3"], 1), (["value:!=3"], 1), (["value:<>3"], 1), (["value:ne3"], 1), (["value:<=3"], 1),
    (["value:le3"], 1), (["value:<3"], 1), (["value:>3"], 1), (["value:@1>=#4294967295"], 1),
    (["label:==#5"], 2), (["label:eq0b101"], 2), (["label:@1ne@2"], 2), (["label:@2<=0xFFFFFFFFFFFFFFFF"], 2),
    (["bases:gc:ge12"], 2), (["bases:GC:ge12"], 1), (["bases:a:eq0"], 1), (["bases:acgt:<=21"], 1), (["bases:t:3<@0"], 1),
    (["input:3-all"], 4), (["input:2:@1"], 3), (["input:all"], 8), (["input:any"], 2), (["input:1"], 1), (["input:2-3"], 5), (["input:first"], 2),
    (["input:@1-@3,2-all"], 4), (["input:@1:@32"], 32), (["input:32"], 32), (["input:1-all"], 32), (["input:"], 3), (["input:any:@2"], 3),
    (["input:2-all", "value:ge2"], 3), (["input:2-all", "and", "value:ge2"], 3), (["not", "value:@2>@1"], 2), (["not", "not", "value:>1"], 1),
    (["bases:gc:ge12", "or", "label:eq5"], 2), (["value:>1", "or", "not", "input:all", "or", "bases:a:lt3", "label:@1==@2"], 2),
    (["value:>%d" % i for i in range(16)], 1),
    ([], 2),
]
BAD_WORDS = {
    "an index above the input count": (["value:@3>1"], 2),
    "an index above the input count on the right": (["label:==@5"], 4),
    "@0 in an input list": (["input:@0"], 2),
    "@0 in an input range": (["input:@0-@2"], 2),
    "a required input above the count": (["input:@3"], 2),
    "a count above the inputs": (["input:5"], 4),
    "a count range above the inputs": (["input:2-5"], 4),
    "at least more than the inputs": (["input:5-all"], 4),
    "count zero": (["input:0"], 4),
    "both sides the same input": (["value:@1>@1"], 2),
    "both sides constants": (["value:3>1"], 2),
    "both sides the output": (["label:==@0"], 2),
    "bases naming an input": (["bases:gc:@1>3"], 2),
    "bases naming an input on the right": (["bases:gc:>@1"], 2),
    "bases without letters": (["bases::>3"], 2),
    "bases with another letter": (["bases:gn:>3"], 2),
    "bases without a comparison": (["bases:gc"], 2),
    "17 terms": (["value:>1"] * 17, 1),
    "an empty product before or": (["or", "value:>1"], 1),
    "or or": (["value:>1", "or", "or", "value:>2"], 1),
    "a dangling not": (["value:>1", "not"], 1),
    "not before or": (["value:>1", "not", "or", "value:>2"], 1),
    "a dangling or": (["value:>1", "or"], 1),
    "no relation": (["value:5"], 1),
    "no right side": (["value:>"], 1),
    "not a number": (["value:>five"], 1),
    "an unknown input word": (["input:most"], 2),
    "distinct= in a selector": (["value:>=distinct=0.5"], 1),
    "word-frequency= in a selector": (["value:<word-frequency=0.001"], 1),
    "threshold= in a selector": (["value:>=threshold=5"], 1),
    "not a selector word": (["values:>1"], 1),
}


def test_parser_against_the_model_and_every_refusal(native_lib):
    from meryl_amd import capi, db
    for words, n in GOOD_WORDS:
        got, want = db.parse_selector(words, n), S.parse(words, n)
        assert len(got) == len(want), words
        for c, t in zip(got, want):
            assert S.same_term(t, c), (words, t, [(f, getattr(c, f)) for f in S.FIELDS])
        arr = S.to_ctypes(want)
        assert native_lib.mgc_select_check(arr, len(want), n) == 0, words
    # what the words mean
    t, = db.parse_selector(["input:3-all"], 4)
    assert (t.count_mask, t.required_mask) == (0b11000, 0)               # in at least 3 of 4: not "inputs 3 and 4 required"
    t, = db.parse_selector(["value:ge5"], 1)
    assert (t.quantity, t.relation, t.lhs_index, t.rhs_index, t.rhs_constant) == (capi.SEL_VALUE, capi.REL_GEQ, 0, -1, 5)
    a, b = db.parse_selector(["bases:gc:ge12", "or", "label:eq5"], 2)
    assert (a.base_mask, a.ends_product, b.quantity, b.ends_product) == (2 | 8, 1, capi.SEL_LABEL, 0)
    for what, (words, n) in BAD_WORDS.items():
        with pytest.raises(ValueError):
            S.parse(words, n)
        with pytest.raises(capi.MgcError) as e:
            db.parse_selector(words, n)
        assert e.value.args and len(str(e.value)) > 20, what
    for w in ("distinct=", "word-frequency=", "threshold="):
        with pytest.raises(capi.MgcError, match="stays on the value operations"):
            db.parse_selector(["value:>=%s1" % w], 1)


def bad_programs():
    T = S.term
    return {
        "an index above the input count": ([T(S.VALUE, S.GT, 0, 0, 0, 3, -1, 0, 1)], 2),
        "a count above the inputs": ([T(S.INPUT, count_mask=1 << 3)], 2),
        "a required input above the inputs": ([T(S.INPUT, count_mask=2, required_mask=1 << 2)], 2),
        "both sides the same source": ([T(S.LABEL, S.EQ, 0, 0, 0, 1, 1)], 2),
        "both sides constants": ([T(S.VALUE, S.EQ, 0, 0, 0, -1, -1, 1, 1)], 2),
        "bases naming an input": ([T(S.BASES, S.GT, 0, 0, 2, 1, -1, 0, 3)], 2),
        "bases without letters": ([T(S.BASES, S.GT, 0, 0, 0, 0, -1, 0, 3)], 2),
        "17 terms": ([T(S.VALUE, S.GT, 0, 0, 0, 0, -1, 0, 1)] * 17, 2),
        "an unknown quantity": ([T(5, S.GT, 0, 0, 0, 0, -1, 0, 1)], 2),
        "an unknown relation": ([T(S.VALUE, 7, 0, 0, 0, 0, -1, 0, 1)], 2),
        "an index below -1": ([T(S.VALUE, S.GT, 0, 0, 0, -2, 0)], 2),
    }


def test_device_entry_points_check_their_arguments_before_any_launch(native_lib):
    from meryl_amd import capi
    L = native_lib
    n_out = ctypes.c_uint64(0)
    ok = S.to_ctypes([S.term(S.VALUE, S.GT, 0, 0, 0, 0, -1, 0, 1)])

    def many(n_inputs, op, lop, terms, n_terms, k=21, kw=1):
        m = max(n_inputs, 1)
        kp = (ctypes.c_void_p * m)(*[4096] * m)
        ns = (ctypes.c_uint64 * m)(*[8] * m)
        a = L.mgc_dev_merge_many_count_selected(kp, kp, kp, ns, n_inputs, kw, k, op, lop, 0, terms, n_terms, 4096, 1 << 30, ctypes.byref(n_out), None)
        b = L.mgc_dev_merge_many_emit_selected(kp, kp, kp, ns, n_inputs, kw, k, op, lop, 0, terms, n_terms, 4096, 1 << 30, 4096, 4096, 4096, None)
        return a, b

    def one(fop, lop, terms, n_terms, k=21, kw=1):
        a = L.mgc_dev_select_count_selected(4096, 4096, 4096, 8, kw, k, fop, 1, lop, 0, terms, n_terms, 4096, 1 << 30, ctypes.byref(n_out), None)
        b = L.mgc_dev_select_emit_selected(4096, 4096, 4096, 8, kw, k, fop, 1, lop, 0, terms, n_terms, 4096, 1 << 30, 4096, 4096, 4096, None)
        return a, b
    E = (capi.MGC_EINVAL, capi.MGC_EINVAL)
    for n_inputs, op, lop in ((0, 0, 0), (33, 0, 0), (2, 11, 0), (2, -1, 0), (2, 0, 13), (2, 0, -1), (2, 0, capi.LABEL_OPS["invert"])):
        assert many(n_inputs, op, lop, ok, 1) == E, (n_inputs, op, lop)
    assert many(2, 0, 0, ok, 1, k=0) == E and many(2, 0, 0, ok, 1, k=33) == E and many(2, 0, 0, ok, 1, k=65, kw=2) == E
    assert one(12, 0, ok, 1) == E and one(-1, 0, ok, 1) == E and one(2, 13, ok, 1) == E and one(2, 0, ok, 1, k=40) == E
    for what, (terms, n) in bad_programs().items():
        arr = S.to_ctypes(terms)
        assert many(n, 0, 0, arr, len(terms)) == E, what
        msg = L.mgc_last_error(None)
        assert msg and b"selector" in msg, (what, msg)
        if "input" not in what and "inputs" not in what:
            assert one(2, 0, arr, len(terms)) == E, what
        assert L.mgc_select_check(arr, len(terms), n) == capi.MGC_EINVAL, what
    # a value operation has one input: @2 does not exist there
    assert one(2, 0, S.to_ctypes([S.term(S.VALUE, S.GT, 0, 0, 0, 2, -1, 0, 1)]), 1) == E


def test_eval_selected_refuses_every_violation_before_the_device(native_lib, tmp_path):
    from meryl_amd import capi, db
    a, b = tiny_db(tmp_path / "a", 21), tiny_db(tmp_path / "b", 21)
    lab = tiny_db(tmp_path / "lab", 21, label_size=4)
    many = [tiny_db(tmp_path / ("m%02d" % i), 21) for i in range(33)]
    out = str(tmp_path / "out")
    before = sorted(os.listdir(tmp_path))
    N = capi.EvalNodeSelected
    DB, MERGE, VALUE = capi.NODE_DATABASE, capi.NODE_MERGE, capi.NODE_VALUE

    def raw(nodes, children, root, terms, n_terms=None, with_labels=0):
        arr = (N * len(nodes))()
        for e, (kind, op, path, first, n, first_term, nt) in zip(arr, nodes):
            e.kind, e.op, e.constant, e.path, e.first_child, e.n_children = kind, op, 1, path.encode() if path else None, first, n
            e.label_op, e.label_constant, e.first_term, e.n_terms = 0, 0, first_term, nt
        kids = (ctypes.c_uint32 * max(len(children), 1))(*children)
        return native_lib.mgc_db_eval_selected(arr, len(nodes), kids, len(children), root, S.to_ctypes(terms), len(terms) if n_terms is None else n_terms,
                                               with_labels, 0, ctypes.cast(None, capi.EVAL_SLICE_LABELLED_CB), None, -1, 2)

    def refused(what, rc):
        msg = native_lib.mgc_db_stream_error(None)
        assert rc == capi.MGC_EINVAL, (what, rc, msg)
        assert msg and b"mgc_db_eval_selected" in msg, (what, msg)
        assert sorted(os.listdir(tmp_path)) == before, what
        return msg

    two = lambda nt, first=0: [(MERGE, 0, out, 0, 2, first, nt), (DB, 0, a, 0, 0, 0, 0), (DB, 0, b, 0, 0, 0, 0)]      # noqa: E731
    for what, (terms, n) in bad_programs().items():
        assert n == 2
        msg = refused(what, raw(two(len(terms)), [1, 2], 0, terms))
        assert b"selector" in msg, (what, msg)
    good = [S.term(S.VALUE, S.GT, 0, 0, 0, 0, -1, 0, 1)]
    refused("a range outside the terms", raw(two(2), [1, 2], 0, good))
    refused("a range that starts outside the terms", raw(two(1, first=5), [1, 2], 0, good))
    refused("a program on a database", raw([(MERGE, 0, out, 0, 2, 0, 0), (DB, 0, a, 0, 0, 0, 1), (DB, 0, b, 0, 0, 0, 0)], [1, 2], 0, good))
    refused("@2 on a value operation", raw([(VALUE, 2, out, 0, 1, 0, 1), (DB, 0, a, 0, 0, 0, 0)], [1], 0, [S.term(S.VALUE, S.GT, 0, 0, 0, 2, -1, 0, 1)]))
    refused("a 33-input merge with a program", raw([(MERGE, 0, out, 0, 33, 0, 1)] + [(DB, 0, m, 0, 0, 0, 0) for m in many], list(range(1, 34)), 0, good))
    # what the other entry points refuse is refused here in the same way
    assert b"stores labels" in refused("a labelled leaf when labels do not travel", raw(two(1)[:2] + [(DB, 0, lab, 0, 0, 0, 0)], [1, 2], 0, good))
    refused("a value node with two children", raw([(VALUE, 2, out, 0, 2, 0, 1), (DB, 0, a, 0, 0, 0, 0), (DB, 0, b, 0, 0, 0, 0)], [1, 2], 0, good))
    refused("the output is also a leaf", raw([(MERGE, 0, a + "/", 0, 2, 0, 1), (DB, 0, a, 0, 0, 0, 0), (DB, 0, b, 0, 0, 0, 0)], [1, 2], 0, good))
    # through Python: the words are parsed for the node's input count before the call
    for words in (["input:@0"], ["or", "value:>1"], ["value:>1", "not"], ["value:@3>1"], ["input:3"], ["value:>1"] * 17, ["bases:gc:@1>3"],
                  ["value:@1==@1"]):
        with pytest.raises(capi.MgcError):
            db.evaluate_selected(("union-sum", a, b, {"select": words, "output": out}))
        assert sorted(os.listdir(tmp_path)) == before, words
    with pytest.raises(ValueError):
        db.build_tree_selected(("union-sum", a, b, {"selects": ["value:>1"]}))


def test_selected_tree_builder_lays_out_nodes_and_terms(native_lib):
    from meryl_amd import capi, db
    tree = ("intersect-sum", ("union", "a", "b", "c", {"select": ["input:2-all", "value:ge2"], "label": "or"}),
            ("at-least", 2, "d", {"select": "bases:gc:ge3"}), "e", {"output": "o", "select": ["value:@2>@1", "or", "not", "input:@3"]})
    arr, kids, n_kids, root, terms, n_terms = db.build_tree_selected(tree)
    lab, lkids, ln_kids, lroot = db.build_tree_labelled(("intersect-sum", ("union", "a", "b", "c", {"label": "or"}), ("at-least", 2, "d"), "e",
                                                         {"output": "o"}))
    assert (root, n_kids, list(kids)) == (lroot, ln_kids, list(lkids)) and len(arr) == len(lab)
    for e, b in zip(arr, lab):
        assert (e.kind, e.op, e.constant, e.path, e.first_child, e.n_children, e.label_op, e.label_constant) == \
               (b.kind, b.op, b.constant, b.path, b.first_child, b.n_children, b.label_op, b.label_constant)
    assert n_terms == 5
    ranges = sorted((e.first_term, e.n_terms) for e in arr if e.n_terms)
    assert ranges == [(0, 2), (2, 1), (3, 2)]                            # children first, one terms array
    top = arr[root]
    assert (top.first_term, top.n_terms) == (3, 2)
    want = S.parse(["value:@2>@1", "or", "not", "input:@3"], 3)
    assert all(S.same_term(t, terms[3 + i]) for i, t in enumerate(want))
    assert all(e.n_terms == 0 for e in arr if e.kind == capi.NODE_DATABASE)
    # a tree without "select" is the labelled tree, with no terms
    arr, _, _, _, _, n_terms = db.build_tree_selected(("union-sum", "a", "b"))
    assert n_terms == 0 and all(e.n_terms == 0 for e in arr)


@pytest.fixture(scope="module")
def meryl(native_lib):
    from meryl_amd import build
    path = build.build_cli()
    assert os.path.exists(path)
    return path


def test_cli_refuses_malformed_selectors_and_the_words_it_does_not_offer(meryl, native_lib, tmp_path):
    a, b = tiny_db(tmp_path / "a", 21), tiny_db(tmp_path / "b", 21)
    fa = tmp_path / "r.fa"
    fa.write_text(">a\nACGTACGTACGTACGTACGTACGTACGT\n")
    before = sorted(os.listdir(tmp_path))

    def run(*args):
        return subprocess.run([meryl] + [str(x) for x in args], capture_output=True, text=True, timeout=120)
    for words, text in ((["value:@3>1"], "input 3 does not exist"), (["input:@0"], "no 0th input"), (["input:3"], "there are only 2 inputs"),
                        (["value:@1==@1"], "same source"), (["bases:gc:@1>3"], "cannot name an input"), (["value:>1"] * 17, "at most 16 terms"),
                        (["or", "value:>1"], "empty product"), (["value:>1", "not"], "dangling 'not'"), (["value:>five"], "not an integer"),
                        (["value:>=distinct=0.5"], "stays on the value operations"), (["value:>=word-frequency=0.5"], "stays on the value operations"),
                        (["value:>=threshold=5"], "stays on the value operations"), (["input:most"], "unknown word 'most'")):
        p = run("union-sum", *words, a, b, "output", tmp_path / "u")
        assert p.returncode == 1 and text in p.stderr, (words, p.stderr)
        assert sorted(os.listdir(tmp_path)) == before, words
    p = run("union-sum", a, "value:>1", b, "output", tmp_path / "u")
    assert p.returncode == 1 and "must come before the inputs" in p.stderr
    p = run("k=21", "count", "value:>1", fa, "output", tmp_path / "db")
    assert p.returncode == 1 and "needs a set or value operation" in p.stderr
    p = run("print", "at-least", "2", "value:@2>1", a)
    assert p.returncode == 1 and "input 2 does not exist" in p.stderr
    assert sorted(os.listdir(tmp_path)) == before
