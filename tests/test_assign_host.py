"""Value assignment on a machine without a GPU: the new symbols are exported, declared and bound; the rule the kernels run
(meryl_amd/csrc/mgc_value.hpp) agrees with the Python statement of it (assign_helpers) in a stand-alone host program built with the
address and undefined-behaviour sanitizers, and its integer divzero agrees with the reference's round(x / (double)d);
mgc_value_assign_parse agrees with the model's parser on a table of texts and refuses what it must; the device entry points and
mgc_db_eval_assigned refuse every violation before any device call and before any output directory exists; the command line
refuses value= where it does not belong."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import assign_helpers as A
import select_helpers as S
from test_db_eval_host import tiny_db

NEW_SYMBOLS = ("mgc_value_assign_parse", "mgc_value_default_constant", "mgc_dev_merge_many_count_assigned", "mgc_dev_merge_many_emit_assigned",
               "mgc_db_eval_assigned")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M32 = A.M32


def test_new_symbols_are_exported_declared_and_bound(native_lib):
    from meryl_amd import capi
    headers = open(os.path.join(ROOT, "include", "meryl_gpu_count.h")).read() + open(os.path.join(ROOT, "include", "meryl_db.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(native_lib, name), name
        assert name in capi.SYMBOLS, name
        assert re.search(r"\b%s\(" % name, headers), name
        assert getattr(native_lib, name).argtypes, name
    assert "mgc_eval_node_assigned" in headers
    for word, code in (("NONE", 0), ("SET", 1), ("FIRST", 2), ("SELECTED", 3), ("MIN", 4), ("MAX", 5), ("ADD", 6), ("SUB", 7), ("MUL", 8),
                       ("DIV", 9), ("DIVZ", 10), ("MOD", 11), ("COUNT", 12)):
        assert re.search(r"#define MGC_ASSIGN_%s\s+%d\b" % (word, code), headers), word
        assert getattr(A, word) == code
    for word, code in A.WORDS.items():
        assert capi.ASSIGN_OPS[word] == code, word
    assert capi.ASSIGN_OPS["none"] == 0 and capi.ASSIGN_OPS["set"] == 1
    assert ctypes.sizeof(capi.EvalNodeAssigned) == ctypes.sizeof(capi.EvalNodeSelected) + 16
    for code in range(13):
        assert native_lib.mgc_value_default_constant(code) == A.DEFAULT_CONSTANT.get(code, 0), code


# ---- the rule ---------------------------------------------------------------------------------------------------------------
CONSTANTS = (0, 1, 2, 7, 1 << 31, M32 - 1, M32)
SPECIAL = (1, 2, 3, 999, 1 << 31, M32 - 1, M32)


def grid():
    """[(code, constant, values)]: every word; the constants of the list and each word's default; 1, 2, 3 and 32 active values
    drawn from the special ones, from small ones (so that div, mod and sub do not all end at 0) and from the whole range"""
    rng = np.random.default_rng(136)
    draws = []
    for n in (1, 2, 3, 32):
        for _ in range(12):
            draws.append([int(x) for x in rng.choice(SPECIAL, n)])
            draws.append([int(x) for x in rng.integers(1, 12, n)])
            draws.append([int(x) for x in rng.integers(0, 1 << 32, n, dtype=np.uint64)])
            mixed = [int(x) for x in rng.choice(SPECIAL, n)]
            mixed[0] = int(rng.integers(1 << 20, 1 << 32))
            for j in range(1, n):
                if rng.integers(0, 2):
                    mixed[j] = int(rng.integers(0, 5))                # zero divisors and subtrahends included
            draws.append(mixed)
    # the halves of divzero: x / d exactly k + 1/2, and next to it
    for d in (2, 6, 1000, (1 << 31) - 2, M32 - 1):
        for kq in (1, 2, 3):
            x = (2 * kq + 1) * d // 2
            if x <= M32:
                draws += [[x, d], [x - 1, d], [min(x + 1, M32), d]]
    cases = []
    for code in range(1, 13):
        for c in sorted(set(CONSTANTS + (A.DEFAULT_CONSTANT.get(code, 0),))):
            for vals in draws:
                cases.append((code, c, vals))
    return cases


def test_value_rules_on_the_host_against_the_model(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "value_host")
    c = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        os.path.join(ROOT, "tests", "host", "value_host.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert c.returncode == 0, c.stderr
    cases = grid()
    lines = ["%d %d %d %s" % (code, const, len(vals), " ".join(map(str, vals))) for code, const, vals in cases]
    lines += ["13 0 1 5", "-1 0 1 5"]
    p = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    got = p.stdout.split("\n")[:-1]
    assert len(got) == len(lines) > 5000 and got[-2:] == ["refused", "refused"]
    seen = {}
    for (code, const, vals), g in zip(cases, got):
        want = A.value_of(code, const, vals)
        assert int(g.split()[1]) == want, (A.CODE_WORD[code], const, vals, g, want)
        assert int(g.split()[0]) == (A.FIRST if code == A.SELECTED else code)
        seen.setdefault(code, set()).add(0 if want == 0 else M32 if want == M32 else 1)
    # the grid decides: every rule that can reaches zero, and add / mul saturate
    for code in (A.SET, A.SUB, A.DIV, A.DIVZ, A.MOD, A.MUL, A.MIN):
        assert {0, 1} <= seen[code], A.CODE_WORD[code]
    assert M32 in seen[A.ADD] and M32 in seen[A.MUL] and 1 in seen[A.ADD]
    # what the words mean, on the model
    assert A.value_of("sub", 1, [10, 3, 2]) == 4 and A.value_of("sub", 0, [3, 10, 1]) == 0 and A.value_of("sub", 5, [5]) == 0
    assert A.value_of("add", 1, [M32 - 1, 5]) == M32 and A.value_of("mul", 0, [M32, M32]) == 0 and A.value_of("mul", 3, [1 << 31]) == M32
    assert A.value_of("div", 1, [7, 2]) == 3 and A.value_of("div", 1, [7, 0]) == 0 and A.value_of("div", 0, [7]) == 0
    assert A.value_of("divzero", 1, [7, 2]) == 4 and A.value_of("divzero", 1, [0, 2]) == 1 and A.value_of("divzero", 0, [7]) == 0
    assert A.value_of("divzero", 1, [7, 0]) == 1                          # 7 / 0 is 0, and 0 < 1 gives 1, as in the reference
    assert A.value_of("mod", 0, [17, 5]) == 2 + 3 and A.value_of("mod", 4, [17, 5]) == 2 + 3 and A.value_of("mod", 2, [17, 0]) == 17
    assert A.value_of("min", M32, [9, 4]) == 4 and A.value_of("max", 5, [1, 2]) == 5 and A.value_of("count", 0, [9, 9, 9]) == 3
    assert A.value_of("first", 0, [8, 1]) == 8 == A.value_of("selected", M32, [8, 1]) and A.value_of("set", (1 << 32) + 6, [1]) == 6


# ---- the parser -------------------------------------------------------------------------------------------------------------
GOOD_TEXTS = ["#1", "#0", "#4294967295", "#0x10", "#0b101", "first", "selected", "min", "max", "add", "sum", "sub", "dif", "mul", "div", "divzero",
              "mod", "rem", "count", "min#3", "max#5", "add#0xFFFFFFFF", "sum#7", "sub#3", "dif#1", "mul#2", "div#0", "divzero#0b11", "mod#10",
              "rem#0X1f", "max#0"]
BAD_TEXTS = {
    "an unknown word": "nonsense", "nothing": "", "a constant above 2^32-1": "#4294967296", "a word constant above 2^32-1": "max#0x100000000",
    "count with a constant": "count#3", "first with a constant": "first#1", "selected with a constant": "selected#0", "no integer": "sub#three",
    "an empty constant": "min#", "a lone hash constant": "#", "a negative": "add#-1", "a word of the label table": "or", "a prefix of a word": "su",
    "upper case": "SUB", "a float": "mul#1.5", "two constants": "sub#1#2", "a far too large constant": "#99999999999999999999999",
}


def test_parser_against_the_model_and_every_refusal(native_lib):
    from meryl_amd import capi, db
    for text in GOOD_TEXTS:
        assert db.parse_value_assign(text) == A.parse_value(text), text
        assert db.value_assign_option(text) == A.parse_value(text)
    assert db.parse_value_assign("sub#3") == (A.SUB, 3) and db.parse_value_assign("min") == (A.MIN, M32) and db.parse_value_assign("#1") == (A.SET, 1)
    assert db.value_assign_option(("divzero", None)) == (A.DIVZ, 1) and db.value_assign_option(("sub", 3)) == (A.SUB, 3)
    assert db.value_assign_option(None) == (A.NONE, 0)
    for what, text in BAD_TEXTS.items():
        with pytest.raises(ValueError):
            A.parse_value(text)
        with pytest.raises(capi.MgcError) as e:
            db.parse_value_assign(text)
        assert e.value.args and len(str(e.value)) > 20, what
    with pytest.raises(ValueError):
        db.value_assign_option(("nonsense", 1))


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_device_entry_points_check_their_arguments_before_any_launch(native_lib):
    from meryl_amd import capi
    L = native_lib
    n_out = ctypes.c_uint64(0)
    ok = S.to_ctypes([S.term(S.VALUE, S.GT, 0, 0, 0, 0, -1, 0, 1)])

    def many(n_inputs, op, assign, lop, terms, n_terms, k=21, kw=1):
        m = max(n_inputs, 1)
        kp = (ctypes.c_void_p * m)(*[4096] * m)
        ns = (ctypes.c_uint64 * m)(*[8] * m)
        a = L.mgc_dev_merge_many_count_assigned(kp, kp, kp, ns, n_inputs, kw, k, op, assign, 1, lop, 0, terms, n_terms, 4096, 1 << 30, ctypes.byref(n_out), None)
        b = L.mgc_dev_merge_many_emit_assigned(kp, kp, kp, ns, n_inputs, kw, k, op, assign, 1, lop, 0, terms, n_terms, 4096, 1 << 30, 4096, 4096, 4096, None)
        return a, b
    E = (capi.MGC_EINVAL, capi.MGC_EINVAL)
    for assign in (13, -1, 100):
        assert many(2, 0, assign, 0, ok, 1) == E, assign
        assert b"value assignment" in L.mgc_last_error(None)
    for n_inputs, op, lop in ((0, 0, 0), (33, 0, 0), (2, 11, 0), (2, -1, 0), (2, 0, 13), (2, 0, capi.LABEL_OPS["invert"])):
        assert many(n_inputs, op, A.SUB, lop, ok, 1) == E, (n_inputs, op, lop)
    assert many(2, 0, A.SUB, 0, ok, 1, k=0) == E and many(2, 0, A.SUB, 0, ok, 1, k=33) == E
    bad = S.to_ctypes([S.term(S.VALUE, S.GT, 0, 0, 0, 3, -1, 0, 1)])
    assert many(2, 0, A.SUB, 0, bad, 1) == E and b"selector" in L.mgc_last_error(None)


def test_eval_assigned_refuses_every_violation_before_the_device(native_lib, tmp_path):
    from meryl_amd import capi, db
    a, b = tiny_db(tmp_path / "a", 21), tiny_db(tmp_path / "b", 21)
    many = [tiny_db(tmp_path / ("m%02d" % i), 21) for i in range(33)]
    out = str(tmp_path / "out")
    before = sorted(os.listdir(tmp_path))
    N = capi.EvalNodeAssigned
    DB, MERGE, VALUE = capi.NODE_DATABASE, capi.NODE_MERGE, capi.NODE_VALUE

    def raw(nodes, children, root, terms=()):
        arr = (N * len(nodes))()
        for e, (kind, op, path, first, n, nt, assign) in zip(arr, nodes):
            e.kind, e.op, e.constant, e.path, e.first_child, e.n_children = kind, op, 1, path.encode() if path else None, first, n
            e.label_op, e.label_constant, e.first_term, e.n_terms, e.value_assign, e.value_constant = 0, 0, 0, nt, assign, 1
        kids = (ctypes.c_uint32 * max(len(children), 1))(*children)
        return native_lib.mgc_db_eval_assigned(arr, len(nodes), kids, len(children), root, S.to_ctypes(list(terms)), len(terms), 0, 0,
                                               ctypes.cast(None, capi.EVAL_SLICE_LABELLED_CB), None, -1, 2)

    def refused(what, rc, text):
        msg = native_lib.mgc_db_stream_error(None)
        assert rc == capi.MGC_EINVAL, (what, rc, msg)
        assert msg and b"mgc_db_eval_assigned" in msg and text in msg, (what, msg)
        assert sorted(os.listdir(tmp_path)) == before, what

    leaves = [(DB, 0, a, 0, 0, 0, 0), (DB, 0, b, 0, 0, 0, 0)]
    for code in (13, -1, 99):
        refused("an unknown assign code", raw([(MERGE, 0, out, 0, 2, 0, code)] + leaves, [1, 2], 0), b"unknown value assignment")
    refused("an assignment on a database", raw([(MERGE, 0, out, 0, 2, 0, 0), (DB, 0, a, 0, 0, 0, A.SET), leaves[1]], [1, 2], 0), b"a database takes no")
    for vop in range(6, 12):
        refused("an assignment on an arithmetic value node", raw([(VALUE, vop, out, 0, 1, 0, A.MUL), leaves[0]], [1], 0), b"arithmetic value operation")
    refused("a 33-input merge with an assignment", raw([(MERGE, 0, out, 0, 33, 0, A.COUNT)] + [(DB, 0, m, 0, 0, 0, 0) for m in many],
                                                       list(range(1, 34)), 0), b"with a value assignment at most 32")
    # what mgc_db_eval_selected refuses is refused here in the same way
    refused("a bad program beside an assignment", raw([(MERGE, 0, out, 0, 2, 1, A.SUB)] + leaves, [1, 2], 0,
                                                      [S.term(S.VALUE, S.GT, 0, 0, 0, 3, -1, 0, 1)]), b"selector")
    refused("a value node with two children", raw([(VALUE, 2, out, 0, 2, 0, A.SUB)] + leaves, [1, 2], 0), b"exactly one input")
    refused("the output is also a leaf", raw([(MERGE, 0, a + "/", 0, 2, 0, A.SUB)] + leaves, [1, 2], 0), b"also an input")
    # through Python: the text is parsed before the call
    for value in ("nonsense", "count#1", "#4294967296"):
        with pytest.raises(capi.MgcError):
            db.evaluate_assigned(("union", a, b, {"value": value, "output": out}))
        assert sorted(os.listdir(tmp_path)) == before, value
    with pytest.raises(capi.MgcError, match="arithmetic value operation"):
        db.evaluate_assigned(("increase", 3, a, {"value": "mul", "output": out}))
    with pytest.raises(capi.MgcError, match="a database takes no"):
        arr, kids, n_kids, root, terms, n_terms = db.build_tree_assigned(("union", a, b, {"output": out}))
        arr[0].value_assign = A.SET
        rc = native_lib.mgc_db_eval_assigned(arr, len(arr), kids, n_kids, root, terms, n_terms, 0, 0, ctypes.cast(None, capi.EVAL_SLICE_LABELLED_CB),
                                             None, -1, 2)
        raise capi.MgcError(rc, "mgc_db_eval_assigned", native_lib.mgc_db_stream_error(None).decode())
    assert sorted(os.listdir(tmp_path)) == before
    with pytest.raises(ValueError):
        db.build_tree_assigned(("union-sum", a, b, {"values": "sub"}))


def test_assigned_tree_builder_lays_out_nodes_terms_and_assignments(native_lib):
    from meryl_amd import capi, db
    tree = ("intersect", ("union", "a", "b", "c", {"value": "count", "select": ["value:>=2"], "label": "or"}),
            ("at-least", 2, "d", {"value": ("max", 5)}), "e", {"output": "o", "value": "sub#3"})
    arr, kids, n_kids, root, terms, n_terms = db.build_tree_assigned(tree)
    sel, skids, sn_kids, sroot, sterms, sn_terms = db.build_tree_selected(
        ("intersect", ("union", "a", "b", "c", {"select": ["value:>=2"], "label": "or"}), ("at-least", 2, "d"), "e", {"output": "o"}))
    assert (root, n_kids, list(kids), n_terms) == (sroot, sn_kids, list(skids), sn_terms) and len(arr) == len(sel)
    for e, b in zip(arr, sel):
        assert (e.kind, e.op, e.constant, e.path, e.first_child, e.n_children, e.label_op, e.label_constant, e.first_term, e.n_terms) == \
               (b.kind, b.op, b.constant, b.path, b.first_child, b.n_children, b.label_op, b.label_constant, b.first_term, b.n_terms)
    got = sorted((e.value_assign, e.value_constant) for e in arr if e.value_assign)
    assert got == [(A.MAX, 5), (A.SUB, 3), (A.COUNT, 0)]
    assert (arr[root].value_assign, arr[root].value_constant) == (A.SUB, 3)
    assert all(e.value_assign == 0 for e in arr if e.kind == capi.NODE_DATABASE)
    arr, _, _, _, _, _ = db.build_tree_assigned(("union-sum", "a", "b"))
    assert all(e.value_assign == 0 and e.value_constant == 0 for e in arr)


@pytest.fixture(scope="module")
def meryl(native_lib):
    from meryl_amd import build
    path = build.build_cli()
    assert os.path.exists(path)
    return path


def test_cli_refuses_value_assignments_where_they_do_not_belong(meryl, native_lib, tmp_path):
    a, b = tiny_db(tmp_path / "a", 21), tiny_db(tmp_path / "b", 21)
    fa = tmp_path / "r.fa"
    fa.write_text(">a\nACGTACGTACGTACGTACGTACGTACGT\n")
    before = sorted(os.listdir(tmp_path))

    def run(*args):
        return subprocess.run([meryl] + [str(x) for x in args], capture_output=True, text=True, timeout=120)
    p = run("increase", "3", "value=mul", a, "output", tmp_path / "u")
    assert p.returncode == 1 and "is a value assignment itself" in p.stderr, p.stderr
    p = run("k=21", "count", "value=#1", fa, "output", tmp_path / "db")
    assert p.returncode == 1 and "a counting operation takes no value assignment" in p.stderr, p.stderr
    p = run("union", "value=nonsense", a, b, "output", tmp_path / "u")
    assert p.returncode == 1 and "Unknown assign:value=<parameter> in 'value=nonsense'" in p.stderr, p.stderr
    for text, said in (("count#1", "takes no constant"), ("#4294967296", "does not fit a 32-bit value"), ("sub#x", "is not an integer")):
        p = run("union", "value=" + text, a, b, "output", tmp_path / "u")
        assert p.returncode == 1 and said in p.stderr, (text, p.stderr)
    p = run("value=#1", a)
    assert p.returncode == 1 and "needs a set or value-filter operation" in p.stderr, p.stderr
    assert sorted(os.listdir(tmp_path)) == before
