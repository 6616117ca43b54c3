"""The labelled evaluation path on a machine without a GPU: the new symbols are exported and declared, mgc_db_eval_labelled
refuses what it must before any device call and before any output directory exists, build_tree_labelled lays the label
operations out beside the nodes build_tree makes, and the command line refuses the label words it does not offer."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from test_db_eval_host import tiny_db

NEW_SYMBOLS = ("mgc_label_default_constant", "mgc_dev_merge_many_emit_labelled", "mgc_dev_select_emit_labelled", "mgc_dev_decode_blocks",
               "mgc_db_stream_write_labelled", "mgc_db_eval_labelled")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_new_symbols_are_exported_and_declared(native_lib):
    from meryl_amd import capi
    headers = open(os.path.join(ROOT, "include", "meryl_gpu_count.h")).read() + open(os.path.join(ROOT, "include", "meryl_db.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(native_lib, name), name
        assert name in capi.SYMBOLS, name
        assert re.search(r"\b%s\(" % name, headers), name
    for word, code in capi.LABEL_OPS.items():
        assert re.search(r"#define MGC_LABEL_%s\s+%d\b" % (word.upper(), code), headers), word
    ones = 0xFFFFFFFFFFFFFFFF
    want = {"and": ones, "xor": ones, "lightest": ones}
    for word, code in capi.LABEL_OPS.items():
        assert native_lib.mgc_label_default_constant(code) == want.get(word, 0), word
    assert ctypes.sizeof(capi.EvalNodeLabelled) == ctypes.sizeof(capi.EvalNode) + 16


def test_labelled_emits_check_their_arguments_before_any_launch(native_lib):
    from meryl_amd import capi
    L = native_lib
    for n_inputs, op, lop in ((0, 0, 6), (33, 0, 6), (2, 11, 6), (2, 0, 13), (2, 0, -1), (2, 0, capi.LABEL_OPS["invert"])):
        m = max(n_inputs, 1)
        kp = (ctypes.c_void_p * m)(*[4096] * m)
        ns = (ctypes.c_uint64 * m)(*[8] * m)
        rc = L.mgc_dev_merge_many_emit_labelled(kp, kp, kp, ns, n_inputs, 1, op, lop, 0, 4096, 1 << 30, 4096, 4096, 4096, None)
        assert rc == capi.MGC_EINVAL, (n_inputs, op, lop)
    assert L.mgc_dev_select_emit_labelled(4096, 4096, 4096, 8, 1, 2, 1, 13, 0, 4096, 1 << 30, 4096, 4096, 4096, None) == capi.MGC_EINVAL
    assert L.mgc_dev_select_emit_labelled(4096, 4096, 4096, 8, 1, 12, 1, 2, 0, 4096, 1 << 30, 4096, 4096, 4096, None) == capi.MGC_EINVAL
    assert L.mgc_dev_decode_blocks(4096, 4096, 1, 30, 65, 1, 4096, 4096, 4096, None) == capi.MGC_EINVAL


def multiset_db(path, k):
    """tiny_db with the multiset flag (bit 0 of the master index's flags) set"""
    from meryl_amd import db
    p = tiny_db(path, k)
    r = db.Reader(p)
    flags = r.info.flags
    r.close()
    assert flags & 1 == 0
    idx = os.path.join(p, "merylIndex")
    raw = bytearray(open(idx, "rb").read())
    # the master index is an MSB-first bit stream in 64-bit words: (prefixSize, suffixSize), (numFilesBits, numBlocksBits), then
    # flags in the top half of the next word (meryl_db.cpp, A8)
    want = np.array([(6 << 32) | (2 * k - 6), (6 << 32) | 0], dtype=np.uint64).tobytes()
    at = bytes(raw).find(want)
    assert at >= 0 and bytes(raw).find(want, at + 1) < 0
    raw[at + 16 + 4] |= 1
    open(idx, "wb").write(bytes(raw))
    r = db.Reader(p)
    assert r.info.flags & 1
    r.close()
    return p


def test_every_violation_is_refused_before_the_device(native_lib, tmp_path):
    from meryl_amd import capi, db
    a, b = tiny_db(tmp_path / "a", 21, label_size=4), tiny_db(tmp_path / "b", 21)
    k15 = tiny_db(tmp_path / "k15", 15, label_size=4)
    multi = multiset_db(tmp_path / "multi", 21)
    many = [tiny_db(tmp_path / ("m%02d" % i), 21) for i in range(33)]
    out = str(tmp_path / "out")
    before = sorted(os.listdir(tmp_path))
    N = capi.EvalNodeLabelled
    DB, MERGE, VALUE = capi.NODE_DATABASE, capi.NODE_MERGE, capi.NODE_VALUE
    LOP = capi.LABEL_OPS

    def raw(nodes, children, root):
        arr = (N * len(nodes))()
        for e, (kind, op, lop, path, first, n) in zip(arr, nodes):
            e.kind, e.op, e.constant, e.path, e.first_child, e.n_children = kind, op, 1, path.encode() if path else None, first, n
            e.label_op, e.label_constant = lop, 0
        kids = (ctypes.c_uint32 * max(len(children), 1))(*children)
        return native_lib.mgc_db_eval_labelled(arr, len(nodes), kids, len(children), root, 0, ctypes.cast(None, capi.EVAL_SLICE_LABELLED_CB),
                                               None, -1, 2)

    cases = {
        "unknown label operation": ([(MERGE, 0, 13, out, 0, 2), (DB, 0, 0, a, 0, 0), (DB, 0, 0, b, 0, 0)], [1, 2], 0),
        "negative label operation": ([(VALUE, 2, -1, out, 0, 1), (DB, 0, 0, a, 0, 0)], [1], 0),
        "invert on a two-input merge": ([(MERGE, 0, LOP["invert"], out, 0, 2), (DB, 0, 0, a, 0, 0), (DB, 0, 0, b, 0, 0)], [1, 2], 0),
        "a 33-input merge": ([(MERGE, 0, LOP["or"], out, 0, 33)] + [(DB, 0, 0, m, 0, 0) for m in many], list(range(1, 34)), 0),
        "a multiset leaf": ([(MERGE, 0, LOP["or"], out, 0, 2), (DB, 0, 0, a, 0, 0), (DB, 0, 0, multi, 0, 0)], [1, 2], 0),
        "mixed k": ([(MERGE, 0, LOP["or"], out, 0, 2), (DB, 0, 0, a, 0, 0), (DB, 0, 0, k15, 0, 0)], [1, 2], 0),
        # ... and what mgc_db_eval refuses is refused here in the same way
        "value node with two children": ([(VALUE, 2, 0, out, 0, 2), (DB, 0, 0, a, 0, 0), (DB, 0, 0, b, 0, 0)], [1, 2], 0),
        "output is also a leaf": ([(MERGE, 0, 0, a + "/", 0, 2), (DB, 0, 0, a, 0, 0), (DB, 0, 0, b, 0, 0)], [1, 2], 0),
    }
    for what, (nodes, children, root) in cases.items():
        rc = raw(nodes, children, root)
        msg = native_lib.mgc_db_stream_error(None)
        assert rc == capi.MGC_EINVAL, (what, rc, msg)
        assert msg and b"mgc_db_eval_labelled" in msg, (what, msg)
        assert sorted(os.listdir(tmp_path)) == before, what
    assert b"multiset" in (raw(*cases["a multiset leaf"]), native_lib.mgc_db_stream_error(None))[1]
    assert b"15-mers" in (raw(*cases["mixed k"]), native_lib.mgc_db_stream_error(None))[1]
    # the unlabelled entry point still refuses the labelled leaf (tests/test_db_eval_host.py pins it too)
    with pytest.raises(capi.MgcError, match="stores labels"):
        db.evaluate(("union-sum", a, b, {"output": out}))
    # the Python front raises with the message, or before the call for a word it does not know
    with pytest.raises(capi.MgcError, match="invert"):
        db.evaluate_labelled(("union-sum", a, b, {"label": "invert", "output": out}))
    with pytest.raises(ValueError):
        db.evaluate_labelled(("union-sum", a, b, {"label": "rotate-left", "output": out}))
    assert sorted(os.listdir(tmp_path)) == before


def test_labelled_tree_builder_lays_out_nodes_children_and_label_operations(native_lib):
    from meryl_amd import capi, db
    LOP = capi.LABEL_OPS
    tree = ("subtract", ("union-sum", "a", "b", "c", {"label": "or"}), ("multiply", 2, "d", {"label": ("and", 0x0F)}),
            {"output": "o", "label": ("set", 5)})
    arr, kids, n_kids, root = db.build_tree_labelled(tree)
    plain, pkids, pn_kids, proot = db.build_tree(("subtract", ("union-sum", "a", "b", "c"), ("multiply", 2, "d"), {"output": "o"}))
    assert (root, n_kids, list(kids)) == (proot, pn_kids, list(pkids)) and len(arr) == len(plain)
    for e, b in zip(arr, plain):                                     # the fields of mgc_eval_node are the ones build_tree makes
        assert (e.kind, e.op, e.constant, e.path, e.first_child, e.n_children) == (b.kind, b.op, b.constant, b.path, b.first_child, b.n_children)
    top = arr[root]
    assert (top.kind, top.op, top.path, top.n_children, top.label_op, top.label_constant) == (capi.NODE_MERGE, 7, b"o", 2, LOP["set"], 5)
    left, right = (arr[kids[top.first_child + i]] for i in range(2))
    assert (left.kind, left.op, left.n_children, left.label_op, left.label_constant) == (capi.NODE_MERGE, 0, 3, LOP["or"], 0)
    assert [arr[kids[left.first_child + i]].path for i in range(3)] == [b"a", b"b", b"c"]
    assert (right.kind, right.op, right.constant, right.label_op, right.label_constant) == (capi.NODE_VALUE, 8, 2, LOP["and"], 0x0F)
    leaf = arr[kids[right.first_child]]
    assert (leaf.kind, leaf.path, leaf.label_op, leaf.label_constant) == (capi.NODE_DATABASE, b"d", 0, 0)
    # no "label": the operation's default; a word without a constant: the reference's identity for it
    arr, kids, _, root = db.build_tree_labelled(("intersect", "a", ("at-least", 2, "b", {"label": "lightest"})))
    assert (arr[root].label_op, arr[root].label_constant) == (LOP["default"], 0)
    v = arr[kids[arr[root].first_child + 1]]
    assert (v.label_op, v.label_constant) == (LOP["lightest"], 0xFFFFFFFFFFFFFFFF)
    with pytest.raises(ValueError):
        db.build_tree_labelled(("union-sum", "a", "b", {"label": "frobnicate"}))
    with pytest.raises(ValueError):
        db.build_tree_labelled(("union-sum", "a", "b", {"labels": "or"}))


@pytest.fixture(scope="module")
def meryl(native_lib):
    from meryl_amd import build
    path = build.build_cli()
    assert os.path.exists(path)
    return path


def test_cli_refuses_the_label_words_it_does_not_offer(meryl, native_lib, tmp_path):
    a, b = tiny_db(tmp_path / "a", 21), tiny_db(tmp_path / "b", 21)
    fa = tmp_path / "r.fa"
    fa.write_text(">a\nACGTACGTACGTACGTACGTACGTACGT\n")
    before = sorted(os.listdir(tmp_path))

    def run(*args):
        return subprocess.run([meryl] + [str(x) for x in args], capture_output=True, text=True, timeout=120)
    p = run("union-sum", "label=rotate-left", a, b, "output", tmp_path / "u")
    assert p.returncode == 1 and "shift and rotate label words" in p.stderr
    p = run("union-sum", "label=shift-left#2", a, b, "output", tmp_path / "u")
    assert p.returncode == 1 and "shift and rotate label words" in p.stderr
    p = run("union-sum", "label=frobnicate", a, b, "output", tmp_path / "u")
    assert p.returncode == 1 and "Unknown assign:label=<parameter> in 'label=frobnicate'" in p.stderr
    p = run("k=21", "count", "label=7", fa, "output", tmp_path / "db")
    assert p.returncode == 1 and "label=#<integer>" in p.stderr                         # a count keeps its own meaning of label=
    p = run("k=21", "count", "label=or", fa, "output", tmp_path / "db")
    assert p.returncode == 1 and "label=#<integer>" in p.stderr
    assert sorted(os.listdir(tmp_path)) == before


def test_label_table_on_the_host(tmp_path):
    """meryl_amd/csrc/mgc_label.hpp -- the code the kernels run per group of equal k-mers -- in a stand-alone host program
    (tests/host/label_host.cpp) against the Python statement of the table, label_helpers.label_of: every label word under every
    merge operation and as a value operation, 1..5 active inputs, labels over the full 64 bits, values with ties and 2^32-1,
    popcount ties, default and explicit constants"""
    import shutil
    import label_helpers as LH
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "label_host")
    c = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=undefined", "-fno-sanitize-recover=undefined",
                        os.path.join(ROOT, "tests", "host", "label_host.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert c.returncode == 0, c.stderr
    rng = np.random.default_rng(64)
    cases, want = [], []
    pools = [lambda: int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(0, 2)),           # all 64 bits
             lambda: 0b11 << int(rng.integers(0, 62)),                                       # popcount ties
             lambda: int(rng.integers(0, 4))]
    values = [lambda: int(rng.integers(1, 6)), lambda: LH.M32, lambda: int(rng.integers(1, LH.M32))]
    for word_code, word in enumerate(LH.LABEL_WORDS):
        for merge_op in list(range(11)) + [None]:
            for rep in range(12):
                n = 1 if (word == "invert" or merge_op is None) else int(rng.integers(1, 6))
                pool, vpool = pools[rep % 3], values[(rep // 3) % 3]
                L = [pool() for _ in range(n)]
                V = [vpool() for _ in range(n)]
                const = LH.DEFAULT_CONSTANT.get(word, 0) if rep % 2 == 0 else pool()
                cases.append("%d %d %d %x %d %s" % (merge_op is not None, merge_op or 0, word_code, const, n,
                                                   " ".join("%x %d" % lv for lv in zip(L, V))))
                want.append("%x" % LH.label_of(word, const, L, V, merge_op=merge_op))
    for bad in (-1, 13, 14, 99):
        cases.append("1 0 %d 0 1 5 5" % bad)
        want.append("refused")
    p = subprocess.run([exe], input="\n".join(cases) + "\n", capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr
    got = p.stdout.split("\n")[:-1]
    assert len(got) == len(want) > 1500
    for case, g, w in zip(cases, got, want):
        assert g.split()[-1] == w, (case, g, w)
