"""mgc_db_eval validates its tree before any device call and before any output directory exists: every violation returns
MGC_EINVAL with a message, leaves nothing behind, and does so on a machine without a GPU."""
import os

import numpy as np
import pytest


def tiny_db(path, k, label_size=0):
    from meryl_amd import db
    w = db.Writer(str(path), k, 6, label_size)
    for p in range(64):
        some = p in (3, 40)
        w.add_block(p, np.array([5, 9], dtype=np.uint64) if some else np.zeros(0, dtype=np.uint64),
                    np.array([2, 7], dtype=np.uint32) if some else np.zeros(0, dtype=np.uint32), label=1 if label_size else 0)
    w.close()
    return str(path)


def test_new_entry_points_are_exported(native_lib):
    for name in ("mgc_dev_merge_many_tile", "mgc_dev_merge_many_workspace_bytes", "mgc_dev_merge_many_count", "mgc_dev_merge_many_emit",
                 "mgc_db_eval"):
        assert hasattr(native_lib, name), name
    assert native_lib.mgc_dev_merge_many_tile(1) >= 64 and native_lib.mgc_dev_merge_many_tile(2) >= 64


def test_merge_many_checks_its_arguments_before_any_launch(native_lib):
    import ctypes
    from meryl_amd import capi
    n_out = ctypes.c_uint64(0)
    for n_inputs, op in ((1, 0), (33, 0), (2, 11), (2, -1)):
        kp = (ctypes.c_void_p * n_inputs)(*[4096] * n_inputs)
        ns = (ctypes.c_uint64 * n_inputs)(*[8] * n_inputs)
        assert native_lib.mgc_dev_merge_many_count(kp, kp, ns, n_inputs, 1, op, 4096, 1 << 30, ctypes.byref(n_out), None) == capi.MGC_EINVAL
        assert native_lib.mgc_dev_merge_many_emit(kp, kp, ns, n_inputs, 1, op, 4096, 1 << 30, 4096, 4096, None) == capi.MGC_EINVAL


def test_every_violation_is_refused_before_the_device(native_lib, tmp_path):
    from meryl_amd import capi, db
    a, b = tiny_db(tmp_path / "a", 21), tiny_db(tmp_path / "b", 21)
    k15 = tiny_db(tmp_path / "k15", 15)
    labelled = tiny_db(tmp_path / "labelled", 21, label_size=4)
    out = str(tmp_path / "out")
    out2 = str(tmp_path / "out2")
    before = sorted(os.listdir(tmp_path))
    N = capi.EvalNode

    def raw(nodes, children, root):
        arr = (N * len(nodes))()
        for e, (kind, op, path, first, n) in zip(arr, nodes):
            e.kind, e.op, e.constant, e.path, e.first_child, e.n_children = kind, op, 1, path.encode() if path else None, first, n
        kids = (capi.ctypes.c_uint32 * max(len(children), 1))(*children)
        return native_lib.mgc_db_eval(arr, len(nodes), kids, len(children), root, capi.ctypes.cast(None, capi.EVAL_SLICE_CB), None, -1, 2)

    DB, MERGE, VALUE = capi.NODE_DATABASE, capi.NODE_MERGE, capi.NODE_VALUE
    cases = {
        "root out of range": ([(DB, 0, a, 0, 0)], [], 1),
        "child index out of range": ([(MERGE, 0, out, 0, 1)], [7], 0),
        "children range out of range": ([(MERGE, 0, out, 0, 3), (DB, 0, a, 0, 0)], [1], 0),
        "node reached twice": ([(MERGE, 0, out, 0, 2), (DB, 0, a, 0, 0)], [1, 1], 0),
        "cycle": ([(MERGE, 0, out, 0, 1), (MERGE, 0, None, 1, 1)], [1, 0], 0),
        "leaf with children": ([(MERGE, 0, out, 0, 1), (DB, 0, a, 1, 1), (DB, 0, b, 0, 0)], [1, 2], 0),
        "value node with two children": ([(VALUE, 2, out, 0, 2), (DB, 0, a, 0, 0), (DB, 0, b, 0, 0)], [1, 2], 0),
        "value node without children": ([(VALUE, 2, out, 0, 0)], [], 0),
        "merge node without children": ([(MERGE, 0, out, 0, 0)], [], 0),
        "unknown merge operation": ([(MERGE, 11, out, 0, 1), (DB, 0, a, 0, 0)], [1], 0),
        "unknown value operation": ([(VALUE, 12, out, 0, 1), (DB, 0, a, 0, 0)], [1], 0),
        "unknown kind": ([(3, 0, out, 0, 1), (DB, 0, a, 0, 0)], [1], 0),
        "leaf does not open": ([(MERGE, 0, out, 0, 2), (DB, 0, a, 0, 0), (DB, 0, str(tmp_path / "missing"), 0, 0)], [1, 2], 0),
        "leaf without a path": ([(MERGE, 0, out, 0, 1), (DB, 0, None, 0, 0)], [1], 0),
        "another k": ([(MERGE, 0, out, 0, 2), (DB, 0, a, 0, 0), (DB, 0, k15, 0, 0)], [1, 2], 0),
        "labelled": ([(MERGE, 0, out, 0, 2), (DB, 0, a, 0, 0), (DB, 0, labelled, 0, 0)], [1, 2], 0),
        "output named twice": ([(MERGE, 0, out, 0, 2), (VALUE, 2, out, 2, 1), (DB, 0, b, 0, 0), (DB, 0, a, 0, 0)], [1, 2, 3], 0),
        "output is also a leaf": ([(MERGE, 0, a + "/", 0, 2), (DB, 0, a, 0, 0), (DB, 0, b, 0, 0)], [1, 2], 0),
        "inner output is a leaf elsewhere": ([(MERGE, 0, out2, 0, 2), (VALUE, 2, b, 2, 1), (DB, 0, b, 0, 0), (DB, 0, a, 0, 0)], [1, 3, 2], 0),
    }
    for what, (nodes, children, root) in cases.items():
        rc = raw(nodes, children, root)
        msg = native_lib.mgc_db_stream_error(None)
        assert rc == capi.MGC_EINVAL, (what, rc, msg)
        assert msg and b"mgc_db_eval" in msg, (what, msg)
        assert sorted(os.listdir(tmp_path)) == before, what
    assert native_lib.mgc_db_eval(None, 0, None, 0, 0, capi.ctypes.cast(None, capi.EVAL_SLICE_CB), None, -1, 2) == capi.MGC_EINVAL
    # the Python front builds the same arrays and raises with the message
    with pytest.raises(capi.MgcError, match="15-mers"):
        db.evaluate(("union-sum", a, ("at-least", 2, k15), {"output": out}))
    with pytest.raises(ValueError):
        db.evaluate(("at-least", a))
    with pytest.raises(ValueError):
        db.evaluate(("frobnicate", a, b))
    assert sorted(os.listdir(tmp_path)) == before


def test_tree_builder_lays_out_nodes_and_children(native_lib):
    from meryl_amd import capi, db
    arr, kids, n_kids, root = db.build_tree(("subtract", ("union-sum", "a", "b", "c"), ("multiply", 2, "d"), {"output": "o"}))
    assert root == len(arr) - 1 and n_kids == 6
    top = arr[root]
    assert (top.kind, top.op, top.path, top.n_children) == (capi.NODE_MERGE, 7, b"o", 2)
    left, right = (arr[kids[top.first_child + i]] for i in range(2))
    assert (left.kind, left.op, left.path, left.n_children) == (capi.NODE_MERGE, 0, None, 3)
    assert [arr[kids[left.first_child + i]].path for i in range(3)] == [b"a", b"b", b"c"]
    assert (right.kind, right.op, right.constant, right.n_children) == (capi.NODE_VALUE, 8, 2, 1)
    assert arr[kids[right.first_child]].path == b"d" and arr[kids[right.first_child]].kind == capi.NODE_DATABASE
