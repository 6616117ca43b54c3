"""K-mer text lists on a machine without a GPU: the new symbols are exported, declared and bound; the line bound and the per-slice file
names are what include/meryl_list.h says; mgc_list_kmers and mgc_db_eval_listed refuse what they must before any device call; the
command line takes `print [operation]` up to the device."""
import ctypes
import os
import re
import subprocess

import pytest

from test_db_eval_host import tiny_db

NEW_SYMBOLS = {"meryl_list.h": ("mgc_list_max_line", "mgc_list_tile_kmers", "mgc_list_slice_name", "mgc_list_kmers",
                                "mgc_dev_list_workspace_bytes", "mgc_dev_list_lengths", "mgc_dev_list_format"),
               "meryl_db.h": ("mgc_db_eval_listed",)}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_new_symbols_are_exported_declared_and_bound(native_lib):
    from meryl_amd import capi, db
    for header, names in NEW_SYMBOLS.items():
        text = open(os.path.join(ROOT, "include", header)).read()
        for name in names:
            assert hasattr(native_lib, name), name
            assert name in capi.SYMBOLS, name
            assert re.search(r"\b%s\(" % name, text), name
            assert getattr(native_lib, name).argtypes is not None, name
    for name in ("format_kmers", "evaluate_listed", "build_tree_listed", "list_geometry", "list_slice_name"):
        assert callable(getattr(db, name)), name


def test_line_bound_and_tile_geometry(native_lib):
    L = native_lib
    assert L.mgc_list_max_line(1, 0) == 14 and L.mgc_list_max_line(21, 0) == 34 and L.mgc_list_max_line(64, 64) == 141
    for k in (1, 16, 31, 32, 33, 64):
        for label_size in (0, 1, 63, 64):
            line, tile = L.mgc_list_max_line(k, label_size), L.mgc_list_tile_kmers(k, label_size)
            # the longest line that can occur fits the bound, and a tile's text fits the LDS image the kernel declares (36864 bytes)
            assert k + 1 + 10 + ((1 + label_size) if label_size else 0) + 1 <= line <= 141
            assert tile >= 256 and tile % 64 == 0 and tile * line <= 36864, (k, label_size, tile)
    assert L.mgc_list_tile_kmers(0, 0) == 0 and L.mgc_list_tile_kmers(65, 0) == 0 and L.mgc_list_tile_kmers(21, 65) == 0


def test_slice_names(native_lib):
    from meryl_amd import db
    for name, ff, want in (("a.##.txt", 7, "a.07.txt"), ("a.#.txt", 7, "a.07.txt"), ("a.####", 63, "a.0063"), ("##.x.##", 5, "05.x.##"),
                           ("#", 0, "00"), ("dir#/u.###.txt", 12, "dir12/u.###.txt"), ("u.##.txt", 63, "u.63.txt")):
        assert db.list_slice_name(name, ff) == want, name
    for name in ("a.txt", "", "-"):
        assert db.list_slice_name(name, 3) is None, name
    # the buffer: exactly the name and its NUL is enough, one byte less is not (and nothing is written)
    buf = ctypes.create_string_buffer(b"x" * 16, 16)
    assert native_lib.mgc_list_slice_name(b"a.##.txt", 7, buf, 9) == 8 and buf.raw[:9] == b"a.07.txt\0" and buf.raw[9:] == b"x" * 7
    buf = ctypes.create_string_buffer(b"x" * 16, 16)
    assert native_lib.mgc_list_slice_name(b"a.##.txt", 7, buf, 8) == 0 and buf.raw == b"x" * 16
    assert native_lib.mgc_list_slice_name(b"a.##.txt", 7, None, 0) == 0 and native_lib.mgc_list_slice_name(None, 7, buf, 16) == 0


def test_list_kmers_refuses_bad_arguments_without_a_device(native_lib):
    from meryl_amd import capi
    L = native_lib
    calls = []
    cb = capi.LIST_WRITE_CB(lambda text, n, user: calls.append(n) or 0)
    none = ctypes.cast(None, capi.LIST_WRITE_CB)

    def refused(rc, text):
        msg = L.mgc_db_stream_error(None)
        assert rc == capi.MGC_EINVAL and msg and b"mgc_list_kmers" in msg and text in msg, (rc, msg)
    refused(L.mgc_list_kmers(4096, 4096, None, 8, 0, 0, 1 << 20, cb, None, None), b"outside 1..64")
    refused(L.mgc_list_kmers(4096, 4096, None, 8, 65, 0, 1 << 20, cb, None, None), b"outside 1..64")
    refused(L.mgc_list_kmers(4096, 4096, None, 8, 21, 65, 1 << 20, cb, None, None), b"at most 64 bits")
    refused(L.mgc_list_kmers(4096, 4096, None, 8, 21, 0, 33, cb, None, None), b"shorter than the longest line (34 bytes)")
    refused(L.mgc_list_kmers(4096, 4096, None, 8, 64, 64, 140, cb, None, None), b"shorter than the longest line (141 bytes)")
    refused(L.mgc_list_kmers(4096, 4096, None, 8, 21, 0, 1 << 20, none, None, None), b"no callback")
    refused(L.mgc_list_kmers(None, 4096, None, 8, 21, 0, 1 << 20, cb, None, None), b"NULL array of 8 k-mers")
    assert L.mgc_dev_list_workspace_bytes(5000, 21, 0) >= 8 * 5 and L.mgc_dev_list_workspace_bytes(5000, 65, 0) == 0
    total = ctypes.c_uint64(0)
    assert L.mgc_dev_list_lengths(4096, 8, 0, 0, 4096, 1 << 20, ctypes.byref(total), None) == capi.MGC_EINVAL
    assert L.mgc_dev_list_lengths(4096, 8, 21, 0, 4096, 8, ctypes.byref(total), None) == capi.MGC_EINVAL          # a workspace too small
    assert L.mgc_dev_list_format(4096, 4096, None, 8, 21, 0, 4096, 1 << 20, 4097, None) == capi.MGC_EINVAL       # text not 16-byte aligned
    assert L.mgc_dev_list_format(4096, 4096, None, 8, 21, 65, 4096, 1 << 20, 4096, None) == capi.MGC_EINVAL
    # the checks come before "nothing to do"; nothing to do is success, without a callback and without a device
    refused(L.mgc_list_kmers(None, None, None, 0, 21, 0, 33, cb, None, None), b"shorter than the longest line")
    assert L.mgc_list_kmers(None, None, None, 0, 21, 0, 34, cb, None, None) == 0 and calls == []


def test_eval_listed_refuses_before_the_device(native_lib, tmp_path):
    from meryl_amd import capi, db
    a, b, c = tiny_db(tmp_path / "a", 21), tiny_db(tmp_path / "b", 21), tiny_db(tmp_path / "c", 21)
    out = str(tmp_path / "out")
    before = sorted(os.listdir(tmp_path))
    arr, kids, n_kids, root, terms, n_terms, want, want_list = db.build_tree_listed(
        ("union-sum", ("at-least", 2, a, {"list": True}), b, {"output": out, "list": True}))
    assert list(want) == [0, 0, 0, 0] and list(want_list) == [0, 1, 0, 1] and root == 3
    calls = []
    cb = capi.EVAL_LIST_CB(lambda user, node, ff, text, n: calls.append(node) or 0)
    none = ctypes.cast(None, capi.EVAL_LIST_CB)

    def call(arr, want_list, list_cb, want=None, hists=None, label_size=0):
        return native_lib.mgc_db_eval_listed(arr, len(arr), kids, n_kids, root, terms, n_terms, 0, label_size,
                                             ctypes.cast(None, capi.EVAL_SLICE_LABELLED_CB), None, -1, 2, want, hists, want_list, list_cb, None)

    def refused(what, rc, text):
        msg = native_lib.mgc_db_stream_error(None)
        assert rc == capi.MGC_EINVAL, (what, rc, msg)
        assert msg and b"mgc_db_eval_listed" in msg and text in msg, (what, msg)
        assert sorted(os.listdir(tmp_path)) == before and calls == [], what
    refused("no callback", call(arr, want_list, none), b"node 1: a list is wanted but there is no callback to receive it")
    # a flagged node the root does not reach: a fifth node nobody names
    arr5 = (capi.EvalNodeAssigned * 5)()
    for i in range(4):
        ctypes.memmove(ctypes.byref(arr5[i]), ctypes.byref(arr[i]), ctypes.sizeof(capi.EvalNodeAssigned))
    arr5[4].kind, arr5[4].path = capi.NODE_DATABASE, c.encode()
    refused("an unreached node", call(arr5, (ctypes.c_uint8 * 5)(0, 1, 0, 1, 1), cb), b"node 4: a list is wanted of a node the root does not reach")
    # the evaluator's own checks fire first, and in the same words
    refused("label size", call(arr, want_list, none, label_size=65), b"a label has at most 64 bits")
    refused("histogram without hists", call(arr, want_list, none, want=(ctypes.c_uint8 * 4)(0, 0, 0, 1)), b"nowhere to return it")
    arr[3].value_assign = 99
    refused("an unknown assign code", call(arr, want_list, cb), b"unknown value assignment")
    arr[3].value_assign = 0
    arr[0].n_children = 1
    refused("a database with inputs", call(arr, want_list, cb), b"a database has no inputs")
    arr[0].n_children = 0
    # the Python tree: "list" is an option of the listed evaluation only, on operations and on databases
    with pytest.raises(ValueError):
        db.build_tree_reported(("union-sum", a, b, {"list": True}))
    with pytest.raises(ValueError):
        db.build_tree_reported(("union-sum", {"database": a, "list": True}, b))
    got = db.build_tree_listed(("union-sum", {"database": a, "list": True}, ("at-least", 2, b, {"histogram": True}), c))
    assert list(got[6]) == [0, 0, 1, 0, 0] and list(got[7]) == [1, 0, 0, 0, 0] and got[3] == 4


@pytest.fixture(scope="module")
def meryl(native_lib):
    from meryl_amd import build
    path = build.build_cli()
    assert os.path.exists(path)
    return path


def run(meryl, *args):
    return subprocess.run([meryl] + [str(x) for x in args], capture_output=True, text=True, timeout=120)


def test_cli_takes_print_of_an_operation_up_to_the_device(meryl, native_lib, tmp_path):
    a, b = tiny_db(tmp_path / "a", 21), tiny_db(tmp_path / "b", 21)
    p = run(meryl, "print", "[union-sum", a, b + "]")
    # accepted: whatever stops it is the device (none here), and it is the listed evaluation that says so
    assert "Can't interpret" not in p.stderr and "not part of this build" not in p.stderr, p.stderr
    assert p.returncode == 0 or "mgc_db_eval_listed" in p.stderr, p.stderr
    # a database is printed without a device: the host reader's lines
    p = run(meryl, "-Q", "print", a)
    assert p.returncode == 0 and p.stdout.count("\n") == 4 and p.stdout.endswith("\t7\n"), p.stderr
