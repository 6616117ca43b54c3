"""Histogram and statistics reports on a machine without a GPU: the new symbols are exported, declared and bound; the statistics
formatter gives the reference's table (written out by hand, the uint64 wrap of k = 32 included), also in a stand-alone host program
built with the address and undefined-behaviour sanitizers; the accumulator ABI and mgc_db_eval_reported refuse what they must before
any device call; the command line takes `histogram [operation]`, `statistics` and the output: words, and refuses what it refused."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import hist_helpers as HH
from test_db_eval_host import tiny_db

NEW_SYMBOLS = ("mgc_value_hist_open", "mgc_value_hist_add", "mgc_value_hist_len", "mgc_value_hist_get", "mgc_value_hist_totals",
               "mgc_value_hist_close", "mgc_value_hist_geometry", "mgc_db_eval_reported", "mdb_format_statistics")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_new_symbols_are_exported_declared_and_bound(native_lib):
    from meryl_amd import capi, db
    header = open(os.path.join(ROOT, "include", "meryl_db.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(native_lib, name), name
        assert name in capi.SYMBOLS, name
        assert re.search(r"\b%s\(" % name, header), name
        assert getattr(native_lib, name).argtypes is not None, name
    dense, group = db.ValueHistogram.geometry()
    assert dense >= 1024 and dense & (dense - 1) == 0 and group % 64 == 0 and group >= 256


def test_statistics_formatter_on_hand_made_histograms(native_lib):
    from meryl_amd import db
    assert db.format_statistics(21, [2, 7], [2, 2], 0, 4, 18) == HH.TINY_K21_STATISTICS
    assert db.format_statistics(32, [1, 4], [3, 2], 3, 5, 11) == HH.K32_STATISTICS
    # above 32 the mask stays all ones: the same wrap
    assert "  missing  18446744073709551611  " in db.format_statistics(51, [1, 4], [3, 2], 3, 5, 11)
    assert "  missing  %20d  " % 11 in db.format_statistics(2, [1, 4], [3, 2], 3, 5, 11)
    # an empty histogram: the header and the titles only
    empty = db.format_statistics(21, [], [], 0, 0, 0)
    assert empty.count("\n") == 10 and empty.endswith("------------\n")
    # the length is reported whatever the buffer holds, and a short buffer is cut and terminated
    v = np.array([2, 7], dtype=np.uint64)
    n = native_lib.mdb_format_statistics(21, v.ctypes.data, v.ctypes.data, 2, 0, 4, 18, None, 0)
    assert n == len(db.format_statistics(21, [2, 7], [2, 7], 0, 4, 18))
    buf = ctypes.create_string_buffer(b"x" * 16, 16)
    assert native_lib.mdb_format_statistics(21, v.ctypes.data, v.ctypes.data, 2, 0, 4, 18, buf, 10) == n
    assert buf.raw[:10] == b"Number of\0" and buf.raw[10:] == b"x" * 6


def test_statistics_formatter_alone_under_the_sanitizers(native_lib, tmp_path):
    from meryl_amd import db
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "statistics_host")
    c = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        os.path.join(ROOT, "tests", "host", "statistics_host.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert c.returncode == 0, c.stderr
    rng = np.random.default_rng(7)
    cases = [(21, 0, 4, 18, [2, 7], [2, 2]), (32, 3, 5, 11, [1, 4], [3, 2]), (64, 0, 0, 0, [], []), (1, 1, 1, 1, [1], [1])]
    for k in (5, 31, 33):
        vals = np.unique(np.concatenate([rng.integers(1, 50, 30), rng.integers(1, 1 << 32, 30)])).astype(np.uint64)
        occ = rng.integers(1, 1 << 40, vals.size).astype(np.uint64)
        occ[0] = np.uint64(1 << 62)                                       # value * occurrences and the running sums wrap in uint64
        cases.append((k, int(occ[0]) if vals[0] == 1 else 0, int(occ.sum() & np.uint64(0xFFFFFFFFFFFFFFFF)), 1 << 63, vals.tolist(), occ.tolist()))
    lines = ["%d %d %d %d %d %s" % (k, u, d, t, len(v), " ".join("%d %d" % p for p in zip(v, o))) for k, u, d, t, v, o in cases]
    p = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    got = p.stdout.split("==\n")[:-1]
    assert len(got) == len(cases)
    assert got[0] == HH.TINY_K21_STATISTICS and got[1] == HH.K32_STATISTICS
    for (k, u, d, t, v, o), text in zip(cases, got):
        assert text == db.format_statistics(k, v, o, u, d, t), k


def test_accumulator_refuses_bad_arguments_without_a_device(native_lib):
    from meryl_amd import capi, db
    L = native_lib
    n = ctypes.c_uint64(7)

    def said(text):
        msg = L.mgc_db_stream_error(None)
        return msg is not None and text in msg
    assert L.mgc_value_hist_add(None, 4096, 8, None) == capi.MGC_EINVAL and said(b"NULL accumulator")
    assert L.mgc_value_hist_len(None, ctypes.byref(n)) == capi.MGC_EINVAL and L.mgc_value_hist_get(None, None, None) == capi.MGC_EINVAL
    assert L.mgc_value_hist_totals(None, None, None, None) == capi.MGC_EINVAL and said(b"mgc_value_hist_totals")
    h = L.mgc_value_hist_open(-1)
    assert h
    assert L.mgc_value_hist_add(h, None, 8, None) == capi.MGC_EINVAL and said(b"NULL array of 8 values")
    assert L.mgc_value_hist_add(h, 4098, 8, None) == capi.MGC_EINVAL and said(b"not aligned to 4 bytes")
    assert L.mgc_value_hist_len(h, None) == capi.MGC_EINVAL
    # nothing was added: an empty histogram, read without a device
    assert L.mgc_value_hist_add(h, None, 0, None) == 0
    assert L.mgc_value_hist_len(h, ctypes.byref(n)) == 0 and n.value == 0
    assert L.mgc_value_hist_get(h, None, None) == 0
    u, d, t = ctypes.c_uint64(9), ctypes.c_uint64(9), ctypes.c_uint64(9)
    assert L.mgc_value_hist_totals(h, ctypes.byref(u), ctypes.byref(d), ctypes.byref(t)) == 0 and (u.value, d.value, t.value) == (0, 0, 0)
    assert L.mgc_value_hist_totals(h, None, None, None) == 0
    L.mgc_value_hist_close(h)
    L.mgc_value_hist_close(None)
    vh = db.ValueHistogram()
    assert [a.tolist() for a in vh.get()] == [[], []] and vh.totals() == (0, 0, 0)
    vh.close()
    vh.close()


def test_eval_reported_refuses_before_the_device(native_lib, tmp_path):
    from meryl_amd import capi, db
    a, b, c = tiny_db(tmp_path / "a", 21), tiny_db(tmp_path / "b", 21), tiny_db(tmp_path / "c", 21)
    out = str(tmp_path / "out")
    before = sorted(os.listdir(tmp_path))
    arr, kids, n_kids, root, terms, n_terms, want = db.build_tree_reported(("union-sum", a, b, {"output": out, "histogram": True}))
    assert list(want) == [0, 0, 1] and root == 2

    def call(arr, want, hists, n_nodes=None):
        return native_lib.mgc_db_eval_reported(arr, len(arr) if n_nodes is None else n_nodes, kids, n_kids, root, terms, n_terms, 0, 0,
                                               ctypes.cast(None, capi.EVAL_SLICE_LABELLED_CB), None, -1, 2, want, hists)

    def refused(what, rc, text, hists=None):
        msg = native_lib.mgc_db_stream_error(None)
        assert rc == capi.MGC_EINVAL, (what, rc, msg)
        assert msg and b"mgc_db_eval_reported" in msg and text in msg, (what, msg)
        assert sorted(os.listdir(tmp_path)) == before, what
        assert hists is None or all(x is None for x in hists), what
    # a flagged node the root does not reach: a fourth node nobody names
    arr4 = (capi.EvalNodeAssigned * 4)()
    for i in range(3):
        ctypes.memmove(ctypes.byref(arr4[i]), ctypes.byref(arr[i]), ctypes.sizeof(capi.EvalNodeAssigned))
    arr4[3].kind, arr4[3].path = capi.NODE_DATABASE, c.encode()
    hists = (ctypes.c_void_p * 4)(1, 1, 1, 1)
    refused("an unreached node", call(arr4, (ctypes.c_uint8 * 4)(0, 0, 1, 1), hists), b"node 3: a histogram is wanted of a node the root does not reach", hists)
    hists = (ctypes.c_void_p * 3)(1, 1, 1)
    refused("nowhere to return it", call(arr, want, None), b"nowhere to return it")
    # what mgc_db_eval_assigned refuses is refused here in the same way, and no handle comes back
    arr[2].value_assign = 99
    refused("an unknown assign code", call(arr, want, hists), b"unknown value assignment", hists)
    arr[2].value_assign = 0
    arr[0].n_children = 1
    refused("a database with inputs", call(arr, want, hists), b"a database has no inputs", hists)
    with pytest.raises(ValueError):
        db.build_tree_reported(("union-sum", a, b, {"histograms": True}))
    with pytest.raises(ValueError):
        db.build_tree_reported(("union-sum", {"database": a, "output": out}, b))
    with pytest.raises(ValueError):
        db.build_tree_assigned(("union-sum", a, b, {"histogram": True}))
    # the flags follow the nodes: children before their parent, a database flagged through its dict
    got = db.build_tree_reported(("union-sum", {"database": a, "histogram": True}, ("at-least", 2, b, {"histogram": True}), c))
    assert list(got[6]) == [1, 0, 1, 0, 0] and got[3] == 4


@pytest.fixture(scope="module")
def meryl(native_lib):
    from meryl_amd import build
    path = build.build_cli()
    assert os.path.exists(path)
    return path


def run(meryl, *args):
    return subprocess.run([meryl] + [str(x) for x in args], capture_output=True, text=True, timeout=120)


def test_cli_reports_of_a_database_run_on_the_host(meryl, native_lib, tmp_path):
    a = tiny_db(tmp_path / "a", 21)
    p = run(meryl, "statistics", a)
    assert p.returncode == 0 and p.stdout == HH.TINY_K21_STATISTICS, p.stderr
    p = run(meryl, "-Q", "histogram", a)
    assert p.returncode == 0 and p.stdout == "2\t2\n7\t2\n", p.stderr
    a32 = tiny_db(tmp_path / "a32", 32)
    p = run(meryl, "statistics", a32)
    assert p.returncode == 0 and "Number of 32-mers" in p.stdout and "  missing  18446744073709551612  " in p.stdout, p.stderr


def test_cli_takes_a_report_of_an_operation_up_to_the_device(meryl, native_lib, tmp_path):
    a, b = tiny_db(tmp_path / "a", 21), tiny_db(tmp_path / "b", 21)
    before = sorted(os.listdir(tmp_path))
    for verb in ("histogram", "statistics"):
        p = run(meryl, verb, "[intersect", a, b + "]")
        # accepted: whatever stops it is the device (none here), not the command line
        assert "needs an 'output" not in p.stderr and "not part of this build" not in p.stderr and "Can't interpret" not in p.stderr, p.stderr
        assert p.returncode == 0 or "mgc_db_eval_reported" in p.stderr, p.stderr
    p = run(meryl, "print", "[union-sum", "output:histogram", "output:statistics=-", a, b + "]")
    assert "Can't interpret" not in p.stderr and (p.returncode == 0 or "mgc_db_eval_reported" in p.stderr), p.stderr
    assert sorted(os.listdir(tmp_path)) == before


def test_cli_refusals_and_their_messages(meryl, native_lib, tmp_path):
    a, b = tiny_db(tmp_path / "a", 21), tiny_db(tmp_path / "b", 21)
    before = sorted(os.listdir(tmp_path))
    f1, f2 = str(tmp_path / "one.hist"), str(tmp_path / "two.hist")
    p = run(meryl, "union-sum", "output:histogram=" + f1, "output:histogram=" + f2, a, b)
    assert p.returncode == 1 and "already has 'histogram' output to file '%s', can't add another output to file '%s'" % (f1, f2) in p.stderr, p.stderr
    p = run(meryl, "union-sum", "output:statistics", "output:stats=" + f2, a, b)
    assert p.returncode == 1 and "already has 'statistics' output to file '-', can't add another output to file '%s'" % f2 in p.stderr, p.stderr
    p = run(meryl, "output:histogram", a)
    assert p.returncode == 1 and "needs a set or value operation before it" in p.stderr, p.stderr
    p = run(meryl, "print", "output:histogram", a)
    assert p.returncode == 1 and "needs a set or value operation before it" in p.stderr, p.stderr
    p = run(meryl, "union-sum", "output:s", a, b)
    assert p.returncode == 1 and "is ambiguous; use output:show or output:stats" in p.stderr, p.stderr
    for word in ("output:show", "output:list=x", "output:database=x", "output:"):
        p = run(meryl, "union-sum", word, a, b)
        assert p.returncode == 1 and "only output:histogram[=file] and output:statistics[=file]" in p.stderr, (word, p.stderr)
    for verb in ("compare", "ploidy", "noise"):
        p = run(meryl, verb, a)
        assert p.returncode == 1 and "operation '%s' is not part of this build" % verb in p.stderr, p.stderr
    for verb in ("histogram", "statistics"):
        p = run(meryl, verb, a, b)
        assert p.returncode == 1 and "told to dump a histogram for more than one input" in p.stderr, p.stderr
    assert sorted(os.listdir(tmp_path)) == before
