"""meryl-import -labelwidth without a GPU: every function include/meryl_import_labelled.h declares is exported by the library
and bound in meryl_amd.capi, the entry points check their arguments before anything touches the device (on a box without a
GPU a device call would fail with a HIP message), and the command line refuses bad -labelwidth / -valuewidth with the usage
text.  include/meryl_import.h keeps its 13 functions."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "meryl_import_labelled.h")
OLD_HEADER = os.path.join(ROOT, "include", "meryl_import.h")


@pytest.fixture(scope="module")
def import_cli(native_lib):
    from meryl_amd import build
    return build.build_import_cli()


def declared_functions(header):
    src = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(mgc_[a-z0-9_]+)\s*\(", src)))


# ---- exports and bindings ----------------------------------------------------------------------------------------------
def test_header_functions_exported_and_bound(native_lib):
    from meryl_amd import capi, kmer_import
    names = declared_functions(HEADER)
    assert len(names) == 12, names
    assert names == sorted([
        "mgc_dev_import2_parse_state_bytes", "mgc_dev_import2_parse_workspace_bytes", "mgc_dev_import2_parse_begin",
        "mgc_dev_import2_parse_count", "mgc_dev_import2_parse", "mgc_dev_sort_triples_workspace_bytes", "mgc_dev_sort_triples",
        "mgc_dev_reduce_triples_workspace_bytes", "mgc_dev_reduce_triples_count", "mgc_dev_reduce_triples_emit",
        "mgc_import_labelled_file", "mgc_import_labelled_text"])
    assert not [n for n in names if not hasattr(native_lib, n)]
    assert set(names) <= set(capi.SYMBOLS), set(names) - set(capi.SYMBOLS)
    for n in names:                                   # bound: a signature is set, not the ctypes default
        assert getattr(native_lib, n).argtypes is not None, n
    for f in ("sort_triples", "reduce_triples"):
        assert hasattr(kmer_import, f)
    assert kmer_import.BAD_NAMES[5] == "label" and kmer_import.BAD_NAMES[6] == "assign"
    # the header includes the meryl 1 one for the shared types and says what it restates
    text = open(HEADER).read()
    assert '#include "meryl_import.h"' in text
    assert "meryl2-import/meryl-import.C" in text and "merylCountArray.C:381-400" in text and "reference.rst:615-617" in text
    # the meryl 1 header is as it was
    assert len(declared_functions(OLD_HEADER)) == 13
    assert "labelled" not in open(OLD_HEADER).read()


# ---- arguments are checked before the device ---------------------------------------------------------------------------
def test_entry_points_check_arguments_before_the_device(native_lib, tmp_path):
    from meryl_amd import capi
    L = native_lib
    info = capi.ImportInfo()
    out = str(tmp_path / "o.meryl").encode()
    text = b"ACGTAC 1 1\n"
    for lw in (0, 65):
        assert L.mgc_import_labelled_text(text, len(text), 6, 0, lw, out, -1, 1, ctypes.byref(info)) == capi.MGC_EINVAL
        assert b"label width" in L.mgc_import_error()
        assert L.mgc_import_labelled_file(b"/dev/null", 6, 0, lw, out, -1, 1, None) == capi.MGC_EINVAL
    for k in (5, 65):
        assert L.mgc_import_labelled_text(text, len(text), k, 0, 2, out, -1, 1, ctypes.byref(info)) == capi.MGC_EINVAL
        assert b"out of range" in L.mgc_import_error() and b"6-bit prefix" in L.mgc_import_error()
    assert L.mgc_import_labelled_text(text, len(text), 6, 3, 2, out, -1, 1, ctypes.byref(info)) == capi.MGC_EINVAL
    assert b"mode" in L.mgc_import_error()
    assert L.mgc_import_labelled_text(None, 9, 6, 0, 2, out, -1, 1, ctypes.byref(info)) == capi.MGC_EINVAL
    assert b"NULL text" in L.mgc_import_error()
    assert L.mgc_import_labelled_text(text, len(text), 6, 0, 2, None, -1, 1, None) == capi.MGC_EINVAL
    assert L.mgc_import_labelled_file(None, 21, 0, 2, out, -1, 1, None) == capi.MGC_EINVAL
    assert L.mgc_import_labelled_file(str(tmp_path / "missing.txt").encode(), 21, 0, 2, out, -1, 1, None) == capi.MGC_EINVAL
    assert b"cannot open" in L.mgc_import_error()
    assert not os.path.exists(out)

    # the device steps: bad k / label width / key words / bit ranges; n = 0 is MGC_OK without a launch (no device here)
    res = capi.ImportParseResult()
    plab = ctypes.c_uint64(0)
    assert L.mgc_dev_import2_parse_count(None, 0, 5, 2, None, None, 0, ctypes.byref(res), ctypes.byref(plab), None) == capi.MGC_EINVAL
    assert L.mgc_dev_import2_parse_count(None, 0, 21, 0, None, None, 0, ctypes.byref(res), ctypes.byref(plab), None) == capi.MGC_EINVAL
    assert L.mgc_dev_import2_parse_count(None, 0, 21, 65, None, None, 0, ctypes.byref(res), ctypes.byref(plab), None) == capi.MGC_EINVAL
    assert L.mgc_dev_import2_parse_count(None, 5, 21, 2, None, None, 0, ctypes.byref(res), ctypes.byref(plab), None) == capi.MGC_EINVAL
    assert L.mgc_dev_import2_parse(None, 5, 21, 3, 2, None, None, 0, None, None, None, None) == capi.MGC_EINVAL
    assert L.mgc_dev_import2_parse(None, 5, 65, 0, 2, None, None, 0, None, None, None, None) == capi.MGC_EINVAL
    assert L.mgc_dev_import2_parse_begin(None, None) == capi.MGC_EINVAL
    ia = ctypes.c_int(7)
    sort = L.mgc_dev_sort_triples
    assert sort(None, None, None, None, None, None, 5, 1, 10, 4, None, 0, ctypes.byref(ia), None) == capi.MGC_EINVAL
    assert sort(None, None, None, None, None, None, 5, 3, 0, 64, None, 0, ctypes.byref(ia), None) == capi.MGC_EINVAL
    assert sort(None, None, None, None, None, None, 5, 1, 0, 65, None, 0, ctypes.byref(ia), None) == capi.MGC_EINVAL
    assert sort(None, None, None, None, None, None, 0, 2, 0, 128, None, 0, ctypes.byref(ia), None) == capi.MGC_OK and ia.value == 0
    assert sort(None, None, None, None, None, None, 5, 1, 0, 42, None, 0, ctypes.byref(ia), None) == capi.MGC_EINVAL       # NULL buffers
    # the mechanism's limit is an error with a message, never a wrong result
    assert sort(None, None, None, None, None, None, 1 << 32, 1, 0, 42, None, 0, ctypes.byref(ia), None) == capi.MGC_EINVAL
    assert b"32-bit record numbers" in L.mgc_import_error()
    nd = ctypes.c_uint64(9)
    assert L.mgc_dev_reduce_triples_count(None, None, None, 5, 1, None, 0, ctypes.byref(nd), None) == capi.MGC_EINVAL
    assert L.mgc_dev_reduce_triples_count(None, None, None, 0, 3, None, 0, ctypes.byref(nd), None) == capi.MGC_EINVAL
    assert L.mgc_dev_reduce_triples_count(None, None, None, 0, 1, None, 0, ctypes.byref(nd), None) == capi.MGC_OK and nd.value == 0
    assert L.mgc_dev_reduce_triples_emit(None, None, None, 0, 1, 8, None, 0, None, None, None, None) == capi.MGC_OK
    assert L.mgc_dev_reduce_triples_emit(None, None, None, 0, 1, 0, None, 0, None, None, None, None) == capi.MGC_EINVAL
    assert L.mgc_dev_reduce_triples_emit(None, None, None, 0, 1, 65, None, 0, None, None, None, None) == capi.MGC_EINVAL
    assert L.mgc_dev_reduce_triples_emit(None, None, None, 5, 1, 8, None, 0, None, None, None, None) == capi.MGC_EINVAL

    prev = [0, 0, 0]
    for n in (0, 1, 4096, 10 ** 6, 10 ** 9):
        sizes = [L.mgc_dev_sort_triples_workspace_bytes(n), L.mgc_dev_reduce_triples_workspace_bytes(n),
                 L.mgc_dev_import2_parse_workspace_bytes(n)]
        for i, w in enumerate(sizes):
            assert w > 0 and w >= prev[i]
        # the triple sort holds the pair sort's workspace and two arrays of record numbers
        assert sizes[0] >= L.mgc_dev_sort_pairs_workspace_bytes(n) + 8 * n
        prev = sizes
    # both persistent words and the chunk's: more than the meryl 1 state
    assert L.mgc_dev_import2_parse_state_bytes() >= L.mgc_dev_import_parse_state_bytes() + 16


def test_python_arguments_exist(native_lib):
    import inspect
    from meryl_amd import kmer_import
    for f in (kmer_import.import_file, kmer_import.import_text, kmer_import.Parser.__init__):
        p = inspect.signature(f).parameters
        assert "label_width" in p and p["label_width"].default == 0
    assert list(inspect.signature(kmer_import.Parser.__init__).parameters)[1:4] == ["k", "mode", "label_width"]
    assert list(inspect.signature(kmer_import.sort_triples).parameters) == ["keys", "values", "labels", "begin_bit", "end_bit"]
    assert list(inspect.signature(kmer_import.reduce_triples).parameters) == ["keys", "values", "labels", "label_width"]


# ---- command line ------------------------------------------------------------------------------------------------------
def _kmers_file(tmp_path, name="in.txt"):
    p = tmp_path / name
    p.write_bytes(b"ACGTACGTACGTACGTACGTA 3 1\n")
    return p


def refused(import_cli, tmp_path, args, needle):
    out = tmp_path / "out.meryl"
    p = subprocess.run([import_cli] + [str(a).replace("@OUT@", str(out)) for a in args], capture_output=True, timeout=120)
    err = p.stderr.decode()
    assert p.returncode == 1, (p.returncode, err)
    assert err.startswith("usage: "), err
    assert needle in err, err
    # nothing reached the device or the output path: no HIP message, no directory
    assert "HIP" not in err, err
    assert not os.path.exists(out)
    return err


def test_labelwidth_65_is_refused(import_cli, tmp_path):
    refused(import_cli, tmp_path, ["-k", 21, "-kmers", _kmers_file(tmp_path), "-output", "@OUT@", "-labelwidth", 65], "(-labelwidth) '65'")


def test_labelwidth_not_a_number_is_refused(import_cli, tmp_path):
    refused(import_cli, tmp_path, ["-k", 21, "-kmers", _kmers_file(tmp_path), "-output", "@OUT@", "-labelwidth", "x"], "(-labelwidth) 'x'")


def test_labelwidth_as_the_last_word_is_refused(import_cli, tmp_path):
    refused(import_cli, tmp_path, ["-k", 21, "-kmers", _kmers_file(tmp_path), "-output", "@OUT@", "-labelwidth"],
            "Option '-labelwidth' needs a value.")


def test_valuewidth_3_is_refused(import_cli, tmp_path):
    refused(import_cli, tmp_path, ["-k", 21, "-kmers", _kmers_file(tmp_path), "-output", "@OUT@", "-valuewidth", 3, "-labelwidth", 2],
            "(-valuewidth) '3'")


def test_multiset_stays_refused_with_labelwidth(import_cli, tmp_path):
    err = refused(import_cli, tmp_path, ["-k", 21, "-kmers", _kmers_file(tmp_path), "-output", "@OUT@", "-labelwidth", 2, "-multiset"],
                  "Option '-multiset' is not part of this build.")
    assert "Unknown option" not in err and "(-labelwidth)" not in err          # -labelwidth 2 itself is fine


def test_valuewidth_0_and_labelwidth_are_accepted(import_cli, tmp_path):
    err = refused(import_cli, tmp_path, ["-kmers", _kmers_file(tmp_path), "-output", "@OUT@", "-valuewidth", 0, "-labelwidth", 2],
                  "No kmer size (-k) supplied.")
    assert "Unknown option" not in err and "(-labelwidth)" not in err and "(-valuewidth)" not in err
    assert err.count("supplied.") == 1                 # -k is the only complaint
    # the usage names the option and the dialect
    assert "-labelwidth <lw>" in err and "value=<n>" in err and "label=<n>" in err and "1111011b" in err and "modulo 2^lw" in err
