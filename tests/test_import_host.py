"""meryl-import without a GPU: the binary builds, its command line is checked before anything touches the device (on a box
without a GPU a device call would fail with a HIP message instead of the usage text), and every function
include/meryl_import.h declares is exported by the library and bound in meryl_amd.capi."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "meryl_import.h")


@pytest.fixture(scope="module")
def import_cli(native_lib):
    from meryl_amd import build
    return build.build_import_cli()


def run_import(cli, args, stdin=None):
    return subprocess.run([cli] + [str(a) for a in args], capture_output=True, input=stdin, timeout=120)


def test_build_import_cli_yields_the_binary(import_cli):
    assert os.path.isfile(import_cli) and os.access(import_cli, os.X_OK)
    assert os.path.basename(import_cli) == "meryl-import"
    assert os.path.dirname(import_cli) == os.path.join(ROOT, "meryl_amd", "bin")


def _kmers_file(tmp_path, name="in.txt"):
    p = tmp_path / name
    p.write_bytes(b"ACGTACGTACGTACGTACGTA 3\n")
    return p


def refused(import_cli, tmp_path, args, needle):
    out = tmp_path / "out.meryl"
    p = run_import(import_cli, [str(a).replace("@OUT@", str(out)) for a in args])
    err = p.stderr.decode()
    assert p.returncode == 1, (p.returncode, err)
    assert err.startswith("usage: "), err
    assert needle in err, err
    # nothing reached the device or the output path: no HIP message, no directory
    assert "HIP" not in err, err
    assert not os.path.exists(out)
    return err


def test_no_arguments_prints_usage(import_cli, tmp_path):
    err = refused(import_cli, tmp_path, [], "No input kmer file (-kmers) supplied.")
    assert "No output database name (-output) supplied." in err and "No kmer size (-k) supplied." in err
    assert "right-most" in err                      # the usage says which bases of a longer word are used


def test_missing_k(import_cli, tmp_path):
    refused(import_cli, tmp_path, ["-kmers", _kmers_file(tmp_path), "-output", "@OUT@"], "No kmer size (-k) supplied.")


def test_unknown_option(import_cli, tmp_path):
    refused(import_cli, tmp_path, ["-k", 21, "-kmers", _kmers_file(tmp_path), "-output", "@OUT@", "-frobnicate"],
            "Unknown option '-frobnicate'.")


def test_multiset_is_refused(import_cli, tmp_path):
    refused(import_cli, tmp_path, ["-k", 21, "-kmers", _kmers_file(tmp_path), "-output", "@OUT@", "-multiset"],
            "not part of this build")


@pytest.mark.parametrize("k", [5, 65])
def test_k_out_of_range(import_cli, tmp_path, k):
    refused(import_cli, tmp_path, ["-k", k, "-kmers", _kmers_file(tmp_path), "-output", "@OUT@"], "is outside 6..64")


def test_bz2_input_is_refused_by_suffix(import_cli, tmp_path):
    refused(import_cli, tmp_path, ["-k", 21, "-kmers", _kmers_file(tmp_path, "in.txt.bz2"), "-output", "@OUT@"],
            "other than gzip")


def test_hint_options_take_their_values(import_cli, tmp_path):
    # -threads / -maxvalue / -memory are accepted with a value each: the only complaint left is the missing -k
    err = refused(import_cli, tmp_path, ["-kmers", _kmers_file(tmp_path), "-output", "@OUT@", "-threads", 4, "-maxvalue", 100,
                                         "-memory", 8, "-forward"], "No kmer size (-k) supplied.")
    assert "Unknown option" not in err


def declared_functions():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(mgc_[a-z0-9_]+)\s*\(", src)))


def test_header_functions_exported_and_bound(native_lib):
    from meryl_amd import capi
    names = declared_functions()
    assert len(names) == 13, names
    assert not [n for n in names if not hasattr(native_lib, n)]
    assert set(names) <= set(capi.SYMBOLS), set(names) - set(capi.SYMBOLS)
    for n in names:                                   # bound: a signature is set, not the ctypes default
        assert getattr(native_lib, n).argtypes is not None, n
    from meryl_amd import kmer_import
    for f in ("import_file", "import_text", "Parser", "sort_pairs", "reduce_pairs"):
        assert hasattr(kmer_import, f)


def test_entry_points_check_arguments_before_the_device(native_lib, tmp_path):
    from meryl_amd import capi
    L = native_lib
    info = capi.ImportInfo()
    out = str(tmp_path / "o.meryl").encode()
    for k in (0, 5, 65):
        assert L.mgc_import_text(b"ACGTAC 1\n", 9, k, 0, out, -1, 1, ctypes.byref(info)) == capi.MGC_EINVAL
        assert b"out of range" in L.mgc_import_error()
    assert L.mgc_import_text(b"ACGTAC 1\n", 9, 6, 3, out, -1, 1, ctypes.byref(info)) == capi.MGC_EINVAL
    assert L.mgc_import_text(None, 9, 6, 0, out, -1, 1, ctypes.byref(info)) == capi.MGC_EINVAL
    assert L.mgc_import_file(None, 21, 0, out, -1, 1, None) == capi.MGC_EINVAL
    assert L.mgc_import_file(str(tmp_path / "missing.txt").encode(), 21, 0, out, -1, 1, None) == capi.MGC_EINVAL
    assert b"cannot open" in L.mgc_import_error()
    assert not os.path.exists(out)
    ia = ctypes.c_int(7)
    assert L.mgc_dev_sort_pairs(None, None, None, None, 5, 1, 10, 4, None, 0, ctypes.byref(ia), None) == capi.MGC_EINVAL
    assert L.mgc_dev_sort_pairs(None, None, None, None, 5, 3, 0, 64, None, 0, ctypes.byref(ia), None) == capi.MGC_EINVAL
    assert L.mgc_dev_sort_pairs(None, None, None, None, 5, 1, 0, 65, None, 0, ctypes.byref(ia), None) == capi.MGC_EINVAL
    assert L.mgc_dev_sort_pairs(None, None, None, None, 0, 2, 0, 128, None, 0, ctypes.byref(ia), None) == capi.MGC_OK and ia.value == 0
    assert L.mgc_dev_sort_pairs(None, None, None, None, 5, 1, 0, 42, None, 0, ctypes.byref(ia), None) == capi.MGC_EINVAL   # NULL buffers
    nd = ctypes.c_uint64(0)
    assert L.mgc_dev_reduce_pairs_count(None, None, 5, 1, None, 0, ctypes.byref(nd), None) == capi.MGC_EINVAL
    res = capi.ImportParseResult()
    assert L.mgc_dev_import_parse_count(None, 5, 21, None, None, 0, ctypes.byref(res), None) == capi.MGC_EINVAL
    assert L.mgc_dev_import_parse_count(None, 0, 5, None, None, 0, ctypes.byref(res), None) == capi.MGC_EINVAL
    prev = 0
    for n in (0, 1, 4096, 10 ** 6, 10 ** 9):
        for f in (L.mgc_dev_sort_pairs_workspace_bytes, L.mgc_dev_reduce_pairs_workspace_bytes, L.mgc_dev_import_parse_workspace_bytes):
            assert f(n) > 0
        w = L.mgc_dev_sort_pairs_workspace_bytes(n)
        assert w >= prev
        prev = w
    assert L.mgc_dev_import_parse_state_bytes() >= 48
