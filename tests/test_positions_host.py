"""What include/meryl_positions.h and the position-lookup front end do without a device: the exported symbols, the argument
errors that return before any device work, the front end's refusals (src/meryl-lookup/position-lookup.C:398-423), and
meryl-lookup's usage text after its FASTA/FASTQ parser moved into a header shared with position-lookup."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "meryl_positions.h")


def declared_functions():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(mgc_[a-z0-9_]+)\s*\(", src)))


def test_header_symbols_exported_and_listed(native_lib):
    from meryl_amd import capi
    names = declared_functions()
    assert names == sorted(["mgc_posidx_build", "mgc_posidx_free", "mgc_posidx_get_info", "mgc_posidx_arrays", "mgc_posidx_find",
                            "mgc_paint_open", "mgc_paint_add", "mgc_paint_get", "mgc_paint_close"])
    assert not [n for n in names if not hasattr(native_lib, n)]
    assert set(names) <= set(capi.SYMBOLS), set(names) - set(capi.SYMBOLS)
    for n in names:                                            # every one has its prototype in the binding
        assert getattr(native_lib, n).argtypes is not None, n


def test_sources_are_in_the_build_recipe():
    from meryl_amd import build
    assert "mgc_positions.hip" in build.SOURCES and "mgc_positions.cpp" in build.SOURCES
    assert "mgc_positions_dev.hpp" in build.HEADERS and any(h.endswith("meryl_positions.h") for h in build.HEADERS)
    assert os.path.basename(build.build_position_lookup_cli()) == "position-lookup"


def test_argument_errors_touch_no_device(native_lib):
    """this box has no GPU: anything that got past the checks would fail with a HIP error instead"""
    from meryl_amd import capi
    L = native_lib

    def err():
        return L.mgc_lookup_error().decode()

    assert not L.mgc_posidx_build(None, None, 0, None) and "mgc_posidx_build: no lookup table" in err()
    info = capi.PosIndexInfo()
    assert L.mgc_posidx_get_info(None, ctypes.byref(info)) == capi.MGC_EINVAL and "mgc_posidx_get_info" in err()
    assert L.mgc_posidx_arrays(None, None, None, None) == capi.MGC_EINVAL and "mgc_posidx_arrays: no index" in err()
    assert L.mgc_posidx_find(None, None, 0, None, None, None) == capi.MGC_EINVAL and "mgc_posidx_find: no index" in err()
    assert not L.mgc_paint_open(None, 7) and "mgc_paint_open: no index" in err()
    assert L.mgc_paint_add(None, None, 0, None, 0, None, None, None) == capi.MGC_EINVAL and "mgc_paint_add: no painter" in err()
    assert L.mgc_paint_get(None, 2, None, None) == capi.MGC_EINVAL and "mgc_paint_get: no painter" in err()
    L.mgc_posidx_free(None)
    L.mgc_paint_close(None)


def run_position_lookup(args):
    from meryl_amd import build
    return subprocess.run([build.build_position_lookup_cli()] + [str(a) for a in args], capture_output=True)


def test_front_end_refusals(native_lib, tmp_path):
    q = tmp_path / "q.fa"
    q.write_text(">a\nACGT\n")
    db, ref = tmp_path / "missing.meryl", tmp_path / "missing.fa"
    cases = [
        (["-s", ref, "-hpq", tmp_path / "h", q], "No meryl database (-m) supplied."),
        (["-m", db, "-hpq", tmp_path / "h", q], "No reference sequence (-s) supplied."),
        (["-m", db, "-s", ref, q], "No output (-hpq, -mpb, -qpb) supplied."),
        (["-m", db, "-s", ref, "-mpb", tmp_path / "o.gz", q],
         "ERROR: output '%s' names a compressed file; this build writes position reports uncompressed only." % (tmp_path / "o.gz")),
        (["-m", db, "-s", ref, "-qpb", tmp_path / "o.zst", q], "names a compressed file"),
        (["-m", db, "-s", ref, "-hpq", tmp_path / "h", q, "nonesuch"], "unknown option 'nonesuch'\n"),
        (["-m", db, "-s", ref, "-hpq", tmp_path / "h", "-window", "5", q], "unknown option '-window'\n"),
    ]
    for args, msg in cases:
        p = run_position_lookup(args)
        assert p.returncode == 1 and msg in p.stderr.decode(), (args, p.stderr)
        assert "Loading" not in p.stderr.decode()             # refused before the database was touched
    assert not list(tmp_path.glob("o.*")) and not (tmp_path / "h").exists()


def test_meryl_lookup_usage_unchanged(native_lib, tmp_path):
    """the parser's move into mgc_fastx.hpp left meryl-lookup as it was: same usage text, same refusals, same parse error"""
    from meryl_amd import build
    exe = build.build_lookup_cli()
    p = subprocess.run([exe, "-bed"], capture_output=True)
    want = ("usage: %s -existence | -bed | -bed-runs | -wig-count | -wig-depth -sequence <in.fa|fq[.gz]> -mers <db.meryl> [...] "
            "[-labels l ...] [-min v] [-max v] [-memory GB] [-estimate] [-output out]\n"
            "       %s -include | -exclude [-10x] -sequence <in1> [<in2>] -mers <db.meryl> [-min v] [-max v] -output <out1> [<out2>]\n" % (exe, exe))
    assert p.returncode == 1 and p.stderr.decode() == want and p.stdout == b""
    p = subprocess.run([exe, "-bed", "-frobnicate"], capture_output=True)
    assert p.returncode == 1 and p.stderr.decode() == "ERROR: unknown option '-frobnicate'.\n"
