"""Build recipe for the native library (gfx950 only, in-tree).

    python -m meryl_amd.build            # builds meryl_amd/libmeryl_gpu_count.so

hipcc cross-compiles for gfx950 without a GPU.  The built .so stays in-tree
(git-ignored) so that it travels with the source snapshot to the GPU box.
"""
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libmeryl_gpu_count.so")
SOURCES = ["mgc_kmer.hip", "mgc_sort.hip", "mgc_scan.hip", "mgc_finish.hip", "mgc_misc.hip", "mgc_parse.hip",
           "mgc_encode.hip", "mgc_decode.hip", "mgc_merge.hip", "mgc_merge_many.hip", "mgc_lookup.hip", "mgc_filter.hip", "mgc_import.hip", "mgc_analyze.hip", "mgc_value_hist.hip", "mgc_positions.hip", "mgc_list.hip", "mgc_bam.hip", "mgc_gzip.hip",
           "mgc_api.cpp", "mgc_input.cpp", "mgc_textfile.cpp", "mgc_import.cpp", "mgc_analyze.cpp", "mgc_dbfile.cpp", "mgc_positions.cpp", "mgc_count.cpp", "mgc_stream.cpp", "mgc_eval.cpp", "mgc_runs.cpp", "mgc_node.cpp", "meryl_db.cpp", "meryl_seq.cpp"]
HEADERS = ["mgc_device.h", "mgc_common.hpp", "mgc_compact.hpp", "mgc_bases.hpp", "mgc_stream_geom.hpp", "mdb_layout.h", "mdb_statistics.hpp", "mgc_session.hpp", "mgc_devbuf.hpp", "mgc_dbfile.hpp", "mgc_hist_list.hpp", "mgc_clock.hpp", "mgc_chunk_ring.hpp", "mgc_bgzf.hpp", "mgc_bam_walk.hpp", "mgc_gzip_par.hpp", "mgc_gzip_crc.hpp", "mgc_input.hpp", "mgc_runs.hpp", "mgc_lookup_dev.hpp", "mgc_import_dev.hpp", "mgc_analyze_dev.hpp", "mgc_positions_dev.hpp", "mgc_fastx.hpp", "mgc_label.hpp", "mgc_selector.hpp", "mgc_value.hpp", "mgc_route.hpp", "mgc_group_route.hpp", "mgc_group_batch.hpp", "mgc_pack_plan.hpp", "mgc_list.hpp",
           os.path.join("..", "..", "include", "meryl_gpu_count.h"),
           os.path.join("..", "..", "include", "meryl_db.h"), os.path.join("..", "..", "include", "meryl_seq.h"),
           os.path.join("..", "..", "include", "meryl_lookup.h"), os.path.join("..", "..", "include", "meryl_import.h"),
           os.path.join("..", "..", "include", "meryl_import_labelled.h"),
           os.path.join("..", "..", "include", "meryl_analyze.h"), os.path.join("..", "..", "include", "meryl_positions.h"),
           os.path.join("..", "..", "include", "meryl_list.h")]
OBJDIR = os.path.join(HERE, "build")
# -no-hip-rt: the library carries no DT_NEEDED on a particular libamdhip64; it binds to the
# HIP runtime already in the process (torch's bundled one under Python -- two HIP/HSA runtimes
# in one process cannot share streams or ordering -- or /opt/rocm's for the standalone CLI).
CFLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-pthread", "-Wall", "-Wno-unused-function"]
LFLAGS = ["--offload-arch=gfx950", "-shared", "-fPIC", "-pthread", "-no-hip-rt"]


def hipcc():
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found: the native library cannot be built")


def _sources():
    return [f for f in SOURCES if os.path.exists(os.path.join(CSRC, f))]


def _header_mtime():
    deps = [os.path.join(CSRC, f) for f in HEADERS if os.path.exists(os.path.join(CSRC, f))]
    deps.append(os.path.abspath(__file__))
    return max(os.path.getmtime(d) for d in deps)


def _obj(f):
    return os.path.join(OBJDIR, f + ".o")


def _stale_objects(force=False):
    """sources whose object is missing or older than the source / any header"""
    ht = _header_mtime()
    out = []
    for f in _sources():
        o = _obj(f)
        if force or not os.path.exists(o) or os.path.getmtime(o) < max(os.path.getmtime(os.path.join(CSRC, f)), ht):
            out.append(f)
    return out


def _stale():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    if max([_header_mtime()] + [os.path.getmtime(os.path.join(CSRC, f)) for f in _sources()]) <= t:
        return False                                      # newer than every source and header: current, with or without its objects
    if _stale_objects():
        return True
    return any(os.path.getmtime(_obj(f)) > t for f in _sources())


CLI = os.path.join(HERE, "bin", "meryl")
LOOKUP_CLI = os.path.join(HERE, "bin", "meryl-lookup")
IMPORT_CLI = os.path.join(HERE, "bin", "meryl-import")
ANALYZE_CLI = os.path.join(HERE, "bin", "meryl-analyze")
POSITION_LOOKUP_CLI = os.path.join(HERE, "bin", "position-lookup")


def _build_front_end(source, out, force, verbose, headers=()):
    """One front end (meryl_amd/bin/*): links the library and the system HIP runtime.  headers: what it includes from csrc/."""
    src = os.path.join(CSRC, source)
    newest = max(os.path.getmtime(os.path.join(CSRC, f)) for f in (source,) + tuple(headers))
    if (not force and os.path.exists(out) and os.path.getmtime(out) >= newest
            and os.path.getmtime(out) >= os.path.getmtime(LIB)):
        return out
    os.makedirs(os.path.dirname(out), exist_ok=True)
    rocm_lib = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib")
    tmp = "%s.tmp%d" % (out, os.getpid())             # several ranks may build at once: private file, atomic rename
    cmd = [hipcc(), "-O2", "-std=c++17", "-pthread", src, "-o", tmp, "-L" + HERE, "-lmeryl_gpu_count",
           "-Wl,-rpath,$ORIGIN/..", "-L" + rocm_lib, "-lamdhip64", "-Wl,-rpath," + rocm_lib, "-lz"]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.check_call(cmd)
    os.replace(tmp, out)
    return out


def build_cli(force=False, verbose=False):
    """The `meryl` front end (meryl_amd/bin/meryl)."""
    return _build_front_end("meryl_main.cpp", CLI, force, verbose)


def build_lookup_cli(force=False, verbose=False):
    """`meryl-lookup` (meryl_amd/bin/meryl-lookup: -existence and the position reports)."""
    return _build_front_end("meryl_lookup_main.cpp", LOOKUP_CLI, force, verbose, ("mgc_fastx.hpp",))


def build_import_cli(force=False, verbose=False):
    """`meryl-import` (meryl_amd/bin/meryl-import: `kmer value` text -> database)."""
    return _build_front_end("meryl_import_main.cpp", IMPORT_CLI, force, verbose)


def build_analyze_cli(force=False, verbose=False):
    """`meryl-analyze` (meryl_amd/bin/meryl-analyze: -gc / -ga / -gt histograms of a database)."""
    return _build_front_end("meryl_analyze_main.cpp", ANALYZE_CLI, force, verbose)


def build_position_lookup_cli(force=False, verbose=False):
    """`position-lookup` (meryl_amd/bin/position-lookup: -hpq / -mpb / -qpb of query sequences against a reference)."""
    return _build_front_end("position_lookup_main.cpp", POSITION_LOOKUP_CLI, force, verbose, ("mgc_fastx.hpp",))


def build(force=False, verbose=False):
    """Compile every HIP/C++ source for gfx950 (one object per source, rebuilt only when the source or a
    header changed, in parallel) and link libmeryl_gpu_count.so (and the CLI).  Returns the library path."""
    if not force and not _stale():
        build_cli(False, verbose)
        build_lookup_cli(False, verbose)
        build_import_cli(False, verbose)
        build_analyze_cli(False, verbose)
        build_position_lookup_cli(False, verbose)
        return LIB
    os.makedirs(OBJDIR, exist_ok=True)
    todo = _stale_objects(force)
    procs = []
    for f in todo:
        tmp = "%s.tmp%d" % (_obj(f), os.getpid())
        cmd = [hipcc()] + CFLAGS + ["-c", os.path.join(CSRC, f), "-o", tmp]
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        procs.append((f, tmp, cmd, subprocess.Popen(cmd)))
    failed = []
    for f, tmp, cmd, p in procs:
        if p.wait() != 0:
            failed.append(f)
        else:
            os.replace(tmp, _obj(f))
    if failed:
        raise subprocess.CalledProcessError(1, "hipcc -c " + " ".join(failed))
    tmp = "%s.tmp%d" % (LIB, os.getpid())
    cmd = [hipcc()] + LFLAGS + ["-o", tmp] + [_obj(f) for f in _sources()] + ["-lz"]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.check_call(cmd)
    os.replace(tmp, LIB)
    build_cli(True, verbose)
    build_lookup_cli(True, verbose)
    build_import_cli(True, verbose)
    build_analyze_cli(True, verbose)
    build_position_lookup_cli(True, verbose)
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
