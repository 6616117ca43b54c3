"""The host side of the parallel gzip reader (meryl_amd/csrc/mgc_gzip_par.hpp: inflater with markers, block finder, chunk
plan, confirmation, cuts, members) in a stand-alone program (tests/host/gzip_host.cpp) that resolves the markers on the CPU,
built plain, with the thread sanitizer and with the address + undefined-behaviour sanitizers.  The sanitizer runtimes are linked
statically into the program: nothing sanitized is loaded into Python, nothing is preloaded.

The files come from Python's zlib (tests/gzip_cases.py), the expected values from zlib.crc32."""
import os
import shutil
import subprocess
import sys
import zlib

import pytest

sys.path.insert(0, os.path.dirname(__file__))
import gzip_cases as gc  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host", "gzip_host.cpp")
VARIANTS = {
    "plain": [],
    "thread": ["-fsanitize=thread", "-static-libtsan"],
    "address_undefined": ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"],
}
HELLO = """#include <thread>
int main() { int x = 0; std::thread t([&] { x = 1; }); t.join(); return x - 1; }
"""
TIMEOUT = 60                                     # seconds: a pump that hangs fails here, it does not hold the suite up
THREADS = 4


def _compile(flags, src, out):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    return subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-pthread"] + flags + [src, "-o", out, "-lz"],
                          capture_output=True, text=True, timeout=300)


@pytest.fixture(scope="module", params=list(VARIANTS))
def program(request, tmp_path_factory):
    """the program built one way; a sanitized build is skipped only where a hello-threads program built the same way does not work"""
    d = tmp_path_factory.mktemp("gzip_host_" + request.param)
    flags = VARIANTS[request.param]
    if flags:
        hello = str(d / "hello.cpp")
        open(hello, "w").write(HELLO)
        c = _compile(flags, hello, str(d / "hello"))
        if c.returncode != 0 or subprocess.run([str(d / "hello")], capture_output=True, timeout=TIMEOUT).returncode != 0:
            pytest.skip("this machine cannot build or run a %s program" % " ".join(flags))
    exe = str(d / "gzip_host")
    c = _compile(flags, SRC, exe)
    assert c.returncode == 0, c.stderr
    return exe


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("gzip_files")
    paths = {}
    for name, (data, _, _) in gc.good_files().items():
        paths[name] = d / (name + ".gz")
        paths[name].write_bytes(data)
    for name, data in gc.damaged_files().items():
        paths[name] = d / (name + ".gz")
        paths[name].write_bytes(data)
    return paths


def _run(program, path, span=gc.SPAN, cap=gc.CAP, threads=THREADS, *force):
    p = subprocess.run([program, str(path), str(span), str(cap), str(threads)] + [str(a) for a in force],
                       capture_output=True, text=True, timeout=TIMEOUT)
    assert p.returncode == 0, p.stdout + p.stderr
    return dict(kv.split("=", 1) for kv in p.stdout.split())


def _exact(f, name):
    _, text, members = gc.good_files()[name]
    assert f["status"] == "ok", f
    assert (int(f["len"]), int(f["crc"]), int(f["members"])) == (len(text), zlib.crc32(text) & 0xffffffff, members), f


@pytest.mark.parametrize("name", ["level1", "level6", "level9"])
def test_every_span_is_inflated_by_its_own_worker(program, files, name):
    f = _run(program, files[name])
    _exact(f, name)
    spans = len(gc.good_files()[name][0]) // gc.SPAN
    assert int(f["chunks"]) >= 4 and int(f["chunks"]) == spans + int(f["cuts"])
    assert int(f["confirmed"]) == int(f["chunks"]) - 1 - int(f["cuts"]), f
    assert int(f["discarded"]) == 0 and int(f["symbol_bytes"]) > 0


def test_fixed_blocks_inflate_serially_and_exactly(program, files):
    f = _run(program, files["fixed"])
    _exact(f, "fixed")
    assert int(f["confirmed"]) == 0                                    # (a candidate the finder believed in is discarded, not confirmed)


@pytest.mark.parametrize("name", ["stored", "full_flush", "sync_flush", "three_members", "header_flags", "trailing_bytes"])
def test_block_kinds_flush_points_members_and_header_flags(program, files, name):
    f = _run(program, files[name])
    _exact(f, name)
    assert int(f["confirmed"]) >= 1                                    # stored blocks and flush points are found as well


def test_member_that_ends_just_before_a_chunk_start(program, files):
    f = _run(program, files["near_chunk"])
    _exact(f, "near_chunk")
    assert int(f["confirmed"]) == int(f["chunks"]) - 1
    assert 0 < int(f["min_window"]) < 32768, f                         # the piece of span 1 has less than a whole window behind it


def test_one_thread_and_more_threads_than_spans(program, files):
    for threads in (1, 16):
        f = _run(program, files["level6"], gc.SPAN, gc.CAP, threads)
        _exact(f, "level6")
        assert int(f["confirmed"]) == int(f["chunks"]) - 1


def test_a_false_candidate_is_discarded(program, files):
    f = _run(program, files["level6"], gc.SPAN, gc.CAP, THREADS, 2, 2 * gc.SPAN * 8 + 12345)
    _exact(f, "level6")
    assert int(f["discarded"]) == 1 and int(f["confirmed"]) == int(f["chunks"]) - 2, f


@pytest.mark.parametrize("name", ["level6", "fixed", "three_members"])
def test_a_small_cap_forces_cuts(program, files, name):
    f = _run(program, files[name], gc.SPAN, gc.SMALL_CAP)
    _exact(f, name)
    assert int(f["cuts"]) >= 4 and int(f["max_piece"]) <= gc.SMALL_CAP
    if name == "level6":
        assert int(f["confirmed"]) == int(f["chunks"]) - 1 - int(f["cuts"])


@pytest.mark.parametrize("cap", [100_000, gc.SMALL_CAP])
def test_a_head_task_that_falls_behind_is_never_starved_of_slots(program, files, cap):
    # 16 workers and 20 slots, tasks of three and more pieces, and the worker of span 0 sleeps before every slot it takes: the others
    # run ahead and take every slot they may.  (With one slot kept back for the head, not lag + 1, this hung.)
    f = _run(program, files["level1"], gc.SPAN, cap, 16, -1, 0, 30)
    _exact(f, "level1")
    spans = int(f["chunks"]) - int(f["cuts"])
    assert int(f["cuts"]) >= (3 if cap == 100_000 else 1) * (spans - 1)        # tasks of four and more pieces / of two


def test_spans_without_a_block_start(program, files):
    f = _run(program, files["level6"], gc.SMALL_SPAN)
    _exact(f, "level6")
    assert int(f["discarded"]) + int(f["confirmed"]) < int(f["chunks"])
    assert int(f["confirmed"]) >= 1


def test_a_block_that_no_slot_holds_refuses_the_file(program, files):
    f = _run(program, files["level6"], gc.SPAN, 20_000)
    assert f["status"] == "format", f


@pytest.mark.parametrize("name,status", [("flipped_bit", ("format", "crc", "marker")), ("cut_in_block", ("format",)),
                                         ("cut_in_trailer", ("format",)), ("wrong_isize", ("isize",))])
def test_damaged_files_are_refused(program, files, name, status):
    f = _run(program, files[name])
    assert f["status"] in status, f
    if name == "cut_in_trailer":
        assert int(f["off"]) == len(gc.damaged_files()[name]) - 3      # where the trailer starts
