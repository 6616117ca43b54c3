"""The CRC ledger of the gzip input route (meryl_amd/csrc/mgc_gzip_crc.hpp: the table of CRC entries of a piece, crc32_combine_4096,
the fold of the device's values into the members' CRCs, the trailer checks and the verdicts) in a stand-alone program
(tests/host/gzip_crc_host.cpp) that plays the device with zlib's crc32, built plain and with the address + undefined-behaviour
sanitizers.  The sanitizer runtimes are linked statically into the program: nothing sanitized is loaded into Python, nothing is
preloaded.  The ledger is single-threaded, so there is no thread-sanitizer variant."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host", "gzip_crc_host.cpp")
VARIANTS = {
    "plain": [],
    "address_undefined": ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"],
}
HELLO = """#include <vector>
int main(int argc, char **) { std::vector<int> v(argc, 1); return v[0] - 1; }
"""
TIMEOUT = 60


def _compile(flags, src, out):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    return subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-pthread"] + flags + [src, "-o", out, "-lz"],
                          capture_output=True, text=True, timeout=300)


@pytest.fixture(scope="module", params=list(VARIANTS))
def program(request, tmp_path_factory):
    """the program built one way; a sanitized build is skipped only where a hello program built the same way does not work"""
    d = tmp_path_factory.mktemp("gzip_crc_host_" + request.param)
    flags = VARIANTS[request.param]
    if flags:
        hello = str(d / "hello.cpp")
        open(hello, "w").write(HELLO)
        c = _compile(flags, hello, str(d / "hello"))
        if c.returncode != 0 or subprocess.run([str(d / "hello")], capture_output=True, timeout=TIMEOUT).returncode != 0:
            pytest.skip("this machine cannot build or run a %s program" % " ".join(flags))
    exe = str(d / "gzip_crc_host")
    c = _compile(flags, SRC, exe)
    assert c.returncode == 0, c.stderr
    return exe


def _run(program, what):
    p = subprocess.run([program, what], capture_output=True, text=True, timeout=TIMEOUT)
    assert p.returncode == 0 and p.stdout.startswith("ok "), p.stdout + p.stderr
    return int(p.stdout.split()[1])


def test_combine_4096_equals_zlibs(program):
    # 100 000 random pairs and every pair of the words 0, 1, 0x80000000, 0xffffffff
    assert _run(program, "combine") == 100_016


def test_table_entries_tile_the_piece_and_never_cross_a_member_end(program):
    # pieces of 1, 4095, 4096, 4097, 12288 bytes x {no end, one at 0, one at the piece's end, one at 4096, two at the same offset, ends at
    # 100 and 5000}: in order, at most 4096 bytes each, one 0-byte entry per end without text and none behind the last end, no more
    # entries than the submit reserves; ends out of order or beyond the piece are bad arguments
    assert _run(program, "table") > 300


def test_fold_three_members_over_two_pieces(program):
    # right trailers: no verdict, 3 members; a wrong CRC, a wrong ISIZE, the device's error words 1 and 2 with the piece's compressed
    # offset; the first verdict stands
    assert _run(program, "fold") > 0


def test_empty_piece_trailers(program):
    assert _run(program, "empty") > 0
