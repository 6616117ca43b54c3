"""The base decoders both front-end kernels share (meryl_amd/csrc/mgc_bases.hpp: enc4, inv4 by expected letter, encode16), on a
machine without a GPU: a stand-alone host program built with the address and undefined-behaviour sanitizers compares them with the
expressions they replaced (one zero-byte test per letter, written out in tests/host/decode_host.cpp) and with the byte-by-byte
definition -- every byte value in every byte position, every pair of neighbouring byte values, and four million random groups of
sixteen bytes."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_RANDOM = 4_000_000
N_FILL = 28                                               # neighbour bytes of decode_host.cpp


def test_decoders_match_the_expressions_they_replaced(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "decode_host")
    c = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        os.path.join(ROOT, "tests", "host", "decode_host.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert c.returncode == 0, c.stderr
    p = subprocess.run([exe, str(N_RANDOM)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    tag, words, groups = p.stdout.split()
    assert tag == "ok"
    assert int(words) == 4 * 256 * N_FILL * N_FILL + 3 * 256 * 256 + 4 * N_RANDOM
    assert int(groups) == 16 * 256 * N_FILL + N_RANDOM
