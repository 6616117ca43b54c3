"""The host-only parts of whole-file text input (meryl_amd/csrc/mgc_chunk_ring.hpp, mgc_bgzf.hpp) in a stand-alone program
(tests/host/input_host.cpp), built plain, with the thread sanitizer and with the address + undefined-behaviour sanitizers.
The sanitizer runtimes are linked statically into the program: nothing sanitized is loaded into Python, nothing is preloaded.

The ring cases (slot wrap, a producer failing mid-file, a slot allocation failing, the consumer stopping early, ...) live in
the program; the BGZF cases get their files from here and have their output compared with zlib here."""
import gzip
import os
import shutil
import subprocess
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
from test_seq_bam import bgzf_block  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host", "input_host.cpp")
VARIANTS = {
    "plain": [],
    "thread": ["-fsanitize=thread", "-static-libtsan"],
    "address_undefined": ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"],
}
HELLO = """#include <thread>
int main() { int x = 0; std::thread t([&] { x = 1; }); t.join(); return x - 1; }
"""
TIMEOUT = 20                                     # seconds: a ring that hangs fails here, it does not hold the suite up
CAP = 100_000


def _compile(flags, src, out):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    return subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-pthread"] + flags + [src, "-o", out, "-lz"],
                          capture_output=True, text=True, timeout=300)


@pytest.fixture(scope="module", params=list(VARIANTS))
def program(request, tmp_path_factory):
    """the program built one way; a sanitized build is skipped only where a hello-threads program built the same way does not work"""
    d = tmp_path_factory.mktemp("input_host_" + request.param)
    flags = VARIANTS[request.param]
    if flags:
        hello = str(d / "hello.cpp")
        open(hello, "w").write(HELLO)
        c = _compile(flags, hello, str(d / "hello"))
        if c.returncode != 0 or subprocess.run([str(d / "hello")], capture_output=True, timeout=TIMEOUT).returncode != 0:
            pytest.skip("this machine cannot build or run a %s program" % " ".join(flags))
    exe = str(d / "input_host")
    c = _compile(flags, SRC, exe)
    assert c.returncode == 0, c.stderr
    return exe


def _run(program, *args):
    p = subprocess.run([program] + [str(a) for a in args], capture_output=True, text=True, timeout=TIMEOUT)
    assert p.returncode == 0, p.stdout + p.stderr
    return p.stdout


def _fields(out):
    return dict(kv.split("=", 1) for kv in out.split())


@pytest.fixture(scope="module")
def bgzf_file():
    """~300 KB of text in blocks of mixed sizes, an empty block in the middle, the end-of-file marker: (text, blocks)"""
    rng = np.random.default_rng(11)
    text = rng.choice(np.frombuffer(b"ACGT\n", dtype=np.uint8), size=300_000).tobytes()
    sizes, left = [], len(text)
    while left:
        sizes.append(min(left, int(rng.integers(1, 0xff00)) if rng.random() < 0.5 else 0xff00))
        left -= sizes[-1]
    blocks, at = [], 0
    for i, n in enumerate(sizes):
        if i == len(sizes) // 2:
            blocks.append(bgzf_block(b""))
        blocks.append(bgzf_block(text[at:at + n]))
        at += n
    blocks.append(bgzf_block(b""))
    assert len(blocks) >= 6
    return text, blocks


def test_ring_cases(program):
    assert "ring: ok" in _run(program, "ring")


def test_bgzf_plan_and_inflate(program, bgzf_file, tmp_path):
    text, blocks = bgzf_file
    path = tmp_path / "good.gz"
    path.write_bytes(b"".join(blocks))
    f = _fields(_run(program, "bgzf", path, CAP))
    assert int(f["chunks"]) >= 3 and int(f["blocks"]) == len(blocks)
    assert int(f["max_text"]) <= CAP and f["partition"] == "1"
    assert f["bad_blocks"] == "none"
    assert (int(f["len"]), int(f["crc"])) == (len(text), zlib.crc32(text) & 0xffffffff)


def test_bgzf_corrupt_block_is_the_only_one_that_fails(program, bgzf_file, tmp_path):
    _, blocks = bgzf_file
    third = bytearray(blocks[2])
    third[18 + (len(third) - 18 - 8) // 2] ^= 0x40                   # inside its deflate data
    path = tmp_path / "flipped.gz"
    path.write_bytes(b"".join(blocks[:2]) + bytes(third) + b"".join(blocks[3:]))
    f = _fields(_run(program, "bgzf", path, CAP))
    assert f["bad_blocks"] == "2" and f["partition"] == "1"


def test_bgzf_refuses_plain_gzip_and_a_truncated_file(program, bgzf_file, tmp_path):
    text, blocks = bgzf_file
    gz = tmp_path / "plain.gz"
    gz.write_bytes(gzip.compress(text[:5000]))
    f = _fields(_run(program, "bgzf", gz, CAP))
    assert (f["refused"], int(f["off"])) == ("not_a_block", 0)
    whole = b"".join(blocks)
    cut = tmp_path / "cut.gz"
    cut.write_bytes(whole[:-10])
    f = _fields(_run(program, "bgzf", cut, CAP))
    assert (f["refused"], int(f["off"])) == ("not_a_block", len(whole) - len(blocks[-1]))
