"""The resumable BAM record walker (meryl_amd/csrc/mgc_bam_walk.hpp) in a stand-alone program (tests/host/bam_walk_host.cpp),
built plain and with the address + undefined-behaviour sanitizers linked statically into it: nothing sanitized is loaded into
Python, nothing is preloaded.

The program feeds a BAM byte stream to the walker in pieces of a given size, each piece from a heap block of exactly its size,
checks what the walker promises of every segment, and expands the segments on the CPU; here the stream it prints is compared
with SEQ + "." per record.  The BAM bytes are written by tests/test_seq_bam.py's writer, from the SAM specification."""
import os
import random
import shutil
import struct
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(__file__))
from test_seq_bam import NT16, bam_bytes, random_records  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host", "bam_walk_host.cpp")
VARIANTS = {
    "plain": [],
    "address_undefined": ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"],
}
HELLO = """#include <vector>
int main() { std::vector<int> v(3, 1); return v[0] + v[2] - 2; }
"""
TIMEOUT = 60
PIECES = [1, 7, 35, 36, 37, 4099, 65536, 0]                  # 0: the whole stream at once


def _compile(flags, src, out):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    return subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall"] + flags + [src, "-o", out], capture_output=True, text=True, timeout=300)


@pytest.fixture(scope="module", params=list(VARIANTS))
def program(request, tmp_path_factory):
    """the program built one way; a sanitized build is skipped only where a hello program built the same way does not work"""
    d = tmp_path_factory.mktemp("bam_walk_host_" + request.param)
    flags = VARIANTS[request.param]
    if flags:
        hello = str(d / "hello.cpp")
        open(hello, "w").write(HELLO)
        c = _compile(flags, hello, str(d / "hello"))
        if c.returncode != 0 or subprocess.run([str(d / "hello")], capture_output=True, timeout=TIMEOUT).returncode != 0:
            pytest.skip("this machine cannot build or run a %s program" % " ".join(flags))
    exe = str(d / "bam_walk_host")
    c = _compile(flags, SRC, exe)
    assert c.returncode == 0, c.stderr
    return exe


def _run(program, piece, *files):
    """-> per file: ("ok", stream bytes, records) or ("error", message)"""
    p = subprocess.run([program, str(piece)] + [str(f) for f in files], capture_output=True, timeout=TIMEOUT)
    assert p.returncode == 0, (p.stdout[-2000:] + p.stderr[-4000:]).decode("utf-8", "replace")
    out, at, res = p.stdout, 0, []
    while at < len(out):
        nl = out.index(b"\n", at)
        words = out[at:nl].split(b" ", 1)
        if words[0] == b"ok":
            n, recs = (int(x) for x in words[1].split())
            res.append(("ok", out[nl + 1:nl + 1 + n], recs))
            assert out[nl + 1 + n:nl + 2 + n] == b"\n"
            at = nl + 2 + n
        else:
            assert words[0] == b"error", out[at:nl]
            res.append(("error", words[1].decode()))
            at = nl + 1
    assert len(res) == len(files)
    return res


def stream_of(records):
    return "".join(s + "." for _, _, s in records).encode()


@pytest.fixture(scope="module")
def records():
    rng = random.Random(5)
    recs = random_records(400, 21)
    recs += [("len%d" % n, 0, "".join(rng.choice("ACGT") for _ in range(n))) for n in (0, 1, 2, 3, 15, 16, 17, 31, 32, 33)]
    recs += [("long", 0, "".join(rng.choice("ACGT") for _ in range(200_001)))]
    recs += [("n", 4, "ACGTN"), ("N" * 254, 16, "TTGCA" * 7)]                  # read names of 1 and 254 characters
    recs += [("codes", 0, NT16), ("codes_odd", 0, NT16[::-1] + "A")]           # all 16 codes, on both nibbles
    return recs


@pytest.fixture(scope="module")
def good(records, tmp_path_factory):
    p = tmp_path_factory.mktemp("bam_walk") / "good.bamraw"
    p.write_bytes(bam_bytes(records))
    return p


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    """a small good stream, walked after every refused one: (path, stream)"""
    recs = random_records(30, 8, longest=60)
    p = tmp_path_factory.mktemp("bam_walk") / "small.bamraw"
    p.write_bytes(bam_bytes(recs))
    return p, stream_of(recs)


@pytest.mark.parametrize("piece", PIECES)
def test_every_piece_size_gives_seq_and_a_breaker_per_record(program, records, good, piece):
    # a piece size of 1 puts every header field, every block_size + fixed part and every SEQ byte across a border
    (kind, stream, n_records), = _run(program, piece, good)
    assert kind == "ok" and n_records == len(records)
    assert stream == stream_of(records)


def test_no_references_and_no_records(program, tmp_path):
    p = tmp_path / "empty.bamraw"
    p.write_bytes(bam_bytes([], refs=()))
    for piece in (1, 0):
        assert _run(program, piece, p) == [("ok", b"", 0)]


def _record(block_size=None, l_read_name=2, n_cigar=0, l_seq=4, body=b"r\0" + b"\x12\x48" + b"\xff" * 4):
    fixed = struct.pack("<iiBBHHHiiii", 0, 10, l_read_name, 30, 4681, n_cigar, 0, l_seq, -1, -1, 0)
    size = len(fixed) + len(body) if block_size is None else block_size
    return struct.pack("<i", size) + fixed + body


@pytest.mark.parametrize("piece", [1, 36, 0])
def test_damage_is_named_and_the_walker_works_again_after_it(program, small, tmp_path, piece):
    small_path, small_stream = small
    head = bam_bytes([])
    ok_rec = _record()
    at = len(head) + len(ok_rec)                                               # stream offset of the damaged record
    cases = {
        "magic": (b"BAM\x02" + head[4:] + ok_rec, "bad magic at stream offset 0"),
        "bs31": (head + ok_rec + _record(block_size=31), "stream offset %d: block_size 31 < 32" % at),
        "bs_negative": (head + ok_rec + _record(block_size=-5), "stream offset %d: block_size -5 < 32" % at),
        "fields": (head + ok_rec + _record(block_size=32 + 2 + 1, l_seq=4), "stream offset %d: its fields" % at),   # SEQ needs 2 bytes
        "cigar": (head + ok_rec + _record(n_cigar=3), "stream offset %d: its fields" % at),
        "l_seq": (head + ok_rec + _record(l_seq=-(1 << 31) + 5), "negative l_seq (%d) at stream offset %d" % (-(1 << 31) + 5, at + 20)),
        "l_text": (b"BAM\x01" + struct.pack("<i", -1) + head[8:], "negative l_text (-1) at stream offset 4"),
    }
    names = sorted(cases)
    files = []
    for name in names:
        p = tmp_path / (name + ".bamraw")
        p.write_bytes(cases[name][0])
        files += [p, small_path]
    res = _run(program, piece, *files)
    for i, name in enumerate(names):
        assert res[2 * i][0] == "error" and cases[name][1] in res[2 * i][1], (name, res[2 * i])
        assert res[2 * i + 1] == ("ok", small_stream, 30), name
    # the good record alone, for the record: "ACGT" is 0x12 0x48
    p = tmp_path / "one.bamraw"
    p.write_bytes(head + ok_rec)
    assert _run(program, piece, p) == [("ok", b"ACGT.", 1)]


def _borders(raw):
    """stream offsets at which a BAM stream may end: after the header and after every record"""
    l_text, = struct.unpack_from("<i", raw, 4)
    at = 8 + l_text
    n_ref, = struct.unpack_from("<i", raw, at)
    at += 4
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", raw, at)
        at += 8 + l_name
    header_end = at
    out = {at}
    while at < len(raw):
        at += 4 + struct.unpack_from("<i", raw, at)[0]
        out.add(at)
    return header_end, out


@pytest.mark.parametrize("piece", [1, 7, 0])
def test_a_stream_cut_anywhere_but_at_a_record_border_is_truncated(program, small, tmp_path, piece):
    small_path, small_stream = small
    recs = [("a", 0, "ACG"), ("b", 4, ""), ("c", 0, "ACGTACGTAC" * 30), ("d", 16, "TT")]
    raw = bam_bytes(recs)
    header_end, borders = _borders(raw)
    assert header_end < 150 and len(raw) > 200 and max(borders) == len(raw)
    mid_seq = raw.index(bytes([0x12, 0x48, 0x12])) + 40                        # inside the SEQ of "c"
    cuts = list(range(200)) + [mid_seq]
    files = []
    for c in cuts:
        p = tmp_path / ("cut%d.bamraw" % c)
        p.write_bytes(raw[:c])
        files += [p, small_path]
    res = _run(program, piece, *files)
    for i, c in enumerate(cuts):
        got = res[2 * i]
        if c in borders:
            done = [r for r in recs[:sum(1 for b in borders if header_end < b <= c)]]
            assert got == ("ok", stream_of(done), len(done)), c
        else:
            want = "truncated BAM %s: the stream ends at offset %d" % ("header" if c < header_end else "record", c)
            assert got == ("error", want), (c, got)
        assert res[2 * i + 1] == ("ok", small_stream, 30), c
