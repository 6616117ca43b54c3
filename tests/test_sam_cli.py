"""SAM input of `meryl count` through the device routes: the same few thousand reads as a .sam, as a BGZF .sam.gz, as a .sam.gz of one
plain gzip member, on stdin and as a .cram served by a stand-in `samtools` on the PATH (as tests/test_seq.py does it).  Every one
is counted at k=21 and is the oracle's count and the MERYL_HOST_PARSER=1 run's; the file routes say so in their [io] trace line.
A .sam the device refuses still gives what the host reader gives: its database, or its error message."""
import os
import stat
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import gzip_cases as gc  # noqa: E402
import sam_model as sm  # noqa: E402
from test_seq_bam import bgzf  # noqa: E402

pytestmark = pytest.mark.gpu

K = 21


@pytest.fixture(scope="module")
def meryl(native_lib):
    from meryl_amd import build
    path = build.build_cli()
    assert os.path.exists(path)
    return path


@pytest.fixture(scope="module")
def reads(oracle_lib):
    text, seqs = sm.reads_sam(3000, 401)
    assert text.startswith(b"@HD\t")
    _, wlo, wcn, wni = oracle_lib.count_brute(b"".join(s + b"." for s in seqs), K)
    return text, (wlo, wcn, wni)


def count(meryl, src, out, host=False, stdin=None, check=True, path=None):
    env = dict(os.environ, MGC_IO_TRACE="1")
    env.pop("MERYL_HOST_PARSER", None)
    if host:
        env["MERYL_HOST_PARSER"] = "1"
    if path:
        env["PATH"] = path + os.pathsep + env.get("PATH", "")
    p = subprocess.run([meryl, "-Q", "k=%d" % K, "memory=2", "threads=4", "count", str(src), "output", str(out)], capture_output=True, timeout=600,
                       env=env, input=stdin)
    assert (p.returncode == 0) == check, p.stderr[-2000:]
    return p.stderr.decode(errors="replace")


def database(path):
    from meryl_amd import db
    r = db.Reader(str(path))
    lo, hi, cn = r.read_all()
    total = r.info.num_total
    r.close()
    return lo, cn, total


def same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]


@pytest.fixture(scope="module")
def arrivals(reads, tmp_path_factory):
    """{name: (source, stdin, directory to put in front of PATH)}"""
    text, _ = reads
    d = tmp_path_factory.mktemp("sam_cli")
    plain, bgz, gz, cram = d / "reads.sam", d / "bgzf" / "reads.sam.gz", d / "gzip" / "reads.sam.gz", d / "reads.cram"
    bgz.parent.mkdir()
    gz.parent.mkdir()
    plain.write_bytes(text)
    bgz.write_bytes(bgzf(text, 30_000))
    gz.write_bytes(gc.member(text, 6))
    cram.write_bytes(b"CRAM\x03\x00 not a real container: the stand-in never reads it")
    fake = d / "bin"
    fake.mkdir()
    tool = fake / "samtools"
    tool.write_text("#!/bin/sh\n[ \"$1\" = view ] || exit 2\ncat '%s'\n" % plain)
    tool.chmod(tool.stat().st_mode | stat.S_IXUSR | stat.S_IXGRP | stat.S_IXOTH)
    return {"plain": (plain, None, None), "bgzf": (bgz, None, None), "gzip": (gz, None, None), "stdin": ("-", text, None), "cram": (cram, None, str(fake))}


TRACE = {"plain": "[io] SAM file", "bgzf": "[io] BGZF SAM file", "gzip": "[io] gzip SAM file"}


@pytest.mark.parametrize("name", ["plain", "bgzf", "gzip", "stdin", "cram"])
def test_every_way_a_sam_arrives_gives_the_oracles_count(meryl, reads, arrivals, tmp_path, name):
    want = reads[1]
    src, stdin, path = arrivals[name]
    for host in (False, True):
        out = tmp_path / ("%s.%s.meryl" % (name, "host" if host else "device"))
        err = count(meryl, src, out, host=host, stdin=stdin, path=path)
        assert same(database(out), want), (name, host)
        if name in TRACE:
            assert (TRACE[name] in err) == (not host), (name, host, err[-500:])
        else:
            assert "SAM file" not in err                                # a pipe: the pieces come through mgc_push_text


def test_a_sam_the_device_refuses_takes_the_host_reader(meryl, reads, oracle_lib, tmp_path):
    text, want = reads
    # a line of nine columns: the device route refuses the file, the host reader reads it again and says what is wrong
    lines = text.splitlines(keepends=True)
    bad = tmp_path / "nine.sam"
    bad.write_bytes(b"".join(lines[:100]) + sm.NINE + b"".join(lines[100:]))
    errs = [count(meryl, bad, tmp_path / ("nine%d.meryl" % host), host=host, check=False) for host in (False, True)]
    for err in errs:
        assert "SAM alignment line with fewer than 10 columns" in err and "nine.sam" in err
    assert "[io] SAM file" in errs[0] and "[io] SAM file" not in errs[1]
    # "\r\n" line ends and a blank "\r\n" line: refused by the device route (a line starts with '\r'), right through the fallback
    crlf = tmp_path / "crlf.sam"
    crlf.write_bytes(b"".join(lines[:50]).replace(b"\n", b"\r\n") + b"\r\n" + b"".join(lines[50:]).replace(b"\n", b"\r\n"))
    assert sm.CR in sm.refusals(crlf.read_bytes())
    err = count(meryl, crlf, tmp_path / "crlf.meryl")
    assert "[io] SAM file" in err
    assert same(database(tmp_path / "crlf.meryl"), want)
