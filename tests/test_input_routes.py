"""Every input route of a session in turn -- host-pushed bases, text through mgc_push_text, plain / BGZF / gzip files, BAM through
mgc_push_bam and as a file -- in ONE session: the routes share the two device input buffers, their events and the parity of the
next piece, so each must leave that state fit for whichever route comes next, and a refused file must leave the stream as it was.

The inputs are tens of KB.  What each route must add to the stream comes from the parser's model (tests/text_model.py) and from
the BAM records themselves (stream_of), not from the device."""
import os
import struct
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import gzip_cases as gc  # noqa: E402
import text_model as tm  # noqa: E402
from test_bam_device import count_of_stream, ops, stream_of, torch_cuda  # noqa: E402,F401
from test_gzip_device import push_gz  # noqa: E402
from test_seq_bam import bam_bytes, bgzf, random_records  # noqa: E402

pytestmark = pytest.mark.gpu

GZ_SPAN = 8192                                   # compressed bytes per span: the gzip file below is several spans
BAM_PIECE = 40                                   # bytes per mgc_push_bam call: the first holds header bytes only


class Inputs:
    """the files, and what each adds to the stream"""

    def __init__(self, d):
        self.fq = gc.fastq_text(n_reads=300, seed=11)                                  # about 80 KB
        self.fa = gc.fasta_text(n_seqs=6, seed=12)
        self.fq_stream = tm.model(self.fq, tm.FASTQ)[0]
        self.fa_stream = tm.model(self.fa, tm.FASTA)[0]
        assert not tm.model(self.fq, tm.FASTQ)[1]
        self.recs = random_records(120, 71, longest=200)
        self.raw = bam_bytes(self.recs)
        self.bam_stream = stream_of(self.recs)
        assert struct.unpack_from("<i", self.raw, 4)[0] + 12 > BAM_PIECE               # the first piece lies inside the header text
        a, b = len(self.fq) // 3, 2 * len(self.fq) // 3
        # four members, an empty one among them, a sync flush (a block start that keeps the window) every 10 KB of text: every span
        # holds a block start, and the pieces that begin there come with unresolved symbols
        flush = dict(flush_every=10_000, flush_mode=zlib.Z_SYNC_FLUSH)
        self.gz_data = gc.member(self.fq[:a], 6, **flush) + gc.member(b"", 6) + gc.member(self.fq[a:b], 1, **flush) + gc.member(self.fq[b:], 9, **flush)
        assert len(self.gz_data) > 3 * GZ_SPAN
        self.gz = d / "reads.fq.gz"
        self.gz.write_bytes(self.gz_data)
        flipped = bytearray(self.gz_data)                                              # gzip_cases' flipped_bit, of this file
        flipped[len(flipped) // 2] ^= 0x10
        self.gz_flipped = d / "flipped_bit.gz"
        self.gz_flipped.write_bytes(bytes(flipped))
        self.fa_plain = d / "seqs.fa"
        self.fa_plain.write_bytes(self.fa)
        self.fq_bgzf = d / "reads.bgzf.fq.gz"
        self.fq_bgzf.write_bytes(bgzf(self.fq, 3000))
        self.bam = d / "reads.bam"
        self.bam.write_bytes(bgzf(self.raw, 3000))


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    return Inputs(tmp_path_factory.mktemp("input_routes"))


@pytest.fixture(scope="module")
def cfg(ops):
    from meryl_amd import capi
    return capi.configure(21, 1 << 20, 2 << 30)


def staged(s):
    return s.staged_bases().cpu().numpy().tobytes()


def push_gzip(s, path, monkeypatch):
    info = push_gz(s, path, monkeypatch, span=GZ_SPAN, cap=gc.SMALL_CAP)
    assert info["members"] == 4 and info["chunks"] >= 3 and info["symbol_bytes"] > 0, info     # several pieces
    return info


def routes(inp, monkeypatch):
    """[(name, what it does to a session, what that adds to the stream)]: every route, the gzip file twice so that it meets both parities"""
    from meryl_amd import capi
    L = capi.lib()

    def text_file(s):
        capi.check(L.mgc_push_text_file(s._h, os.fsencode(str(inp.fa_plain)), 0, 2), "mgc_push_text_file", s._h)

    def bgzf_file(s):
        capi.check(L.mgc_push_text_bgzf_file(s._h, os.fsencode(str(inp.fq_bgzf)), 0, 3), "mgc_push_text_bgzf_file", s._h)

    return [
        ("push_bases", lambda s: s.push_bases("ACGTA", end_of_sequence=False), b"ACGTA"),
        ("push_text x3", lambda s: s.push_text(inp.fq, "fastq", pieces=(len(inp.fq) + 2) // 3), inp.fq_stream),
        ("gzip file", lambda s: push_gzip(s, inp.gz, monkeypatch), inp.fq_stream),
        ("push_bam", lambda s: s.push_bam(inp.raw, BAM_PIECE), inp.bam_stream),
        ("text file", text_file, inp.fa_stream),
        ("BGZF file", bgzf_file, inp.fq_stream),
        ("BAM file", lambda s: s.push_bam_file(str(inp.bam), 3), inp.bam_stream),
        ("gzip file again", lambda s: push_gzip(s, inp.gz, monkeypatch), inp.fq_stream),
    ]


@pytest.mark.parametrize("order", ["forward", "reversed"])
def test_one_session_every_route_in_turn(ops, torch_cuda, cfg, inputs, monkeypatch, order):
    steps = routes(inputs, monkeypatch)
    assert (len(inputs.fq) + 2) // 3 * 2 < len(inputs.fq)                              # three calls of mgc_push_text
    if order == "reversed":
        steps = steps[::-1]
    want = b""
    with ops.Session(cfg) as s:
        for name, push, adds in steps:
            push(s)
            want += adds
            got = staged(s)
            assert len(got) == len(want) and got == want, (order, name)
        s.count()
        res, n_inst = s.result_wide(), s.info().n_instances
    want_res, want_inst = count_of_stream(ops, torch_cuda, cfg, want)
    assert n_inst == want_inst > 0
    for a, b in zip(res, want_res):
        assert np.array_equal(a, b)


def test_refusals_across_routes(ops, torch_cuda, cfg, inputs, monkeypatch):
    from meryl_amd import capi
    multi_line = b"@a\nACGTACGTACGTACGTACGTACGTAC\nGTACGTTT\n+\nIIIIIIIIIIIIIIIIIIIIIIIIII\nIIIIIIII\n" + inputs.fq[:30_000]
    assert tm.model(multi_line, tm.FASTQ)[1]
    bad_bam = bam_bytes(inputs.recs[:80]) + struct.pack("<i", 31) + bytes(40)

    def refused(s, push, word):
        before = staged(s)
        with pytest.raises(capi.MgcError) as e:
            push()
        assert e.value.code == capi.EFORMAT, (word, e.value)
        assert word in capi.last_error(s._h), capi.last_error(s._h)
        assert staged(s) == before, word
        return before

    with ops.Session(cfg) as s:
        s.push_bases("ACGTTGCATTGACCAGGATTACAGGAT")
        before = refused(s, lambda: push_gz(s, inputs.gz_flipped, monkeypatch, span=GZ_SPAN, cap=gc.SMALL_CAP), "flipped_bit.gz")
        s.push_bam_file(str(inputs.bam), 3)
        assert staged(s) == before + inputs.bam_stream
        before = refused(s, lambda: s.push_bam(bad_bam, 5000), "block_size 31 < 32")
        s.push_text(inputs.fq, "fastq", pieces=30_011)
        assert staged(s) == before + inputs.fq_stream
        before = refused(s, lambda: s.push_text(multi_line, "fastq", pieces=10_007), "FASTQ")
        push_gzip(s, inputs.gz, monkeypatch)
        want = before + inputs.fq_stream
        assert staged(s) == want
        s.count()
        res, n_inst = s.result_wide(), s.info().n_instances
    want_res, want_inst = count_of_stream(ops, torch_cuda, cfg, want)
    assert n_inst == want_inst > 0
    for a, b in zip(res, want_res):
        assert np.array_equal(a, b)
