"""SAM text among the other inputs of one session: FASTQ text, a plain .sam file, BAM pieces, a BGZF .sam.gz, a refused SAM file, a
plain-gzip .sam.gz and host-pushed bases all go through the one piece-slot protocol into one base stream.  Each adds its model's
stream (tests/sam_model.py, tests/text_model.py), the refused file adds nothing, and the count of the whole is the oracle's count of
the concatenation -- also when the batches are small enough that one is cut inside the SAM input (batches are cut at a '.')."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import gzip_cases as gc  # noqa: E402
import sam_model as sm  # noqa: E402
import text_model as tm  # noqa: E402
from test_seq_bam import bam_bytes, bgzf, random_records  # noqa: E402

pytestmark = pytest.mark.gpu

K = 21


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "the -m gpu tests need a GPU"
    torch.cuda.set_device(0)
    return torch


@pytest.fixture(scope="module")
def ops(native_lib, torch_cuda):
    from meryl_amd import count
    return count


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """what is pushed, in order, and the stream each part adds"""
    d = tmp_path_factory.mktemp("sam_routes")
    fastq = gc.fastq_text(600, 11)
    sam_a, sam_b, sam_c = sm.reads_sam(2500, 301)[0], sm.reads_sam(2000, 302)[0], sm.reads_sam(3000, 303, header=False)[0]
    recs = random_records(400, 31)
    plain, bgz, gz = d / "a.sam", d / "b.sam.gz", d / "c.sam.gz"
    plain.write_bytes(sam_a)
    bgz.write_bytes(bgzf(sam_b, 30_000))
    gz.write_bytes(gc.member(sam_c, 6))
    lines = sam_a.splitlines(keepends=True)
    bad, bad_first = b"".join(lines[:40]) + sm.NINE + b"".join(lines[40:80]), sm.NINE + b"".join(lines[:80])
    assert sm.refusals(bad) == {sm.FEW} == sm.refusals(bad_first)
    host = b"GATTACAGATTACAGATTACAGATTACAGATTACA"
    streams = [tm.model(fastq, tm.FASTQ)[0], sm.model(sam_a)[0], "".join(s + "." for _, _, s in recs).encode(), sm.model(sam_b)[0], b"",
               sm.model(sam_c)[0], host + b"."]
    return dict(fastq=fastq, plain=plain, bam=bam_bytes(recs), bgz=bgz, bad=bad, bad_first=bad_first, gz=gz, host=host, sam_c=sam_c, streams=streams)


def push_all(s, x, sam_text_pieces=None):
    """sam_text_pieces: None -- one batch; 0 -- batches, the last SAM input as a gzip file; n -- as text in pieces of n bytes"""
    from meryl_amd import capi
    L = capi.lib()
    s.push_text(x["fastq"], "fastq")
    capi.check(L.mgc_push_text_file(s._h, os.fsencode(str(x["plain"])), capi.TEXT_SAM, 3), "mgc_push_text_file", s._h)
    s.push_bam(x["bam"], 4099)
    capi.check(L.mgc_push_text_bgzf_file(s._h, os.fsencode(str(x["bgz"])), capi.TEXT_SAM, 3), "mgc_push_text_bgzf_file", s._h)
    with pytest.raises(capi.MgcError) as e:
        # (with batches the line that is wrong comes first: a file cannot be taken back once a batch was cut inside it)
        s.push_text(x["bad_first" if sam_text_pieces is not None else "bad"], "sam", 3000)
    assert e.value.code == capi.EFORMAT and sm.FEW in str(e.value)
    if sam_text_pieces:
        s.push_text(x["sam_c"], "sam", sam_text_pieces)
    else:
        info = s.push_text_gzip_file(str(x["gz"]), 4, "sam")
        assert info["text_bytes"] == len(x["sam_c"]) and info["members"] == 1 and (sam_text_pieces is None or info["cuts"] >= 1)
    s.push_bases(x["host"])


def counted(s, tmp_path):
    from meryl_amd import db
    s.count()
    if s.out_of_core():
        out = str(tmp_path / "batched.meryl")
        s.write_database(out)
        r = db.Reader(out)
        lo, hi, cn = r.read_all()
        r.close()
    else:
        lo, hi, cn = s.result_wide()[:3]
    return lo, cn, s.info().n_instances


def test_every_route_adds_its_stream_and_the_count_is_the_oracles(ops, oracle_lib, inputs, tmp_path, monkeypatch):
    from meryl_amd import capi
    monkeypatch.setenv("MGC_GZIP_SPAN", str(gc.SPAN))
    want = b"".join(inputs["streams"])
    _, wlo, wcn, wni = oracle_lib.count_brute(want, K)
    with ops.Session(capi.configure(K, 4 * len(want), 2 << 30)) as s:
        push_all(s, inputs)
        got = s.staged_bases().cpu().numpy().tobytes()
        if got != want:
            n = min(len(got), len(want))
            diff = np.flatnonzero(np.frombuffer(got, dtype=np.uint8)[:n] != np.frombuffer(want, dtype=np.uint8)[:n])
            o, ends = int(diff[0]) if diff.size else n, np.cumsum([len(x) for x in inputs["streams"]])
            pytest.fail("the stream differs first at output offset %d (input %d of 7): got %r, want %r (%d bytes staged, %d wanted)"
                        % (o, int(np.searchsorted(ends, o, side="right")), got[o:o + 12], want[o:o + 12], len(got), len(want)))
        lo, cn, n_inst = counted(s, tmp_path)
    assert n_inst == wni and np.array_equal(lo, wlo) and np.array_equal(cn, wcn)


@pytest.mark.parametrize("route", ["gzip pieces", "text pieces"])
def test_batches_cut_inside_the_sam_input(ops, oracle_lib, inputs, tmp_path, monkeypatch, route):
    """the plain-gzip .sam.gz arrives in pieces of at most 300 000 bytes of text (three of them), or the same text through
    mgc_push_text in pieces of 50 000 bytes: with 100 000 bases to a batch, batches are cut while that SAM input is open"""
    from meryl_amd import capi
    monkeypatch.setenv("MGC_GZIP_SPAN", str(gc.SPAN))
    monkeypatch.setenv("MGC_GZIP_TEXT_CAP", str(gc.SMALL_CAP))
    want = b"".join(inputs["streams"])
    assert len(inputs["streams"][5]) > 200_000
    _, wlo, wcn, wni = oracle_lib.count_brute(want, K)
    with ops.Session(capi.configure(K, 4 * len(want), 2 << 30)) as s:
        s.set_batch_bases(100_000)
        push_all(s, inputs, 50_000 if route == "text pieces" else 0)
        lo, cn, n_inst = counted(s, tmp_path)
        assert s.profile().n_batches >= 4
    assert n_inst == wni and np.array_equal(lo, wlo) and np.array_equal(cn, wcn)
