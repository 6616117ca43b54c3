"""The device text parser (meryl_amd/csrc/mgc_parse.hip) byte for byte: the base stream that mgc_push_text, mgc_push_text_file and
the gzip reader stage (Session.staged_bases) against the sequential model of tests/text_model.py, at the shapes the count-parity
tests of tests/test_gpu_parity.py do not reach -- tiles of 16 KiB that hold no line start, a line start on every offset round a
thread, wave, tile and piece edge, a second batch of 1024 tiles in the compose kernel -- and the refusals of FASTQ that is not in
strict four-line records.  tests/test_text_model_host.py checks that every case holds the edge it is named after.

Every comparison is byte equality, or an exact return code.  Many files go into one session (opening one pins 64 MiB): the
stream must be the models one after the other, and a difference is reported by its file and the input offset it comes from."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import gzip_cases as gc  # noqa: E402
import text_model as tm  # noqa: E402

pytestmark = pytest.mark.gpu

FASTA, FASTQ = tm.FASTA, tm.FASTQ


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


def session(ops, total_text):
    """no batch is cut at this size, so the whole stream stays where mgc_staged_bases can see it"""
    from meryl_amd import capi
    return ops.Session(capi.configure(21, 4 * max(total_text, 1 << 20), 2 << 30))


def push(s, text, fmt, cuts=None):
    """begin / push / end with the text cut at the given offsets (tm.piece_bounds: None, a piece size or a list of offsets)"""
    from meryl_amd import capi
    L = capi.lib()
    capi.check(L.mgc_begin_text(s._h, 1 if fmt == FASTA else 2), "mgc_begin_text", s._h)
    for b, e in tm.piece_bounds(len(text), cuts):
        capi.check(L.mgc_push_text(s._h, text[b:e], e - b), "mgc_push_text", s._h)
    capi.check(L.mgc_end_text(s._h), "mgc_end_text", s._h)


def staged(s):
    return s.staged_bases().cpu().numpy().tobytes()


@functools.lru_cache(maxsize=16)
def good_model(text, fmt):
    stream, refused, src = tm.model(text, fmt)
    assert not refused
    return stream, src


def assert_stream(got, files, lead=b""):
    """files: [(label, fmt, text)] in the order they were pushed, after `lead` bytes that were staged before them"""
    models = [good_model(text, fmt) for _, fmt, text in files]
    want = lead + b"".join(m[0] for m in models)
    if got == want:
        return
    n = min(len(got), len(want))
    diff = np.flatnonzero(np.frombuffer(got, dtype=np.uint8)[:n] != np.frombuffer(want, dtype=np.uint8)[:n])
    o = int(diff[0]) if diff.size else n
    where, at = "past the last file" if o >= len(want) else "in the bytes staged before the files", len(lead)
    for (label, fmt, text), (stream, src) in zip(files, models):
        if at <= o < at + len(stream):
            where = "file %r (%s, %d bytes), taken from its input offset %d" % (label, fmt, len(text), int(src[o - at]))
        at += len(stream)
    pytest.fail("the stream differs first at output offset %d: got %r, want %r (%d bytes staged, %d wanted): %s"
                % (o, got[o:o + 12], want[o:o + 12], len(got), len(want), where))


def refused(s, text, fmt=FASTQ, cuts=None):
    from meryl_amd import capi
    with pytest.raises(capi.MgcError) as e:
        push(s, text, fmt, cuts)
    return e.value.code == capi.EFORMAT


# ---- 1: lines longer than a tile -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [FASTA, FASTQ])
def test_lines_longer_than_a_tile(ops, fmt):
    text = tm.long_line_fasta() if fmt == FASTA else tm.long_read_fastq()
    pieces = (None, 1023, 16384, 16385)
    with session(ops, len(pieces) * len(text)) as s:
        for p in pieces:
            push(s, text, fmt, p)
        assert_stream(staged(s), [("pieces of %s" % p, fmt, text) for p in pieces])


# ---- 2: a line start at every offset round an edge -----------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [FASTA, FASTQ])
def test_line_start_on_every_offset_round_an_edge(ops, fmt):
    cases = tm.edge_cases(fmt)
    assert len(cases) > 250 * len(tm.EDGE_KINDS[fmt])
    with session(ops, sum(len(c[4]) for c in cases)) as s:
        files = []
        for edge, d, eol, kind, text in cases:
            push(s, text, fmt)
            files.append(("%s line start at %d%+d, %s" % (kind, edge, d, "CRLF" if eol == b"\r\n" else "LF"), fmt, text))
        assert_stream(staged(s), files)


# ---- 3: piece edges ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [FASTA, FASTQ])
def test_two_pieces_cut_at_every_offset_round_a_hand_off(ops, fmt):
    text, _ = tm.piece_text(fmt)
    cuts = tm.piece_cuts(fmt)
    with session(ops, len(cuts) * len(text)) as s:
        for p in cuts:
            push(s, text, fmt, [p])
        assert_stream(staged(s), [("cut at %d" % p, fmt, text) for p in cuts])


@pytest.mark.parametrize("fmt", [FASTA, FASTQ])
def test_uniform_pieces(ops, fmt):
    text, tiny = tm.piece_text(fmt)[0], tm.tiny_piece_text(fmt)
    with session(ops, (len(tm.PIECE_SIZES) + 1) * len(text)) as s:
        push(s, tiny, fmt, 1)
        for p in tm.PIECE_SIZES:
            push(s, text, fmt, p)
        assert_stream(staged(s), [("pieces of 1", fmt, tiny)] + [("pieces of %d" % p, fmt, text) for p in tm.PIECE_SIZES])


# ---- 4: more than 1024 tiles in one piece --------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["header", "sequence"])
def test_second_batch_of_tiles_entered_inside_a_fasta_line(ops, kind):
    text, begin = tm.many_tiles_fasta(kind)
    with session(ops, len(text)) as s:
        push(s, text, FASTA)
        assert_stream(staged(s), [("%s line from %d over the batch edge" % (kind, begin), FASTA, text)])


def test_second_batch_of_tiles_entered_inside_a_fastq_quality_line(ops):
    """the violation of the refused file lies in tile 1025, the second tile of the second batch"""
    good, bad = tm.many_tiles_fastq(False), tm.many_tiles_fastq(True)
    with session(ops, 2 * len(good)) as s:
        s.push_bases("ACGTA", end_of_sequence=False)
        assert refused(s, bad)
        assert staged(s) == b"ACGTA"
        push(s, good, FASTQ)
        assert_stream(staged(s), [("1026 tiles", FASTQ, good)], b"ACGTA")


# ---- 5: small and odd files ----------------------------------------------------------------------------------------------
def test_small_and_odd_files(ops):
    """Sequence lines before the first header are emitted without a leading '.' (the device contract; the host reader of
    include/meryl_seq.h skips white space there and refuses anything else as neither FASTA nor FASTQ)."""
    assert tm.model(b"", FASTA)[0] == b"." and tm.model(b">h", FASTA)[0] == b".." and tm.model(b"@a\n\n+\n\n", FASTQ)[0] == b".."
    assert tm.model(b"ACGT\nAC\n>r\nGG\n", FASTA)[0] == b"ACGTAC.GG."
    with session(ops, 1 << 20) as s:
        s.push_bases("ACGTA", end_of_sequence=False)                   # the first file begins at an odd stream offset
        for fmt, text in tm.SMALL_FILES:
            push(s, text, fmt)
        assert_stream(staged(s), [("small file %d" % i, fmt, text) for i, (fmt, text) in enumerate(tm.SMALL_FILES)], b"ACGTA")


# ---- 6: refusals and files that must not be refused ----------------------------------------------------------------------
def test_refused_fastq_leaves_the_stream_as_it_was(ops):
    good = tm.accepted_fastq()
    files = [("accepted 0", FASTQ, good[0])]
    with session(ops, 64 * len(good[0])) as s:
        push(s, good[0], FASTQ)
        before = staged(s)
        assert_stream(before, files)
        for name, text in list(tm.REFUSED_FASTQ.items()) + [("violation first in a piece", tm.PIECE_VIOLATION[0])]:
            assert tm.model(text, FASTQ)[1]
            cuts = [tm.PIECE_VIOLATION[1]] if text is tm.PIECE_VIOLATION[0] else None
            assert refused(s, text, FASTQ, cuts), name
            assert staged(s) == before, name
            follow = good[len(files) % len(good)]                      # after every refusal a good file still comes out right
            push(s, follow, FASTQ)
            files.append(("after %s" % name, FASTQ, follow))
            before = staged(s)
            assert_stream(before, files)


def test_qualities_that_begin_like_a_header_or_a_separator_are_accepted(ops):
    good = tm.accepted_fastq()
    with session(ops, 8 * len(good[0])) as s:
        files = []
        for i, text in enumerate(good):
            for p in (None, 7):
                push(s, text, FASTQ, p)
                files.append(("accepted %d in pieces of %s" % (i, p), FASTQ, text))
        assert_stream(staged(s), files)


# ---- 7: the other routes that end in the same parser ---------------------------------------------------------------------
def test_whole_file_reader_and_gzip_reader_on_long_lines(ops, tmp_path, monkeypatch):
    from meryl_amd import capi
    L = capi.lib()
    texts = {"long_lines.fa": (FASTA, tm.long_line_fasta()), "long_reads.fq": (FASTQ, tm.long_read_fastq())}
    files = []
    with session(ops, 8 * sum(len(t) for _, t in texts.values())) as s:
        for name, (fmt, text) in texts.items():
            plain = tmp_path / name
            plain.write_bytes(text)
            capi.check(L.mgc_push_text_file(s._h, os.fsencode(str(plain)), 0, 3), "mgc_push_text_file", s._h)
            files.append((name, fmt, text))
            packed = tmp_path / (name + ".gz")
            packed.write_bytes(gc.member(text, 6))
            monkeypatch.setenv("MGC_GZIP_SPAN", str(gc.SPAN))
            monkeypatch.setenv("MGC_GZIP_TEXT_CAP", str(gc.SMALL_CAP))   # pieces of at most that much text: cut inside the long reads
            info = s.push_text_gzip_file(str(packed), 4)
            assert info["text_bytes"] == len(text) and info["members"] == 1
            assert info["cuts"] >= (1 if len(text) > gc.SMALL_CAP else 0), info
            files.append((name + ".gz", fmt, text))
        assert_stream(staged(s), files)
