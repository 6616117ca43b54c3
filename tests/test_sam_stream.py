"""The device SAM parser (MGC_TEXT_SAM; meryl_amd/csrc/mgc_parse.hip) byte for byte: the base stream that mgc_push_text and the
file readers stage (Session.staged_bases) against the sequential model of tests/sam_model.py, at the smallest shapes at which the
kernels can go wrong -- the tab that opens column 9, what closes it and the line's '\\n' on every offset round a thread, wave, tile
and piece edge; tiles that hold no line start and no tab, inside SEQ, QUAL and a header line; QUAL that begins with '@' as the
first byte of a tile and of a piece; 10, 11 and 30 columns; a last line without its line end; a second batch of 1024 tiles in the
compose kernel entered between a record's column-9 tab and its bases -- and the refusals.  tests/test_sam_model_host.py checks
that every case holds the edge it is named after, and that the model is what the host reader gives.

Every comparison is byte equality, or an exact return code.  Many files go into one session (opening one pins 64 MiB): the stream
must be the models one after the other, and a difference is reported by its file and the input offset it comes from."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import sam_model as sm  # noqa: E402
import text_model as tm  # noqa: E402

pytestmark = pytest.mark.gpu

SAM = "sam"
FORMAT = {tm.FASTA: 1, tm.FASTQ: 2, SAM: 3}


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


def push(s, text, fmt=SAM, cuts=None):
    """begin / push / end with the text cut at the given offsets (tm.piece_bounds: None, a piece size or a list of offsets)"""
    from meryl_amd import capi
    L = capi.lib()
    capi.check(L.mgc_begin_text(s._h, FORMAT[fmt]), "mgc_begin_text", s._h)
    for b, e in tm.piece_bounds(len(text), cuts):
        capi.check(L.mgc_push_text(s._h, text[b:e], e - b), "mgc_push_text", s._h)
    capi.check(L.mgc_end_text(s._h), "mgc_end_text", s._h)


def staged(s):
    return s.staged_bases().cpu().numpy().tobytes()


@functools.lru_cache(maxsize=16)
def good_model(text, fmt):
    stream, refused, src = sm.model(text) if fmt == SAM else tm.model(text, fmt)
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


def refused(s, text, cuts=None):
    from meryl_amd import capi
    with pytest.raises(capi.MgcError) as e:
        push(s, text, SAM, cuts)
    return e.value.code == capi.EFORMAT, str(e.value)


# ---- 1: the column-9 tab, what closes the column and the line end on every offset round an edge --------------------------
def test_column_nine_on_every_offset_round_a_thread_wave_and_tile_edge(ops):
    cases = sm.edge_cases()
    assert len(cases) >= 2 * len(sm.FEATURES) * len(sm.EDGES) * len(sm.EDGE_DELTAS) - 4
    with session(ops, sum(len(c[4]) for c in cases)) as s:
        files = []
        for feature, edge, d, pad_with, text in cases:
            push(s, text)
            files.append(("%s at %d%+d, padded by a %s" % (feature, edge, d, pad_with), SAM, text))
        assert_stream(staged(s), files)


def test_two_pieces_cut_at_every_offset_round_column_nine(ops):
    text, _ = sm.piece_text()
    cuts = sm.piece_cuts()
    with session(ops, len(cuts) * len(text)) as s:
        for p in cuts:
            push(s, text, SAM, [p])
        assert_stream(staged(s), [("cut at %d" % p, SAM, text) for p in cuts])


def test_uniform_pieces(ops):
    text = sm.piece_text()[0]
    with session(ops, (len(sm.PIECE_SIZES) + 1) * len(text)) as s:
        push(s, sm.TINY, SAM, 1)
        for p in sm.PIECE_SIZES:
            push(s, text, SAM, p)
        assert_stream(staged(s), [("pieces of 1", SAM, sm.TINY)] + [("pieces of %d" % p, SAM, text) for p in sm.PIECE_SIZES])


# ---- 2: tiles with no line start and no tab; QUAL that begins with '@' ---------------------------------------------------
def test_tiles_inside_seq_qual_and_a_header_line(ops):
    text = sm.long_read_sam()
    pieces = (None, 1023, 16384, 16385)
    with session(ops, len(pieces) * len(text)) as s:
        for p in pieces:
            push(s, text, SAM, p)
        assert_stream(staged(s), [("pieces of %s" % p, SAM, text) for p in pieces])


def test_qual_that_begins_with_at_first_in_a_tile_and_in_a_piece(ops):
    text, at = sm.qual_at_tile_text()
    with session(ops, 4 * len(text)) as s:
        push(s, text)
        push(s, text, SAM, [at])
        push(s, text, SAM, [at - 1, at, at + 1])
        assert_stream(staged(s), [("whole", SAM, text), ("cut before the '@'", SAM, text), ("the tab and the '@' as pieces of one byte", SAM, text)])


# ---- 3: column counts, odd bytes, a last line without its line end -------------------------------------------------------
def test_column_counts_small_and_odd_files(ops):
    assert sm.model(sm.LAST_LINE_3_COLUMNS)[0] == b"ACGT.." and sm.model(sm.LAST_LINE_10_COLUMNS)[0] == b"ACGT.GATTACA."
    with session(ops, 1 << 20) as s:
        s.push_bases("ACGTA", end_of_sequence=False)                   # the first file begins at an odd stream offset
        files = [("10, 11 and 30 columns", SAM, sm.column_count_text())] + [("small file %d" % i, SAM, t) for i, t in enumerate(sm.SMALL_FILES)]
        for _, _, text in files:
            push(s, text)
        assert_stream(staged(s), files, b"ACGTA")


# ---- 4: more than 1024 tiles in one piece --------------------------------------------------------------------------------
def test_second_batch_of_tiles_entered_behind_the_column_nine_tab(ops):
    text, tab9 = sm.many_tiles_sam()
    assert tab9 == sm.BATCH * sm.TILE - 1
    with session(ops, len(text)) as s:
        push(s, text)
        assert_stream(staged(s), [("1026 tiles, a record across the batch edge at %d" % tab9, SAM, text)])


# ---- 5: refusals ---------------------------------------------------------------------------------------------------------
def test_refused_sam_leaves_the_stream_as_it_was(ops):
    good = sm.good_files()
    files = [("accepted 0", SAM, good[0])]
    with session(ops, 64 * sum(map(len, good))) as s:
        s.push_bases("ACGTA", end_of_sequence=False)
        push(s, good[0])
        before = staged(s)
        assert_stream(before, files, b"ACGTA")
        for name, (text, cuts, why) in sm.REFUSED.items():
            assert sm.model(text)[1]
            eformat, message = refused(s, text, cuts)
            assert eformat, (name, message)
            assert why in message, (name, message)
            assert staged(s) == before, name
            follow = good[len(files) % len(good)]                      # after every refusal a good file still comes out right
            push(s, follow)
            files.append(("after %s" % name, SAM, follow))
            before = staged(s)
            assert_stream(before, files, b"ACGTA")


# ---- 6: the state is set up again at every begin -------------------------------------------------------------------------
def test_fastq_sam_and_fasta_one_after_the_other(ops):
    fastq, fasta = tm.accepted_fastq()[2], b">ends in a header ACGT"    # neither ends with a line end
    sam = sm.SMALL_FILES[16]                                            # ends inside column 9
    with session(ops, 1 << 20) as s:
        files = []
        for fmt, text in ((tm.FASTQ, fastq), (SAM, sam), (tm.FASTA, fasta), (SAM, sm.LAST_LINE_3_COLUMNS), (tm.FASTQ, fastq), (SAM, sm.TINY)):
            push(s, text, fmt)
            files.append(("%s file" % fmt, fmt, text))
        assert_stream(staged(s), files)


# ---- 7: the file readers -------------------------------------------------------------------------------------------------
def test_two_windows_of_a_file_cut_at_a_record_start(ops, tmp_path):
    import ctypes
    from meryl_amd import capi
    L = capi.lib()
    text = sm.long_read_sam()
    path = tmp_path / "windows.sam"
    path.write_bytes(text)
    inside = text.index(b"read1") + 30_000                              # inside the SEQ of a record
    start = ctypes.c_uint64(0)
    capi.check(L.mgc_text_record_start(os.fsencode(str(path)), capi.TEXT_SAM, inside, ctypes.byref(start)), "mgc_text_record_start")
    cut = start.value
    assert cut == text.index(b"\n", inside) + 1 and 0 < cut < len(text)
    capi.check(L.mgc_text_record_start(os.fsencode(str(path)), capi.TEXT_SAM, cut, ctypes.byref(start)), "mgc_text_record_start")
    assert start.value == cut                                           # a line start is its own answer
    with session(ops, 4 * len(text)) as s:
        capi.check(L.mgc_push_text_file_range(s._h, os.fsencode(str(path)), capi.TEXT_SAM, 2, 0, cut), "mgc_push_text_file_range", s._h)
        capi.check(L.mgc_push_text_file_range(s._h, os.fsencode(str(path)), capi.TEXT_SAM, 2, cut, len(text) + 5), "mgc_push_text_file_range", s._h)
        two = staged(s)
        capi.check(L.mgc_push_text_file(s._h, os.fsencode(str(path)), capi.TEXT_SAM, 3), "mgc_push_text_file", s._h)
        assert_stream(staged(s), [("window 0", SAM, text[:cut]), ("window 1", SAM, text[cut:]), ("whole", SAM, text)])
        whole = sm.model(text)[0]
        first = len(sm.model(text[:cut])[0])
        assert two[:first - 1] + two[first:] == whole                   # the whole file's stream but for the first window's end-of-file '.'
        # format 0 never means SAM: the leading '@' of the header is taken for FASTQ, which this file is not
        assert L.mgc_push_text_file(s._h, os.fsencode(str(path)), 0, 2) == capi.EFORMAT


def test_the_parse_alone_device_to_device(ops, torch_cuda):
    """mgc_dev_text_parse, what scripts/sam_bench.py times: the stream without the final '.', its length and the error word"""
    import ctypes
    from meryl_amd import capi
    L = capi.lib()
    for text, refused in ((sm.long_read_sam(), 0), (sm.REFUSED["nine columns, last line"][0], 1), (sm.REFUSED["line starts with a carriage return"][0], 3)):
        d_text = torch_cuda.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda()
        d_out = torch_cuda.zeros(len(text) + 64, dtype=torch_cuda.uint8, device="cuda")
        d_ws = torch_cuda.zeros(int(L.mgc_dev_text_parse_workspace_bytes(len(text))), dtype=torch_cuda.uint8, device="cuda")
        st = ctypes.c_void_p(torch_cuda.cuda.current_stream().cuda_stream)
        capi.check(L.mgc_dev_text_parse(ctypes.c_void_p(d_text.data_ptr()), len(text), capi.TEXT_SAM, ctypes.c_void_p(d_ws.data_ptr()),
                                        ctypes.c_void_p(d_out.data_ptr()), st), "mgc_dev_text_parse")
        torch_cuda.cuda.synchronize()
        state = d_ws[:32].cpu().numpy()
        want = sm.model(text)[0][:-1]
        assert int(state[:8].view(np.uint64)[0]) == len(want) and int(state[24:28].view(np.uint32)[0]) == refused
        assert d_out[:len(want)].cpu().numpy().tobytes() == want and not d_out[len(want):].any()
