"""tests/text_model.py without a GPU: its two forms against each other, the model against the host reader (include/meryl_seq.h) on
well-formed files, and every case builder against the edge it is named after."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import text_model as tm  # noqa: E402

FASTA, FASTQ, TILE = tm.FASTA, tm.FASTQ, tm.TILE


def load_all(lib, path, max_len=1 << 16):
    """the sequences the host reader finds in the file (as tests/test_seq.py reads them)"""
    r = lib.msr_open(path.encode())
    assert r, lib.msr_last_error()
    buf = ctypes.create_string_buffer(max_len)
    n, eos = ctypes.c_uint64(0), ctypes.c_int(0)
    seqs, cur = [], b""
    while True:
        rc = lib.msr_load_bases(r, buf, max_len, ctypes.byref(n), ctypes.byref(eos))
        assert rc >= 0, lib.msr_last_error()
        if rc == 0:
            break
        cur += buf.raw[:n.value]
        if eos.value:
            seqs.append(cur)
            cur = b""
    assert cur == b""
    lib.msr_close(r)
    return seqs


def same(text, fmt):
    a, b = tm.model_loop(text, fmt), tm.model(text, fmt)
    assert a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2]), (fmt, text[:80])
    return b


def test_both_forms_agree_on_random_short_texts():
    rng = np.random.default_rng(7)
    alphabet = np.frombuffer(b"ACGTacgtN>@+ \t\r\n.I" + b"\n" * 6, dtype=np.uint8)
    refused = 0
    for i in range(4000):
        text = rng.choice(alphabet, size=int(rng.integers(0, 64))).tobytes()
        same(text, FASTA)
        refused += same(text, FASTQ)[1]
    assert 0 < refused < 4000


def test_both_forms_agree_on_the_built_cases():
    for fmt in (FASTA, FASTQ):
        for edge, d, _, _, text in tm.edge_cases(fmt):
            if edge <= tm.WAVE or d in (-17, -1, 0, 1, 2, 16):         # (the loop form takes a second per two megabytes)
                same(text, fmt)
        same(tm.piece_text(fmt)[0], fmt)
        same(tm.tiny_piece_text(fmt), fmt)
    for fmt, text in tm.SMALL_FILES:
        assert not same(text, fmt)[1], text
    for name, text in tm.REFUSED_FASTQ.items():
        assert same(text, FASTQ)[1], name
    assert same(tm.PIECE_VIOLATION[0], FASTQ)[1]
    for text in tm.accepted_fastq():
        assert not same(text, FASTQ)[1]
    same(tm.long_line_fasta(), FASTA)
    assert tm.model(tm.long_read_fastq(), FASTQ)[1] is False


def test_model_examples():
    """the contract, spelled out on texts small enough to read"""
    assert tm.model(b"", FASTA)[0] == b"." and tm.model(b"", FASTQ)[0] == b"."
    assert tm.model(b">r1 ACGT\nAC GT\r\nac>t\n\n>r2\n>r3\nG", FASTA)[0] == b".ACGTac>t..G."
    assert tm.model(b"ACGT\n>r\nGG\n", FASTA)[0] == b"ACGT.GG."            # no header first: no '.' first
    got = tm.model(b"@r1 ACGT\nAC GT\r\n+r1\n@+II\n@r2\n\n+\n\n@r3\nG\n+\n@", FASTQ)
    assert got[0] == b".ACGT..G." and not got[1]
    assert got[2].tolist() == [0, 9, 10, 12, 13, 25, 33, 37, 42]
    assert tm.model(b"@a\nA\n+\nI\n", FASTQ)[1] is False                    # one trailing line end makes no line ...
    assert tm.model(b"@a\nA\n+\nI\n\n", FASTQ)[1] is True                   # ... a second one makes an empty type-0 line
    assert tm.model(b"@a\nA\n\nI\n", FASTQ)[1] is True
    assert tm.line_starts(b"ab\n\ncd\n").tolist() == [0, 3, 4] and tm.line_starts(b"").size == 0
    assert tm.tile_bounds(2 * TILE + 5, [TILE + 1]) == [(0, TILE), (TILE, TILE + 1), (TILE + 1, 2 * TILE + 1), (2 * TILE + 1, 2 * TILE + 5)]
    text = b">" + b"h" * (2 * TILE) + b"\n" + b"A" * (2 * TILE)
    assert tm.tiles_without_line_start(text) == {0: [1], 1: [3, 4]}
    assert tm.tiles_without_line_start(text, TILE + 1) == {0: [1, 2, 3], 1: [5, 6]}


# ---- the model against the host reader -----------------------------------------------------------------------------------
def well_formed_files():
    rng = np.random.default_rng(8)
    reads = [tm._letters(rng, int(n), b"ACGTacgtN") for n in (150, 0, 10, 1, 21, 20, 0, 0, 333, 70, 140)]
    fa = b"".join(b">r%d ACGTACGT\n" % i + b"".join(r[j:j + 70] + b"\n" for j in range(0, len(r), 70)) + (b"\n" if i % 3 == 0 else b"")
                  for i, r in enumerate(reads))
    fq = b"".join(b"@r%d ACGTACGT\n%s\n+%s\n%s\n" % (i, r, b"r%d" % i if i % 2 else b"", tm._letters(rng, len(r), b"@+>I#5")) for i, r in enumerate(reads))
    files = {
        "test_seq.fa": b">r1 some description\nACGTACGT\nNNacgt\n\n>r2\nTTTT\n>empty\n>r4\nGATTACA",
        "reads.fa": fa, "reads_crlf.fa": fa.replace(b"\n", b"\r\n"), "reads_open_end.fa": fa.rstrip(b"\n"),
        "reads.fq": fq, "reads_crlf.fq": fq.replace(b"\n", b"\r\n"), "reads_open_end.fq": fq[:-1],
        "empty_read.fq": b"@a\n\n+\n\n", "white.fa": b">s\nAC GT\tAC\n A C\t\n\t\nGG\n",
        "long_lines.fa": tm.long_line_fasta(), "long_reads.fq": tm.long_read_fastq(), "pieces.fa": tm.piece_text(FASTA)[0],
        "pieces.fq": tm.piece_text(FASTQ)[0], "tiny.fa": tm.tiny_piece_text(FASTA), "tiny.fq": tm.tiny_piece_text(FASTQ),
    }
    for i, text in enumerate(tm.accepted_fastq()):
        files["accepted%d.fq" % i] = text
    return files


@pytest.mark.parametrize("name", list(well_formed_files()))
def test_model_is_what_the_host_reader_gives(native_lib, tmp_path, name):
    """a well-formed file -- a header first, FASTQ in strict four-line records -- gives '.' + '.'.join(sequences) + '.'"""
    text = well_formed_files()[name]
    fmt = FASTQ if name.endswith(".fq") else FASTA
    path = tmp_path / name
    path.write_bytes(text)
    seqs = load_all(native_lib, str(path))
    stream, refused, _ = tm.model(text, fmt)
    assert not refused
    assert stream == b"." + b".".join(seqs) + b"."


# ---- every case holds its edge -------------------------------------------------------------------------------------------
def test_long_line_cases_hold_runs_of_tiles_without_a_line_start():
    fa = tm.tiles_without_line_start(tm.long_line_fasta())
    assert tm.has_run(fa[0]) and tm.has_run(fa[1]), fa                  # entered in a header / in sequence
    text = tm.long_line_fasta()
    assert text.index(b">", 10) == TILE + 5000 + len(b">r0 ACGT\n") and text[TILE + 5008] != 10   # a '>' that starts no line
    fq = tm.tiles_without_line_start(tm.long_read_fastq(), fmt=FASTQ)
    assert tm.has_run(fq[1]) and tm.has_run(fq[3]), fq                  # inside a sequence line / a quality line
    text, starts = tm.long_read_fastq(), tm.line_starts(tm.long_read_fastq())
    firsts = bytes(text[s] for s in starts[3::4])
    assert firsts.count(b"@") >= 2 and firsts.count(b"+") >= 2          # qualities that begin like a header / a separator
    assert sum(text[s + 1] != 10 for s in starts[2::4]) >= 2            # '+name'
    for fmt, text in ((FASTA, tm.long_line_fasta()), (FASTQ, tm.long_read_fastq())):
        for piece in (1023, 16384, 16385):
            assert sum(map(len, tm.tiles_without_line_start(text, piece, fmt).values())) >= 4


@pytest.mark.parametrize("fmt", [FASTA, FASTQ])
def test_edge_sweep_puts_a_line_start_on_every_offset(fmt):
    seen = set()
    for edge, d, eol, kind, text in tm.edge_cases(fmt):
        at = edge + d
        starts = tm.line_starts(text)
        assert at in starts and len(text) >= at + 64, (edge, d, eol, kind)
        assert text[at - len(eol):at] == eol
        want = {"sequence": b"T", "header": b">", "type0": b"@", "type1": b"A", "type2": b"+", "type3": b"@"}[kind]
        assert text[at:at + 1] == want
        if fmt == FASTQ:
            assert (int(np.searchsorted(starts, at)) - int(kind[-1])) % 4 == 0
            assert not tm.model(text, fmt)[1]
        seen.add((edge, d, eol, kind))
    for edge in tm.EDGES:
        for d in tm.EDGE_DELTAS:
            for eol in (b"\n", b"\r\n"):
                for kind in tm.EDGE_KINDS[fmt]:
                    assert (edge, d, eol, kind) in seen or edge == tm.THREAD, (edge, d, eol, kind)
    assert sum(1 for c in seen if c[0] == tm.THREAD) >= 20 * len(tm.EDGE_KINDS[fmt])


@pytest.mark.parametrize("fmt", [FASTA, FASTQ])
def test_piece_text_marks(fmt):
    text, marks = tm.piece_text(fmt)
    assert 2 * TILE + TILE // 2 < len(text) < 3 * TILE + TILE // 2 and not tm.model(text, fmt)[1]
    assert text[marks["crlf"]:marks["crlf"] + 2] == b"\r\n"
    assert text[marks["record"]:marks["record"] + 2] == (b"\n>" if fmt == FASTA else b"\n@")
    starts = tm.line_starts(text)
    state = tm.entry_states(text, fmt)
    h = marks["header"]
    line = starts[np.searchsorted(starts, h, side="right") - 1]
    assert text[line:line + 1] == (b">" if fmt == FASTA else b"@") and state[h] == 0
    for p in range(h - 3, h + 4):                                       # the second piece begins with a tile without a line start
        first_tile = len(tm.tile_bounds(p))
        assert first_tile in tm.tiles_without_line_start(text, [p], fmt)[0], p
    if fmt == FASTQ:
        q = marks["quality"]
        line = starts[np.searchsorted(starts, q, side="right") - 1]
        assert state[q] == 3 and text[line:line + 1] == b"@"
    cuts = tm.piece_cuts(fmt)
    assert 1 in cuts and len(text) - 1 in cuts and all(0 < p < len(text) for p in cuts)
    for at in marks.values():
        assert set(range(at - 3, at + 4)) <= set(cuts)
    assert len(tm.tiny_piece_text(fmt)) < 2048


@pytest.mark.parametrize("kind", ["header", "sequence"])
def test_many_tiles_fasta_crosses_the_batch_edge_in_one_line(kind):
    text, begin = tm.many_tiles_fasta(kind)
    assert len(text) == tm.MANY_TILES * TILE
    starts = tm.line_starts(text)
    i = int(np.searchsorted(starts, begin))
    assert starts[i] == begin and text[begin:begin + 1] == (b">" if kind == "header" else b"G")
    assert begin // TILE == tm.BATCH - 2 and starts[i + 1] // TILE == tm.BATCH + 1
    none = tm.tiles_without_line_start(text)
    assert none == {0 if kind == "header" else 1: [tm.BATCH - 1, tm.BATCH]}, none
    assert text.count(b">", begin + 1, int(starts[i + 1])) > 100        # the header lines it swallowed


def test_many_tiles_fastq_batch_edge_and_violation():
    good, bad = tm.many_tiles_fastq(False), tm.many_tiles_fastq(True)
    assert len(good) == len(bad) and (tm.MANY_TILES - 1) * TILE < len(good) <= tm.MANY_TILES * TILE
    assert good.count(b"\n", 0, tm.BATCH * TILE) % 4 == 3               # the second batch is entered inside a quality line
    none = tm.tiles_without_line_start(good, fmt=FASTQ)
    assert tm.BATCH in none[3] and tm.has_run(none[1]) and tm.has_run(none[3])
    assert tm.model(good, FASTQ)[1] is False and tm.model(bad, FASTQ)[1] is True
    diff = [i for i in range(tm.FASTQ_LAST - 5, len(good)) if good[i] != bad[i]]
    assert good[:tm.FASTQ_LAST - 5] == bad[:tm.FASTQ_LAST - 5] and diff == [tm.FASTQ_LAST] and bad[tm.FASTQ_LAST:tm.FASTQ_LAST + 1] == b"A"
    assert tm.FASTQ_LAST // TILE == tm.BATCH + 1 and tm.FASTQ_LAST in tm.line_starts(bad)


def test_refused_cases_put_their_violation_where_they_say():
    at = {"violation first in a tile": TILE, "+ violation first in a tile": 2 * TILE}
    for name, offset in at.items():
        text = tm.REFUSED_FASTQ[name]
        assert offset in tm.line_starts(text) and tm.model(text, FASTQ)[1]
        mended = text[:offset] + (b"@" if text[offset] == 65 else b"+") + text[offset + 1:]
        assert not tm.model(mended, FASTQ)[1]                           # that byte is the only violation
    text, cut = tm.PIECE_VIOLATION
    assert cut in tm.line_starts(text) and not tm.model(text[:cut] + b"@" + text[cut + 1:], FASTQ)[1]
