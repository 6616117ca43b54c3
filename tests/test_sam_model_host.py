"""tests/sam_model.py against itself and against the host reader, without a GPU: the two forms of the model agree on every case of
tests/test_sam_stream.py, every case holds the edge it is named after, and for every accepted case the model's stream is what the
host reader of include/meryl_seq.h gives for the same bytes (msr_open on a file, msr_load_stream) plus the end-of-file breaker the
command line adds -- so a count through the device route and one through the host route see the same sequences.

One difference is by contract (include/meryl_gpu_count.h): a last alignment line WITHOUT its '\\n' that reaches column 9 ends with
mgc_end_text's single '.', where the host reader ends the record with a '.' of its own before the end-of-file breaker.  The two
streams then differ by that one '.' at the very end (no k-mer spans either)."""
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(__file__))
import sam_model as sm  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def all_cases():
    """[(name, text)] -- every text of the GPU tests but the 16 MiB one"""
    cases = [("%s at %d%+d padded by %s" % c[:4], c[4]) for c in sm.edge_cases()]
    cases += [("piece text", sm.piece_text()[0]), ("tiny", sm.TINY), ("long reads", sm.long_read_sam()), ("QUAL at a tile", sm.qual_at_tile_text()[0]),
              ("column counts", sm.column_count_text()), ("reads", sm.reads_sam(300)[0])]
    cases += [("small file %d" % i, t) for i, t in enumerate(sm.SMALL_FILES)]
    cases += [("good file %d" % i, t) for i, t in enumerate(sm.good_files())]
    cases += [("refused: " + name, t) for name, (t, _, _) in sm.REFUSED.items()]
    return cases


def host_stream(lib, path):
    """(stream, error) of the host reader: msr_load_stream until the end, b'' or the message"""
    r = lib.msr_open(str(path).encode())
    assert r, lib.msr_last_error()
    assert lib.msr_format(r) == 2                                      # MSR_FORMAT_SAM, by the name
    buf, n, out = ctypes.create_string_buffer(1 << 16), ctypes.c_uint64(0), bytearray()
    try:
        while True:
            rc = lib.msr_load_stream(r, buf, len(buf), ctypes.byref(n))
            if rc < 0:
                return bytes(out), lib.msr_last_error()
            if rc == 0:
                return bytes(out), b""
            out += buf.raw[:n.value]
    finally:
        lib.msr_close(r)


def test_the_two_forms_of_the_model_agree():
    for name, text in all_cases():
        a, b = sm.model_loop(text), sm.model(text)
        assert a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2]), name
        assert len(a[0]) == len(a[2]) and a[2][-1] == len(text)
    text, _ = sm.many_tiles_sam()
    stream, refused, src = sm.model(text)
    assert not refused and stream.count(b".") > 40_000 and np.all(np.diff(src) > 0)


def test_every_case_holds_the_edge_it_is_named_after():
    a = lambda text: sm.columns(text)                                   # noqa: E731
    seen = set()
    for feature, edge, d, pad_with, text in sm.edge_cases():
        at = edge + d
        b, ls, align, col = a(text)
        assert align[at] and not sm.model(text)[1]
        if feature == "tab9":
            assert b[at] == 9 and col[at] == 8 and col[at + 1] == 9 and b[at + 1] in b"ACGT"
        elif feature == "close9_tab":
            assert b[at] == 9 and col[at] == 9 and b[at + 1] == 64      # QUAL begins with '@' right behind it
        elif feature == "close9_nl":
            assert b[at] == 10 and col[at] == 9
        else:
            assert b[at] == 10 and col[at] >= 10
        assert (np.flatnonzero(ls)[0] == 0) and (pad_with == "header") == (text[0] in b"@\n")
        seen.add((feature, edge, d))
    assert seen == {(f, e, d) for f in sm.FEATURES for e in sm.EDGES for d in sm.EDGE_DELTAS}

    text, marks = sm.piece_text()
    b, ls, align, col = a(text)
    assert b[marks["tab9"]] == 9 and col[marks["tab9"]] == 8 and b[marks["close9"]] == 9 and col[marks["close9"]] == 9 and b[marks["close9"] + 1] == 64
    assert b[marks["nl"]] == 10 and marks["tab9"] < sm.TILE < marks["close9"]          # the record's SEQ lies across the tile edge
    assert marks["tab9"] + 1 in sm.piece_cuts()                         # a cut between the tab and the first base
    assert {1, 15, 16, 17} <= set(sm.PIECE_SIZES) | {1}

    within = sm.tiles_within(sm.long_read_sam())
    assert within.get("seq") and within.get("qual") and within.get("header"), within
    assert any(t + 1 in within["qual"] or t + 2 in within["qual"] for t in within["seq"])
    long_text = sm.long_read_sam()
    co = long_text.index(b"@CO\ttabs")
    assert long_text[co:long_text.index(b"\n", co)].count(b"\t") >= 4 and long_text.index(b"\n", co) - co > 2 * sm.TILE

    text, at = sm.qual_at_tile_text()
    b, ls, align, col = a(text)
    assert at == sm.TILE and b[at] == 64 and not ls[at] and col[at] == 10 and b[at - 1] == 9 and b"q@1" in text

    assert sm.column_counts(sm.column_count_text()) == {10, 11, 30}
    odd = b"".join(sm.SMALL_FILES)
    assert b"\t*\t*\n" in odd and b"\n\n" in odd and b"GGCC\r\n" in odd and b"acgtnN" in odd and b"\n@CO\tbetween\n" in odd
    for text, emits in ((sm.LAST_LINE_10_COLUMNS, True), (sm.LAST_LINE_3_COLUMNS, False)):
        last = text[text.rindex(b"\n") + 1:]
        assert last and not text.endswith(b"\n") and (last.count(b"\t") >= 9) == emits
        stream, refused, _ = sm.model(text)
        assert not refused and stream == (b"ACGT.GATTACA." if emits else b"ACGT..")

    text, tab9 = sm.many_tiles_sam()
    b, ls, align, col = a(text)
    assert len(text) > (sm.BATCH + 1) * sm.TILE and tab9 == sm.BATCH * sm.TILE - 1 and b[tab9] == 9 and col[tab9] == 8 and col[tab9 + 1] == 9
    assert not ls[tab9:tab9 + 10_000].any() and np.flatnonzero(ls[:tab9])[-1] >= (sm.BATCH - 1) * sm.TILE

    for name, (text, cuts, why) in sm.REFUSED.items():
        assert why in sm.refusals(text) and sm.model(text)[1], name
    t = sm.REFUSED["nine columns, line end first in a tile"][0]
    assert t[sm.TILE] == 10 and sm.columns(t)[3][sm.TILE] == 8
    t, cuts, _ = sm.REFUSED["nine columns, in the second piece"]
    assert sm.model(t[:cuts[0]])[1] is False and t[:cuts[0]].count(b"\n") == 1
    assert sm.REFUSED["nine columns, first line"][0].startswith(sm.NINE) and sm.REFUSED["nine columns, last line"][0].endswith(sm.NINE)


def test_model_equals_the_host_reader(native_lib, tmp_path):
    checked = 0
    for i, (name, text) in enumerate(all_cases()):
        path = tmp_path / ("case%d.sam" % i)
        path.write_bytes(text)
        stream, refused, _ = sm.model(text)
        got, err = host_stream(native_lib, path)
        if refused:
            if sm.refusals(text) == {sm.FEW}:
                assert b"fewer than 10 columns" in err, name
            continue                                                    # (a refused file goes to the host reader, whatever it makes of it)
        assert not err, (name, err)
        last = text[text.rfind(b"\n") + 1:]
        open_record = bool(last) and last[:1] != b"@" and last.count(b"\t") >= 9       # the host reader closes it with a '.' of its own
        assert got + b"." == stream + (b"." if open_record else b""), name
        checked += 1
    assert checked > 150


def test_sam_is_a_text_format_of_the_interface():
    from meryl_amd import capi
    assert capi.TEXT_SAM == 3 and capi.TEXT_FORMATS["sam"] == 3
    with open(os.path.join(ROOT, "include", "meryl_gpu_count.h")) as f:
        header = f.read()
    assert "#define MGC_TEXT_SAM   3" in header and "fewer than 9 tabs" in header
