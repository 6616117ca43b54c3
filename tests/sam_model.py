"""A sequential model of the device SAM parser (MGC_TEXT_SAM; the kernels are in meryl_amd/csrc/mgc_parse.hip) and the texts that
try it.

The model is written from the contract in include/meryl_gpu_count.h, not from the kernels.  A LINE START is a byte that begins
the file or follows '\\n' (as in tests/text_model.py).

  line start '\\n'   an empty line: emits nothing
  line start '@'    a header line: emits nothing through its '\\n'
  line start '\\r'   the file is refused
  anything else     an alignment line: a byte's column is the number of tabs before it in the line; the bytes of column 9 that
                    are not '\\t' '\\n' '\\r' '*' are emitted as they are; the line's '\\n' emits '.', and refuses the file when
                    fewer than 9 tabs precede it in the line
  mgc_end_text adds one '.'.  A last line without '\\n' emits its column-9 bytes and is no error if it has none.

Two forms that must agree: model_loop (a byte at a time) and model (numpy; 17 MB in about a second).  Both return
(stream, refused, src): src[i] is the input offset output byte i was taken from, len(text) for the final '.'.  refusals(text) says
why.  The case builders return bytes; the predicates below are what tests/test_sam_model_host.py uses to make sure that a case
really holds the edge it is named after.  No GPU is used here."""
import functools

import numpy as np

from text_model import BATCH, THREAD, TILE, WAVE, piece_bounds, tile_bounds  # noqa: F401

FEW, CR = "alignment line with fewer than 10 columns", "line starts with a carriage return"
NOT_EMITTED = (9, 10, 13, 42)                                          # '\t' '\n' '\r' '*'


# ---- the model -----------------------------------------------------------------------------------------------------------
def _loop(text):
    out, src, why = bytearray(), [], set()
    kind, tabs = None, 0                                               # of the current line
    for i, c in enumerate(text):
        if i == 0 or text[i - 1] == 10:
            kind, tabs = ("empty" if c == 10 else "header" if c == 64 else "alignment"), 0
            if c == 13:
                why.add(CR)
            if c == 10:
                continue
        if kind != "alignment":
            continue
        if c == 10:
            if tabs >= 9:
                out.append(46)
                src.append(i)
            else:
                why.add(FEW)
        elif c == 9:
            tabs += 1
        elif tabs == 9 and c not in NOT_EMITTED:
            out.append(c)
            src.append(i)
    out.append(46)
    src.append(len(text))
    return bytes(out), why, np.asarray(src, dtype=np.int64)


def model_loop(text):
    stream, why, src = _loop(text)
    return stream, bool(why), src


def columns(text):
    """per byte: (a, line start, is in an alignment line, column -- tabs before it in its line)"""
    a = np.frombuffer(text, dtype=np.uint8)
    ls = np.empty(a.size, dtype=bool)
    if a.size:
        ls[0] = True
        ls[1:] = a[:-1] == 10
    starts = np.flatnonzero(ls)
    line = np.cumsum(ls) - 1
    tab = (a == 9).astype(np.int64)
    tabs_before = np.cumsum(tab) - tab
    col = tabs_before - tabs_before[starts][line] if a.size else tabs_before
    first = a[starts][line] if a.size else a
    return a, ls, (first != 10) & (first != 64), col


def _numpy(text):
    a, ls, align, col = columns(text)
    nl = (a == 10) & align                                            # (an empty line's '\n' is its own line start: not aligned)
    dot = nl & (col >= 9)
    emit = dot | (align & (col == 9) & ~np.isin(a, NOT_EMITTED))
    why = set()
    if (nl & (col < 9)).any():
        why.add(FEW)
    if (ls & (a == 13)).any():
        why.add(CR)
    src = np.flatnonzero(emit)
    out = np.where(dot, np.uint8(46), a)[src]
    return out.tobytes() + b".", why, np.append(src, a.size).astype(np.int64)


def model(text):
    stream, why, src = _numpy(text)
    return stream, bool(why), src


def refusals(text):
    return _numpy(text)[1]


# ---- predicates ----------------------------------------------------------------------------------------------------------
def tiles_within(text, piece=None):
    """{what: [tile index]} of the whole tiles that hold no line start and no tab, by what covers them: 'seq' (column 9 of an
    alignment line), 'qual' (column 10), 'header'; tiles are numbered through all pieces in order"""
    a, ls, align, col = columns(text)
    busy = np.concatenate([[0], np.cumsum(ls | (a == 9))])
    found = {}
    for t, (b, e) in enumerate(tile_bounds(len(text), piece)):
        if e - b == TILE and busy[e] == busy[b]:
            what = "header" if a[np.flatnonzero(ls[:b + 1])[-1]] == 64 else {9: "seq", 10: "qual"}.get(int(col[b]), "other")
            found.setdefault(what, []).append(t)
    return found


def column_counts(text):
    """the set of column counts of the alignment lines that end with '\\n'"""
    a, _, align, col = columns(text)
    return set((col[(a == 10) & align] + 1).tolist())


# ---- texts ---------------------------------------------------------------------------------------------------------------
def _letters(rng, n, alphabet=b"ACGT"):
    return rng.choice(np.frombuffer(alphabet, dtype=np.uint8), size=n).tobytes()


def record(qname, seq, qual=None, aux=(), eol=b"\n", flag=b"0"):
    """one alignment line; qual None: a line of exactly 10 columns"""
    cols = [qname, flag, b"chr1", b"100", b"60", b"50M", b"*", b"0", b"0", seq]
    if qual is not None:
        cols.append(qual)
        cols.extend(aux)
    return b"\t".join(cols) + eol


HEADER = b"@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:chr1\tLN:1000000\n"
TAIL = (record(b"t1", b"GATTACAGATTACA", b"IIIIIIIIIIIIII", (b"NM:i:0",)) + b"@CO\ta header line between\talignment lines\n"
        + record(b"t@2", b"acgtnNACGT") + record(b"t3", b"*", b"*") + b"\n" + record(b"t4", b"CCCCGGGG", b"@@@@IIII", (b"RG:Z:x", b"NM:i:1")))

FEATURES = ("tab9", "close9_tab", "close9_nl", "nl")
EDGES = (THREAD, WAVE, TILE)
EDGE_DELTAS = (-2, -1, 0, 1, 2)


def edge_text(feature, at, pad_with):
    """(text, offset) -- a text in which byte `at` is: 'tab9' the tab that opens column 9 of the first alignment line,
    'close9_tab' / 'close9_nl' the tab / the '\\n' that closes its column 9, 'nl' the '\\n' of that line.  The bytes
    before are made up by `pad_with`: 'qname' (the line starts the file and its QNAME is as long as it takes) or 'header' (a
    header line, or an empty line, of that length in front).  None when `at` is too small."""
    if at >= 64:
        seq, qual = b"ACGTTGCAAC", (b"@IIIIIIIII" if feature == "close9_tab" else b"IIIIIIIIII") + b"\tNM:i:0"
    else:                                                               # round the first thread edge: as short as a line can be
        seq, qual = b"A", b"@" if feature == "close9_tab" else b"I"
    rest = b"\n" if feature == "close9_nl" else b"\t" + qual + b"\n"
    fixed = b"\t0\t\t\t\t*\t\t\t"                                         # columns 1 .. 8 (most of them empty) and the tabs before them: 10 bytes
    off = {"tab9": len(fixed), "close9_tab": len(fixed) + 1 + len(seq), "close9_nl": len(fixed) + 1 + len(seq),
           "nl": len(fixed) + 1 + len(seq) + len(rest) - 1}[feature]   # of the feature in the line when QNAME is empty
    assert fixed.count(b"\t") == 8 and len(fixed) == 10
    pad = at - off
    if pad < 0:
        return None
    if pad_with == "qname":
        lead, qname = b"", (b"r@ame" * (pad // 5 + 1))[:pad]
    else:
        if pad < 1:
            return None
        lead, qname, pad = (b"\n" if pad == 1 else b"@" + (b"CO\tx " * (pad // 5 + 1))[:pad - 2] + b"\n"), b"", 0
    text = lead + qname + fixed + b"\t" + seq + rest + TAIL
    assert len(lead) + len(qname) + off == at and text[at] == (10 if feature in ("close9_nl", "nl") else 9)
    return text


def edge_cases():
    """[(feature, edge, delta, pad_with, text)]"""
    cases = []
    for feature in FEATURES:
        for edge in EDGES:
            for d in EDGE_DELTAS:
                for pad_with in ("qname", "header"):
                    text = edge_text(feature, edge + d, pad_with)
                    if text is not None:
                        cases.append((feature, edge, d, pad_with, text))
    return cases


@functools.lru_cache(maxsize=None)
def piece_text():
    """(text of about 2.5 tiles, {feature: offset}) -- the places the piece cuts go round, in a record that begins 100 bytes
    before a tile edge, and the '@' that begins the QUAL of the record after it"""
    rng = np.random.default_rng(201)
    lead = HEADER + b"".join(record(b"p%d" % i, _letters(rng, 150), _letters(rng, 150, b"@+>I#"), (b"NM:i:%d" % i,)) for i in range(40))
    lead += record(b"fill", _letters(rng, TILE - 100 - len(lead) - len(record(b"fill", b"", b""))), b"")
    assert len(lead) == TILE - 100
    seq, qual = _letters(rng, 300, b"ACGTacgtN"), b"@" + _letters(rng, 299, b"@+>I#")
    rec = record(b"cut@here", seq, qual, (b"NM:i:3", b"RG:Z:a"))
    tab9 = len(lead) + rec.index(seq) - 1
    marks = {"tab9": tab9, "close9": tab9 + 1 + len(seq), "nl": len(lead) + len(rec) - 1}
    text = lead + rec + record(b"ten", _letters(rng, 200)) + record(b"long", _letters(rng, TILE + 500), _letters(rng, TILE + 500, b"@+>I#")) + TAIL
    return text, marks


def piece_cuts():
    text, marks = piece_text()
    cuts = {1, len(text) - 1}
    for at in marks.values():
        cuts.update(range(at - 2, at + 3))
    return sorted(cuts)


PIECE_SIZES = (15, 16, 17, 1024, 16383, 16384, 16385)
TINY = (HEADER + record(b"a", b"ACGTTGCA", b"IIIIIIII", (b"NM:i:0",)) + record(b"b", b"acgtn") + b"\n" + record(b"c", b"*", b"*")
        + b"@CO\tx\ty\n" + record(b"d", b"GGCC", b"@@@@") + record(b"e", b"TTTT", b"IIII")[:-1])     # under 2 KB: pushed a byte at a time


@functools.lru_cache(maxsize=None)
def long_read_sam(read_len=40_000, n_reads=3):
    """long reads: SEQ and QUAL each cover whole tiles; an @CO header line of more than two tiles that holds tabs near its ends
    only; QUAL begins with '@'"""
    rng = np.random.default_rng(202)
    out = [HEADER]
    for i in range(n_reads):
        out.append(record(b"read%d" % i, _letters(rng, read_len), b"@" + _letters(rng, read_len - 1, b"@+>I#"), (b"NM:i:0", b"RG:Z:hifi")))
        if i == 0:
            out.append(b"@CO\ttabs\there\t" + _letters(rng, 2 * TILE + 3000, b"ACGT @") + b"\tand\there\n")
    out.append(record(b"ten_columns", _letters(rng, read_len)))
    return b"".join(out)


@functools.lru_cache(maxsize=None)
def qual_at_tile_text():
    """(text, offset): the QUAL of a record begins with '@' at byte 16384 -- the first byte of a tile, and of the second piece
    when the text is cut there; the byte before it is a tab, so it is no line start"""
    rng = np.random.default_rng(203)
    seq = _letters(rng, 120)
    stem = HEADER + record(b"q@0", _letters(rng, 90), b"@" * 90)
    rec = record(b"q@1", seq, b"@" + _letters(rng, 119, b"@+>I#"), (b"NM:i:0",))
    pad = TILE - len(stem) - (rec.index(seq) + len(seq) + 1)
    stem += record(b"pad", _letters(rng, pad - len(record(b"pad", b"", b""))), b"")
    text = stem + rec + TAIL
    assert text[TILE] == 64 and text[TILE - 1] == 9
    return text, TILE


def column_count_text():
    rng = np.random.default_rng(204)
    out = []
    for i in range(12):
        seq = _letters(rng, 20 + i, b"ACGTacgtN")
        out.append(record(b"c10_%d" % i, seq))
        out.append(record(b"c11_%d" % i, seq[::-1], b"I" * len(seq)))
        out.append(record(b"c30_%d" % i, seq, b"#" * len(seq), tuple(b"X%d:i:%d" % (j, j) for j in range(19))))
    return b"".join(out)


SMALL_FILES = (
    b"", b"\n", b"@", b"@HD\tVN:1.6", b"@HD\tVN:1.6\n", HEADER,
    record(b"a", b"ACGT", b"IIII"), record(b"a", b"ACGT"), record(b"a", b"*", b"*"), record(b"a", b"", b""),
    record(b"a", b"ACGT", b"IIII") + b"\n\n" + record(b"b", b"GG", b"II") + b"\n",                  # empty lines
    record(b"a", b"ACGT", b"IIII", eol=b"\r\n") + record(b"b", b"GGCC", eol=b"\r\n"),               # '\r' lands in column 9 of the second line
    record(b"a", b"acgtnN*RYKM", b"IIIIIIIIIII"),                                                    # '*' inside SEQ is dropped too
    record(b"a", b"AC GT", b"IIIII"),                                                                # a space is a byte like any other
    HEADER + record(b"a", b"ACGT", b"IIII") + b"@CO\tbetween\n" + record(b"b", b"TTTT", b"IIII"),
    record(b"a", b"ACGT", b"IIII") + record(b"last", b"GATTACA", b"IIIIIII")[:-1],                   # a last line without '\n', 11 columns
    record(b"a", b"ACGT", b"IIII") + record(b"last", b"GATTACA")[:-1],                               # ... 10 columns: ends in SEQ
    record(b"a", b"ACGT", b"IIII") + b"last\t0\tchr1",                                               # ... 3 columns: emits nothing, no error
    record(b"a", b"ACGT", b"IIII") + b"@CO\ta last header line without its line end",
    b"\t\t\t\t\t\t\t\t\tACGT\n", b"\t\t\t\t\t\t\t\t\t\n", b"x\t\t\t\t\t\t\t\t\t\t\t\t\t\n",
    record(b"a\x80\xff", b"AC\xffGT", b"\x80\x81\x82\x83\x84"),
)
LAST_LINE_10_COLUMNS, LAST_LINE_3_COLUMNS = SMALL_FILES[16], SMALL_FILES[17]

NINE = b"n\t0\tchr1\t100\t60\t4M\t*\t0\tACGT\n"                          # SEQ is its ninth column
assert NINE.count(b"\t") == 8


def _nine_at_tile_edge():
    rng = np.random.default_rng(205)
    stem = record(b"a", b"ACGT", b"IIII")
    stem += record(b"pad", _letters(rng, TILE - len(NINE) + 1 - len(stem) - len(record(b"pad", b"", b""))), b"")
    text = stem + NINE + record(b"b", b"GG", b"II")
    assert text[TILE] == 10                                             # the '\n' that comes too early is the first byte of tile 1
    return text


REFUSED = {
    "nine columns, first line": (NINE + record(b"b", b"GG", b"II"), None, FEW),
    "nine columns, last line": (HEADER + record(b"a", b"ACGT", b"IIII") + NINE, None, FEW),
    "nine columns, line end first in a tile": (_nine_at_tile_edge(), None, FEW),
    "nine columns, in the second piece": (record(b"a", b"ACGT", b"IIII") + NINE, [len(record(b"a", b"ACGT", b"IIII")) + 5], FEW),
    "one column": (b"just_a_name\n", None, FEW),
    "line starts with a carriage return": (record(b"a", b"ACGT", b"IIII") + b"\r\n" + record(b"b", b"GG", b"II"), None, CR),
    "CRLF file with a blank line": ((HEADER + record(b"a", b"ACGT", b"IIII") + b"\n" + record(b"b", b"GG", b"II")).replace(b"\n", b"\r\n"), None, CR),
}


def good_files():
    """accepted files pushed after a refusal"""
    return (HEADER + TAIL, column_count_text(), TINY)


MANY_TILES = BATCH + 2
BATCH_EDGE = BATCH * TILE                                              # the first byte of tile 1024: the second batch of the compose kernel


@functools.lru_cache(maxsize=1)
def many_tiles_sam():
    """(text of 1026 tiles, offset of the tab that opens column 9 of the record that lies across the batch edge): short reads of
    150 bases in a cycle of seven records, and one record whose column-9 tab is the last byte of tile 1023 and whose bases begin
    tile 1024"""
    rng = np.random.default_rng(206)
    cycle = b"".join(record(b"s%d" % i, _letters(rng, 150 - i, b"ACGTacgtN"), b"@" + _letters(rng, 149 - i, b"@+>I#"), (b"NM:i:%d" % i, b"AS:i:150"))
                     for i in range(7))
    n = (BATCH_EDGE - 3 * TILE) // len(cycle)
    lead = HEADER + cycle * n
    seq = _letters(rng, 10_000)
    rec = record(b"across", seq, b"@" + _letters(rng, len(seq) - 1, b"@+>I#"), (b"NM:i:0",))
    pad = BATCH_EDGE - len(lead) - rec.index(seq)
    lead += record(b"pad", _letters(rng, pad - len(record(b"pad", b"", b""))), b"")
    text = lead + rec
    text += cycle * ((MANY_TILES * TILE - 100 - len(text)) // len(cycle) + 1)
    text = text[:text.rindex(b"\n", 0, MANY_TILES * TILE - 5) + 1]
    assert (BATCH + 1) * TILE < len(text) <= MANY_TILES * TILE, len(text)
    assert text[BATCH_EDGE - 1] == 9 and text[BATCH_EDGE:BATCH_EDGE + 8] == seq[:8]
    return text, BATCH_EDGE - 1


def reads_sam(n=3000, seed=207, header=True):
    """(text, [SEQ]) -- n short reads with a few aux tags, a tenth of them without QUAL or with SEQ '*'"""
    rng = np.random.default_rng(seed)
    out, seqs = [HEADER] if header else [], []
    for i in range(n):
        seq = _letters(rng, int(rng.integers(30, 151)), b"ACGT" if i % 7 else b"ACGTN")
        if i % 10 == 3:
            out.append(record(b"r%d" % i, seq))
        elif i % 10 == 7:
            out.append(record(b"r%d" % i, b"*", b"*", flag=b"4"))
            seq = b""
        else:
            out.append(record(b"r@%d" % i, seq, b"@" + b"I" * (len(seq) - 1), (b"NM:i:%d" % (i % 5), b"MD:Z:%d" % len(seq), b"RG:Z:grp1"), flag=b"16" if i % 2 else b"0"))
        seqs.append(seq)
    return b"".join(out), seqs
