"""A sequential model of the device text parser (meryl_amd/csrc/mgc_parse.hip) and the texts that try it.

The model is written from the contract of mgc_begin_text / mgc_push_text / mgc_end_text in include/meryl_gpu_count.h and the
header comment of mgc_parse.hip, not from the kernels.  A LINE START is a byte that exists and either begins the file or follows
'\\n'; white space is '\\n' '\\r' ' ' '\\t'.

  FASTA  a line start that is '>' emits '.' and makes its line a header line, which emits nothing else; every other line emits
         its bytes that are not white space, as they are ('>', '@', lower case and bytes >= 0x80 included); mgc_end_text adds
         one '.'.
  FASTQ  the type of a byte's line is (newlines strictly before the byte) mod 4; a type-0 line start emits '.', type-1 lines
         emit their bytes that are not white space, nothing else is emitted, and mgc_end_text adds one '.'.  The file is
         refused iff some type-0 line start is not '@' or some type-2 line start is not '+'.

Two forms that must agree: model_loop (a byte at a time; small texts) and model (numpy; 17 MB in well under a second).  Both
return (stream, refused, src): src[i] is the input offset output byte i was taken from, len(text) for the final '.'.

The case builders return bytes; line_starts and tiles_without_line_start are the predicates by which
tests/test_text_model_host.py makes sure that a case really holds the edge it is named after.  No GPU is used here."""
import functools

import numpy as np

TILE = 16384                        # mgc_parse.hip: 1024 threads of 16 bytes
THREAD = 16
WAVE = 1024                         # 64 threads of 16 bytes
BATCH = 1024                        # tiles the compose kernel takes at a time
WS = b"\n\r \t"
FASTA, FASTQ = "fasta", "fastq"


# ---- the model -----------------------------------------------------------------------------------------------------------
def model_loop(text, fmt):
    out, src, refused = bytearray(), [], False
    newlines, header = 0, False
    for i, c in enumerate(text):
        ls = i == 0 or text[i - 1] == 10
        if fmt == FASTA:
            if ls:
                header = c == 62
                if header:
                    out.append(46)
                    src.append(i)
            if not header and c not in WS:
                out.append(c)
                src.append(i)
        else:
            kind = newlines % 4
            if ls and kind == 0:
                out.append(46)
                src.append(i)
                refused |= c != 64
            elif kind == 1 and c not in WS:
                out.append(c)
                src.append(i)
            if ls and kind == 2:
                refused |= c != 43
            newlines += c == 10
    out.append(46)
    src.append(len(text))
    return bytes(out), bool(refused), np.asarray(src, dtype=np.int64)


def _masks(text):
    a = np.frombuffer(text, dtype=np.uint8)
    nl = a == 10
    ls = np.empty(a.size, dtype=bool)
    if a.size:
        ls[0] = True
        ls[1:] = nl[:-1]
    ws = nl | (a == 13) | (a == 32) | (a == 9)
    return a, nl, ls, ws


def model(text, fmt):
    a, nl, ls, ws = _masks(text)
    refused = False
    if fmt == FASTA:
        starts = np.flatnonzero(ls)
        line = np.cumsum(ls) - 1                                       # every byte lies at or after line start 0
        header = (a[starts] == 62)[line] if a.size else ls
        dot = ls & (a == 62)
        emit = dot | ~(header | ws)
    else:
        kind = (np.cumsum(nl) - nl) & 3                                # newlines strictly before the byte
        dot = ls & (kind == 0)
        emit = dot | ((kind == 1) & ~ws)
        refused = bool((dot & (a != 64)).any() or (ls & (kind == 2) & (a != 43)).any())
    src = np.flatnonzero(emit)
    out = np.where(dot, np.uint8(46), a)[src]
    return out.tobytes() + b".", refused, np.append(src, a.size).astype(np.int64)


# ---- predicates ----------------------------------------------------------------------------------------------------------
def line_starts(text):
    return np.flatnonzero(_masks(text)[2])


def piece_bounds(n, piece=None):
    """[(begin, end)] of the pieces: piece None -- the whole text; an int -- uniform pieces; a list -- the cut offsets"""
    if piece is None:
        cuts = []
    elif isinstance(piece, int):
        cuts = list(range(piece, n, piece))
    else:
        cuts = list(piece)
    edges = [0] + cuts + [n]
    return [(b, e) for b, e in zip(edges[:-1], edges[1:]) if e > b]


def tile_bounds(n, piece=None):
    """[(begin, end)] of the parser's tiles: every piece is cut into tiles of 16 KiB from its own first byte"""
    return [(t, min(t + TILE, e)) for b, e in piece_bounds(n, piece) for t in range(b, e, TILE)]


def entry_states(text, fmt):
    """per byte, the state in which a tile that began there would be entered.  FASTA: 0 = header (or nothing yet), 1 = sequence
    -- the kind of the line the byte BEFORE belongs to; FASTQ: the type of the byte's own line"""
    a, nl, ls, _ = _masks(text)
    if fmt == FASTQ:
        return (np.cumsum(nl) - nl) & 3
    starts = np.flatnonzero(ls)
    seq = (a[starts] != 62).astype(np.int64)
    own = seq[np.cumsum(ls) - 1] if a.size else seq
    return np.concatenate([[0], own[:-1]])


def tiles_without_line_start(text, piece=None, fmt=FASTA):
    """{entry state: [tile index]} of the tiles that hold no line start; tiles are numbered through all pieces in order"""
    ls = _masks(text)[2]
    before = np.concatenate([[0], np.cumsum(ls)])
    state = entry_states(text, fmt)
    found = {}
    for t, (b, e) in enumerate(tile_bounds(len(text), piece)):
        if before[e] == before[b]:
            found.setdefault(int(state[b]), []).append(t)
    return found


def has_run(tiles, length=2):
    """some `length` consecutive numbers among the tile indices"""
    have = set(tiles)
    return any(all(t + j in have for j in range(length)) for t in have)


# ---- texts ---------------------------------------------------------------------------------------------------------------
def _letters(rng, n, alphabet=b"ACGT"):
    return rng.choice(np.frombuffer(alphabet, dtype=np.uint8), size=n).tobytes()


@functools.lru_cache(maxsize=None)
def long_line_fasta():
    """about 8 tiles: a sequence line of 3 tiles + 5 with a '>' in its middle (tiles 1 and 2 hold no line start, entered in
    sequence state), short records up to 60 bytes before tile 4, a header line of 2 tiles + 100 full of ACGT> letters (tiles 4
    and 5: none, entered in header state), directly after it a second long sequence line, a last record without a line end"""
    rng = np.random.default_rng(101)
    seq = bytearray(_letters(rng, 3 * TILE + 5))
    seq[TILE + 5000] = 62
    out = [b">r0 ACGT\n", bytes(seq), b"\n"]
    at, i = sum(map(len, out)), 0
    while at < 4 * TILE - 60 - 80:
        rec = b">f%d\n" % i + _letters(rng, 60, b"ACGTacgtN") + b"\n"
        out.append(rec)
        at += len(rec)
        i += 1
    pad = 4 * TILE - 60 - at                                           # one more record of exactly the bytes that are left
    assert pad >= 6
    out.append(b">p\n" + _letters(rng, pad - 4) + b"\n")
    out.append(b">" + _letters(rng, 2 * TILE + 98, b"ACGT>") + b"\n")
    out.append(_letters(rng, 2 * TILE + 50) + b"\n")
    out.append(b">last\nacgtnACGT")
    return b"".join(out)


@functools.lru_cache(maxsize=None)
def long_read_fastq(n_reads=6, read_len=40_000):
    """reads of 40 000 bases: sequence and quality lines cover whole tiles; qualities of '@+>I#' that begin with '@' on reads
    0, 3, .. and with '+' on reads 1, 4, ..; a '+name' separator on every other read"""
    rng = np.random.default_rng(102)
    out = []
    for i in range(n_reads):
        q = bytearray(_letters(rng, read_len, b"@+>I#"))
        if i % 3 < 2:
            q[0] = b"@+"[i % 3]
        out.append(b"@read%d ACGT\n" % i + _letters(rng, read_len) + b"\n" + (b"+read%d\n" % i if i % 2 else b"+\n") + bytes(q) + b"\n")
    return b"".join(out)


EDGES = (THREAD, WAVE, TILE, 2 * TILE)
EDGE_DELTAS = tuple(range(-18, 19))
EDGE_KINDS = {FASTA: ("sequence", "header"), FASTQ: ("type0", "type1", "type2", "type3")}


def edge_text(fmt, eol, kind, at):
    """a text of at least `at` + 64 bytes whose first header is padded so that a line start of the wanted kind is byte `at`;
    None when `at` is too small for that.  FASTA kinds: the first sequence line, the second header; FASTQ kinds: the line of
    that type (type0: the second record's '@' line)"""
    if fmt == FASTA:
        before = {"sequence": b"", "header": b"ACgT" + eol}[kind]
        after = (b"TTGCA" + eol if kind == "sequence" else b"") + b">s ACGT" + eol + b"GATTACAGATTACAGATTACAGATTACA" + eol + b"CCCC" + eol + b">e" + eol + b"AC" * 20
    else:
        lines = [b"ACGTA", b"+", b"@+>I#", b"@x ACGT"]
        n = ("type1", "type2", "type3", "type0").index(kind)
        before = b"".join(ln + eol for ln in lines[:n])
        after = b"".join(ln + eol for ln in lines[n:]) + b"GATTACAGATTACAGATTACAGATTACA" + eol + b"+x" + eol + b"@@@@++++>>>>IIII####@@@@++++" + eol + b"@y" + eol + b"AC" + eol + b"+" + eol + b"+@"
    pad = at - len(before) - len(eol) - 1
    if pad < 0:
        return None
    lead = b">" if fmt == FASTA else b"@"
    text = lead + (b"ACGT>@+ " * (pad // 8 + 1))[:pad] + eol + before + after
    assert len(text) >= at + 64
    return text


def edge_cases(fmt):
    """[(edge, delta, line end, kind, text)] for every edge, every delta in -18 .. +18, both line ends and every kind"""
    cases = []
    for edge in EDGES:
        for d in EDGE_DELTAS:
            for eol in (b"\n", b"\r\n"):
                for kind in EDGE_KINDS[fmt]:
                    text = edge_text(fmt, eol, kind, edge + d)
                    if text is not None:
                        cases.append((edge, d, eol, kind, text))
    return cases


@functools.lru_cache(maxsize=None)
def piece_text(fmt):
    """(text of about 3 tiles, {name: offset}) -- the places the two-piece cuts go round: 'crlf' (the '\\r' of a pair), 'record'
    (the '\\n' before a '>' / '@' line start), 'header' (inside a header line of more than a tile: a piece cut there begins with
    a tile that holds no line start and is entered in header state), 'quality' (FASTQ: inside a quality line that begins with
    '@'), 'tile' (16384)"""
    rng = np.random.default_rng(103 + (fmt == FASTQ))
    marks = {"tile": TILE}
    if fmt == FASTA:
        out = [b">a ACGT\r\n", _letters(rng, 70), b"\r\n", _letters(rng, 33, b"acgtn"), b"\r\n"]
        marks["crlf"] = sum(map(len, out)) - 2
        out += [b">b\n", _letters(rng, TILE + 300), b"\n"]
        marks["record"] = sum(map(len, out)) - 1
        out += [b">c "]
        marks["header"] = sum(map(len, out)) + 200
        out += [_letters(rng, TILE + 2000, b"ACGT> "), b"\n", _letters(rng, 9000), b"\n>d\n\nAC GT\tA\n>e\nacgt"]
    else:
        out = [b"@a ACGT\r\n", _letters(rng, 70), b"\r\n+\r\n", _letters(rng, 70, b"@+>I#"), b"\r\n"]
        marks["crlf"] = sum(map(len, out)) - 2
        out += [b"@b\n", _letters(rng, TILE + 300), b"\n+b\n@", _letters(rng, TILE + 299, b"@+>I#"), b"\n"]
        marks["quality"] = sum(map(len, out)) - 8000
        marks["record"] = sum(map(len, out)) - 1
        out += [b"@c "]
        marks["header"] = sum(map(len, out)) + 200
        out += [_letters(rng, TILE + 2000, b"ACGT@+ "), b"\n", _letters(rng, 500), b"\n+\n+", _letters(rng, 499, b"@+>I#"), b"\n@d\n\n+\n\n@e\nAC\n+\n@+"]
    return b"".join(out), marks


def piece_cuts(fmt):
    text, marks = piece_text(fmt)
    cuts = {1, len(text) - 1}
    for at in marks.values():
        cuts.update(range(at - 3, at + 4))
    return sorted(cuts)


PIECE_SIZES = (15, 16, 17, 1024, 16383, 16384, 16385)


def tiny_piece_text(fmt):
    """under 2 KB: pushed a byte at a time"""
    if fmt == FASTA:
        return b">a ACGT\r\nACGTTGCA\r\nacgt\r\n\r\n>b\n\n>c\nGG CC\tTT\n>d" + b"ACGT" * 300 + b"\nGATTACA>\n"
    return b"@a ACGT\r\nACGTTGCA\r\n+a\r\n@+>I#@+>\r\n@b\n\n+\n\n@c\n" + b"ACGT" * 200 + b"\n+\n@" + b"+@I#" * 199 + b"+++\n"


MANY_TILES = BATCH + 2                                                 # one piece of 1026 tiles: a second batch of two tiles
LONG_BEGIN = (BATCH - 2) * TILE + 777                                  # where the line that crosses the batch edge begins ...
LONG_END = (BATCH + 1) * TILE + 4321                                   # ... and from where its line end is looked for


@functools.lru_cache(maxsize=2)
def many_tiles_fasta(kind):
    """1026 tiles of FASTA, lines of 60 bytes, every fifth a header (of base letters), and one line that begins in tile 1022
    and ends in tile 1025: a header line (kind "header") or a sequence line ("sequence"; the '>' of the header lines it
    swallowed are bytes of it).  Returns (text, offset of that line's start)."""
    rng = np.random.default_rng(104)
    n = MANY_TILES * TILE
    a = rng.choice(np.frombuffer(b"ACGTacgtN", dtype=np.uint8), size=n)
    a[60::61] = 10
    a[0::5 * 61] = 62
    begin = (LONG_BEGIN // 61 + 1) * 61
    if begin % (5 * 61) == 0:
        begin += 61
    a[begin:LONG_END][a[begin:LONG_END] == 10] = 65
    a[begin] = 62 if kind == "header" else 71
    return a.tobytes(), begin


FASTQ_READ = 40_000
FASTQ_RECORD = 4 + FASTQ_READ + 1 + 2 + FASTQ_READ + 1
FASTQ_RECORDS = 210
FASTQ_LAST = FASTQ_RECORDS * FASTQ_RECORD                              # the offset of the last, short record: in tile 1025


@functools.lru_cache(maxsize=2)
def many_tiles_fastq(violation):
    """1026 tiles (the last one partial) of FASTQ: 210 records of 40 000 bases whose qualities, of '@+>I#', begin with '@', and
    a short last record that begins in tile 1025.  With `violation` that record's line begins with 'A' in place of '@'."""
    rng = np.random.default_rng(105)
    rec = np.empty((FASTQ_RECORDS, FASTQ_RECORD), dtype=np.uint8)
    rec[:, 0:4] = np.frombuffer(b"@rA\n", dtype=np.uint8)
    rec[:, 4:4 + FASTQ_READ] = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=(FASTQ_RECORDS, FASTQ_READ))
    rec[:, 4 + FASTQ_READ:7 + FASTQ_READ] = np.frombuffer(b"\n+\n", dtype=np.uint8)
    rec[:, 7 + FASTQ_READ:-1] = rng.choice(np.frombuffer(b"@+>I#", dtype=np.uint8), size=(FASTQ_RECORDS, FASTQ_READ))
    rec[:, 7 + FASTQ_READ] = 64
    rec[:, -1] = 10
    return rec.tobytes() + (b"A" if violation else b"@") + b"z\nGATTACAGATTACAGATTACAGATTACA\n+\n@+@+@+@+@+@+@+@+@+@+@+@+@+@+\n"


SMALL_FILES = (
    (FASTA, b""), (FASTQ, b""), (FASTA, b"\n"), (FASTA, b">"), (FASTQ, b"@"), (FASTA, b">h"), (FASTQ, b"@h"),
    (FASTA, b"ACGT\nAC\n>r\nGG\n"),                                    # sequence before any header: emitted, no leading '.'
    (FASTQ, b"@a\n\n+\n\n"),                                           # an empty read
    (FASTA, b">a\n>b\n\n>c\nA\n>d\n"),                                 # empty records, one base
    (FASTA, b">ends in a header ACGT"), (FASTA, b"TTTT\n>x\nAC"),      # the second file starts in sequence state: begin resets
    (FASTQ, b"@ends in a header ACGT"), (FASTQ, b"@x\nAC"),
    (FASTA, b">s\nAC GT\tAC\n A C\t\n\t\nGG\n"), (FASTQ, b"@s\nAC GT\tAC \n+\n@@ @@\t@@\n"),
    (FASTA, b">iupac\nACGTURYKMSWBDHVN-acgturykmswbdhvn*\n"), (FASTQ, b"@iupac\nACGTURYKMSWBDHVN-acgturykmswbdhvn*\n+\n" + b"I" * 34 + b"\n"),
    (FASTA, b">h\x80\xff\xc3\xa9>\n" + bytes(range(0x80, 0x100)) + b"\nAC\xffGT\n"),
    (FASTQ, b"@h\x80\xff\n" + bytes(range(0x80, 0x100)) + b"\n+\x80\n" + bytes(range(0x80, 0x100)) + b"\n"),
    (FASTA, b">a\r\nAC\rGT\r\n\r\n>b\r\n\rA\r\n"), (FASTA, b"\n\n>a\nAC\n"), (FASTA, b">a\n>>\n@\n+\n.\n"),
)

REFUSED_FASTQ = {
    "blank line between records": b"@a\nACGT\n+\nIIII\n\n@b\nAC\n+\nII\n",
    "two-line sequence": b"@a\nACGT\nACGT\n+\nIIII\nIIII\n",
    "missing + line": b"@a\nACGT\nIIII\n@b\nAC\n+\nII\n",
    "trailing blank line": b"@a\nACGT\n+\nIIII\n\n",
    "first byte is not @": b">a\nACGT\n+\nIIII\n",
    "first byte is a line end": b"\n@a\nACGT\n+\nIIII\n",
    "empty + line": b"@a\nACGT\n\nIIII\n",
    "violation first in a tile": b"@" + b"h" * (TILE - 14) + b"\nACGT\n+\nIIII\nAb\nAC\n+\nII\n",
    "+ violation first in a tile": b"@" + b"h" * (2 * TILE - 7) + b"\nACGT\n-\nIIII\n@b\nAC\n+\nII\n",
}
assert REFUSED_FASTQ["violation first in a tile"][TILE] == 65 and REFUSED_FASTQ["+ violation first in a tile"][2 * TILE] == 45
PIECE_VIOLATION = (b"@a\nACGT\n+\nIIII\nAb\nAC\n+\nII\n", 15)                # the violation is the first byte of the second piece


def accepted_fastq():
    """model-good files whose qualities begin with '@' or '+' on every record"""
    rng = np.random.default_rng(106)
    plain = b"".join(b"@r%d\n%s\n+\n%s%s\n" % (i, _letters(rng, 30 + i), b"@+"[i % 2:i % 2 + 1], _letters(rng, 29 + i, b"@+>I#")) for i in range(40))
    crlf = plain.replace(b"\n", b"\r\n")
    return plain, crlf, plain[:-1], b"@a\nA\n+\n@\n@b\nC\n+\n+\n"
