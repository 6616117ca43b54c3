"""Shared by the meryl-import tests (test_import.py, test_import_labelled.py, test_import_parse_edges.py and
test_import_edge_inputs_host.py): the parts of the model that do not depend on the dialect, database comparison, and the
inputs that put a parser event on a thread edge (16 bytes of text) or a tile edge (4096 bytes)."""
import os

import numpy as np

CODE = {"A": 0, "C": 1, "T": 2, "G": 3}
THREAD, TILE = 16, 4096                                   # text bytes per thread and per workgroup of the parse kernels


# ---- the model -------------------------------------------------------------------------------------------------------
def pick(word, k, mode):
    """the k-mer a word stands for, as a Python int: its last k bases, packed; canonical / forward / reverse complement"""
    w = word[-k:].upper()
    f = 0
    for ch in w:
        f = (f << 2) | CODE[ch]
    r = 0
    for ch in reversed(w):
        r = (r << 2) | (CODE[ch] ^ 2)
    return f if mode == 1 else r if mode == 2 else min(f, r)


def prefixes(lo, hi, k, w_prefix):
    w_data = 2 * k - w_prefix
    if w_data >= 64:
        return (hi >> np.uint64(w_data - 64)) if w_data > 64 else hi.copy()
    p = lo >> np.uint64(w_data)
    if 2 * k > 64:
        p = p | (hi << np.uint64(64 - w_data))
    return p


def assert_same_dirs(a, b):
    fa, fb = sorted(os.listdir(a)), sorted(os.listdir(b))
    assert fa == fb and len(fa) == 129, (len(fa), len(fb))
    for f in fa:
        assert open(os.path.join(a, f), "rb").read() == open(os.path.join(b, f), "rb").read(), f


def read_db(path, labels=False):
    """-> lo, hi, values, histogram values, histogram occurrences; labels: lo, hi, values, labels, the histogram, the label size"""
    from meryl_amd import db
    r = db.Reader(path)
    try:
        cols = r.read_all(labels=True) if labels else r.read_all()
        hv, ho = r.histogram()
        tail = (hv, ho, int(r.info.label_size)) if labels else (hv, ho)
    finally:
        r.close()
    return tuple(cols) + tail


# ---- inputs ----------------------------------------------------------------------------------------------------------
def rand_kmer(rng, k):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, k))


def codes_to_keys(codes, mode):
    """codes: uint8[n, k] (A0 C1 T2 G3) -> (lo, hi) uint64 of the canonical / forward / reverse k-mer"""
    n, k = codes.shape

    def pack(c):
        lo = np.zeros(n, np.uint64)
        hi = np.zeros(n, np.uint64)
        for i in range(k):
            sh = 2 * (k - 1 - i)
            if sh >= 64:
                hi |= c[:, i].astype(np.uint64) << np.uint64(sh - 64)
            else:
                lo |= c[:, i].astype(np.uint64) << np.uint64(sh)
        return lo, hi

    flo, fhi = pack(codes)
    rlo, rhi = pack(codes[:, ::-1] ^ 2)
    if mode == 1:
        return flo, fhi
    if mode == 2:
        return rlo, rhi
    f_small = (fhi < rhi) | ((fhi == rhi) & (flo < rlo))
    return np.where(f_small, flo, rlo), np.where(f_small, fhi, rhi)


def with_batch(nbytes):
    class _Env:
        def __enter__(self):
            self.old = os.environ.get("MGC_IMPORT_BATCH")
            os.environ["MGC_IMPORT_BATCH"] = str(int(nbytes))

        def __exit__(self, *a):
            if self.old is None:
                del os.environ["MGC_IMPORT_BATCH"]
            else:
                os.environ["MGC_IMPORT_BATCH"] = self.old
    return _Env()


# ---- inputs with an event on a thread or tile edge ---------------------------------------------------------------------
# dialect 1: `kmer [value]` with `#<n>` lines; dialect 2: `kmer [value [label]]` with `value=<n>` / `label=<n>` lines (label width 8)
EDGE_LABEL_WIDTH = 8
SETTERS = {1: ("#7",), 2: ("value=7", "label=5")}
SPANNING_SETTERS = {1: ("#1234567",), 2: ("value=1234567", "label=0000200")}      # 8 bytes and more: from 4090 across 4096
SETTER_PAIRS = {1: (("#1", "#2"),), 2: (("value=1", "value=2"), ("label=1", "label=2"))}
LONG_WORD, LONG_AT = 9000, 4000                            # the word covers the tiles [4096, 8192) and [8192, 12288)
EDGE_OFFSETS = (15, 16, 17, 4095, 4096, 4097, 8192)
REFUSED_OFFSETS = (16, 4096, 4097)


def line_count(chunk):
    """the lines of a chunk: one starts at byte 0 and after every newline that is not the last byte"""
    return chunk.count("\n") + (1 if chunk and not chunk.endswith("\n") else 0)


def fill(rng, k, nbytes):
    """exactly nbytes of whole lines: value-less records, and one blank line that takes up the remainder"""
    n_rec, rest = divmod(nbytes, k + 1)
    lines = [rand_kmer(rng, k) for _ in range(n_rec)]
    if rest:
        lines.insert(len(lines) // 2, " " * (rest - 1))
    return "".join(ln + "\n" for ln in lines)


def edge_cases(dialect, k, seed=0):
    """-> {family: [case]}.  A case: name; chunks (str, to be parsed in order by one parser); marks, what the chunks are built to
    hold, for check_marks; refused, None or the kind of the one refused line.  Every chunk is under 40 KiB."""
    rng = np.random.default_rng(1000 * seed + 10 * k + dialect)
    out = {}

    def case(family, name, chunks, marks, refused=None):
        out.setdefault(family, []).append({"name": name, "chunks": chunks, "marks": marks, "refused": refused})

    def rec():
        return rand_kmer(rng, k)

    for p in EDGE_OFFSETS:
        for s in SETTERS[dialect]:
            r = rec()
            case("setter_at_edge", "%s@%d" % (s, p), [fill(rng, k, p) + s + "\n" + r + "\n" + fill(rng, k, 64)],
                 [("line_at", 0, p, s), ("line_at", 0, p + len(s) + 1, r + "\n")])
    for s in SPANNING_SETTERS[dialect]:
        r = rec()
        case("setter_spanning_tiles", s, [fill(rng, k, TILE - 6) + s + "\n" + r + "\n" + fill(rng, k, 64)],
             [("line_at", 0, TILE - 6, s), ("word_ends_beyond", 0, TILE - 6, TILE), ("line_at", 0, TILE - 6 + len(s) + 1, r + "\n")])
    for a, b in SETTER_PAIRS[dialect]:
        p, r = TILE + 2 * THREAD, rec()
        case("two_setters_one_thread", a + "," + b, [fill(rng, k, p) + a + "\n" + b + "\n" + r + "\n" + fill(rng, k, 64)],
             [("line_at", 0, p, a), ("line_at", 0, p + len(a) + 1, b), ("same_thread", 0, p, p + len(a) + 1),
              ("line_at", 0, p + len(a) + len(b) + 2, r + "\n")])
    for s in SETTERS[dialect]:
        word, r = rand_kmer(rng, LONG_WORD), rec()
        end = LONG_AT + LONG_WORD + 1
        case("word_longer_than_two_tiles", s, [fill(rng, k, LONG_AT) + word + "\n" + s + "\n" + r + "\n" + fill(rng, k, 200)],
             [("line_at", 0, LONG_AT, word + "\n"), ("no_line_start", 0, TILE, 3 * TILE), ("line_at", 0, end, s),
              ("line_at", 0, end + len(s) + 1, r + "\n")])
    for s in SETTERS[dialect]:
        case("exact_tile_chunk", s, [fill(rng, k, 2000) + s + "\n" + fill(rng, k, TILE - 2000 - len(s) - 1)],
             [("length", 0, TILE), ("ends_with_newline", 0, True), ("line_at", 0, 2000, s)])
    for s in SETTERS[dialect]:
        r = rec()
        case("unterminated_last_line", s, [fill(rng, k, 5000) + s + "\n" + r],
             [("ends_with_newline", 0, False), ("line_at", 0, 5000 + len(s) + 1, r)])
    for s in SETTERS[dialect]:
        r = rec()
        case("setter_ends_chunk", s, [fill(rng, k, 3000) + s + "\n", r + "\n" + fill(rng, k, 500)],
             [("line_at", 0, 3000, s + "\n"), ("length", 0, 3000 + len(s) + 1), ("line_at", 1, 0, r + "\n")])
    bad_base = rand_kmer(rng, k // 2) + "N" + rand_kmer(rng, k - k // 2 - 1)
    for kind, bad in (("base", bad_base),) + ((("assign", "value=x"),) if dialect == 2 else ()):
        for p in REFUSED_OFFSETS:
            case("refused_line", "%s@%d" % (kind, p), [fill(rng, k, p) + bad + "\n" + fill(rng, k, 100)], [("line_at", 0, p, bad + "\n")], kind)
        word = rand_kmer(rng, LONG_WORD)
        p = LONG_AT + LONG_WORD + 1
        case("refused_line", "%s@after_long_word" % kind, [fill(rng, k, LONG_AT) + word + "\n" + bad + "\n" + fill(rng, k, 100)],
             [("line_at", 0, LONG_AT, word + "\n"), ("no_line_start", 0, TILE, 3 * TILE), ("line_at", 0, p, bad + "\n")], kind)
    return out


def check_marks(case):
    """every chunk of the case holds what its marks name"""
    for mark in case["marks"]:
        what, text = mark[0], case["chunks"][mark[1]]
        assert len(text.encode()) == len(text) < 40 * 1024, case["name"]
        if what == "line_at":                                # a line starts at byte p, with this text
            p, s = mark[2], mark[3]
            assert (p == 0 or text[p - 1] == "\n") and text[p:p + len(s)] == s, (case["name"], mark)
            assert text[p + len(s):p + len(s) + 1] in ("", "\n", " ") or s.endswith("\n"), (case["name"], mark)
        elif what == "word_ends_beyond":                     # the word that starts at p has bytes at and beyond `edge`
            p, edge = mark[2], mark[3]
            assert p < edge < p + len(text[p:].split("\n")[0].split(" ")[0]), (case["name"], mark)
        elif what == "same_thread":
            assert mark[2] // THREAD == mark[3] // THREAD, (case["name"], mark)
        elif what == "no_line_start":                        # no line starts in [a, b)
            a, b = mark[2], mark[3]
            assert a % TILE == 0 and b % TILE == 0 and b - a >= 2 * TILE and "\n" not in text[a - 1:b - 1], (case["name"], mark)
        elif what == "length":
            assert len(text) == mark[2], (case["name"], mark)
        elif what == "ends_with_newline":
            assert text.endswith("\n") == mark[2], (case["name"], mark)
        else:
            raise AssertionError(mark)
