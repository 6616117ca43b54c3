"""The import parser with its events on thread edges (16 bytes of text) and tile edges (4096 bytes), in both dialects.

The inputs of test_import.py / test_import_labelled.py have lines of under 100 bytes at random offsets; the ones here
(import_helpers.edge_cases; test_import_edge_inputs_host.py holds them to what they name) put a setter line, a refused line,
the end of a chunk or a word of two tiles and more exactly there.  kmer_import.Parser alone, no database; what it must
give comes from the two models, model_records (meryl 1) and model_parse (meryl 2)."""
import numpy as np
import pytest

import import_helpers as IH
from test_import import model_records
from test_import_labelled import model_parse

pytestmark = pytest.mark.gpu

MODE = 0
PARAMS = [(d, k) for d in (1, 2) for k in (21, 33)]           # both dialects; u64 and u128 keys
IDS = ["meryl%d-k%d" % p for p in PARAMS]


def model_chunks(dialect, k, chunks):
    """per chunk, by the dialect's model: ([(k-mer, value, label)] in input order, the persistent value and the persistent label
    that hold after it).  model_records has no state to hand on: it reads the text so far, and a value-less record appended
    to that text tells the persistent value"""
    out = []
    if dialect == 2:
        pval, plab = 1, 0
        for c in chunks:
            recs, pval, plab = model_parse(c, k, MODE, pval, plab)
            out.append((recs, pval, plab))
        return out
    seen, done = "", 0
    for c in chunks:
        assert seen == "" or seen.endswith("\n")
        seen += c
        recs = model_records(seen, k, MODE)
        probe = model_records(seen + "\n" + "A" * k, k, MODE)[-1][1]
        out.append(([(key, v, 0) for key, v in recs[done:]], probe, 0))
        done = len(recs)
    return out


def first_refused_line(dialect, k, text):
    """the 1-based number of the first line the dialect's model cannot read (None: it reads them all)"""
    for i, line in enumerate(text.split("\n")):
        try:
            model_chunks(dialect, k, [line])
        except (KeyError, ValueError):
            return i + 1
    return None


def run_case(dialect, k, case):
    import torch
    from meryl_amd import kmer_import
    lw = IH.EDGE_LABEL_WIDTH if dialect == 2 else 0
    parser = kmer_import.Parser(k, MODE, label_width=lw)
    want = model_chunks(dialect, k, case["chunks"]) if not case["refused"] else [None] * len(case["chunks"])
    for chunk, w in zip(case["chunks"], want):
        out = parser.parse(torch.frombuffer(bytearray(chunk.encode()), dtype=torch.uint8).cuda())
        res = out[-1]
        if case["refused"]:
            assert out[0] is None and kmer_import.BAD_NAMES[res.bad_kind] == case["refused"], (case["name"], res.bad_kind)
            assert res.bad_line == first_refused_line(dialect, k, chunk), (case["name"], res.bad_line)
            continue
        recs, pval, plab = w
        assert res.bad_kind == 0 and res.bad_line == 0, case["name"]
        assert res.n_lines == IH.line_count(chunk) and res.n_records == len(recs), case["name"]
        kk = out[0].cpu().numpy().view(np.uint64)
        vv = out[1].cpu().numpy().view(np.uint32)
        ll = out[2].cpu().numpy().view(np.uint64) if dialect == 2 else np.zeros(len(recs), np.uint64)
        got = [((int(kk[j]) if k <= 32 else int(kk[j, 0]) | (int(kk[j, 1]) << 64)), int(vv[j]), int(ll[j])) for j in range(kk.shape[0])]
        assert got == recs, case["name"]
        assert res.persistent_value == pval, case["name"]
        if dialect == 2:
            assert parser.persistent_label == plab, case["name"]


@pytest.fixture(scope="module")
def cases():
    return {p: IH.edge_cases(*p) for p in PARAMS}


FAMILIES = ["setter_at_edge", "setter_spanning_tiles", "two_setters_one_thread", "word_longer_than_two_tiles", "exact_tile_chunk",
            "unterminated_last_line", "setter_ends_chunk", "refused_line"]


@pytest.mark.parametrize("dialect,k", PARAMS, ids=IDS)
@pytest.mark.parametrize("family", FAMILIES)
def test_parser_at_edges(native_lib, cases, family, dialect, k):
    """setter_at_edge: a setter line whose first byte is at 15, 16, 17, 4095, 4096, 4097, 8192, then a value-less record;
    setter_spanning_tiles: one from 4090 whose number ends beyond 4096; two_setters_one_thread: the later one wins;
    word_longer_than_two_tiles: 9000 bases, two whole tiles without a line start, the key is the last k bases and every later
    slot is right; exact_tile_chunk: 4096 bytes ending in a newline; unterminated_last_line; setter_ends_chunk: the next chunk
    opens with a value-less record (commit); refused_line: bad base / `value=x` at 16, 4096, 4097 and after the long word"""
    todo = cases[(dialect, k)][family]
    assert todo
    for case in todo:
        run_case(dialect, k, case)
