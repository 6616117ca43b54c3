"""The inputs of test_import_parse_edges.py, without a device: every one holds the edge it names, and the dialect's model
gives an expectation for every one -- so the edge test compares each of its cases and skips none."""
import pytest

import import_helpers as IH
from test_import_parse_edges import FAMILIES, PARAMS, IDS, first_refused_line, model_chunks


@pytest.mark.parametrize("dialect,k", PARAMS, ids=IDS)
def test_inputs_hold_their_edges(dialect, k):
    cases = IH.edge_cases(dialect, k)
    assert sorted(cases) == sorted(FAMILIES)
    for family in FAMILIES:
        assert cases[family], family
        for case in cases[family]:
            assert case["marks"] and all(0 < len(c) < 40 * 1024 for c in case["chunks"])
            IH.check_marks(case)
    # the offsets the families are built around
    starts = {m[2] for c in cases["setter_at_edge"] for m in c["marks"][:1]}
    assert starts == {15, 16, 17, 4095, 4096, 4097, 8192} and len(cases["setter_at_edge"]) == 7 * len(IH.SETTERS[dialect])
    for case in cases["setter_spanning_tiles"]:
        assert case["marks"][0][2] == 4090
    for case in cases["word_longer_than_two_tiles"]:
        word = case["chunks"][0][IH.LONG_AT:].split("\n")[0]
        assert len(word) == 9000 and set(word) <= set("ACGT")
    for case in cases["exact_tile_chunk"]:
        assert len(case["chunks"][0]) == 4096 and case["chunks"][0][-1] == "\n"
    for case in cases["setter_ends_chunk"]:
        assert len(case["chunks"]) == 2 and case["chunks"][0].split("\n")[-2] in IH.SETTERS[dialect]
    at = sorted(str(c["name"]).split("@")[1] for c in cases["refused_line"] if c["refused"] == "base")
    assert at == sorted(["16", "4096", "4097", "after_long_word"])
    assert {c["refused"] for c in cases["refused_line"]} == ({"base", "assign"} if dialect == 2 else {"base"})


@pytest.mark.parametrize("dialect,k", PARAMS, ids=IDS)
def test_the_model_reads_every_input(dialect, k):
    for family, todo in IH.edge_cases(dialect, k).items():
        for case in todo:
            if case["refused"]:
                # one refused line, where the mark says; the model reads the text once that line is taken out
                (chunk,), mark = case["chunks"], case["marks"][-1]
                line = first_refused_line(dialect, k, chunk)
                assert line == chunk[:mark[2]].count("\n") + 1 >= 2, case["name"]
                rest = chunk[:mark[2]] + chunk[mark[2] + len(mark[3]):]
                assert first_refused_line(dialect, k, rest) is None and model_chunks(dialect, k, [rest])[0][0], case["name"]
                continue
            want = model_chunks(dialect, k, case["chunks"])
            assert len(want) == len(case["chunks"]) and all(recs for recs, _, _ in want), case["name"]
            for chunk, (recs, _, _) in zip(case["chunks"], want):
                assert first_refused_line(dialect, k, chunk) is None
                assert IH.line_count(chunk) > len(recs), case["name"]
            # the setter governs the value-less record behind it: the input is about what it says it is about
            if family in ("setter_at_edge", "word_longer_than_two_tiles", "unterminated_last_line", "setter_ends_chunk"):
                setter = case["name"].split("@")[0]
                recs, pval, plab = want[-1]
                n = int(setter.split("=")[-1].lstrip("#"))
                assert (plab if setter.startswith("label") else pval) == n
                assert [r for r in recs if (r[2] if setter.startswith("label") else r[1]) == n], case["name"]
            if family == "two_setters_one_thread":
                recs, pval, plab = want[-1]
                assert (plab if "label" in case["name"] else pval) == 2
