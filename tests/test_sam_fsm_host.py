"""The SAM parse of the device as composable summaries (meryl_amd/csrc/mgc_sam_fsm.hpp: the summary of a run of bytes as a function
of its entry state, the composition of two summaries, the entry-state lookup -- what the kernels of mgc_parse.hip are made of),
pinned on a machine without a GPU: a stand-alone host program built with the address and undefined-behaviour sanitizers
(tests/host/sam_fsm_host.cpp) holds them against a byte-at-a-time loop of its own on the texts of tests/sam_model.py, cut at every
offset round the edges each text is named after, cut at random, and cut the way the kernels cut."""
import os
import shutil
import subprocess
import sys

sys.path.insert(0, os.path.dirname(__file__))
import sam_model as sm  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANDOM_CUTS = 300


def texts():
    """[(name, text, [centre])]"""
    out = []
    for feature in sm.FEATURES:
        for edge in sm.EDGES:
            for pad_with in ("qname", "header"):
                text = sm.edge_text(feature, edge, pad_with)
                out.append(("%s_%d_%s" % (feature, edge, pad_with), text, [edge]))
    text, marks = sm.piece_text()
    out.append(("piece", text, sorted(marks.values()) + [sm.TILE, 2 * sm.TILE]))
    text = sm.long_read_sam(17_000, 1)
    out.append(("long_reads", text, [sm.TILE * i for i in range(1, len(text) // sm.TILE + 1)]))
    text, at = sm.qual_at_tile_text()
    out.append(("qual_at_tile", text, [at]))
    out.append(("column_counts", sm.column_count_text(), [16, 1024]))
    out.append(("tiny", sm.TINY, [16, 64]))
    for i, text in enumerate(sm.SMALL_FILES):
        out.append(("small_%d" % i, text, []))
    for i, (text, cuts, _) in enumerate(sm.REFUSED.values()):
        out.append(("refused_%d" % i, text, list(cuts or []) + ([sm.TILE] if len(text) > sm.TILE else [])))
    return out


def two_part_cuts(n, centres):
    return len({c + d for c in list(centres) + [0, n] for d in range(-18, 19) if 1 <= c + d < n})


def test_sam_summaries_compose_to_what_a_byte_loop_gives(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "sam_fsm_host")
    c = subprocess.run([cxx, "-std=c++17", "-O2", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        os.path.join(ROOT, "tests", "host", "sam_fsm_host.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert c.returncode == 0, c.stderr
    args, cases = [], texts()
    for name, text, centres in cases:
        path = tmp_path / (name + ".sam")
        path.write_bytes(text)
        args += [str(path)] + ["@%d" % c for c in centres]
    p = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    tag, n_texts, two_part, random_cuts, entry_checks = p.stdout.split()
    assert tag == "ok"
    assert int(n_texts) == len(cases)
    assert int(two_part) == sum(two_part_cuts(len(text), centres) for _, text, centres in cases)
    assert int(random_cuts) == RANDOM_CUTS * sum(1 for _, text, _ in cases if text)
    assert int(entry_checks) >= 12 * (len(cases) + 2 * int(two_part) + int(random_cuts))
