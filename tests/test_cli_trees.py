"""`meryl` with nested set and value operations: a tree runs as one evaluation, `output` is optional on every operation of
it, `print [operation]` prints the tree's result (the reference's quick-start ends with such a command,
documentation/source/quick-start.rst:327-333) -- against the same commands staged with a database at every operation."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def meryl(native_lib):
    from meryl_amd import build
    path = build.build_cli()
    assert os.path.exists(path)
    return path


def run(meryl, *args, check=True):
    p = subprocess.run([meryl] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
    if check:
        assert p.returncode == 0, p.stderr[-2000:]
    return p


def dir_bytes(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d))}


@pytest.fixture(scope="module")
def counts(meryl, oracle_lib, tmp_path_factory):
    """two small counts of overlapping read sets, and the value filters of the tests staged as databases"""
    d = tmp_path_factory.mktemp("cli_trees")
    paths = {}
    for i, name in enumerate(("A", "B")):
        reads = oracle_lib.synth_reads(21, 60_000, i * 1500, 4000).tobytes().decode()
        fa = d / ("%s.fa" % name)
        fa.write_text("".join(">r%d\n%s\n" % (j, r) for j, r in enumerate(reads.split(".")) if r))
        paths[name] = d / ("%s.meryl" % name)
        run(meryl, "-Q", "k=21", "memory=2", "count", fa, "output", paths[name])
    return d, paths["A"], paths["B"]


def test_quick_start_print_of_a_tree(meryl, counts):
    d, A, B = counts
    run(meryl, "-Q", "at-least", "3", A, "output", d / "qa.meryl")
    run(meryl, "-Q", "at-least", "2", B, "output", d / "qb.meryl")
    run(meryl, "-Q", "intersect", d / "qa.meryl", d / "qb.meryl", "output", d / "q.meryl")
    want = run(meryl, "-Q", "print", d / "q.meryl").stdout
    assert want.count("\n") > 100
    before = sorted(os.listdir(d))
    got = run(meryl, "-Q", "print", "intersect", "[at-least", "3", str(A) + "]", "[at-least", "2", str(B) + "]").stdout
    assert got == want
    assert sorted(os.listdir(d)) == before                          # nothing was written


def test_tree_with_output_equals_the_staged_run(meryl, counts):
    d, A, B = counts
    run(meryl, "-Q", "greater-than", "1", A, "output", d / "ga.meryl")
    run(meryl, "-Q", "greater-than", "1", B, "output", d / "gb.meryl")
    run(meryl, "-Q", "union-sum", d / "ga.meryl", d / "gb.meryl", "output", d / "staged_u.meryl")
    run(meryl, "-Q", "union-sum", "[greater-than", "1", str(A) + "]", "[greater-than", "1", str(B) + "]", "output", d / "U.meryl")
    a, b = dir_bytes(d / "U.meryl"), dir_bytes(d / "staged_u.meryl")
    assert sorted(a) == sorted(b) and len(a) == 129
    assert all(a[n] == b[n] for n in a), [n for n in a if a[n] != b[n]][:5]


def test_root_without_output_writes_the_inner_output(meryl, counts):
    d, A, B = counts
    run(meryl, "-Q", "greater-than", "1", A, "output", d / "staged_inner.meryl")
    before = set(os.listdir(d))
    p = run(meryl, "-Q", "union-max", "[greater-than", "1", A, "output", str(d / "inner.meryl") + "]", B)
    assert p.stdout == ""
    assert set(os.listdir(d)) - before == {"inner.meryl"}
    assert dir_bytes(d / "inner.meryl") == dir_bytes(d / "staged_inner.meryl")


def test_threshold_from_statistics_needs_a_database(meryl, counts):
    d, A, B = counts
    before = sorted(os.listdir(d))
    p = run(meryl, "-Q", "less-than", "distinct=0.9", "[union-sum", A, str(B) + "]", "output", d / "no.meryl", check=False)
    assert p.returncode == 1 and "is not a meryl database" in p.stderr          # merylOp-nextMer.C:85-96
    assert sorted(os.listdir(d)) == before
    # with an output on the input operation its stored histogram gives the threshold, as before
    run(meryl, "-Q", "union-sum", A, B, "output", d / "ts.meryl")
    run(meryl, "-Q", "less-than", "distinct=0.9", d / "ts.meryl", "output", d / "t_staged.meryl")
    run(meryl, "-Q", "less-than", "distinct=0.9", "[union-sum", A, B, "output", str(d / "t_inner.meryl") + "]", "output", d / "t.meryl")
    assert dir_bytes(d / "t.meryl") == dir_bytes(d / "t_staged.meryl")
