"""Value assignment in operation trees (meryl2; merylOpCompute::findOutputValue, src/meryl2/merylOpCompute.C:136-282), on the device:
the ASSIGN instantiations of merge_many_kernel against the Python statement of the rules in assign_helpers.py, the count pass
against the emit pass, assignments beside programs and label operations, the identities with the existing entry points, whole
trees through mgc_db_eval_assigned against the model applied to the decoded leaves, and the command line.  Everything is exact."""
import os
import subprocess

import numpy as np
import pytest

import assign_helpers as A
import eval_helpers as H
import label_helpers as LH
import select_helpers as S
import test_merge_many as TM
import test_select as TS
from test_labels import dir_bytes, host_keys

pytestmark = pytest.mark.gpu

M32 = A.M32
PRESENCE = (10, 6, 7, 8, 9)                      # union, intersect, subtract, difference, symmetric-difference
# every word with its default constant (None) and an explicit one that decides with the values of test_select.World (1..999, every
# third of every other input anywhere below 2^32)
RULES = [("set", 0), ("set", 7), ("first", None), ("selected", None), ("min", None), ("min", 5), ("max", None), ("max", 500), ("add", None),
         ("add", M32 - 300), ("sub", None), ("sub", 30), ("mul", None), ("mul", 3), ("div", None), ("div", 50), ("divzero", None), ("divzero", 2),
         ("mod", None), ("mod", 7), ("count", None)]


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


def constant_of(word, c):
    return A.DEFAULT_CONSTANT.get(A.SET if word == "set" else A.WORDS[word], 0) if c is None else c


def text_of(word, c):
    return ("#%d" % c) if word == "set" else word if c is None else "%s#%d" % (word, c)


class World(TS.World):
    """test_select.World with the groups of equal keys kept for the model"""

    def __init__(self, torch, rng, keys, kw):
        super().__init__(torch, rng, keys, kw)
        self.groups = A.groups_of(self.inputs)

    def check(self, ops, op, word, c, words=(), label_word="default", label_constant=None, stats=None):
        from meryl_amd import db
        terms, model_terms = db.parse_selector(list(words), self.N), S.parse(list(words), self.N)
        lc = LH.DEFAULT_CONSTANT.get(label_word, 0) if label_constant is None else label_constant
        wk, wv, wl = A.merge_assigned(self.inputs, op, (word, constant_of(word, c)), (label_word, lc), model_terms, self.k, groups=self.groups,
                                      stats=stats)
        what = (TM.OP_WORDS[op], word, c, words, label_word)
        value = text_of(word, c)                                     # through the one parser, as the command line does
        n = ops.dev_merge_many_assigned(self.dk, self.dc, self.dl, self.k, op, value, terms, label_word, label_constant, count_only=True)
        assert n == len(wk), what                                    # the count pass alone: the length the emit pass is given room for
        ok, oc, ol, n2 = ops.dev_merge_many_assigned(self.dk, self.dc, self.dl, self.k, op, value, terms, label_word, label_constant)
        assert n2 == n and ok.shape[0] == n, what
        assert host_keys(ok, self.kw) == wk, what
        assert oc.cpu().numpy().view(np.uint32).tolist() == wv, what
        assert ol.cpu().numpy().view(np.uint64).tolist() == wl, what
        return len(wk)


@pytest.mark.parametrize("shape", TS.SHAPE_NAMES)
@pytest.mark.parametrize("kw", [1, 2])
@pytest.mark.parametrize("N", [1, 2, 3, 32])
def test_merge_many_with_an_assignment_against_the_model(ops, torch_cuda, native_lib, N, kw, shape):
    T = native_lib.mgc_dev_merge_many_tile(kw)
    rng = np.random.default_rng(13600 + 100 * N + 10 * kw + TS.SHAPE_NAMES.index(shape))
    keys = TS.shapes(N, T)[shape](rng, kw)
    assert len(keys) == N and sum(a.shape[0] for a in keys) <= 3 * T + 64 * N
    w = World(torch_cuda, rng, keys, kw)
    stats = {}
    for word, c in RULES:
        st = stats.setdefault(word, {})
        for op in PRESENCE:
            w.check(ops, op, word, c, stats=st)
    if shape in ("all-empty", "single-elements"):
        return
    # on the model: a kernel that ignores the rule cannot pass -- zero values drop k-mers and others stay, sums and products saturate
    for word in ("sub", "div", "mod", "set"):
        assert stats[word].get("zero", 0) > 0 and stats[word].get("kept", 0) > 0, (word, stats[word])
    for word in ("add", "mul"):
        assert stats[word].get("saturated", 0) > 0, (word, stats[word])


@pytest.fixture(scope="module")
def plain_world(torch_cuda, native_lib):
    """three overlapping streams of 8-byte keys over a little more than one tile"""
    T = native_lib.mgc_dev_merge_many_tile(1)
    rng = np.random.default_rng(137)
    return World(torch_cuda, rng, TM.shapes(3, T)["sum-T+1"](rng, 1), 1)


def test_programs_see_the_assigned_value(ops, plain_world):
    w = plain_world
    everything = len(w.groups)
    n = w.check(ops, 10, "count", None, ["value:>=2"])                   # value:>=2 after value=count: in at least two inputs
    assert n == sum(1 for _, a in w.groups if len(a) >= 2) and 0 < n < everything
    st = {}
    n = w.check(ops, 10, "sub", None, ["value:@1>@2"], stats=st)          # the inputs' values beside the assigned one
    assert 0 < n < st["present"] - st["zero"]
    n = w.check(ops, 6, "sub", 3, ["value:<10", "or", "value:@3>500"])
    assert n > 0
    w.check(ops, 0, "max", 500, ["not", "value:==#500"])                  # the floor itself is the output value
    w.check(ops, 9, "divzero", 2, ["input:@2", "value:>1"])


def test_label_selected_follows_the_assignment(ops, plain_world):
    w = plain_world
    for op in (10, 6, 1, 5):                                             # also where the operation's default is `selected`
        for word in ("min", "max", "sub"):
            w.check(ops, op, word, None, (), "selected" if op in (10, 6) else "default")
    # min -> the label of the first active input with the smallest value, max -> the largest, anything else -> the first
    _, a = next((key, a) for key, a in w.groups if len(a) == 3 and len({v for _, v, _ in a}) == 3 and a[0][1] not in (min(v for _, v, _ in a), max(v for _, v, _ in a)))
    L, V = [l for _, _, l in a], [v for _, v, _ in a]
    assert A.label_under(("min", M32), "selected", 0, L, V, 10) == L[V.index(min(V))]
    assert A.label_under(("max", 0), "selected", 0, L, V, 10) == L[V.index(max(V))]
    assert A.label_under(("sub", 0), "default", 0, L, V, 1) == L[0]
    w.check(ops, 10, "add", None, ["label:>=4"], "or")                    # a label term in the count pass beside an assignment
    w.check(ops, 7, "div", 2, (), "difference", 0b1)


def test_identities_with_the_existing_entry_points(ops, torch_cuda, native_lib):
    from meryl_amd import db
    torch = torch_cuda
    T = native_lib.mgc_dev_merge_many_tile(1)
    rng = np.random.default_rng(138)
    w = World(torch, rng, TM.shapes(3, T)["sum-T+1"](rng, 1), 1)
    small = [torch.from_numpy(rng.integers(1, 1000, c.shape[0]).astype(np.int32)).cuda() for c in w.dc]      # nothing overflows
    for value, op_assigned, op_plain in (("sum", 10, 0), ("add", 0, 0), ("min", 6, 4), ("count", 10, 10), ("count", 0, 10), ("max", 3, 5)):
        ak, ac, _, n = ops.dev_merge_many_assigned(w.dk, small, None, w.k, op_assigned, value, with_labels=False)
        pk, pc = ops.dev_merge_many(w.dk, small, op_plain)
        assert n == pk.shape[0] > 0 and torch.equal(ak, pk) and torch.equal(ac, pc), (value, op_assigned, op_plain)
    # MGC_ASSIGN_NONE is the selected entry point, with and without a program, labels and huge values included
    for op, words in ((0, []), (7, ["value:@1>5"]), (1, ["label:>=2", "or", "input:all"])):
        terms = db.parse_selector(words, 3)
        for value in (None, ("none", 0), 0):
            got = ops.dev_merge_many_assigned(w.dk, w.dc, w.dl, w.k, op, value, terms)
            want = ops.dev_merge_many_selected(w.dk, w.dc, w.dl, w.k, op, terms)
            assert got[3] == want[3] > 0 and all(torch.equal(g, x) for g, x in zip(got[:3], want[:3])), (op, words, value)
        assert ops.dev_merge_many_assigned(w.dk, w.dc, w.dl, w.k, op, None, terms, count_only=True) == want[3]
    # union-sum keeps wrapping where value=add saturates
    ak, ac, _, _ = ops.dev_merge_many_assigned(w.dk, w.dc, None, w.k, 0, "add", with_labels=False)
    pk, pc = ops.dev_merge_many(w.dk, w.dc, 0)
    assert torch.equal(ak, pk) and not torch.equal(ac, pc)
    assert (ac.cpu().numpy().view(np.uint32) == M32).any()


# ---- whole trees against the model on the decoded leaves -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def world(native_lib, torch_cuda, tmp_path_factory):
    """databases A, B, C, D (k = 21, 3000-5000 k-mers from one pool, values 1..9)"""
    wdir = str(tmp_path_factory.mktemp("assign_world"))
    rng = np.random.default_rng(139)
    plo, phi = H.random_kmers(rng, 21, 9000)
    for name, n in (("A", 5000), ("B", 4000), ("C", 3000), ("D", 4000)):
        idx = np.sort(rng.choice(plo.size, n, replace=False))
        H.write_db(os.path.join(wdir, name), plo[idx], phi[idx], rng.integers(1, 10, idx.size).astype(np.uint32), 21, 8)
    return wdir


def as_input(d):
    keys = sorted(d)
    return keys, [d[x][0] for x in keys], [d[x][1] for x in keys]


def run_assigned(tree, **kw):
    from meryl_amd import db
    got = [[], [], [], []]
    files = []

    def on_slice(ff, lo, hi, v, lab):
        files.append(ff)
        for col, a in zip(got, (lo, hi if hi is not None else np.zeros(lo.size, np.uint64), v, lab)):
            col.append(a)
    db.evaluate_assigned(tree, on_slice, **kw)
    assert files == list(range(64))
    lo, hi, v, lab = (np.concatenate(c) for c in got)
    return [(int(h) << 64) | int(l) for l, h in zip(lo.tolist(), hi.tolist())], v.tolist(), lab.tolist()


def check_output(path, keys, vals):
    """an output written by an assigned node reads back equal, and its stored histogram is the histogram of its values"""
    from meryl_amd import db
    on_disk, _ = LH.read_db(path)
    assert sorted(on_disk) == keys and [on_disk[x][0] for x in keys] == vals
    r = db.Reader(path)
    hv, ho = r.histogram()
    info = r.info
    want_v, want_o = np.unique(np.array(vals, dtype=np.uint64), return_counts=True)
    assert hv.tolist() == want_v.tolist() and ho.tolist() == want_o.tolist()
    assert (info.num_distinct, info.num_total, info.num_unique) == (len(vals), sum(vals), sum(1 for x in vals if x == 1))
    r.close()


def test_assigned_trees_equal_the_model_on_the_decoded_leaves(world, tmp_path):
    p = lambda n: os.path.join(world, n)                          # noqa: E731
    A_, B, C, D = p("A"), p("B"), p("C"), p("D")
    out = lambda n: str(tmp_path / n)                             # noqa: E731
    k = 21
    dbs = {n: as_input(LH.read_db(p(n))[0]) for n in "ABCD"}
    none, lab0 = [], ("default", 0)
    # intersect value=sub A B: the shared k-mers with the count difference, equal counts dropped
    st = {}
    want = A.merge_assigned([dbs["A"], dbs["B"]], 6, ("sub", 0), lab0, none, k, stats=st)
    got = run_assigned(("intersect", A_, B, {"value": "sub", "output": out("t1")}))
    assert got[:2] == want[:2] and st["zero"] > 0 and st["kept"] > 0 and not any(got[2])
    check_output(out("t1"), want[0], want[1])
    # at-least 2 [union value=count A B C]: a node with an assignment under a node without one
    inner = A.merge_assigned([dbs[n] for n in "ABC"], 10, ("count", 0), lab0, none, k)
    want = S.value_selected(*inner, 2, 2, "default", 0, none, k)
    got = run_assigned(("at-least", 2, ("union", A_, B, C, {"value": "count", "output": out("t2-inner")}), {"output": out("t2")}))
    assert got[:2] == want[:2] and 0 < len(want[0]) < len(inner[0])
    check_output(out("t2-inner"), inner[0], inner[1])
    check_output(out("t2"), want[0], want[1])
    # a value filter with an assignment and a program: the filter and the program test the assigned value, @1 the input's
    words = ["value:@1<=8"]
    want = A.merge_assigned([dbs["A"]], 0, ("mul", 2), lab0, S.parse(words, 1), k, value_filter=(1, 6))
    got = run_assigned(("greater-than", 6, A_, {"value": "mul#2", "select": words, "output": out("t3")}))
    assert got[:2] == want[:2] and 0 < len(want[0]) < len(dbs["A"][0]) and min(want[1]) == 8 and max(want[1]) == 16
    check_output(out("t3"), want[0], want[1])
    # nested assignments, a program beside one, a 4-input node over two inner nodes and two leaves, presence by subtract and difference
    left = A.merge_assigned([dbs["A"], dbs["B"]], 7, ("divzero", 1), lab0, none, k)
    right = A.merge_assigned([dbs["C"], dbs["D"]], 9, ("max", 5), lab0, none, k)
    words = ["value:@1>=2", "or", "input:3-all"]
    want = A.merge_assigned([left, right, dbs["D"], dbs["B"]], 10, ("add", 100), lab0, S.parse(words, 4), k)
    got = run_assigned(("union", ("subtract", A_, B, {"value": "divzero"}), ("symmetric-difference", C, D, {"value": ("max", 5)}), D, B,
                        {"value": "add#100", "select": words, "output": out("t4")}))
    assert got[:2] == want[:2] and 0 < len(want[0])
    check_output(out("t4"), want[0], want[1])
    # #0 writes nothing, and an empty output is a database
    got = run_assigned(("union", A_, B, {"value": "#0", "output": out("t5")}))
    assert got == ([], [], [])
    check_output(out("t5"), [], [])


def test_a_tree_without_assignments_writes_the_bytes_of_the_selected_evaluation(world, tmp_path):
    from meryl_amd import db
    p = lambda n: os.path.join(world, n)                          # noqa: E731
    tree = lambda d: ("subtract", ("union-sum", p("A"), p("B"), p("C"), {"select": ["value:>=3"], "output": str(tmp_path / d / "inner")}),   # noqa: E731
                      ("at-most", 4, p("D")), ("union-min", p("B"), p("C")), {"output": str(tmp_path / d / "root")})
    for d in ("sel", "asg", "asg-labels"):
        os.makedirs(tmp_path / d)
    db.evaluate_selected(tree("sel"))
    db.evaluate_assigned(tree("asg"))
    for name in ("inner", "root"):
        assert dir_bytes(str(tmp_path / "asg" / name)) == dir_bytes(str(tmp_path / "sel" / name)), name
    assert len(LH.read_db(str(tmp_path / "asg" / "root"))[0]) > 0


# ---- the command line -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def meryl(native_lib):
    from meryl_amd import build
    path = build.build_cli()
    assert os.path.exists(path)
    return path


def kmer_text(keys, vals, k):
    return [("".join("ACTG"[(key >> (2 * (k - 1 - i))) & 3] for i in range(k)), str(v)) for key, v in zip(keys, vals)]


def test_cli_evaluates_trees_with_value_assignments(meryl, world, tmp_path):
    p = lambda n: os.path.join(world, n)                          # noqa: E731
    k = 21
    dbs = {n: as_input(LH.read_db(p(n))[0]) for n in "ABC"}
    lab0 = ("default", 0)

    def run(*args):
        r = subprocess.run([meryl] + [str(x) for x in args], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        return [tuple(line.split("\t")) for line in r.stdout.splitlines()]
    # print union value=#1 A B: the presence set
    want = A.merge_assigned([dbs["A"], dbs["B"]], 10, ("set", 1), lab0, [], k)
    assert run("print", "union", "value=#1", p("A"), p("B")) == kmer_text(want[0], want[1], k) and set(want[1]) == {1}
    # intersect value=sub A B output d
    want = A.merge_assigned([dbs["A"], dbs["B"]], 6, ("sub", 0), lab0, [], k)
    assert run("intersect", "value=sub", p("A"), p("B"), "output", tmp_path / "d") == []
    check_output(str(tmp_path / "d"), want[0], want[1])
    assert 0 < len(want[0])
    # print at-least 2 [union value=count A B C]
    inner = A.merge_assigned([dbs[n] for n in "ABC"], 10, ("count", 0), lab0, [], k)
    want = S.value_selected(*inner, 2, 2, "default", 0, [], k)
    assert run("print", "at-least", "2", "[", "union", "value=count", p("A"), p("B"), p("C"), "]") == kmer_text(want[0], want[1], k)
    assert 0 < len(want[0]) < len(inner[0])
    # a value filter with an assignment, a constant in hexadecimal, and a selector after it
    want = A.merge_assigned([dbs["A"]], 0, ("max", 5), lab0, S.parse(["value:@1<9"], 1), k, value_filter=(4, 5))
    assert run("print", "equal-to", "5", "value=max#0x5", "value:@1<9", p("A")) == kmer_text(want[0], want[1], k) and 0 < len(want[0])
