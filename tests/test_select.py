"""Selectors in operation trees (meryl2; merylSelector::isTrue, src/meryl2/merylSelector.C:72-156), on the device: the SELECT
instantiations of merge_many_kernel and select_kernel against the Python statement of the rules in select_helpers.py (beside the
value rules of test_merge_many.py and the label table of label_helpers.py), the count pass against the emit pass, whole trees
through mgc_db_eval_selected against the staged results of the existing paths, and the command line.  Everything is exact."""
import os
import subprocess

import numpy as np
import pytest

import eval_helpers as H
import label_helpers as LH
import select_helpers as S
import test_merge_many as TM
from test_labels import SELECT_TILE, dir_bytes, host_keys, key_tensor, u64_tensor

pytestmark = pytest.mark.gpu

M32 = LH.M32
K_OF = {1: 31, 2: 47}                            # the pools of test_merge_many.make_pool hold 62 and 64 + 30 key bits


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


def shapes(N, T):
    """the border shapes of test_merge_many.shapes at no more than about 3T elements whatever N is"""
    base = TM.shapes(N, T)

    def group_at(pos):
        def b(rng, kw):
            pool = TM.make_pool(rng, pos + 1 + T + 64, kw)
            below, x, above = pool[:pos], pool[pos:pos + 1], pool[pos + 1:]
            which = rng.integers(0, N, pos)
            return [np.concatenate([below[which == i], x, TM.draw(rng, above, max(2 * T // N, 3))]) for i in range(N)]
        return b
    out = {n: base[n] for n in ("all-empty", "single-elements", "sum-T-1", "sum-T", "sum-T+1")}
    out.update({"group-at-T-1": group_at(T - 1), "group-at-T": group_at(T), "group-at-T+1": group_at(T + 1)})
    return out


SHAPE_NAMES = sorted(shapes(2, 64))


def programs(N, k):
    """name -> selector words for a node of N inputs"""
    at_least_2 = "input:2-all" if N >= 2 else "input:all"
    second = "@2" if N >= 2 else "#400"
    return {
        "input:2-all": [at_least_2],
        "input:@1:@N": ["input:@1:@%d" % N],
        "value:@2>@1": ["value:%s>@1" % second],
        "not value:@2>@1": ["not", "value:%s>@1" % second],              # the absent-input rule: false under `not` too
        "label:==#5": ["label:==#5"],
        "bases:gc": ["bases:gc:ge%d" % (k // 2)],
        "three products, 16 terms": ["input:1", "value:ge500", "bases:a:ge1", "bases:c:ge1", "bases:g:ge1", "bases:t:ge1", "or",
                                     at_least_2, "not", "value:@1<300", "label:ne0", "label:<=7", "value:>0", "value:ne7", "or",
                                     "bases:gc:ge%d" % (k // 2), "and", "value:lt100", "label:ge1", "not", "label:eq3"],
    }


class World:
    """N sorted streams with values and small labels (so that label tests decide both ways) on the device and as lists"""

    def __init__(self, torch, rng, keys, kw):
        self.N, self.kw, self.k = len(keys), kw, K_OF[kw]
        self.ints = [TM.key_ints(a) for a in keys]
        self.vals = [rng.integers(1, 1000, a.shape[0]).astype(np.uint32) for a in keys]
        for v in self.vals[::2]:
            v[::3] = rng.integers(1, M32, v[::3].size, dtype=np.uint64).astype(np.uint32)
        self.labs = [rng.integers(0, 8, a.shape[0]).astype(np.uint64) for a in keys]
        self.labs[self.N // 2][:] = 0                                    # passed without a buffer
        self.dk = [key_tensor(torch, a, kw) for a in keys]
        self.dc = [torch.from_numpy(c.view(np.int32).copy()).cuda() for c in self.vals]
        self.dl = [None if i == self.N // 2 else u64_tensor(torch, l) for i, l in enumerate(self.labs)]
        self.inputs = [(ki, v.tolist(), l.tolist()) for ki, v, l in zip(self.ints, self.vals, self.labs)]

    def check(self, ops, op, words, label_word="default", label_constant=None):
        from meryl_amd import db
        terms = db.parse_selector(words, self.N)
        model_terms = S.parse(words, self.N)
        assert len(terms) == len(model_terms) and all(S.same_term(t, c) for t, c in zip(model_terms, terms)), words
        cc = LH.DEFAULT_CONSTANT.get(label_word, 0) if label_constant is None else label_constant
        wk, wv, wl = S.merge_selected(self.inputs, op, label_word, cc, model_terms, self.k)
        what = (TM.OP_WORDS[op], words, label_word)
        # the count pass alone first: its total is the length the emit pass is given room for
        n = ops.dev_merge_many_selected(self.dk, self.dc, self.dl, self.k, op, terms, label_word, label_constant, count_only=True)
        assert n == len(wk), what
        ok, oc, ol, n2 = ops.dev_merge_many_selected(self.dk, self.dc, self.dl, self.k, op, terms, label_word, label_constant)
        assert n2 == n and ok.shape[0] == n
        assert host_keys(ok, self.kw) == wk, what
        assert oc.cpu().numpy().view(np.uint32).tolist() == wv, what
        assert ol.cpu().numpy().view(np.uint64).tolist() == wl, what
        return len(wk)


@pytest.mark.parametrize("shape", SHAPE_NAMES)
@pytest.mark.parametrize("kw", [1, 2])
@pytest.mark.parametrize("N", [1, 2, 3, 32])
def test_merge_many_with_a_program_against_the_model(ops, torch_cuda, native_lib, N, kw, shape):
    T = native_lib.mgc_dev_merge_many_tile(kw)
    rng = np.random.default_rng(9000 + 100 * N + 10 * kw + SHAPE_NAMES.index(shape))
    keys = shapes(N, T)[shape](rng, kw)
    assert len(keys) == N and sum(a.shape[0] for a in keys) <= 3 * T + 64 * N
    w = World(torch_cuda, rng, keys, kw)
    kept = total = 0
    for name, words in programs(N, w.k).items():
        for op in (0, 3, 7, 10) if name in ("input:2-all", "value:@2>@1", "three products, 16 terms") else (0,):
            kept += w.check(ops, op, words)
            total += 1
    kept += w.check(ops, 1, ["label:@1==#5", "or", "label:ge6"], "selected")        # the label of the smallest value decides
    kept += w.check(ops, 0, ["label:==#5"], "and", 0b0101)
    assert total == 16 and (kept > 0 or shape in ("all-empty", "single-elements"))


def test_programs_decide_both_ways_and_without_labels(ops, torch_cuda, native_lib):
    """every program of the list keeps some k-mers and drops some on a plain overlapping shape; an emit without a label buffer
    writes the same k-mers and values; an empty program is the labelled merge"""
    from meryl_amd import db
    kw, N = 1, 3
    T = native_lib.mgc_dev_merge_many_tile(kw)
    rng = np.random.default_rng(9)
    w = World(torch_cuda, rng, TM.shapes(N, T)["sum-T+1"](rng, kw), kw)
    everything = len(S.merge_selected(w.inputs, 0, "default", 0, [], w.k)[0])
    for name, words in programs(N, w.k).items():
        n = w.check(ops, 0, words)
        assert 0 < n < everything, (name, n, everything)
        terms = db.parse_selector(words, N)
        ok, oc, ol, _ = ops.dev_merge_many_selected(w.dk, w.dc, w.dl, w.k, 0, terms)
        pk, pc, pl, _ = ops.dev_merge_many_selected(w.dk, w.dc, None if "label" not in name and "16" not in name else w.dl, w.k, 0, terms,
                                                    with_labels=False)
        assert pl is None and torch_cuda.equal(pk, ok) and torch_cuda.equal(pc, oc), name
    ek, ec, el, n = ops.dev_merge_many_selected(w.dk, w.dc, w.dl, w.k, 0, [])
    lk, lc_, ll = ops.dev_merge_many_labelled(w.dk, w.dc, w.dl, 0)
    assert n == everything and torch_cuda.equal(ek, lk) and torch_cuda.equal(ec, lc_) and torch_cuda.equal(el, ll)


@pytest.mark.parametrize("kw", [1, 2])
@pytest.mark.parametrize("n", [0, 1, SELECT_TILE - 1, SELECT_TILE, SELECT_TILE + 1, 3 * SELECT_TILE + 17])
def test_select_kernel_with_a_program_against_the_model(ops, torch_cuda, native_lib, n, kw):
    from meryl_amd import db
    torch = torch_cuda
    k = K_OF[kw]
    rng = np.random.default_rng(500 + n + kw)
    keys = TM.draw(rng, TM.make_pool(rng, n + 64, kw), n)
    vals = rng.integers(1, 20, n).astype(np.uint32)
    vals[::5] = rng.integers(1, M32, vals[::5].size, dtype=np.uint64).astype(np.uint32)
    labs = rng.integers(0, 8, n).astype(np.uint64)
    dk, dc, dl = key_tensor(torch, keys, kw), torch.from_numpy(vals.view(np.int32).copy()).cuda(), u64_tensor(torch, labs)
    ints = TM.key_ints(keys)
    kept = 0
    cases = [(2, 5, ["value:@1<12"], "default", None),                                   # at-least 5, then the input's value
             (8, 3, ["value:ge30", "value:@1le15"], "default", None),                     # multiply 3: the output value is the new one
             (7, 4, ["not", "value:>#6"], "default", None),                               # decrease 4
             (2, 1, ["label:==#5", "or", "label:@1<2"], "default", None),
             (2, 1, ["label:>=0xFFFFFFFFFFFFFFF9"], "invert", None),
             (2, 1, ["bases:gc:ge%d" % (k // 2)], "default", None),
             (2, 1, ["bases:a:lt3", "or", "bases:t:%d<=@0" % (k // 3)], "default", None),
             (2, 1, ["input:1"], "default", None), (2, 1, ["not", "input:1"], "default", None), (2, 1, ["input:@1"], "default", None),
             (5, 7, ["value:ne3", "label:ne4", "bases:gc:ge%d" % (k // 3), "or", "label:==#7", "not", "value:@1>10"], "or", 0b100)]
    for fop, c, words, word, lc in cases:
        terms, model_terms = db.parse_selector(words, 1), S.parse(words, 1)
        cc = LH.DEFAULT_CONSTANT.get(word, 0) if lc is None else lc
        wk, wv, wl = S.value_selected(ints, vals.tolist(), labs.tolist(), fop, c, word, cc, model_terms, k)
        what = (fop, c, words)
        cnt = ops.dev_select_selected(dk, dc, dl, k, fop, c, terms, word, lc, count_only=True)
        assert cnt == len(wk), what
        ok, oc, ol, cnt2 = ops.dev_select_selected(dk, dc, dl, k, fop, c, terms, word, lc)
        assert cnt2 == cnt and host_keys(ok, kw) == wk, what
        assert oc.cpu().numpy().view(np.uint32).tolist() == wv and ol.cpu().numpy().view(np.uint64).tolist() == wl, what
        if "label" not in " ".join(words):
            pk, pc, pl, _ = ops.dev_select_selected(dk, dc, None, k, fop, c, terms, word, lc, with_labels=False)
            assert pl is None and torch.equal(pk, ok) and torch.equal(pc, oc), what
        if words == ["not", "input:1"]:
            assert cnt == 0
        kept += cnt
    assert kept > 0 or n == 0


# ---- whole trees against the existing paths ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def world(native_lib, torch_cuda, tmp_path_factory):
    """databases A, B, C, D (k = 21, 3000-5000 k-mers from one pool, values 1..9)"""
    wdir = str(tmp_path_factory.mktemp("select_world"))
    rng = np.random.default_rng(21)
    plo, phi = H.random_kmers(rng, 21, 9000)
    for name, n in (("A", 5000), ("B", 4000), ("C", 3000), ("D", 4000)):
        idx = np.sort(rng.choice(plo.size, n, replace=False))
        H.write_db(os.path.join(wdir, name), plo[idx], phi[idx], rng.integers(1, 10, idx.size).astype(np.uint32), 21, 8)
    return wdir


def run_selected(tree, with_labels=False):
    from meryl_amd import db
    got = [[], [], [], []]

    def on_slice(ff, lo, hi, v, lab):
        for col, a in zip(got, (lo, hi if hi is not None else np.zeros(lo.size, np.uint64), v, lab)):
            col.append(a)
    db.evaluate_selected(tree, on_slice, with_labels=with_labels)
    return tuple(np.concatenate(c) for c in got)


def test_selected_trees_equal_the_staged_results_of_the_existing_paths(world, tmp_path):
    p = lambda n: os.path.join(world, n)                          # noqa: E731
    A, B, C, D = p("A"), p("B"), p("C"), p("D")
    out = lambda n: str(tmp_path / n)                             # noqa: E731
    # union-sum value:ge5 == at-least 5 [union-sum ...]
    staged = H.run_staged(("at-least", 5, ("union-sum", A, B, C), {"output": "root"}), out("staged1"))
    lo, hi, v, lab = run_selected(("union-sum", A, B, C, {"select": ["value:ge5"], "output": out("sel1")}))
    assert dir_bytes(out("sel1")) == dir_bytes(staged) and 0 < lo.size and not lab.any() and (v >= 5).all()
    # union input:all holds the k-mers of intersect
    staged = H.run_staged(("intersect", A, B, C, D, {"output": "root"}), out("staged2"))
    run_selected(("union", A, B, C, D, {"select": ["input:all"], "output": out("sel2")}))
    got, _ = LH.read_db(out("sel2"))
    want, _ = LH.read_db(staged)
    assert sorted(got) == sorted(want) and len(got) > 0 and all(val == 4 for val, _ in got.values())
    # union-sum input:1:@1 over two inputs == difference
    staged = H.run_staged(("difference", A, B, {"output": "root"}), out("staged3"))
    run_selected(("union-sum", A, B, {"select": ["input:1:@1"], "output": out("sel3")}))
    assert dir_bytes(out("sel3")) == dir_bytes(staged)
    # a selector deep in a tree, and nodes without one beside it (the two-input fold, a value node)
    staged = H.run_staged(("subtract", ("at-least", 3, ("union-sum", A, B)), ("at-most", 4, C), {"output": "root"}), out("staged4"))
    run_selected(("subtract", ("union-sum", A, B, {"select": ["value:>=3"]}), ("at-most", 4, C), {"output": out("sel4")}))
    assert dir_bytes(out("sel4")) == dir_bytes(staged)


def test_labelled_tree_with_empty_programs_equals_the_labelled_evaluation(native_lib, torch_cuda, tmp_path):
    from meryl_amd import db
    wdir = str(tmp_path / "w")
    os.makedirs(wdir)
    LH.make_tree_world(wdir, 21)
    os.makedirs(tmp_path / "lab")
    os.makedirs(tmp_path / "sel")
    lab = [[], [], []]
    db.evaluate_labelled(LH.the_tree(wdir, str(tmp_path / "lab")), lambda ff, lo, hi, v, l: [c.append(a) for c, a in zip(lab, (lo, v, l))])
    sel = [[], [], []]
    db.evaluate_selected(LH.the_tree(wdir, str(tmp_path / "sel")), lambda ff, lo, hi, v, l: [c.append(a) for c, a in zip(sel, (lo, v, l))],
                         with_labels=True)
    for name in ("inner", "root"):
        assert dir_bytes(str(tmp_path / "sel" / name)) == dir_bytes(str(tmp_path / "lab" / name)), name
    for a, b in zip(lab, sel):
        assert np.array_equal(np.concatenate(a), np.concatenate(b))
    assert np.concatenate(lab[2]).any()
    # and a label: selector makes labels travel on its own: the k-mers of the root whose label is in a range
    got = [[], [], []]
    t = LH.the_tree(wdir, str(tmp_path / "sel2"))
    t = t[:-1] + ({"select": ["label:>=#1", "label:<0x40"]},)
    os.makedirs(tmp_path / "sel2")
    db.evaluate_selected(t, lambda ff, lo, hi, v, l: [c.append(a) for c, a in zip(got, (lo, v, l))])
    full = [np.concatenate(c) for c in lab]
    pick = (full[2] >= np.uint64(1)) & (full[2] < np.uint64(0x40))
    assert 0 < pick.sum() < pick.size
    for a, b in zip(full, got):
        assert np.array_equal(a[pick], np.concatenate(b))


# ---- the command line -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def meryl(native_lib):
    from meryl_amd import build
    path = build.build_cli()
    assert os.path.exists(path)
    return path


def test_cli_prints_a_nested_tree_with_selectors(meryl, world, tmp_path):
    p = lambda n: os.path.join(world, n)                          # noqa: E731
    k = 21
    dbs = {n: LH.read_db(p(n))[0] for n in "ABCD"}
    as_input = lambda d: (sorted(d), [d[x][0] for x in sorted(d)], [0] * len(d))      # noqa: E731
    # print union-sum value:@2gt@1 [at-least 2 bases:gc:ge9 A] [union input:2-all B C D]
    left = S.value_selected(*as_input(dbs["A"]), 2, 2, "default", 0, S.parse(["bases:gc:ge9"], 1), k)
    right = S.merge_selected([as_input(dbs[n]) for n in "BCD"], 10, "default", 0, S.parse(["input:2-all"], 3), k)
    wk, wv, _ = S.merge_selected([left, right], 0, "default", 0, S.parse(["value:@2gt@1", "or", "not", "input:@2"], 2), k)
    r = subprocess.run([meryl, "print", "union-sum", "value:@2gt@1", "or", "not", "input:@2", "[", "at-least", "2", "bases:gc:ge9", p("A"), "]",
                        "[", "union", "input:2-all", p("B"), p("C"), p("D"), "output", str(tmp_path / "right"), "]"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    got = [line.split("\t") for line in r.stdout.splitlines()]
    want = [("".join("ACTG"[(key >> (2 * (k - 1 - i))) & 3] for i in range(k)), str(v)) for key, v in zip(wk, wv)]
    assert [tuple(g) for g in got] == want and 0 < len(want) < len(dbs["A"])
    on_disk, _ = LH.read_db(str(tmp_path / "right"))
    assert sorted(on_disk) == right[0] and [on_disk[x][0] for x in right[0]] == right[1]
