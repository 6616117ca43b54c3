"""The value-histogram accumulator (mgc_value_hist_*), histograms of operation-tree nodes (mgc_db_eval_reported) and the command
line's `histogram [operation]`, `statistics` and output:histogram, on the device.  The oracle is numpy.unique of the values."""
import os
import subprocess

import numpy as np
import pytest

import eval_helpers as H
import hist_helpers as HH
import label_helpers as LH
from test_db_eval_host import tiny_db
from test_labels import dir_bytes

pytestmark = pytest.mark.gpu

M32 = 0xFFFFFFFF


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "the -m gpu tests need a GPU"
    torch.cuda.set_device(0)
    return torch


@pytest.fixture(scope="module")
def geometry(native_lib):
    from meryl_amd import db
    return db.ValueHistogram.geometry()                  # (dense limit D, values one workgroup takes per iteration)


def on_device(torch, values):
    return torch.from_numpy(np.ascontiguousarray(values, dtype=np.uint32).view(np.int32)).cuda()


def histogram_of(torch, *arrays):
    from meryl_amd import db
    h = db.ValueHistogram()
    for a in arrays:
        h.add(a if hasattr(a, "is_cuda") else on_device(torch, a))
    got = h.get(), h.totals()
    h.close()
    return got


def check(torch, *arrays):
    (v, o), (unique, distinct, total) = histogram_of(torch, *arrays)
    allv = np.concatenate([np.asarray(a.cpu().numpy().view(np.uint32) if hasattr(a, "is_cuda") else a, dtype=np.uint32) for a in arrays])
    wv, wo = HH.unique_counts(allv)
    assert v.dtype == np.uint64 and o.dtype == np.uint64
    assert v.tolist() == wv.tolist() and o.tolist() == wo.tolist()
    assert distinct == allv.size and unique == int((allv == 1).sum())
    assert total == sum(int(a) * int(b) for a, b in zip(wv.tolist(), wo.tolist())) % (1 << 64)
    return v, o


def count_like(rng, n, D):
    """the shape of count data with a tail: mostly small values, some above the dense limit, a few anywhere below 2^32"""
    v = rng.geometric(0.4, n).astype(np.uint64)
    far = rng.random(n)
    v = np.where(far < 0.05, rng.integers(D, 8 * D, n, dtype=np.uint64), v)
    v = np.where(far < 0.01, rng.integers(0, 1 << 32, n, dtype=np.uint64), v)
    return v.astype(np.uint32)


SIZES = ("0", "1", "63", "64", "65", "group-1", "group", "group+1", "200003")


@pytest.mark.parametrize("size", SIZES)
def test_sizes_at_which_the_kernel_takes_another_path(torch_cuda, geometry, size):
    D, group = geometry
    n = {"group-1": group - 1, "group": group, "group+1": group + 1}.get(size) if size.startswith("group") else int(size)
    rng = np.random.default_rng(1000 + n)
    check(torch_cuda, count_like(rng, n, D))
    # every value on the list: the aggregated append of a partial wave, of a partial vector, of the scalar ends
    check(torch_cuda, rng.integers(D, 1 << 32, n, dtype=np.uint64).astype(np.uint32))


@pytest.mark.parametrize("offset", [1, 2, 3])
def test_values_that_do_not_begin_on_a_16_byte_boundary(torch_cuda, geometry, offset):
    D, group = geometry
    rng = np.random.default_rng(offset)
    for n in (1, 2, 5, group + 2, 5003):
        whole = on_device(torch_cuda, count_like(rng, n + offset, D))
        part = whole[offset:]
        assert part.data_ptr() % 16 == 4 * offset and part.is_contiguous()
        check(torch_cuda, part)


def test_the_hot_bin(torch_cuda, geometry):
    v, o = check(torch_cuda, np.ones(200_003, dtype=np.uint32))
    assert v.tolist() == [1] and o.tolist() == [200_003]
    # a few hot values: what the peels do not take goes through plain LDS atomics
    rng = np.random.default_rng(5)
    check(torch_cuda, rng.choice(np.array([1, 1, 1, 1, 2, 2, 3, 4, 5, 6], dtype=np.uint32), 100_001))


def test_values_around_the_dense_limit(torch_cuda, geometry):
    D, _ = geometry
    for value in (D - 1, D, D + 1):
        v, o = check(torch_cuda, np.full(70_001, value, dtype=np.uint32))
        assert v.tolist() == [value] and o.tolist() == [70_001]
    rng = np.random.default_rng(6)
    v, o = check(torch_cuda, rng.choice(np.array([D - 1, D], dtype=np.uint32), 70_001))
    assert v.tolist() == [D - 1, D]
    v, o = check(torch_cuda, np.array([0, 0, D - 1, D, M32, M32, M32, 1, 1 << 31, (1 << 31) - 1, (1 << 31) + 1], dtype=np.uint32))
    assert v.tolist()[0] == 0 and v.tolist()[-1] == M32 and o.tolist()[-1] == 3


def test_every_value_distinct(torch_cuda, geometry):
    D, _ = geometry
    rng = np.random.default_rng(8)
    vals = np.concatenate([np.arange(0, 3000, dtype=np.uint64), np.arange(D - 50, D + 50, dtype=np.uint64) + 100_000,
                           np.unique(rng.integers(1 << 20, 1 << 32, 30_000, dtype=np.uint64)), np.array([M32], dtype=np.uint64)])
    vals = np.unique(vals)
    v, o = check(torch_cuda, rng.permutation(vals).astype(np.uint32))
    assert v.size == vals.size > 30_000 and set(o.tolist()) == {1}


def test_two_adds_accumulate_and_totals_pass_2_to_the_32(torch_cuda, geometry):
    D, _ = geometry
    rng = np.random.default_rng(9)
    a = count_like(rng, 150_001, D)
    b = rng.integers((1 << 31) - 40, (1 << 31) + 40, 90_003, dtype=np.uint64).astype(np.uint32)   # the same large values again and again
    c = count_like(rng, 777, D)
    (v, o), (unique, distinct, total) = histogram_of(torch_cuda, a, b, c)
    wv, wo = HH.unique_counts(np.concatenate([a, b, c]))
    assert v.tolist() == wv.tolist() and o.tolist() == wo.tolist()
    want_total = sum(int(x) * int(y) for x, y in zip(wv.tolist(), wo.tolist()))
    assert (1 << 32) < want_total < (1 << 64) and total == want_total and distinct == a.size + b.size + c.size
    check(torch_cuda, a, b, c)
    # an empty add between two others changes nothing
    check(torch_cuda, a, np.zeros(0, dtype=np.uint32), c)


# ---- histograms of tree nodes ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def worlds(native_lib, torch_cuda, tmp_path_factory):
    """k -> directory with databases A, B, C (3000-5000 k-mers of one pool, values 1..9, every 50th k-mer of A a value above any dense
    limit) for k = 21 and k = 51; "labelled": label_helpers' databases a..f at k = 21"""
    out = {}
    for k, wp in ((21, 8), (51, 10)):
        wdir = str(tmp_path_factory.mktemp("hist_world_%d" % k))
        rng = np.random.default_rng(170 + k)
        plo, phi = H.random_kmers(rng, k, 9000)
        for name, n in (("A", 5000), ("B", 4000), ("C", 3000)):
            idx = np.sort(rng.choice(plo.size, n, replace=False))
            cn = rng.integers(1, 10, idx.size).astype(np.uint32)
            if name == "A":
                cn[::50] = rng.integers(1 << 20, 1 << 32, cn[::50].size, dtype=np.uint64).astype(np.uint32)
            H.write_db(os.path.join(wdir, name), plo[idx], phi[idx], cn, k, wp)
        out[k] = wdir
    ldir = str(tmp_path_factory.mktemp("hist_world_labelled"))
    LH.make_tree_world(ldir, 21)
    out["labelled"] = ldir
    return out


def run_reported(tree, **kw):
    from meryl_amd import db
    vals, files = [], []

    def on_slice(ff, lo, hi, v, lab):
        files.append(ff)
        vals.append(v)
    hists = db.evaluate_reported(tree, on_slice, **kw)
    assert files == list(range(64))
    return hists, np.concatenate(vals)


def same(hist, want):
    return hist[0].dtype == np.uint64 and hist[0].tolist() == want[0].tolist() and hist[1].tolist() == want[1].tolist()


def stored(path):
    from meryl_amd import db
    r = db.Reader(path)
    got = r.histogram()
    r.close()
    return got


@pytest.mark.parametrize("k", [21, 51])
def test_root_inner_node_and_leaf_histograms(worlds, tmp_path, k):
    p = lambda n: os.path.join(worlds[k], n)                      # noqa: E731
    inner = str(tmp_path / "inner")
    tree = ("union-max", ("intersect-sum", {"database": p("A"), "histogram": True}, p("B"), {"output": inner, "histogram": True}),
            ("at-least", 2, p("C")), {"histogram": True})
    hists, root_values = run_reported(tree)
    assert len(hists) == 3                                         # pre-order: the root, the inner node, the leaf
    assert root_values.size > 3000 and same(hists[0], HH.unique_counts(root_values))
    assert same(hists[1], stored(inner)) and hists[1][0].size > 5
    assert same(hists[2], stored(p("A"))) and int(hists[2][0].max()) >= (1 << 20)
    assert not same(hists[0], hists[1]) and not same(hists[1], hists[2])


def test_trees_with_labels_a_selector_and_an_assignment(worlds, geometry, tmp_path):
    D, _ = geometry
    p = lambda n: os.path.join(worlds[21], n)                     # noqa: E731
    q = lambda n: os.path.join(worlds["labelled"], n)             # noqa: E731
    # labels travelling
    hists, values = run_reported(("union-sum", q("a"), q("b"), ("at-least", 2, q("c")), {"label": "or", "histogram": True}), with_labels=True)
    assert values.size > 6000 and same(hists[0], HH.unique_counts(values)) and len(hists) == 1
    # a selector
    hists, values = run_reported(("union-sum", p("A"), p("B"), {"select": ["value:>=5"], "histogram": True}))
    assert values.size > 1000 and int(values.min()) == 5 and same(hists[0], HH.unique_counts(values))
    # value=mul#1000: every value from 1000 up, most of them above the dense limit
    hists, values = run_reported(("union", p("B"), p("C"), {"value": "mul#1000", "histogram": True}))
    assert int(values.min()) == 1000 and int(values.max()) == 81_000 and same(hists[0], HH.unique_counts(values))
    # ... and a constant that takes every value past it
    hists, values = run_reported(("union", p("B"), p("C"), {"value": "mul#100000", "histogram": True}))
    assert int(values.min()) == 100_000 > D and same(hists[0], HH.unique_counts(values))
    assert hists[0][0].size == np.unique(values).size > 20


def test_a_tree_with_nothing_flagged_writes_the_bytes_of_the_assigned_evaluation(worlds, tmp_path):
    from meryl_amd import db
    p = lambda n: os.path.join(worlds[21], n)                     # noqa: E731
    tree = lambda d: ("subtract", ("union-sum", p("A"), p("B"), p("C"), {"select": ["value:>=3"], "output": str(tmp_path / d / "inner")}),   # noqa: E731
                      ("at-most", 4, p("B"), {"value": "mul#3"}), {"output": str(tmp_path / d / "root")})
    for d in ("asg", "rep"):
        os.makedirs(tmp_path / d)
    db.evaluate_assigned(tree("asg"))
    assert db.evaluate_reported(tree("rep")) == []
    for name in ("inner", "root"):
        assert dir_bytes(str(tmp_path / "rep" / name)) == dir_bytes(str(tmp_path / "asg" / name)), name
    assert stored(str(tmp_path / "rep" / "root"))[0].size > 0


# ---- the command line ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def meryl(native_lib):
    from meryl_amd import build
    path = build.build_cli()
    assert os.path.exists(path)
    return path


def run(meryl, *args):
    r = subprocess.run([meryl] + [str(x) for x in args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return r.stdout


def test_cli_histogram_and_statistics_of_an_operation(meryl, worlds, tmp_path):
    p = lambda n: os.path.join(worlds[21], n)                     # noqa: E731
    t = tmp_path / "t"
    fused = run(meryl, "histogram", "[union-sum", p("A"), p("B") + "]")
    assert sorted(os.listdir(tmp_path)) == []                      # nothing is written unless a node says output
    assert run(meryl, "union-sum", p("A"), p("B"), "output", t) == ""
    assert fused == run(meryl, "histogram", t) and fused.count("\n") > 10
    fused = run(meryl, "statistics", "[union-sum", p("A"), p("B") + "]")
    assert fused == run(meryl, "statistics", t) and fused.startswith("Number of 21-mers that are:\n") and fused.count("\n") > 20
    # the table, written out by hand for one tiny input (hist_helpers), from a tree and from the database
    a = tiny_db(tmp_path / "a", 21)
    assert run(meryl, "statistics", a) == HH.TINY_K21_STATISTICS
    assert run(meryl, "statistics", "[at-least", "1", a + "]") == HH.TINY_K21_STATISTICS
    assert run(meryl, "histogram", "[union-max", a, a + "]".replace(a, str(tiny_db(tmp_path / "a2", 21)))) == "2\t2\n7\t2\n"
    # a root that also says output writes it, as before
    assert run(meryl, "histogram", "[intersect-sum", p("A"), p("B"), "output", tmp_path / "i]") == run(meryl, "histogram", tmp_path / "i")


def test_cli_output_histogram_on_an_inner_node(meryl, worlds, tmp_path):
    p = lambda n: os.path.join(worlds[21], n)                     # noqa: E731
    f, s = tmp_path / "inner.hist", tmp_path / "inner.stats"
    printed = run(meryl, "print", "[at-least", "3", "[union-sum", "output:histogram=%s" % f, "output:statistics=%s" % s, p("A"), p("B") + "]]")
    assert printed == run(meryl, "print", "[at-least", "3", "[union-sum", p("A"), p("B") + "]]") and printed.count("\n") > 1000
    t = tmp_path / "t"
    run(meryl, "union-sum", p("A"), p("B"), "output", t)
    assert f.read_text() == run(meryl, "histogram", t) and s.read_text() == run(meryl, "statistics", t)
    assert f.read_text() == HH.histogram_text(*stored(str(t)))
    # no file: the report follows the printed k-mers on stdout
    both = run(meryl, "print", "[at-least", "3", "[union-sum", "output:histogram", p("A"), p("B") + "]]")
    assert both == printed + f.read_text()
