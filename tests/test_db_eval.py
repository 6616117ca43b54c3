"""mgc_db_eval (meryl_amd.db.evaluate): a whole tree of merge and value operations per file slice, intermediate results in
HBM -- held to the same tree staged through mgc_db_merge / mgc_db_filter with a database at every node: every database the
evaluation writes has the staged node's files byte for byte, and what the callback receives is the staged root's content.
The same under MGC_MERGE_MANY=0 (every merge node through the left fold), in a fresh process."""
import os
import subprocess
import sys

import numpy as np
import pytest

import eval_helpers as H

pytestmark = pytest.mark.gpu

TREE_NAMES = sorted(H.trees("x"))


def dir_bytes(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d))}


def assert_same_database(a, b):
    da, db_ = dir_bytes(a), dir_bytes(b)
    assert sorted(da) == sorted(db_) and len(da) == 129, (a, b)
    for n in da:
        assert da[n] == db_[n], "%s differs between %s and %s" % (n, a, b)


@pytest.fixture(scope="module", params=sorted(H.CONFIGS))
def world(request, native_lib, tmp_path_factory):
    """the databases of one k, and every tree staged once: name -> (staged directory, staged root database)"""
    import torch
    assert torch.cuda.is_available(), "the -m gpu tests need a GPU"
    k = request.param
    base = str(tmp_path_factory.mktemp("eval_k%d" % k))
    wdir = os.path.join(base, "world")
    os.makedirs(wdir)
    H.make_world(wdir, k)
    staged = {}
    for name, t in H.trees(wdir).items():
        sdir = os.path.join(base, "staged", name)
        staged[name] = (sdir, H.run_staged(t, sdir))
    return {"k": k, "base": base, "dir": wdir, "staged": staged}


def check_against_staged(world, name, fused_dir, lo, hi, v):
    from meryl_amd import db
    t = H.trees(world["dir"])[name]
    sdir, sroot = world["staged"][name]
    for out in H.output_names(t):
        assert_same_database(os.path.join(fused_dir, out), os.path.join(sdir, out))
    assert sorted(n for n in os.listdir(fused_dir) if not n.endswith(".npz")) == sorted(H.output_names(t))   # nothing else was written
    r = db.Reader(sroot)
    wlo, whi, wv = r.read_all()
    w_prefix = r.info.prefix_size
    r.close()
    assert np.array_equal(lo, wlo) and np.array_equal(hi, whi) and np.array_equal(v, wv), name
    return wlo.size, w_prefix


@pytest.mark.parametrize("name", TREE_NAMES)
def test_tree_equals_the_staged_run(world, name):
    fdir = os.path.join(world["base"], "fused", name)
    lo, hi, v = H.run_fused(H.trees(world["dir"])[name], fdir)
    n, w_prefix = check_against_staged(world, name, fdir, lo, hi, v)
    if not name.startswith("merge34-subtract"):
        assert n > 0, "the case checks nothing"
    # an output takes the prefix size of its leftmost leaf: E (wider) leads merge5-max
    assert w_prefix == H.CONFIGS[world["k"]] + (2 if name == "merge5-max" else 0)


def test_every_merge_through_the_fold_in_a_fresh_process(world):
    """MGC_MERGE_MANY=0 is read per call, but the library is loaded once: a child process runs all the trees"""
    out = os.path.join(world["base"], "fold")
    env = dict(os.environ, MGC_MERGE_MANY="0")
    p = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "eval_helpers.py"), world["dir"], out],
                       capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    for name in TREE_NAMES:
        d = os.path.join(out, name)
        z = np.load(os.path.join(d, "callback.npz"))
        check_against_staged(world, name, d, z["lo"], z["hi"], z["v"])


def test_root_without_output_or_callback_still_writes_inner_outputs(world):
    from meryl_amd import db
    name = "three-level"
    body, _ = H._split(H.trees(world["dir"])[name])
    fdir = os.path.join(world["base"], "fused-inner-only")
    os.makedirs(fdir)
    db.evaluate(H.with_paths(body, fdir))                           # the root's {"output": ...} is gone
    assert os.listdir(fdir) == ["inner"]
    assert_same_database(os.path.join(fdir, "inner"), os.path.join(world["staged"][name][0], "inner"))
