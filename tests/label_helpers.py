"""Shared by test_labels.py, test_labels_host.py and the child process test_labels.py starts: the label table of
include/meryl_gpu_count.h (merylOpCompute::findOutputLabel, src/meryl2/merylOpCompute.C:286-395) as a short Python statement,
small labelled databases written by the HOST writer, and the tree of the tests run through meryl_amd.db.evaluate_labelled."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

M32 = 0xFFFFFFFF
M64 = 0xFFFFFFFFFFFFFFFF
LABEL_WORDS = ["default", "set", "first", "min", "max", "and", "or", "xor", "difference", "lightest", "heaviest", "invert", "selected"]
DEFAULT_CONSTANT = {"and": M64, "xor": M64, "lightest": M64}          # every other word: 0
# what `default` means under each merge operation (src/meryl2/merylCommandBuilder-processText.C:384-499)
DEFAULT_OF_MERGE = {0: "or", 10: "or", 3: "and", 6: "and", 1: "selected", 2: "selected", 4: "selected", 5: "selected", 7: "difference",
                    8: "first", 9: "first"}


def popcount(x):
    return bin(x).count("1")


def label_of(word, c, L, V, merge_op=None):
    """the label of a written k-mer: L[j], V[j] = label and value of active input j, in input order; c = the constant;
    merge_op = MGC_MERGE_* (None: a value operation)"""
    if word == "default":
        word = DEFAULT_OF_MERGE[merge_op] if merge_op is not None else "first"
    if word == "selected":
        if merge_op in (1, 4):
            return L[V.index(min(V))]                     # the first active input with the smallest value
        if merge_op in (2, 5):
            return L[V.index(max(V))]
        word = "first"
    if word == "set":
        return c
    if word == "first":
        return L[0]
    if word == "min":
        l, v = c, M32
        for lj, vj in zip(L, V):
            if vj < v:
                l, v = lj, vj
        return l
    if word == "max":
        return max([c] + list(L))
    if word in ("and", "or", "xor"):
        l = c
        for lj in L:
            l = (l & lj) if word == "and" else (l | lj) if word == "or" else (l ^ lj)
        return l
    if word == "difference":
        l = L[0] & ~c & M64
        for lj in L[1:]:
            l &= ~lj & M64
        return l
    if word in ("lightest", "heaviest"):
        l = c
        for lj in L:
            if (popcount(lj) < popcount(l)) if word == "lightest" else (popcount(lj) > popcount(l)):
                l = lj
        return l
    if word == "invert":
        assert len(L) == 1
        return ~L[0] & M64
    raise ValueError(word)


def sel_value(fop, v, c):
    """mgc_merge.hip sel_value for the value operations (src/meryl/merylOp-nextMer.C:490-557); 0 = dropped"""
    if fop <= 5:
        keep = [v < c, v > c, v >= c, v <= c, v == c, v != c][fop]
        return v if keep else 0
    if fop == 6:
        return M32 if v + c > M64 else (v + c) & M32
    if fop == 7:
        return 0 if v < c else (v - c) & M32
    if fop == 8:
        return M32 if v * c > M64 else (v * c) & M32
    if c == 0:
        return 0
    if fop == 9:
        return (v // c) & M32
    if fop == 10:
        return 1 if v < c else int(v / c + 0.5) & M32            # round half away from zero (values are positive)
    return (v % c) & M32


# ---- databases ------------------------------------------------------------------------------------------------------------
def prefixes(lo, hi, k, wp):
    import eval_helpers as H
    return H.prefixes(lo, hi, k, wp)


def write_labelled_db(path, lo, hi, cn, lab, k, wp, label_size):
    """ascending distinct k-mers (lo, hi), values and labels -> a database written by the host writer"""
    from meryl_amd import db
    w_data = 2 * k - wp
    starts = np.searchsorted(prefixes(lo, hi, k, wp), np.arange(0, (1 << wp) + 1, dtype=np.uint64))
    mlo = np.uint64((1 << w_data) - 1) if w_data < 64 else np.uint64(M64)
    mhi = np.uint64((1 << (w_data - 64)) - 1) if w_data > 64 else np.uint64(0)
    w = db.Writer(str(path), k, wp, label_size)
    for p in range(1 << wp):
        s, e = int(starts[p]), int(starts[p + 1])
        w.add_block(p, lo[s:e] & mlo, cn[s:e], (hi[s:e] & mhi) if w_data > 64 else None,
                    labels=lab[s:e] if label_size else None)
    w.close()


def read_db(path):
    """-> {k-mer int: (value, label)} and the label size"""
    from meryl_amd import db
    r = db.Reader(str(path))
    lo, hi, cn, lb = r.read_all(labels=True)
    ls = r.info.label_size
    r.close()
    keys = [(int(h) << 64) | int(l) for l, h in zip(lo.tolist(), hi.tolist())]
    assert keys == sorted(keys)
    return dict(zip(keys, zip(cn.tolist(), lb.tolist()))), ls


TREE_K = {21: 8, 51: 10}                         # k -> w_prefix of the tree test's databases
TREE_LABEL_SIZES = {"a": 7, "b": 12, "c": 0, "d": 12, "e": 0, "f": 0}


def make_tree_world(wdir, k):
    """databases a, b, c, d, e, f (c, e and f unlabelled) over one pool of k-mers, labels drawn over the full 64 bits (the writer keeps the
    low label_size of them)"""
    import eval_helpers as H
    rng = np.random.default_rng(100 + k)
    plo, phi = H.random_kmers(rng, k, 12_000)
    for name, n in (("a", 6000), ("b", 5000), ("c", 4000), ("d", 5000), ("e", 3000), ("f", 3000)):
        idx = np.sort(rng.choice(plo.size, n, replace=False))
        cn = rng.integers(1, 5, idx.size).astype(np.uint32)
        lab = rng.integers(0, 1 << 63, idx.size, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, idx.size, dtype=np.uint64)
        write_labelled_db(os.path.join(wdir, name), plo[idx], phi[idx], cn, lab, k, TREE_K[k], TREE_LABEL_SIZES[name])


def the_tree(wdir, out_dir):
    """subtract(union-sum[label=or](a, b, c) -> inner, at-least 2 (d)) -> root"""
    p = lambda n: os.path.join(wdir, n)                   # noqa: E731
    return ("subtract", ("union-sum", p("a"), p("b"), p("c"), {"label": "or", "output": os.path.join(out_dir, "inner")}),
            ("at-least", 2, p("d")), {"output": os.path.join(out_dir, "root")})


def run_tree(wdir, out_dir, label_size=0):
    """-> the root's slices as the callback received them: (lo, hi, values, labels), concatenated"""
    from meryl_amd import db
    os.makedirs(out_dir, exist_ok=True)
    got = [[], [], [], []]
    files = []

    def on_slice(ff, lo, hi, v, lab):
        files.append(ff)
        for col, a in zip(got, (lo, hi if hi is not None else np.zeros(lo.size, np.uint64), v, lab)):
            col.append(a)
    db.evaluate_labelled(the_tree(wdir, out_dir), on_slice, label_size=label_size)
    assert files == list(range(64))
    return tuple(np.concatenate(c) for c in got)


def main(argv):
    """child process (MGC_DECODE_HOST=1 is read once per call, the library is loaded once): the tree into out_dir"""
    wdir, out_dir = argv
    lo, hi, v, lab = run_tree(wdir, out_dir)
    np.savez(os.path.join(out_dir, "callback.npz"), lo=lo, hi=hi, v=v, lab=lab)
    print(json.dumps({"n": int(lo.size)}))


if __name__ == "__main__":
    main(sys.argv[1:])
