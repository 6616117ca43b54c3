"""Shared by test_db_eval.py (and the child process it starts): small random databases written by the HOST writer, the
operation trees under test, the same tree run fused (mgc_db_eval) and staged (mgc_db_merge / mgc_db_filter with a database at
every node)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CONFIGS = {21: 10, 51: 12}                       # k -> w_prefix
EMPTY_FILES = (0, 1, 17, 40, 63)                 # database D holds nothing in these files


def random_kmers(rng, k, n):
    """about n distinct ascending k-mers as (lo, hi)"""
    bits = 2 * k
    lo = rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n, dtype=np.uint64)
    hi = np.zeros(n, np.uint64)
    if bits < 64:
        lo &= np.uint64((1 << bits) - 1)
    if bits > 64:
        hi = rng.integers(0, 1 << 62, n, dtype=np.uint64) & np.uint64((1 << (bits - 64)) - 1)
        hi[: n // 3] = hi[0]                      # runs that differ in the low word only
    order = np.lexsort((lo, hi))
    lo, hi = lo[order], hi[order]
    keep = np.ones(n, bool)
    keep[1:] = (lo[1:] != lo[:-1]) | (hi[1:] != hi[:-1])
    return lo[keep], hi[keep]


def prefixes(lo, hi, k, wp):
    w_data = 2 * k - wp
    if w_data >= 64:
        return (hi >> np.uint64(w_data - 64)) if w_data > 64 else hi.copy()
    p = lo >> np.uint64(w_data)
    if 2 * k > 64:
        p = p | (hi << np.uint64(64 - w_data))
    return p


def write_db(path, lo, hi, cn, k, wp):
    from meryl_amd import db
    w_data = 2 * k - wp
    starts = np.searchsorted(prefixes(lo, hi, k, wp), np.arange(0, (1 << wp) + 1, dtype=np.uint64))
    mlo = np.uint64((1 << w_data) - 1) if w_data < 64 else np.uint64(0xFFFFFFFFFFFFFFFF)
    mhi = np.uint64((1 << (w_data - 64)) - 1) if w_data > 64 else np.uint64(0)
    w = db.Writer(str(path), k, wp)
    for p in range(1 << wp):
        s, e = int(starts[p]), int(starts[p + 1])
        w.add_block(p, lo[s:e] & mlo, cn[s:e], (hi[s:e] & mhi) if w_data > 64 else None)
    w.close()


def make_world(world_dir, k):
    """Databases A..E (20,000-60,000 k-mers drawn from one pool, 30-60 % shared between any two; D empty in some files; E
    with a wider prefix than the others) and S00..S33 (500 k-mers each from a pool of 3000)."""
    wp = CONFIGS[k]
    rng = np.random.default_rng(k)
    plo, phi = random_kmers(rng, k, 90_000)
    pfile = prefixes(plo, phi, k, 6)

    def one(name, n, wp_, pool_lo, pool_hi, drop_files=()):
        idx = np.sort(rng.choice(pool_lo.size, n, replace=False))
        if drop_files:
            idx = idx[~np.isin(prefixes(pool_lo[idx], pool_hi[idx], k, 6), np.array(drop_files, dtype=np.uint64))]
        cn = rng.integers(1, 60, idx.size).astype(np.uint32)
        cn[::97] = np.uint32(0xFFFFFFF0)             # sums that wrap (to something above 0)
        write_db(os.path.join(world_dir, name), pool_lo[idx], pool_hi[idx], cn, k, wp_)
    assert pfile.max() == 63
    one("A", 60_000, wp, plo, phi)
    one("B", 45_000, wp, plo, phi)
    one("C", 30_000, wp, plo, phi)
    one("D", 40_000, wp, plo, phi, EMPTY_FILES)
    one("E", 20_000, wp + 2, plo, phi)
    slo, shi = plo[::30], phi[::30]
    for i in range(34):
        one("S%02d" % i, 500, wp, slo, shi)


def trees(world_dir):
    """name -> tree; {"output": <name>} is relative to the run's output directory"""
    p = lambda n: os.path.join(world_dir, n)                      # noqa: E731
    A, B, C, D, E = p("A"), p("B"), p("C"), p("D"), p("E")
    S = [p("S%02d" % i) for i in range(34)]
    out = {"output": "root"}
    return {
        "merge2": ("union-sum", A, B, out),
        "merge3": ("subtract", A, D, C, out),
        "merge3-union": ("union", D, B, C, out),
        "merge5": ("symmetric-difference", A, B, C, D, E, out),
        "merge5-max": ("union-max", E, D, C, B, A, out),
        "quick-start": ("intersect", ("at-least", 3, A), ("at-least", 2, B)),
        "subtract-tree": ("subtract", ("union-sum", A, B, C), ("multiply", 2, D), out),
        "three-level": ("union-max", ("intersect-sum", ("greater-than", 1, A), B, {"output": "inner"}), ("decrease", 1, E), C, out),
        "merge34-union": tuple(["union"] + S + [out]),
        "merge34-symmetric-difference": tuple(["symmetric-difference"] + S + [out]),
        "merge34-subtract": tuple(["subtract"] + S + [out]),
    }


def _split(t):
    t = tuple(t)
    name = None
    if isinstance(t[-1], dict):
        name = t[-1].get("output")
        t = t[:-1]
    return t, name


def with_paths(t, out_dir):
    """the tree with its output names turned into paths under out_dir"""
    if isinstance(t, str):
        return t
    body, name = _split(t)
    from meryl_amd import db
    if body[0] in db.VALUE_WORDS:
        new = (body[0], body[1], with_paths(body[2], out_dir))
    else:
        new = (body[0],) + tuple(with_paths(c, out_dir) for c in body[1:])
    return new + (({"output": os.path.join(out_dir, name)},) if name else ())


def run_fused(t, out_dir):
    """mgc_db_eval of the tree; -> the root's k-mers and values as the callback received them, concatenated"""
    from meryl_amd import db
    os.makedirs(out_dir, exist_ok=True)
    files, los, his, vals = [], [], [], []

    def on_slice(ff, lo, hi, v):
        files.append(ff)
        los.append(lo)
        his.append(hi if hi is not None else np.zeros(lo.size, np.uint64))
        vals.append(v)
    db.evaluate(with_paths(t, out_dir), on_slice)
    assert files == list(range(64))
    return np.concatenate(los), np.concatenate(his), np.concatenate(vals)


def run_staged(t, out_dir):
    """the same tree with a database at every node (mgc_db_merge / mgc_db_filter); -> the root's database"""
    import ctypes
    from meryl_amd import capi, db
    os.makedirs(out_dir, exist_ok=True)
    L = capi.lib()
    counter = [0]

    def go(t):
        if isinstance(t, str):
            return t
        body, name = _split(t)
        if name is None:
            counter[0] += 1
            name = "node%d" % counter[0]
        out = os.path.join(out_dir, name)
        if body[0] in db.VALUE_WORDS:
            src = go(body[2])
            capi.check(L.mgc_db_filter(src.encode(), db.VALUE_WORDS[body[0]], int(body[1]), out.encode(), -1, 4), "mgc_db_filter")
        else:
            srcs = [go(c).encode() for c in body[1:]]
            arr = (ctypes.c_char_p * len(srcs))(*srcs)
            capi.check(L.mgc_db_merge(arr, len(srcs), db.MERGE_WORDS[body[0]], out.encode(), -1, 4), "mgc_db_merge")
        return out
    return go(t)


def output_names(t):
    if isinstance(t, str):
        return []
    body, name = _split(t)
    kids = body[2:] if isinstance(body[1], int) else body[1:]
    return sum((output_names(c) for c in kids), []) + ([name] if name else [])


def main(argv):
    """child process: every tree fused, outputs under <out_dir>/<tree>/, the callback's arrays in <out_dir>/<tree>/callback.npz"""
    world_dir, out_dir = argv
    for name, t in trees(world_dir).items():
        d = os.path.join(out_dir, name)
        lo, hi, v = run_fused(t, d)
        np.savez(os.path.join(d, "callback.npz"), lo=lo, hi=hi, v=v)
    print(json.dumps({"trees": len(trees(world_dir))}))


if __name__ == "__main__":
    main(sys.argv[1:])
