"""Shared by test_dbfile.py and the child process it starts (MGC_DECODE_HOST=1 is read once per call, the library is loaded once):
small databases of three shapes written by the host writer, data files made readable by the host decoder only or damaged, and what
the three consumers of whole databases -- the lookup load, the operation trees and meryl-analyze -- give for one of them."""
import json
import os
import shutil
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# name -> (k, w_prefix, label_size, k-mers per block at most, every third prefix empty)
SHAPES = {"k4": (4, 6, 0, 4, True),          # one block per file, a handful of k-mers each, empty files
          "k16": (16, 12, 0, 6, False),
          "k40": (40, 8, 9, 7, False)}       # two key words, labels


def data_file(path, ff):
    return os.path.join(path, "0x" + format(ff, "06b") + ".merylData")


def write_db(path, shape, seed):
    from meryl_amd import db
    k, wp, label_size, per_block, gaps = SHAPES[shape]
    rng = np.random.default_rng(seed)
    sbits = 2 * k - wp
    w = db.Writer(path, k, wp, label_size)
    for prefix in range(1 << wp):
        if gaps and prefix % 3 == 1:
            continue
        n = int(rng.integers(1, per_block + 1))
        if sbits <= 8:
            n = min(n, 1 << sbits)
            lo = np.arange(n, dtype=np.uint64)
        else:
            lo = np.cumsum(rng.integers(1, 1 << (min(sbits, 64) - 4), n, dtype=np.uint64), dtype=np.uint64)
        hi = np.cumsum(rng.integers(0, 3, n, dtype=np.uint64), dtype=np.uint64) if sbits > 64 else None
        w.add_block(prefix, lo, rng.integers(1, 6, n).astype(np.uint32), hi,
                    labels=rng.integers(0, 1 << label_size, n, dtype=np.uint64) if label_size else None)
    w.close()


def first_block(path, ff):
    """position of the first block of file ff that holds k-mers, or None"""
    from meryl_amd import db
    r = db.Reader(path)
    rows = r.file_index(ff)
    r.close()
    for _, position, n in rows:
        if n:
            return position
    return None


def nonempty_files(path):
    return [ff for ff in range(64) if first_block(path, ff) is not None]


def make_host_only(path, ff):
    """doubles the 8-byte lenmax field of a block of file ff: the raw reader answers MGC_EUNSUPPORTED, the host decoder reads the same k-mers"""
    pos = first_block(path, ff)
    assert pos is not None
    with open(data_file(path, ff), "r+b") as f:
        f.seek(pos)
        (lenmax,) = struct.unpack("<Q", f.read(8))
        f.seek(pos)
        f.write(struct.pack("<Q", 2 * lenmax))


def truncate(path, ff):
    size = os.path.getsize(data_file(path, ff))
    assert size
    with open(data_file(path, ff), "r+b") as f:
        f.truncate(size // 2)


def overwrite_magic(path, ff):
    """the first word of one block's bit stream: the framing stays canonical, the device decoder reports the block through its error word"""
    pos = first_block(path, ff)
    with open(data_file(path, ff), "r+b") as f:
        f.seek(pos + 8)
        (nsb,) = struct.unpack("<I", f.read(4))
        f.seek(pos + 16 + 16 * nsb + 16)                  # header, the sub-blocks' begins and lengths, the first sub-block's two words
        f.write(struct.pack("<Q", 0x0123456789ABCDEF))


def copy_db(src, dst):
    shutil.copytree(src, dst)
    return dst


def read_host(path):
    """-> lo, hi, values, labels of the whole database, by the host reader"""
    from meryl_amd import db
    r = db.Reader(path)
    out = r.read_all(labels=True)
    r.close()
    return out


def key_tensor(lo, hi, k):
    import torch
    a = lo.view(np.int64) if k <= 32 else np.stack([lo.view(np.int64), hi.view(np.int64)], axis=1)
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def consume(path, orig, shape):
    """what the three consumers give for database `path` (a copy of `orig` with other framing): a dict of numpy arrays"""
    from meryl_amd import analyze, db
    from meryl_amd.lookup import Lookup
    k, _, label_size, _, _ = SHAPES[shape]
    lo, hi, _, _ = read_host(orig)
    keys = key_tensor(lo, hi, k)
    out = {}
    for tag, min_value in (("all", 0), ("min2", 2)):
        with Lookup.load(path, min_value=min_value) as t:
            out["lookup_" + tag] = t.values(keys).cpu().numpy().view(np.uint32)
            out["info_" + tag] = np.array([t.info.n_kmers, t.info.n_kmers_in_db], dtype=np.uint64)
    cols = [[], [], []]

    def on_sum(ff, l, h, v, *lab):
        for c, a in zip(cols, (l, h if h is not None else np.zeros(0, np.uint64), v)):
            c.append(a)
    # (the plain evaluation refuses databases that store labels)
    (db.evaluate_labelled if label_size else db.evaluate)(("union-sum", orig, path), on_sum)
    out["sum_lo"], out["sum_hi"], out["sum_v"] = (np.concatenate(c) for c in cols)
    if label_size:
        lcols = [[], []]
        db.evaluate_labelled(("at-least", 1, path), lambda ff, l, h, v, lab: [c.append(a) for c, a in zip(lcols, (l, lab))])
        out["lab_lo"], out["lab"] = (np.concatenate(c) for c in lcols)
    with analyze.Analyzer(k, "gc") as a:
        a.add_database(path)
        for which in (0, 1):
            for name, col in zip("svo", a.result(which)):
                out["an%d_%s" % (which, name)] = col
    return out


def main(argv):
    """child process: consume() of every (path, orig, shape) of the JSON job file -> <path>.npz"""
    with open(argv[0]) as f:
        jobs = json.load(f)
    for path, orig, shape in jobs:
        np.savez(path + ".npz", **consume(path, orig, shape))
    print(json.dumps({"n": len(jobs)}))


if __name__ == "__main__":
    main(sys.argv[1:])
