"""The one loader of database files (meryl_amd/csrc/mgc_dbfile.cpp) under its three consumers -- the lookup load, the operation trees
and meryl-analyze -- on databases where some or all data files are framed in a way only the host decoder follows (the natural
fallback, file by file), and the owning device buffers (mgc_devbuf.hpp): after every handle is closed and after every failed call,
mgc_dev_buffers_live is back where it was.  Expected values come from the host reader (meryl_amd.db.Reader), never from the device."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import dbfile_helpers as H

pytestmark = pytest.mark.gpu
VARIANTS = ("orig", "mixed", "all")


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """per shape: the database, a copy with file 0, a middle file and the last non-empty file host-only, a copy with every non-empty
    file host-only; what the consumers give for each, in this process and in one child with MGC_DECODE_HOST=1"""
    base = str(tmp_path_factory.mktemp("dbfile"))
    w = {"base": base}
    jobs = []
    for i, shape in enumerate(H.SHAPES):
        orig = os.path.join(base, shape + ".orig")
        H.write_db(orig, shape, 7 + i)
        files = H.nonempty_files(orig)
        assert len(files) >= 32 and (shape != "k4" or len(files) < 64)
        mixed = H.copy_db(orig, os.path.join(base, shape + ".mixed"))
        for ff in (files[0], files[len(files) // 2], files[-1]):
            H.make_host_only(mixed, ff)
        every = H.copy_db(orig, os.path.join(base, shape + ".all"))
        for ff in files:
            H.make_host_only(every, ff)
        w[shape] = {"orig": orig, "mixed": mixed, "all": every, "host": H.read_host(orig)}
        for v in VARIANTS:
            w[shape]["got_" + v] = H.consume(w[shape][v], orig, shape)
            host_copy = H.copy_db(w[shape][v], os.path.join(base, shape + "." + v + ".child"))
            jobs.append((host_copy, orig, shape))
    job_file = os.path.join(base, "jobs.json")
    with open(job_file, "w") as f:
        json.dump(jobs, f)
    p = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "dbfile_helpers.py"), job_file],
                       capture_output=True, text=True, timeout=600, env=dict(os.environ, MGC_DECODE_HOST="1"))
    assert p.returncode == 0, p.stderr[-3000:]
    for path, _, shape in jobs:
        w[shape]["child_" + path.split(".")[-2]] = dict(np.load(path + ".npz"))
    return w


def gc_rows(lo, hi, v, k):
    """meryl-analyze -gc restated: score = the C and G among the k bases (codes A0 C1 T2 G3: the low bit); the reverse histogram is AT,
    score k - GC -> per histogram (scores, values, occurrences), ascending by (score, value)"""
    gc = np.zeros(lo.size, dtype=np.uint64)
    for j in range(k):
        gc += ((lo if j < 32 else hi) >> np.uint64(2 * (j % 32))) & np.uint64(1)
    out = []
    for score in (gc, np.uint64(k) - gc):
        u, c = np.unique((score << np.uint64(32)) | v.astype(np.uint64), return_counts=True)
        out.append((u >> np.uint64(32), u & np.uint64(0xFFFFFFFF), c.astype(np.uint64)))
    return out


@pytest.mark.parametrize("decode", ("got", "child"))
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("shape", list(H.SHAPES))
def test_mixed_framing_gives_the_same_results(world, shape, variant, decode):
    k, _, label_size, _, _ = H.SHAPES[shape]
    lo, hi, v, lab = world[shape]["host"]
    got = world[shape][decode + "_" + variant]
    # the lookup: every stored k-mer finds its value (a host-decoded file between device-decoded ones lands at its running offset)
    assert np.array_equal(got["lookup_all"], v)
    assert np.array_equal(got["lookup_min2"], np.where(v >= 2, v, 0).astype(np.uint32))
    assert got["info_all"].tolist() == [v.size, v.size]
    assert got["info_min2"].tolist() == [int((v >= 2).sum()), v.size]
    # union-sum(original, this copy): the same k-mers, doubled values
    assert np.array_equal(got["sum_lo"], lo)
    assert np.array_equal(got["sum_hi"], hi if k > 32 else np.zeros(0, np.uint64))
    assert np.array_equal(got["sum_v"], 2 * v)
    if label_size:
        assert np.array_equal(got["lab_lo"], lo) and np.array_equal(got["lab"], lab)
        assert lab.max() > 0
    # meryl-analyze -gc: the rows counted on the host from the host reader's k-mers
    for which, rows in enumerate(gc_rows(lo, hi, v, k)):
        for name, want in zip("svo", rows):
            assert np.array_equal(got["an%d_%s" % (which, name)], want), (which, name)


# ---- every path gives the memory back ---------------------------------------------------------------------------------------------------
def live():
    from meryl_amd import capi
    b, n = ctypes.c_uint64(0), ctypes.c_uint64(0)
    assert capi.lib().mgc_dev_buffers_live(ctypes.byref(b), ctypes.byref(n)) == 0
    return b.value, n.value


@pytest.fixture(scope="module")
def baseline(world):
    from meryl_amd.lookup import Lookup
    Lookup.load(world["k16"]["orig"]).close()                  # warm-up
    return live()


def load_lookup(path):
    from meryl_amd.lookup import Lookup
    with Lookup.load(path, min_value=2) as t:
        assert t.info.n_kmers_in_db > 0


def run_tree(path):
    from meryl_amd import db
    db.evaluate(("union-sum", path, path), lambda ff, lo, hi, v: None)


def run_analyzer(path, k=16):
    from meryl_amd import analyze
    with analyze.Analyzer(k, "gc") as a:
        a.add_database(path)


CONSUMERS = {"lookup": load_lookup, "tree": run_tree, "analyzer": run_analyzer}


@pytest.mark.parametrize("consumer", list(CONSUMERS))
@pytest.mark.parametrize("variant", VARIANTS)
def test_a_successful_call_gives_the_memory_back(world, baseline, consumer, variant):
    CONSUMERS[consumer](world["k16"][variant])
    assert live() == baseline


def test_closed_handles_give_the_memory_back(world, baseline, tmp_path):
    import torch
    from meryl_amd import count, db, poslookup
    from meryl_amd.lookup import Lookup
    lo, hi, v, _ = world["k16"]["host"]
    keys, vals = H.key_tensor(lo, hi, 16), torch.from_numpy(v.view(np.int32)).cuda()
    rng = np.random.default_rng(3)
    bases = torch.from_numpy(np.concatenate([rng.choice(np.frombuffer(b"ACGT", np.uint8), 5000), np.frombuffer(b".", np.uint8)])).cuda()
    t = Lookup.from_device(keys, vals, 16, min_value=2)
    assert live() != baseline
    idx = poslookup.PositionIndex(t, bases)
    p = poslookup.Painter(idx)
    p.add(bases, [0, bases.numel()])
    p.mers()
    p.close()
    idx.close()
    t.close()
    assert live() == baseline
    h = db.ValueHistogram()
    h.add(vals)
    assert h.totals()[1] == v.size and live() != baseline
    h.close()
    assert live() == baseline
    s = count.DbStream(str(tmp_path / "out"), 16, 12)
    s.write(keys, vals, 0, 1 << 12)
    s.sync()
    assert live() != baseline
    s.close()
    assert live() == baseline
    r = count.Runs(16, 12)
    half = v.size // 2
    r.add(keys[:half].contiguous(), vals[:half].contiguous())
    r.add(keys[half:].contiguous(), vals[half:].contiguous())
    s = count.DbStream(str(tmp_path / "merged"), 16, 12)
    r.write(s, 0, 1 << 12)
    s.close()
    r.close()
    assert live() == baseline
    got = H.read_host(str(tmp_path / "merged"))
    assert np.array_equal(got[0], lo) and np.array_equal(got[2], v)


@pytest.mark.parametrize("consumer", list(CONSUMERS))
@pytest.mark.parametrize("damage", ("truncated", "magic"))
def test_a_failed_call_gives_the_memory_back(world, baseline, tmp_path, consumer, damage):
    """file 9 is refused by the host (truncated: after files 0-8 have grown the buffers), or reported by the device decoder through its
    error word (the first word of a block's bit stream overwritten: the framing check passes)"""
    from meryl_amd import capi
    bad = H.copy_db(world["k16"]["orig"], str(tmp_path / "bad"))
    (H.truncate if damage == "truncated" else H.overwrite_magic)(bad, 9)
    with pytest.raises(capi.MgcError) as e:
        CONSUMERS[consumer](bad)
    if damage == "magic":
        assert "corrupt block in a database file (device decoder, code 1)" in str(e.value)
    else:
        assert "corrupt block in" in str(e.value) and "device decoder" not in str(e.value)     # the host reader's message for that file
    assert live() == baseline
