"""meryl-analyze on the device: per-k-mer composition scores and the (score, value) histograms of -gc / -ga / -gt.

Expected results come from a model inside this file.  For small inputs it is a per-base Python loop that restates the
reference's counters (src/meryl-analyze/meryl-analyze.C:176-201, :262-299, :364-401: one counter per letter, a run is scored
when the other alphabet interrupts it and both letters were seen); for large inputs the same counters as numpy arrays, held
to the Python loop on random k-mers below.  The k-mers and values of a database come from the HOST reader
(meryl_amd.db.Reader.read_all), never from the device decoder."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GC, GA, GT = 0, 1, 2
FORWARD, REVERSE, COMBINED = 0, 1, 2
CODE = {"A": 0, "C": 1, "T": 2, "G": 3}
W_PREFIX = 10
NAMES = {GC: (("GC", FORWARD), ("AT", REVERSE)),
         GA: (("GA_TC", COMBINED), ("GA", FORWARD), ("TC", REVERSE)),
         GT: (("GT_AC", COMBINED), ("GT", FORWARD), ("AC", REVERSE))}
# forward alphabet (first letter, second letter), reverse alphabet
ALPHABETS = {GA: ((0, 3), (2, 1)), GT: ((3, 2), (0, 1))}


# ---- the model ---------------------------------------------------------------------------------------------------------
def pack(s):
    """k-mer text -> Python int, first base most significant"""
    x = 0
    for ch in s:
        x = (x << 2) | CODE[ch]
    return x


def py_scores(x, k, type):
    """(fscore, rscore) of the k-mer held by the Python int x, base by base from the last base on"""
    if type == GC:
        c = g = a = t = 0
        for _ in range(k):
            b = x & 3
            if b == 1:
                c += 1
            elif b == 3:
                g += 1
            elif b == 0:
                a += 1
            else:
                t += 1
            x >>= 2
        return c + g, a + t
    (f0, f1), (r0, r1) = ALPHABETS[type]
    fscore = rscore = 0
    fa = fb = ra = rb = 0                       # letters of the open forward run, of the open reverse run
    for _ in range(k):
        b = x & 3
        if b == f0 or b == f1:
            if ra > 0 and rb > 0:
                rscore += ra + rb
            ra = rb = 0
            if b == f0:
                fa += 1
            else:
                fb += 1
        else:
            if fa > 0 and fb > 0:
                fscore += fa + fb
            fa = fb = 0
            if b == r0:
                ra += 1
            else:
                rb += 1
        x >>= 2
    if fa > 0 and fb > 0:
        fscore += fa + fb
    if ra > 0 and rb > 0:
        rscore += ra + rb
    return fscore, rscore


def np_scores(lo, hi, k, type):
    """the same counters over arrays of k-mers (lo, hi uint64) -> (fscore, rscore) uint8 arrays"""
    n = lo.size
    z = lambda: np.zeros(n, dtype=np.uint8)    # noqa: E731
    if type == GC:
        f = z()
        for j in range(k):
            w = lo if j < 32 else hi
            f += ((w >> np.uint64(2 * (j % 32))) & np.uint64(1)).astype(np.uint8)
        return f, (np.uint8(k) - f).astype(np.uint8)
    (f0, f1), (r0, r1) = ALPHABETS[type]
    fscore, rscore, fa, fb, ra, rb = z(), z(), z(), z(), z(), z()
    for j in range(k):
        w = lo if j < 32 else hi
        b = ((w >> np.uint64(2 * (j % 32))) & np.uint64(3)).astype(np.uint8)
        fwd = (b == f0) | (b == f1)
        rev = ~fwd
        rscore += np.where(fwd & (ra > 0) & (rb > 0), ra + rb, 0).astype(np.uint8)
        fscore += np.where(rev & (fa > 0) & (fb > 0), fa + fb, 0).astype(np.uint8)
        ra[fwd] = 0
        rb[fwd] = 0
        fa[rev] = 0
        fb[rev] = 0
        fa += (b == f0)
        fb += (b == f1)
        ra += (b == r0)
        rb += (b == r1)
    fscore += np.where((fa > 0) & (fb > 0), fa + fb, 0).astype(np.uint8)
    rscore += np.where((ra > 0) & (rb > 0), ra + rb, 0).astype(np.uint8)
    return fscore, rscore


def rows_of(score, values):
    """(score, value) pairs -> the rows printHist walks: (scores uint32, values uint32, occurrences uint64), ascending"""
    small = values < 4096                      # counted by index; the few others by sorting.  The two sets share no row
    dense = np.bincount(score[small].astype(np.int64) * 4096 + values[small].astype(np.int64), minlength=65 * 4096)
    idx = np.nonzero(dense)[0].astype(np.uint64)
    key = (score[~small].astype(np.uint64) << np.uint64(32)) | values[~small].astype(np.uint64)
    u, c = np.unique(key, return_counts=True)
    keys = np.concatenate([((idx >> np.uint64(12)) << np.uint64(32)) | (idx & np.uint64(4095)), u])
    occ = np.concatenate([dense[idx.astype(np.int64)].astype(np.uint64), c.astype(np.uint64)])
    order = np.argsort(keys, kind="stable")
    keys, occ = keys[order], occ[order]
    return (keys >> np.uint64(32)).astype(np.uint32), (keys & np.uint64(0xFFFFFFFF)).astype(np.uint32), occ


def np_scores_threaded(lo, hi, k, type, pieces=16):
    """np_scores over slices of the arrays on a few threads (numpy's loops run outside the interpreter lock)"""
    if lo.size < (1 << 20):
        return np_scores(lo, hi, k, type)
    from concurrent.futures import ThreadPoolExecutor
    cuts = np.linspace(0, lo.size, pieces + 1).astype(np.int64)
    with ThreadPoolExecutor(max_workers=8) as pool:
        parts = list(pool.map(lambda i: np_scores(lo[cuts[i]:cuts[i + 1]], hi[cuts[i]:cuts[i + 1]], k, type), range(pieces)))
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def model_rows(lo, hi, values, k, type):
    """{which: rows} of a report"""
    f, r = np_scores_threaded(lo, hi, k, type)
    out = {FORWARD: rows_of(f, values), REVERSE: rows_of(r, values)}
    if type != GC:
        out[COMBINED] = rows_of(np.maximum(f, r), values)
    return out


def rows_text(rows):
    s, v, o = rows
    return "".join("%u\t%u\t%u\n" % (int(a), int(b), int(c)) for a, b, c in zip(s, v, o)).encode()


def test_the_array_model_is_the_per_base_loop():
    rng = np.random.default_rng(5)
    for k in (1, 2, 7, 21, 32, 33, 51, 64):
        lo, hi = random_kmers(rng, 300, k, distinct=False)
        for t in (GC, GA, GT):
            f, r = np_scores(lo, hi, k, t)
            want = [py_scores((int(h) << 64) | int(l), k, t) for l, h in zip(lo, hi)]
            assert [(int(a), int(b)) for a, b in zip(f, r)] == want, (k, t)


# ---- helpers -----------------------------------------------------------------------------------------------------------
def random_kmers(rng, n, k, distinct=True):
    """(lo, hi) of n random k-mers, ascending and distinct when asked"""
    nlo, nhi = min(k, 32), max(k - 32, 0)
    lo = rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n, dtype=np.uint64)
    hi = rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n, dtype=np.uint64)
    lo &= np.uint64((1 << (2 * nlo)) - 1)
    hi &= np.uint64((1 << (2 * nhi)) - 1)
    if distinct:
        if k <= 32:
            lo = np.unique(lo)
            hi = np.zeros(lo.size, dtype=np.uint64)
        else:
            order = np.lexsort((lo, hi))
            lo, hi = lo[order], hi[order]
            keep = np.ones(lo.size, dtype=bool)
            keep[1:] = (lo[1:] != lo[:-1]) | (hi[1:] != hi[:-1])
            lo, hi = lo[keep], hi[keep]
    return lo, hi


def split_int(x):
    return np.uint64(x & 0xFFFFFFFFFFFFFFFF), np.uint64(x >> 64)


def to_device(lo, hi, k):
    import torch
    if k > 32:
        a = np.stack([lo, hi], axis=1).astype(np.uint64)
        return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()
    return torch.from_numpy(np.ascontiguousarray(lo).view(np.int64)).cuda()


def values_to_device(values):
    import torch
    return torch.from_numpy(np.ascontiguousarray(values, dtype=np.uint32).view(np.int32)).cuda()


def prefixes(lo, hi, k):
    w_data = 2 * k - W_PREFIX
    if w_data >= 64:
        return hi >> np.uint64(w_data - 64)
    if k > 32:
        return (hi << np.uint64(64 - w_data)) | (lo >> np.uint64(w_data))
    return lo >> np.uint64(w_data)


def write_db(path, lo, hi, values, k, label_size=0, label=0):
    """ascending distinct k-mers + values -> database directory, by the HOST writer"""
    from meryl_amd import db
    w_data = 2 * k - W_PREFIX
    starts = np.searchsorted(prefixes(lo, hi, k), np.arange(0, (1 << W_PREFIX) + 1, dtype=np.uint64))
    mlo = np.uint64((1 << w_data) - 1) if w_data < 64 else np.uint64(0xFFFFFFFFFFFFFFFF)
    mhi = np.uint64((1 << (w_data - 64)) - 1) if w_data > 64 else np.uint64(0)
    values = np.asarray(values, dtype=np.uint32)
    w = db.Writer(str(path), k, W_PREFIX, label_size)
    for p in range(1 << W_PREFIX):
        s, e = int(starts[p]), int(starts[p + 1])
        w.add_block(p, lo[s:e] & mlo, values[s:e], (hi[s:e] & mhi) if w_data > 64 else None, label=label)
    w.close()


def read_db(path):
    from meryl_amd import db
    r = db.Reader(str(path))
    lo, hi, values = r.read_all()
    r.close()
    return lo, hi, values


def assert_rows(got, want, what):
    for name, g, w in zip(("scores", "values", "occurrences"), got, want):
        assert g.dtype == w.dtype, (what, name, g.dtype)
        assert g.size == w.size, (what, name, g.size, w.size)
        assert np.array_equal(g, w), (what, name)


def assert_report(a, model, type, what):
    for which in model:
        assert_rows(a.result(which), model[which], (what, type, which))


def analyze_db(path, k, type):
    from meryl_amd import analyze
    a = analyze.Analyzer(k, type)
    a.add_database(path, 4)
    return a


# ---- scores ------------------------------------------------------------------------------------------------------------
TABLE = (("GAGAC", (3, 2), (4, 0), (0, 2)),
         ("AAAAA", (0, 5), (0, 0), (0, 0)),
         ("TCTCG", (3, 2), (0, 4), (0, 0)),
         ("GTGTA", (2, 3), (0, 0), (4, 0)),
         ("GGAGCT", (4, 2), (4, 2), (0, 0)),
         ("GAGACTCTGAA", (5, 6), (7, 4), (2, 2)),
         ("ACGTACGTACGTACGTACGTA", (10, 11), (0, 0), (10, 10)))


def device_scores(xs, k, type):
    from meryl_amd import analyze
    pairs = [split_int(x) for x in xs]
    lo = np.array([p[0] for p in pairs], dtype=np.uint64)
    hi = np.array([p[1] for p in pairs], dtype=np.uint64)
    f, r = analyze.scores(to_device(lo, hi, k), k, type)
    return [(int(a), int(b)) for a, b in zip(f.cpu().numpy(), r.cpu().numpy())]


def test_known_answers(native_lib):
    for s, gc, ga, gt in TABLE:
        for t, want in ((GC, gc), (GA, ga), (GT, gt)):
            assert py_scores(pack(s), len(s), t) == want, (s, t)
            assert device_scores([pack(s)], len(s), t) == [want], (s, t)


@pytest.mark.parametrize("k", [1, 2, 7, 21, 31, 32, 33, 51, 64])
def test_random_kmers_against_the_per_base_loop(native_lib, k):
    rng = np.random.default_rng(100 + k)
    lo, hi = random_kmers(rng, 4000, k, distinct=False)
    xs = [(int(h) << 64) | int(l) for l, h in zip(lo, hi)]
    for t in (GC, GA, GT):
        assert device_scores(xs, k, t) == [py_scores(x, k, t) for x in xs], (k, t)


def test_homopolymers_and_alternating_kmers_reach_k_and_0(native_lib):
    k = 64
    want = {  # k-mer -> ((gc), (ga), (gt))
        "A" * k: ((0, k), (0, 0), (0, 0)), "C" * k: ((k, 0), (0, 0), (0, 0)),
        "G" * k: ((k, 0), (0, 0), (0, 0)), "T" * k: ((0, k), (0, 0), (0, 0)),
        "GA" * 32: ((32, 32), (k, 0), (0, 0)), "AG" * 32: ((32, 32), (k, 0), (0, 0)),
        "GT" * 32: ((32, 32), (0, 0), (k, 0)), "TG" * 32: ((32, 32), (0, 0), (k, 0)),
        "AC" * 32: ((32, 32), (0, 0), (0, k)), "CA" * 32: ((32, 32), (0, 0), (0, k)),
        "TC" * 32: ((32, 32), (0, k), (0, 0)), "CT" * 32: ((32, 32), (0, k), (0, 0)),
    }
    for s, per_type in want.items():
        for t, w in zip((GC, GA, GT), per_type):
            assert py_scores(pack(s), k, t) == w, (s, t)
            assert device_scores([pack(s)], k, t) == [w], (s[:4], t)


# ---- histograms ----------------------------------------------------------------------------------------------------------
def tier_values():
    from meryl_amd import analyze
    d = analyze.DENSE_VALUES
    return [0, 1, d - 1, d, d + 1, 65535, 65536, 2 ** 32 - 1]


@pytest.mark.parametrize("k", [21, 51])
def test_values_around_the_tier_bound(native_lib, tmp_path, k):
    rng = np.random.default_rng(k)
    lo, hi = random_kmers(rng, 6000, k)
    tv = np.array(tier_values(), dtype=np.uint32)
    values = tv[rng.integers(0, tv.size, lo.size)]
    path = tmp_path / "db.meryl"
    write_db(path, lo, hi, values, k)
    rlo, rhi, rv = read_db(path)
    assert np.array_equal(rlo, lo) and np.array_equal(rv, values) and set(rv.tolist()) == set(tv.tolist())
    for t in (GC, GA, GT):
        model = model_rows(rlo, rhi, rv, k, t)
        a = analyze_db(path, k, t)
        assert_report(a, model, t, "tier")
        info = a.info()
        above = int((rv >= tv[3]).sum())
        assert info["n_kmers"] == lo.size and info["n_files"] == 64 and info["n_overflow_kmers"] == above
        a.close()


def test_every_value_above_the_dense_tier(native_lib, tmp_path):
    from meryl_amd import analyze
    k = 21
    rng = np.random.default_rng(9)
    lo, hi = random_kmers(rng, 300000, k)
    # few distinct values and many: rows with large counts and rows of one k-mer
    values = np.where(rng.random(lo.size) < 0.5, analyze.DENSE_VALUES + rng.integers(0, 4, lo.size),
                      rng.integers(analyze.DENSE_VALUES, 2 ** 32, lo.size)).astype(np.uint32)
    path = tmp_path / "db.meryl"
    write_db(path, lo, hi, values, k)
    rlo, rhi, rv = read_db(path)
    assert int(rv.min()) >= analyze.DENSE_VALUES
    for t in (GC, GA, GT):
        a = analyze_db(path, k, t)
        assert_report(a, model_rows(rlo, rhi, rv, k, t), t, "all above")
        assert a.info()["n_overflow_kmers"] == lo.size
        a.close()


def test_one_kmer(native_lib, tmp_path):
    k = 21
    x = pack("GAGAGAGAGACTCTCTCTCTG")
    lo, hi = np.array([x], dtype=np.uint64), np.zeros(1, dtype=np.uint64)
    for value in (7, 1000):
        path = tmp_path / ("db%d.meryl" % value)
        write_db(path, lo, hi, [value], k)
        for t in (GC, GA, GT):
            f, r = py_scores(x, k, t)
            a = analyze_db(path, k, t)
            for which, score in ((FORWARD, f), (REVERSE, r)) + (((COMBINED, max(f, r)),) if t != GC else ()):
                s, v, o = a.result(which)
                assert (s.tolist(), v.tolist(), o.tolist()) == ([score], [value], [1]), (t, which)
            a.close()
    assert py_scores(x, k, GA) == (10, 10) and py_scores(x, k, GC) == (11, 10)


def test_empty_database(native_lib, tmp_path):
    k = 21
    path = tmp_path / "empty.meryl"
    z = np.zeros(0, dtype=np.uint64)
    write_db(path, z, z, np.zeros(0, dtype=np.uint32), k)
    for t in (GC, GA, GT):
        a = analyze_db(path, k, t)
        for _, which in NAMES[t]:
            s, v, o = a.result(which)
            assert s.size == 0 and v.size == 0 and o.size == 0
        files = a.write(tmp_path / ("e%d" % t))
        assert len(files) == len(NAMES[t])
        for f in files:
            assert os.path.isfile(f) and os.path.getsize(f) == 0
        assert a.info()["n_kmers"] == 0 and a.info()["n_files"] == 64
        a.close()


def test_labelled_database_gives_the_same_histograms(native_lib, tmp_path):
    k = 21
    rng = np.random.default_rng(77)
    lo, hi = random_kmers(rng, 50000, k)
    values = rng.integers(0, 300, lo.size).astype(np.uint32)
    write_db(tmp_path / "plain.meryl", lo, hi, values, k)
    write_db(tmp_path / "labelled.meryl", lo, hi, values, k, label_size=8, label=0xA5)
    for t in (GC, GA, GT):
        model = model_rows(lo, hi, values, k, t)
        for name in ("plain.meryl", "labelled.meryl"):
            a = analyze_db(tmp_path / name, k, t)
            assert_report(a, model, t, name)
            a.close()


# ---- large ---------------------------------------------------------------------------------------------------------------
def test_large_database_exercises_both_tiers(native_lib, tmp_path):
    from meryl_amd import analyze
    k = 21
    rng = np.random.default_rng(2024)
    lo = np.unique(rng.integers(0, 1 << 42, 21_500_000, dtype=np.uint64))
    hi = np.zeros(lo.size, dtype=np.uint64)
    n = lo.size
    assert n >= 20_000_000
    # a 30x count: a peak near 30, 10 % ones, about 1 % of repeats above the dense tier reaching 10^6
    u = rng.random(n)
    values = rng.poisson(30, n).astype(np.uint32)
    values[u < 0.10] = 1
    tail = u > 0.99
    values[tail] = np.floor(10 ** rng.uniform(2.0, 6.0, int(tail.sum()))).astype(np.uint32)
    # the input meets its conditions before the device is asked anything
    above = float((values >= analyze.DENSE_VALUES).mean())
    assert analyze.DENSE_VALUES <= 100 and 0.005 < above < 0.05, above
    assert 0.09 < float((values == 1).mean()) < 0.11
    peak = 2 + int(np.bincount(values[values < 96], minlength=96)[2:].argmax())      # (the ones aside: they are a spike of their own)
    assert 25 <= peak <= 35, peak
    assert int(values.max()) > 900_000
    # (written by the device encoder -- the host writer takes a second per million k-mers; read back by the host reader)
    path = tmp_path / "large.meryl"
    from meryl_amd import count
    stream = count.DbStream(str(path), k, W_PREFIX)
    stream.write(to_device(lo, hi, k), values_to_device(values), 0, 1 << W_PREFIX)
    stream.close()
    rlo, rhi, rv = read_db(path)
    assert np.array_equal(rlo, lo) and np.array_equal(rv, values)
    for t in (GC, GA, GT):
        model = model_rows(rlo, rhi, rv, k, t)
        a = analyze_db(path, k, t)
        info = a.info()
        share = info["n_overflow_kmers"] / info["n_kmers"]
        print("type %d: %d k-mers, %.3f %% through the overflow list, %d list retries, decode %.1f ms, histogram %.1f ms, "
              "overflow sort %.1f ms, read %.2f s, total %.2f s" % (t, info["n_kmers"], 100 * share, info["n_overflow_retries"],
                                                                    info["decode_ms"], info["hist_ms"], info["overflow_ms"],
                                                                    info["read_s"], info["total_s"]))
        assert info["n_kmers"] == n
        assert 0 < share < 0.05, share
        assert info["n_overflow_kmers"] == int((rv >= analyze.DENSE_VALUES).sum())
        assert_report(a, model, t, "large")
        a.close()


# ---- two ways in ---------------------------------------------------------------------------------------------------------
def test_count_result_and_its_database_agree(native_lib, tmp_path):
    import torch
    from meryl_amd import analyze, capi, count
    k = 21
    torch.cuda.set_device(0)
    bases = count.dev_synth_reads(11, 1_500_000, 0, 300_000, 150)          # 45 Mbp, ~30x
    cfg = capi.configure(k, int(bases.numel()), 4 << 30)
    path = str(tmp_path / "count.meryl")
    with count.Session(cfg, 0) as s:
        s.push_bases_device(bases)
        s.count()
        keys, cnts = s.result_device()
        s.write_database(path, 4)
    n = int(keys.shape[0])
    assert n > 1_000_000
    rlo, rhi, rv = read_db(path)
    assert rlo.size == n
    for t in (GC, GA, GT):
        model = model_rows(rlo, rhi, rv, k, t)
        with analyze.Analyzer(k, t) as one, analyze.Analyzer(k, t) as three, analyze.Analyzer(k, t) as dbase:
            one.add_device(keys, cnts)
            c1, c2 = n // 3, n // 3 + n // 5
            for piece in (slice(0, c1), slice(c1, c2), slice(c2, n)):
                three.add_device(keys[piece].contiguous(), cnts[piece].contiguous())
            dbase.add_database(path)
            for a, what in ((one, "one call"), (three, "three pieces"), (dbase, "database")):
                assert_report(a, model, t, what)
                assert a.info()["n_kmers"] == n


# ---- the binary ----------------------------------------------------------------------------------------------------------
def test_cli_writes_the_model_text(native_lib, tmp_path):
    from meryl_amd import build
    cli = build.build_analyze_cli()
    k = 21
    rng = np.random.default_rng(31)
    lo, hi = random_kmers(rng, 200000, k)
    values = np.where(rng.random(lo.size) < 0.97, rng.poisson(30, lo.size), rng.integers(0, 2 ** 32, lo.size)).astype(np.uint32)
    path = tmp_path / "db.meryl"
    write_db(path, lo, hi, values, k)
    rlo, rhi, rv = read_db(path)
    for t, flag in ((GC, "-gc"), (GA, "-ga"), (GT, "-gt")):
        model = model_rows(rlo, rhi, rv, k, t)
        prefix = tmp_path / ("out" + flag)
        p = subprocess.run([cli, "-mers", str(path), "-prefix", str(prefix), flag], capture_output=True, timeout=300)
        err = p.stderr.decode()
        assert p.returncode == 0, err
        assert p.stdout == b""
        lines = [ln for ln in err.split("\n") if ln]
        assert lines == ["Open meryl database '%s'." % path, "Processed %d kmers in total." % lo.size, "Output histogram",
                         "Clean up..", "Bye!"], err
        made = sorted(os.path.basename(f) for f in os.listdir(tmp_path) if f.startswith("out" + flag))
        assert made == sorted("out%s.%s.hist" % (flag, name) for name, _ in NAMES[t])
        for name, which in NAMES[t]:
            got = open("%s.%s.hist" % (prefix, name), "rb").read()
            assert got == rows_text(model[which]), (flag, name)
