"""meryl-import on the device: text `kmer value` -> database.

Expected results come from a model inside this file -- a line parser in plain Python for the small inputs, numpy (pack,
reverse complement, np.unique + np.add.at in uint32) for the large ones -- and, for the bytes, from the HOST writer
meryl_amd.db.Writer(path, k, 10) fed that model's blocks (the device encoder is held to that writer by test_db_device.py)."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from import_helpers import assert_same_dirs, codes_to_keys, pick, prefixes, rand_kmer, read_db, with_batch

pytestmark = pytest.mark.gpu

W_PREFIX = 10
MODE_NAMES = ("canonical", "forward", "reverse")
LETTERS = np.frombuffer(b"ACTG", dtype=np.uint8)          # code -> letter


# ---- the model -------------------------------------------------------------------------------------------------------
def model_records(text, k, mode):
    """[(k-mer, value)] in input order: meryl-import.C:175-219 restated"""
    persistent = 1
    out = []
    for line in text.split("\n"):
        words = line.replace("\r", " ").replace("\t", " ").split(" ")
        words = [w for w in words if w]
        if not words:
            continue
        if words[0][0] == "#":
            persistent = int(words[0][1:])
            continue
        out.append((pick(words[0], k, mode), int(words[1]) if len(words) > 1 else persistent))
    return out


def model_sums(records):
    """-> lo, hi, values (uint64, uint64, uint32), k-mers ascending, values summed mod 2^32"""
    acc = {}
    for key, v in records:
        acc[key] = (acc.get(key, 0) + v) & 0xFFFFFFFF
    keys = sorted(acc)
    lo = np.array([x & 0xFFFFFFFFFFFFFFFF for x in keys], dtype=np.uint64)
    hi = np.array([x >> 64 for x in keys], dtype=np.uint64)
    return lo, hi, np.array([acc[x] for x in keys], dtype=np.uint32)


def host_write(path, lo, hi, cn, k):
    from meryl_amd import db
    w_data = 2 * k - W_PREFIX
    starts = np.searchsorted(prefixes(lo, hi, k, W_PREFIX), np.arange(0, (1 << W_PREFIX) + 1, dtype=np.uint64))
    mlo = np.uint64((1 << w_data) - 1) if w_data < 64 else np.uint64(0xFFFFFFFFFFFFFFFF)
    mhi = np.uint64((1 << (w_data - 64)) - 1) if w_data > 64 else np.uint64(0)
    w = db.Writer(path, k, W_PREFIX)
    for p in range(1 << W_PREFIX):
        s, e = int(starts[p]), int(starts[p + 1])
        w.add_block(p, lo[s:e] & mlo, cn[s:e], (hi[s:e] & mhi) if w_data > 64 else None)
    w.close()


def assert_db_equals(path, lo, hi, cn, k):
    glo, ghi, gcn, hv, ho = read_db(path)
    assert glo.size == lo.size, (glo.size, lo.size)
    assert np.array_equal(glo, lo) and np.array_equal(gcn, cn)
    if k > 32:
        assert np.array_equal(ghi, hi)
    wv, wo = np.unique(cn, return_counts=True)
    assert np.array_equal(hv, wv.astype(np.uint64)) and np.array_equal(ho, wo.astype(np.uint64))


# ---- inputs ----------------------------------------------------------------------------------------------------------
def messy_text(rng, k, n_records=1200, pool=350, hash_until=1.0):
    """Shuffled records over a small pool (well above 30 % repeats), `#` lines (only in the first `hash_until` of the lines),
    records without a value before and after the first `#`, blank lines, CRLF, tabs and runs of spaces, lower case, words
    longer than k, a third word, values of 0 (explicit, and through `#0`), a k-mer whose only value is 0, no final newline."""
    kmers = [rand_kmer(rng, k) for _ in range(pool)]
    taken = {pick(w, k, 0) for w in kmers}
    zero_only = rand_kmer(rng, k)
    while pick(zero_only, k, 0) in taken:
        zero_only = rand_kmer(rng, k)
    lines = []
    for i in range(n_records):
        w = kmers[int(rng.integers(0, pool))]
        u = rng.random()
        if u < 0.15:
            w = w.lower()
        elif u < 0.25:
            w = "".join(c.lower() if rng.random() < 0.5 else c for c in w)
        if rng.random() < 0.2:
            w = rand_kmer(rng, int(rng.integers(1, 40))) + w               # a longer word: its last k bases count
        sep = [" ", "\t", "   ", " \t ", "\t\t"][int(rng.integers(0, 5))]
        lead = ["", "", "", " ", "\t"][int(rng.integers(0, 5))]
        u = rng.random()
        if u < 0.35:
            line = lead + w                                               # no value: the persistent one
            if rng.random() < 0.3:
                line += sep.replace("\t", " ")                           # trailing blanks, still no second word
        else:
            v = 0 if u < 0.42 else int(rng.integers(1, 2000)) if u < 0.95 else int(rng.integers(2 ** 31, 2 ** 32))
            line = lead + w + sep + ("%d" % v if rng.random() < 0.9 else "%05d" % (v % 100000))
            if rng.random() < 0.25:
                line += sep + ["junk", "42", "#9", "ACGT"][int(rng.integers(0, 4))]   # a third word (meryl print of a labelled database)
        lines.append(line)
    lines.append(zero_only + "\t0")
    lines.append(zero_only.lower() + " 0 x")
    order = rng.permutation(len(lines))
    lines = [lines[i] for i in order]
    n_hash_zone = max(8, int(len(lines) * hash_until))
    # the first `#` comes after some value-less records; later ones anywhere inside the zone
    first_hash = int(n_hash_zone * 0.15)
    at = sorted(set([first_hash] + [int(x) for x in rng.integers(first_hash, n_hash_zone, 6)]), reverse=True)
    hashes = ["#7", "#0", " #12 ", "#4294967295", "#3\tignored", "#0005", "\t#21"]
    for j, pos in enumerate(at):
        lines.insert(pos, hashes[j % len(hashes)])
    for pos in sorted((int(x) for x in rng.integers(0, len(lines), 25)), reverse=True):
        lines.insert(pos, ["", "   ", "\t", " \t "][int(rng.integers(0, 4))])
    # CRLF on a third of the lines; nothing after the last line
    out = []
    for i, ln in enumerate(lines):
        out.append(ln + ("\r" if rng.random() < 0.33 else ""))
    text = "\n".join(out)
    assert not text.endswith("\n")
    return text


def fixed_width_text(codes, values, digits):
    """`KMER<TAB>value<LF>` rows of one width, as a uint8 matrix (vectorised)"""
    n, k = codes.shape
    m = np.empty((n, k + 1 + digits + 1), np.uint8)
    m[:, :k] = LETTERS[codes]
    m[:, k] = 9
    v = values.astype(np.uint64)
    for d in range(digits):
        m[:, k + digits - d] = (48 + (v % np.uint64(10))).astype(np.uint8)
        v = v // np.uint64(10)
    m[:, -1] = 10
    return m


def model_from_arrays(lo, hi, values, idx=None):
    """np.unique + np.add.at in uint32 -> lo, hi, sums with the k-mers ascending (idx: record i holds k-mer idx[i] of lo / hi)"""
    if hi.any():
        both = np.stack([hi, lo], axis=1)
        u, inv = np.unique(both, axis=0, return_inverse=True)
        ulo, uhi = u[:, 1].copy(), u[:, 0].copy()
    else:
        ulo, inv = np.unique(lo, return_inverse=True)
        uhi = np.zeros(ulo.size, np.uint64)
    sums = np.zeros(ulo.size, np.uint32)
    inv = inv.reshape(-1) if idx is None else inv.reshape(-1)[idx]
    np.add.at(sums, inv, values.astype(np.uint32))
    seen = np.bincount(inv, minlength=ulo.size) > 0                 # (a pool k-mer that no record drew is not in the input)
    return ulo[seen], uhi[seen], sums[seen]


def long_segment_input(rng, k=21):
    """one k-mer on 2 000 000 lines with value 3000 among 1 000 000 others: 6 * 10^9 wraps"""
    others = rng.integers(0, 4, (1_000_000, k)).astype(np.uint8)
    hot = rng.integers(0, 4, (1, k)).astype(np.uint8)
    codes = np.concatenate([np.repeat(hot, 2_000_000, axis=0), others])
    values = np.concatenate([np.full(2_000_000, 3000, np.uint64), rng.integers(1000, 10000, 1_000_000).astype(np.uint64)])
    order = rng.permutation(codes.shape[0])
    codes, values = codes[order], values[order]
    lo, hi = codes_to_keys(codes, 0)
    hlo, hhi = codes_to_keys(hot, 0)
    return fixed_width_text(codes, values, 4), (lo, hi, values), (int(hlo[0]), int(hhi[0]))


@pytest.fixture(scope="module")
def clis(native_lib):
    from meryl_amd import build
    return build.build_cli(), build.build_import_cli()


# ---- 1. round trip -----------------------------------------------------------------------------------------------------
def test_round_trip_count_print_import(clis, tmp_path):
    meryl, importer = clis
    rng = np.random.default_rng(21)
    genome = rng.integers(0, 4, 60_000)
    with open(tmp_path / "reads.fa", "w") as f:
        for i in range(3000):
            s = int(rng.integers(0, genome.size - 150))
            f.write(">r%d\n%s\n" % (i, "".join("ACGT"[c] for c in genome[s:s + 150])))
    a = str(tmp_path / "a.meryl")
    subprocess.run([meryl, "-Q", "k=21", "memory=1", "count", str(tmp_path / "reads.fa"), "output", a], check=True, timeout=600)
    text = subprocess.run([meryl, "-Q", "print", a], check=True, stdout=subprocess.PIPE, timeout=600).stdout
    assert text.count(b"\n") > 50_000
    (tmp_path / "a.txt").write_bytes(text)
    with gzip.open(tmp_path / "a.txt.gz", "wb") as f:
        f.write(text)
    want = read_db(a)
    assert want[2].max() > 1
    for name, src, stdin in (("file", str(tmp_path / "a.txt"), None), ("stdin", "-", text), ("gz", str(tmp_path / "a.txt.gz"), None)):
        out = str(tmp_path / ("b_%s.meryl" % name))
        p = subprocess.run([importer, "-k", "21", "-kmers", src, "-output", out], input=stdin, capture_output=True, timeout=600)
        assert p.returncode == 0, p.stderr.decode()
        err = p.stderr.decode()
        assert ("Found %d kmers in the input." % want[0].size) in err and err.rstrip().endswith("Bye."), err
        got = read_db(out)
        for g, w in zip(got, want):
            assert np.array_equal(g, w), name
        assert len(os.listdir(out)) == 129


# ---- 2. bytes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1, 2], ids=MODE_NAMES)
@pytest.mark.parametrize("k", [6, 16, 21, 31, 32, 33, 51, 64])
def test_bytes_equal_the_host_writers(native_lib, tmp_path, k, mode):
    from meryl_amd import kmer_import
    rng = np.random.default_rng(1000 * k + mode)
    text = messy_text(rng, k)
    recs = model_records(text, k, mode)
    lo, hi, cn = model_sums(recs)
    assert len(recs) >= 1.3 * lo.size and (cn == 0).any()
    host_write(str(tmp_path / "host"), lo, hi, cn, k)
    info = kmer_import.import_text(text, k, str(tmp_path / "dev"), mode=mode, host_threads=4)
    assert info["n_records"] == len(recs) and info["n_distinct"] == lo.size and info["n_batches"] == 1
    assert info["n_lines"] == text.count("\n") + 1
    assert_same_dirs(str(tmp_path / "host"), str(tmp_path / "dev"))
    assert_db_equals(str(tmp_path / "dev"), lo, hi, cn, k)


def test_parser_alone_in_chunks(native_lib):
    """the persistent value and the record slots across chunk boundaries, records in input order"""
    import torch
    from meryl_amd import kmer_import
    for k, mode in ((21, 0), (51, 2), (33, 1)):
        rng = np.random.default_rng(77 + k)
        text = messy_text(rng, k, n_records=3000)
        recs = model_records(text, k, mode)
        raw = text.encode()
        cuts = [0]
        for frac in (0.2, 0.21, 0.6):
            cuts.append(raw.index(b"\n", int(len(raw) * frac)) + 1)
        cuts.append(len(raw))
        parser = kmer_import.Parser(k, mode)
        got, lines = [], 0
        for a, b in zip(cuts[:-1], cuts[1:]):
            keys, vals, res = parser.parse(torch.frombuffer(bytearray(raw[a:b]), dtype=torch.uint8).cuda())
            assert res.bad_kind == 0
            lines += res.n_lines
            kk = keys.cpu().numpy().view(np.uint64)
            vv = vals.cpu().numpy().view(np.uint32)
            for i in range(kk.shape[0]):
                key = int(kk[i]) if k <= 32 else int(kk[i, 0]) | (int(kk[i, 1]) << 64)
                got.append((key, int(vv[i])))
        assert lines == text.count("\n") + 1
        assert got == recs


def test_empty_input_gives_an_empty_database(native_lib, tmp_path):
    from meryl_amd import kmer_import
    for i, text in enumerate(("", "\n\n  \n", "#5\n")):
        out = str(tmp_path / ("e%d.meryl" % i))
        info = kmer_import.import_text(text, 21, out)
        assert info["n_records"] == 0 and info["n_distinct"] == 0
        lo, hi, cn, hv, ho = read_db(out)
        assert lo.size == 0 and len(os.listdir(out)) == 129
        host_write(str(tmp_path / ("h%d" % i)), np.zeros(0, np.uint64), np.zeros(0, np.uint64), np.zeros(0, np.uint32), 21)
        assert_same_dirs(str(tmp_path / ("h%d" % i)), out)


# ---- 3. long segment and wrap ------------------------------------------------------------------------------------------
def test_long_segment_wraps_across_workgroups(native_lib, tmp_path):
    from meryl_amd import kmer_import
    rng = np.random.default_rng(3)
    m, (lo, hi, values), hot = long_segment_input(rng)
    ulo, uhi, sums = model_from_arrays(lo, hi, values)
    at = int(np.searchsorted(ulo, np.uint64(hot[0])))
    assert int(sums[at]) == (2_000_000 * 3000) % (1 << 32) == 1705032704
    info = kmer_import.import_text(m.reshape(-1), 21, str(tmp_path / "dev"))
    assert info["n_records"] == 3_000_000 and info["n_lines"] == 3_000_000
    assert_db_equals(str(tmp_path / "dev"), ulo, uhi, sums, 21)


# ---- 4. batches ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,mode", [(21, 0), (51, 0), (33, 2), (6, 1)])
def test_batches_small_input(native_lib, tmp_path, k, mode):
    """a `#` line in batch 1 governs the value-less records of batch 4 and later"""
    from meryl_amd import kmer_import
    rng = np.random.default_rng(40 + k)
    text = messy_text(rng, k, n_records=2500, hash_until=0.1)
    raw = text.encode()
    batch = len(raw) // 7
    last_hash, at = 0, 0
    for ln in raw.split(b"\n"):
        if ln.strip(b" \t\r").startswith(b"#"):
            last_hash = at
        at += len(ln) + 1
    assert last_hash < batch - 200, "every `#` line lies in the first batch"
    tail_lines = raw[3 * batch:].split(b"\n")[1:]
    assert sum(1 for ln in tail_lines if len(ln.split()) == 1) > 50, "value-less records in batch 4 and beyond"
    one = kmer_import.import_text(text, k, str(tmp_path / "one"), mode=mode)
    assert one["n_batches"] == 1
    with with_batch(batch):
        many = kmer_import.import_text(text, k, str(tmp_path / "many"), mode=mode)
    assert many["n_batches"] >= 5, many
    assert many["n_records"] == one["n_records"] and many["n_lines"] == one["n_lines"] and many["n_distinct"] == one["n_distinct"]
    assert_same_dirs(str(tmp_path / "one"), str(tmp_path / "many"))
    lo, hi, cn = model_sums(model_records(text, k, mode))
    assert_db_equals(str(tmp_path / "many"), lo, hi, cn, k)


def test_batches_long_segment(native_lib, tmp_path):
    from meryl_amd import kmer_import
    rng = np.random.default_rng(3)
    m, (lo, hi, values), _ = long_segment_input(rng)
    ulo, uhi, sums = model_from_arrays(lo, hi, values)
    flat = m.reshape(-1)
    one = kmer_import.import_text(flat, 21, str(tmp_path / "one"))
    with with_batch(flat.size // 6 + 1000):
        many = kmer_import.import_text(flat, 21, str(tmp_path / "many"))
    assert one["n_batches"] == 1 and many["n_batches"] >= 5
    assert_same_dirs(str(tmp_path / "one"), str(tmp_path / "many"))
    assert_db_equals(str(tmp_path / "many"), ulo, uhi, sums, 21)


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------
BAD_LINES = {
    "base": ("ACGTACGTACGTANGTACGTA 4", "not one of ACGTacgt"),
    "short": ("ACGTACGTACGTACGTACGT 4", "shorter than k"),
    "value": ("ACGTACGTACGTACGTACGTA 4294967296", "value is not a decimal number"),
    "hash": ("#x", "after '#'"),
}


@pytest.mark.parametrize("where", ["beyond_first_tile", "beyond_first_batch"])
@pytest.mark.parametrize("kind", sorted(BAD_LINES))
def test_refusals_name_the_line(clis, tmp_path, kind, where):
    _, importer = clis
    rng = np.random.default_rng(len(kind))
    good = ["%s %d" % (rand_kmer(rng, 21), int(rng.integers(1, 100))) for _ in range(3000)]
    good[5] = ""                                                    # blank and `#` lines count as lines
    good[9] = "#3"
    bad_at = 400 if where == "beyond_first_tile" else 2500          # 0-based index = lines before it
    lines = good[:bad_at] + [BAD_LINES[kind][0]] + good[bad_at:]
    # a second, later bad line of another kind must not be the one reported
    lines.insert(bad_at + 300, "ACGTACGTACGTACGTACGTA notanumber")
    raw = ("\n".join(lines) + "\n").encode()
    offset = len(("\n".join(lines[:bad_at]) + "\n").encode())
    env = dict(os.environ)
    if where == "beyond_first_tile":
        assert offset > 4096
        env.pop("MGC_IMPORT_BATCH", None)
    else:
        env["MGC_IMPORT_BATCH"] = "8192"
        assert offset > 3 * 8192
    (tmp_path / "in.txt").write_bytes(raw)
    out = tmp_path / "out.meryl"
    p = subprocess.run([importer, "-k", "21", "-kmers", str(tmp_path / "in.txt"), "-output", str(out)], capture_output=True, env=env,
                       timeout=600)
    err = p.stderr.decode()
    assert p.returncode == 1, (p.returncode, err)
    assert ("line %d:" % (bad_at + 1)) in err and BAD_LINES[kind][1] in err, err
    assert "Found" not in err
    assert not os.path.exists(out / "merylIndex")


def test_refusal_through_the_binding(native_lib, tmp_path):
    from meryl_amd import kmer_import
    text = "ACGTACGTACGTACGTACGTA 1\n" * 10 + "ACGTACGTACGTACGTACGTA 1x\n" + "ACGTACGTACGTACGTACGT\n"
    with pytest.raises(kmer_import.ImportRefused) as e:
        kmer_import.import_text(text, 21, str(tmp_path / "o.meryl"))
    assert e.value.line == 11 and e.value.kind == "value"
    assert not os.path.exists(tmp_path / "o.meryl" / "merylIndex")
    # the last line without '\n' is a line too
    with pytest.raises(kmer_import.ImportRefused) as e:
        kmer_import.import_text("ACGTACGTACGTACGTACGTA 1\nACGTACGTACGTACGTACGTA 1\nACGTAC", 21, str(tmp_path / "o2.meryl"))
    assert e.value.line == 3 and e.value.kind == "short"
    # values at the edge that are fine
    info = kmer_import.import_text("ACGTACGTACGTACGTACGTA 4294967295\nACGTACGTACGTACGTACGTA 0000000000000000000001\n", 21,
                                   str(tmp_path / "o3.meryl"))
    lo, hi, cn, _, _ = read_db(str(tmp_path / "o3.meryl"))
    assert info["n_distinct"] == 1 and int(cn[0]) == 0              # 4294967295 + 1 wraps


# ---- 6. the device steps alone ---------------------------------------------------------------------------------------------
def _pairs(rng, n, kw, pattern, bits):
    if pattern == "equal":
        lo = np.full(n, 0x123456789ABCDEF % (1 << min(bits, 64)), np.uint64)
        hi = np.full(n, 0x2A if kw == 2 else 0, np.uint64)
    else:
        distinct = max(1, n // 3)
        pool_lo = rng.integers(0, 1 << min(bits, 64), distinct, dtype=np.uint64, endpoint=False) if bits < 64 else \
            rng.integers(0, 1 << 64, distinct, dtype=np.uint64, endpoint=False)
        pool_hi = rng.integers(0, 1 << (bits - 64), distinct, dtype=np.uint64) if kw == 2 else np.zeros(distinct, np.uint64)
        idx = rng.integers(0, distinct, n)
        lo, hi = pool_lo[idx], pool_hi[idx]
        if pattern in ("ascending", "descending"):
            order = np.lexsort((lo, hi))
            if pattern == "descending":
                order = order[::-1]
            lo, hi = lo[order], hi[order]
    vals = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    return lo, hi, vals


@pytest.mark.parametrize("pattern", ["random", "equal", "ascending", "descending"])
@pytest.mark.parametrize("kw,bits", [(1, 42), (1, 64), (2, 102), (2, 128)])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4096, 4097, 3_000_000])
def test_sort_and_reduce_alone(native_lib, n, kw, bits, pattern):
    import torch
    from meryl_amd import kmer_import
    rng = np.random.default_rng(n * 7 + bits)
    lo, hi, vals = _pairs(rng, n, kw, pattern, bits)
    host_keys = lo if kw == 1 else np.stack([lo, hi], axis=1)
    dk = torch.from_numpy(np.ascontiguousarray(host_keys).view(np.int64)).cuda()
    dv = torch.from_numpy(vals.view(np.int32)).cuda()
    sk, sv = kmer_import.sort_pairs(dk, dv, 0, bits)
    order = np.lexsort((lo, hi))                                     # stable: equal keys keep their input order
    got_k = sk.cpu().numpy().view(np.uint64)
    got_v = sv.cpu().numpy().view(np.uint32)
    assert np.array_equal(got_k, host_keys[order]) and np.array_equal(got_v, vals[order])
    rk, rv = kmer_import.reduce_pairs(sk, sv)
    slo, shi, svals = lo[order], hi[order], vals[order]
    if n:
        head = np.ones(n, bool)
        head[1:] = (slo[1:] != slo[:-1]) | (shi[1:] != shi[:-1])
        starts = np.flatnonzero(head)
        want_v = np.add.reduceat(svals, starts, dtype=np.uint32)
        want_k = host_keys[order][starts]
    else:
        want_v, want_k = np.zeros(0, np.uint32), host_keys
    assert rk.shape[0] == want_k.shape[0]
    assert np.array_equal(rk.cpu().numpy().view(np.uint64), want_k) and np.array_equal(rv.cpu().numpy().view(np.uint32), want_v)


# ---- 7. size ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [21, 51])
def test_ten_million_lines(native_lib, tmp_path, k):
    from meryl_amd import kmer_import
    rng = np.random.default_rng(k)
    n, pool = 10_500_000, 3_000_000
    pool_codes = rng.integers(0, 4, (pool, k)).astype(np.uint8)
    idx = rng.integers(0, pool, n)
    values = rng.integers(0, 100000, n).astype(np.uint64)
    plo, phi = codes_to_keys(pool_codes, 0)
    text = fixed_width_text(pool_codes[idx], values, 5).reshape(-1)
    ulo, uhi, sums = model_from_arrays(plo, phi, values, idx)
    info = kmer_import.import_text(text, k, str(tmp_path / "dev"))
    assert info["n_lines"] == n and info["n_records"] == n and info["n_distinct"] == ulo.size
    assert_db_equals(str(tmp_path / "dev"), ulo, uhi, sums, k)
