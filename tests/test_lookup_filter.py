"""meryl-lookup -include / -exclude (src/meryl-lookup/include-exclude.C) through the C ABI (mgc_lookup_filter_text /
mgc_lookup_filter_files), the Python API and the CLI, against a restatement of include-exclude.C in this file: its own
record reader (the four assumptions of INTEGRATION.md about dnaSeq / outputFASTA / outputFASTQ), rolling k-mers per
sequence (kmerIterator), a dictionary for the table, and the reference's keep rule and header."""
import gzip
import hashlib
import os
import subprocess

import numpy as np
import pytest

CODE = dict(zip(b"ACTGactg", (0, 1, 2, 3, 0, 1, 2, 3)))
M32 = 0xFFFFFFFF


# ---- restatement of src/meryl-lookup/include-exclude.C ---------------------------------------------------------------
def windows(seq, k):
    """kmerIterator: (bgnPosition, fmer, rmer) of every k consecutive ACGT bases (either case), positions from 0"""
    mask = (1 << (2 * k)) - 1
    f = r = load = 0
    for j, ch in enumerate(seq):
        c = CODE.get(ch)
        if c is None:
            f = r = load = 0
            continue
        f = ((f << 2) | c) & mask
        r = (r >> 2) | ((c ^ 2) << (2 * k - 2))
        load += 1
        if load >= k:
            yield j + 1 - k, f, r


def read_records(text):
    """dnaSeqFile::loadSequence as this repository assumes it: (ident, bases, quals) per record.  ident: the header up to the
    first blank or tab; bases: the sequence lines joined with \\r \\n blank tab dropped; FASTQ: four lines per record."""
    lines = text.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    lines = [l[:-1] if l.endswith(b"\r") else l for l in lines]
    recs = []
    if not lines:
        return recs
    ident = lambda h: h[1:].replace(b"\t", b" ").split(b" ")[0]
    if lines[0][:1] == b">":
        for l in lines:
            if l[:1] == b">":
                recs.append([ident(l), b"", b""])
            else:
                recs[-1][1] += l.replace(b" ", b"").replace(b"\t", b"").replace(b"\r", b"")
    else:
        assert len(lines) % 4 == 0
        for i in range(0, len(lines), 4):
            assert lines[i][:1] == b"@" and lines[i + 2][:1] == b"+"
            recs.append([ident(lines[i]), lines[i + 1], lines[i + 3]])
    return [tuple(r) for r in recs]


_found_cache = {}


def n_found(bases, k, table, tid, skip):
    """processSequence (:64-78): windows with value(fmer) > 0 || value(rmer) > 0, those beginning before `skip` left out"""
    key = (bases, k, tid, skip)
    if key not in _found_cache:
        _found_cache[key] = sum(1 for p, f, r in windows(bases, k) if p >= skip and (f in table or r in table))
    return _found_cache[key]


def output_sequence(rec, nf):
    """:100-109 with outputFASTA / outputFASTQ: FASTA when the record has no qualities"""
    ident, bases, quals = rec
    if not quals:
        return b">" + ident + b" nKmers=%d\n" % nf + bases + b"\n"
    return b"@" + ident + b" nKmers=%d\n" % nf + bases + b"\n+\n" + quals + b"\n"


def restated_filter(texts, k, table, tid, include, skip_first):
    """filter() (:44-133): (output bytes per input, records (pairs), kept)"""
    recs = [read_records(t) for t in texts]
    assert len(set(map(len, recs))) == 1
    outs = [bytearray() for _ in texts]
    kept = 0
    for i in range(len(recs[0])):
        nf = n_found(recs[0][i][1], k, table, tid, skip_first)              # :92
        if len(recs) > 1:
            nf += n_found(recs[1][i][1], k, table, tid, 0)                   # :93
        if (nf > 0) == include:                                              # :124-125
            kept += 1
            for o, r in zip(outs, recs):
                o += output_sequence(r[i], nf)
    return [bytes(o) for o in outs], len(recs[0]), kept


def output_idents(out):
    """identifiers of the records of an output: FASTA records (two lines) and FASTQ records (four) may alternate in it"""
    lines, ids, i = out.split(b"\n"), [], 0
    while i < len(lines) - 1:
        ids.append(lines[i][1:].split(b" ")[0])
        i += 2 if lines[i][:1] == b">" else 4
    return ids


# ---- inputs ----------------------------------------------------------------------------------------------------------
def table_dict(hi, lo, cn, vmin=0, vmax=M32):
    return {(int(h) << 64) | int(l): int(c) for h, l, c in zip(hi, lo, cn) if vmin <= int(c) <= vmax}


def make_tables(oracle_lib, seed, k):
    """[(Lookup, dict, id)]: the table counted in process from reads of one genome, and the same with -min 2 -max 5"""
    import torch
    from meryl_amd import capi, count, lookup
    reads = oracle_lib.synth_reads(seed, 40_000, 0, 2000, 150, 5000, 2000)
    cfg = capi.configure(k, reads.size, 1 << 30)
    with count.Session(cfg, 0) as s:
        s.push_bases_device(torch.from_numpy(reads).cuda())
        s.count()
        keys, cnts = s.result_device()
        full = lookup.Lookup.from_device(keys, cnts, k)
        filt = lookup.Lookup.from_device(keys, cnts, k, 2, 5)
    hi, lo, cn, _ = oracle_lib.count_brute(reads.tobytes(), k)
    return [(full, table_dict(hi, lo, cn), (seed, k, 0)), (filt, table_dict(hi, lo, cn, 2, 5), (seed, k, 1))]


def split_reads(arr):
    return [r for r in arr.tobytes().split(b".") if r]


def records_for(oracle_lib, seed, k, table, must=None):
    """(first input, second input) as lists of (header, bases): half reads of the table's genome, half of a foreign one, and
    the hand-made records of the issue.  The -10x reads hold exactly one k-mer of `table`, and that one is in `must` too."""
    must = table if must is None else must
    rng = np.random.default_rng(seed)
    own = split_reads(oracle_lib.synth_reads(seed, 40_000, 2000, 120, 150, 5000, 2000))
    foreign = split_reads(oracle_lib.synth_reads(seed + 7919, 40_000, 0, 260, 150, 5000, 2000))
    rand = lambda n: bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), n))
    # a k-mer of the table whose read prefix of 22 / 23 random bases adds no other table k-mer
    def tenx(prefix_len):
        for read in own:
            for p, f, r in windows(read, k):
                if f in must or r in must:
                    cand = rand(prefix_len) + read[p:p + k]
                    hits = [q for q, f2, r2 in windows(cand, k) if f2 in table or r2 in table]
                    if hits == [prefix_len]:
                        return cand
        raise AssertionError("no -10x read could be built")
    long_rec = rand(60_000) + own[3] + rand(50_000)                          # >= 100 kbp, found through the read inside it
    a = [(b"own%d" % i, r) for i, r in enumerate(own[:100])] + [(b"for%d" % i, r) for i, r in enumerate(foreign[:110])]
    a += [(b"empty", b""), (b"short", own[101][:k - 1]), (b"lower", own[102].lower()), (b"withN", own[103][:70] + b"N" + own[103][70:]),
          (b"described some text\tand more", own[104]), (b"long", long_rec), (b"longforeign", rand(100_003)),
          (b"tenx22", tenx(22)), (b"tenx23", tenx(23)), (b"tenx22mate", tenx(22)), (b"last", foreign[111])]
    b = [(b"m%d/2" % i, foreign[120 + i % 130]) for i in range(len(a))]
    b[150] = (b"matedecides/2", own[105])                                    # a foreign first read kept through its mate
    b[[h for h, _ in a].index(b"tenx22mate")] = (b"tenxmate/2", own[106])    # -10x drops the first read's k-mer: the mate decides
    return a, b


def fmt_text(recs, how, seed=0):
    """single-line FASTA, FASTA wrapped at 60 (also \\r\\n), four-line FASTQ; the last record has no line end"""
    rng = np.random.default_rng(seed)
    out = []
    for h, s in recs:
        if how == "fq":
            q = bytes(rng.integers(33, 74, len(s), dtype=np.uint8))          # '@' and '+' may begin a quality line
            out.append(b"@" + h + b"\n" + s + b"\n+" + (h if len(out) % 2 else b"") + b"\n" + q + b"\n")
        elif how == "fa1":
            out.append(b">" + h + b"\n" + s + b"\n")
        else:
            eol = b"\r\n" if how == "fa60crlf" else b"\n"
            out.append(b">" + h + eol + b"".join(s[i:i + 60] + eol for i in range(0, len(s), 60)))
    text = b"".join(out)
    return text[:-2] if text.endswith(b"\r\n") else text[:-1]


def cuda_bytes(b):
    import torch
    return torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).cuda() if b else torch.empty(0, dtype=torch.uint8, device="cuda")


FORMATS = [("fa1",), ("fa60",), ("fa60crlf",), ("fq",), ("fa1", "fq"), ("fq", "fq"), ("fa60", "fa1")]


# ---- the grid --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("k", [21, 31, 51])
def test_filter_text_grid(native_lib, oracle_lib, k):
    from meryl_amd import lookup
    tables = make_tables(oracle_lib, 300 + k, k)
    a, b = records_for(oracle_lib, 300 + k, k, tables[0][1], tables[1][1])   # the -10x reads hold for the full table and the filtered one
    cases = 0
    for fmts in FORMATS:
        texts = [fmt_text(recs, how, i) for i, (recs, how) in enumerate(zip((a, b), fmts))]
        dev = [cuda_bytes(t) for t in texts]
        for lk, tab, tid in tables:
            for skip in (0, 23):
                want_inc = None
                for mode in ("include", "exclude"):
                    want, n, kept = restated_filter(texts, k, tab, tid, mode == "include", skip)
                    assert n / 4 <= kept <= 3 * n / 4, (k, fmts, tid, skip, mode, kept, n)   # neither output is trivial
                    got, res = lookup.filter_text(lk, mode, dev, skip_first=skip)
                    assert (res.n_records, res.n_kept) == (n, kept), (k, fmts, tid, skip, mode)
                    for i in range(len(texts)):
                        assert got[i] == want[i], (k, fmts, tid, skip, mode, i)
                        assert res.consumed[i] == len(texts[i]) and res.out_bytes[i] == len(want[i])
                    # -include and -exclude partition the input
                    if mode == "include":
                        want_inc = (got, res.n_kept)
                    else:
                        assert want_inc[1] + res.n_kept == n
                        for i in range(len(texts)):
                            assert sorted(output_idents(want_inc[0][i]) + output_idents(got[i])) == sorted(r[0] for r in read_records(texts[i]))
                    cases += 1
                # the -10x reads: the k-mer at base 22 is skipped, the one at base 23 is not; a mate decides
                ids = set(output_idents(lookup.filter_text(lk, "include", dev, skip_first=skip)[0][0]))
                assert b"tenx23" in ids and (b"tenx22" in ids) == (skip == 0)
                assert (b"tenx22mate" in ids) == (skip == 0 or len(texts) == 2)
                assert (a[150][0] in ids) == (len(texts) == 2)               # a foreign read: kept through its mate only
    assert cases == len(FORMATS) * 2 * 2 * 2
    for lk, _, _ in tables:
        lk.close()


# ---- cut invariance --------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_filter_files_cut_invariance(native_lib, oracle_lib, tmp_path):
    from meryl_amd import lookup
    k = 21
    (lk, tab, tid), (lk2, _, _) = make_tables(oracle_lib, 77, k)
    a, b = records_for(oracle_lib, 77, k, tab)
    for fmts in (("fq", "fq"), ("fa60", "fq"), ("fa60crlf",)):
        texts = [fmt_text(recs, how, i) for i, (recs, how) in enumerate(zip((a, b), fmts))]
        paths = []
        for i, t in enumerate(texts):
            paths.append(tmp_path / ("in%d.txt" % i))
            paths[-1].write_bytes(t)
        whole, wres = lookup.filter_text(lk, "include", [cuda_bytes(t) for t in texts], skip_first=23)
        assert whole == restated_filter(texts, k, tab, tid, True, 23)[0]
        for batch in (4096, 0):                                              # 4096: shorter than the long records, the piece grows
            pieces = []
            outs = [tmp_path / ("out%d.txt" % i) for i in range(len(texts))]
            res = lookup.filter_files(lk, "include", paths, outs, skip_first=23, batch_bytes=batch, pieces=pieces)
            assert (res.n_records, res.n_kept) == (wres.n_records, wres.n_kept)
            for i in range(len(texts)):
                assert outs[i].read_bytes() == whole[i], (fmts, batch, i)
                assert b"".join(p for j, p in pieces if j == i) == whole[i]  # the pieces arrive in order
                assert res.out_bytes[i] == len(whole[i]) and res.consumed[i] == len(texts[i])
            if batch:
                assert len(pieces) >= 2 * len(texts)                         # (a piece that grew for a long record stays large)
    lk.close()
    lk2.close()


# ---- errors ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_filter_errors(native_lib, oracle_lib):
    import torch
    from meryl_amd import capi, lookup
    k = 21
    (lk, tab, tid), (lk2, _, _) = make_tables(oracle_lib, 55, k)
    own = split_reads(oracle_lib.synth_reads(55, 40_000, 2000, 10, 150, 5000, 2000))
    recs = [(b"r%d" % i, r) for i, r in enumerate(own[:5])]
    fq = fmt_text(recs, "fq") + b"\n"
    want, n, kept = restated_filter([fq], k, tab, tid, True, 0)
    assert kept == n == 5
    # output capacity too small: nothing written, the sizes reported, a second call with them succeeds
    small = [torch.full((10,), 0xAA, dtype=torch.uint8, device="cuda")]
    with pytest.raises(capi.MgcError) as e:
        lookup.filter_text(lk, "include", [cuda_bytes(fq)], outs=small)
    assert e.value.rc == capi.MGC_EINVAL and e.value.result.out_bytes[0] == len(want[0])
    assert bool((small[0] == 0xAA).all())
    exact = [torch.empty(len(want[0]), dtype=torch.uint8, device="cuda")]
    got, _ = lookup.filter_text(lk, "include", [cuda_bytes(fq)], outs=exact)
    assert got[0] == want[0]
    # multi-line FASTQ, and a third line that does not start with '+'
    s = own[0]
    multi = b"@a\n" + s[:75] + b"\n" + s[75:] + b"\n+\n" + b"I" * 75 + b"\n" + b"I" * 75 + b"\n@b\n" + s + b"\n+\n" + b"I" * 150 + b"\n"
    noplus = b"@a\n" + s + b"\n-\n" + b"I" * 150 + b"\n"
    for bad in (multi, noplus):
        with pytest.raises(capi.MgcError) as e:
            lookup.filter_text(lk, "include", [cuda_bytes(bad)])
        assert e.value.rc == capi.EFORMAT, e.value
    with pytest.raises(capi.MgcError) as e:
        lookup.filter_text(lk, "include", [cuda_bytes(b"ACGT\n")])
    assert e.value.rc == capi.EFORMAT
    # 5 records against 4: the error names both counts
    four = fmt_text(recs[:4], "fa1") + b"\n"
    with pytest.raises(capi.MgcError) as e:
        lookup.filter_text(lk, "include", [cuda_bytes(fq), cuda_bytes(four)])
    assert e.value.rc == capi.MGC_EINVAL and "5 in the first" in str(e.value) and "4 in the second" in str(e.value)
    # not final: min(records) of each, the rest is left to the caller; a piece without a complete record is no fault
    got, res = lookup.filter_text(lk, "include", [cuda_bytes(fq), cuda_bytes(four)], final=False)
    assert res.n_records == 3 and res.consumed[0] == fq.index(b"@r3\n") and res.consumed[1] == four.index(b">r3\n")
    assert got == restated_filter([fq[:res.consumed[0]], four[:res.consumed[1]]], k, tab, tid, True, 0)[0]
    for piece in (b"@r1\nACGT", b">r1\nACGT\nAC", b">r1"):
        got, res = lookup.filter_text(lk, "exclude", [cuda_bytes(piece)], final=False)
        assert got == [b""] and res.n_records == 0 and res.consumed[0] == 0
    got, res = lookup.filter_text(lk, "exclude", [cuda_bytes(b"")])
    assert got == [b""] and res.n_records == 0
    lk.close()
    lk2.close()


# ---- CLI -------------------------------------------------------------------------------------------------------------
def run_lookup(args, env=None):
    from meryl_amd import build
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([build.build_lookup_cli()] + [str(a) for a in args], capture_output=True, env=e)


def test_cli_filter_option_checks(native_lib, tmp_path):
    """lookupGlobal::checkInvalid (meryl-lookup.C:328-367) for -include / -exclude, before a database or a device is touched"""
    q = tmp_path / "q.fa"
    q.write_text(">a\nACGT\n")
    db, o1, o2 = tmp_path / "missing.meryl", tmp_path / "o1.fa", tmp_path / "o2.fa"
    cases = [
        (["-include", "-sequence", q, "-mers", db], "No output file (-output) supplied."),
        (["-include", "-sequence", q, q, "-mers", db, "-output", o1], "No second output file (-output) supplied for second input (-input) file."),
        (["-exclude", "-sequence", q, "-mers", db, "-output", o1, o2], "No second input file (-input) supplied for second output (-output) file."),
        (["-include", "-sequence", q, "-mers", db, db, "-output", o1], "Only one meryl database (-mers) supported for -include."),
        (["-exclude", "-sequence", q, "-mers", db, db, "-output", o1], "Only one meryl database (-mers) supported for -exclude."),
        (["-include", "-10x", "-sequence", q, "-mers", db, "-labels", "A", "-output", o1], "Labels (-labels) not supported for -include."),
        (["-exclude", "-sequence", q, "-mers", db, "-labels", "A", "-output", o1], "Labels (-labels) not supported for -exclude."),
        (["-exclude", "-sequence", q, "-mers", db, "-output", tmp_path / "o.fq.gz"], "compressed"),
    ]
    for args, msg in cases:
        p = run_lookup(args)
        assert p.returncode == 1 and msg in p.stderr.decode(), (args, p.stderr)
        assert "not part of this build" not in p.stderr.decode()
    assert not o1.exists() and not o2.exists() and not (tmp_path / "o.fq.gz").exists()
    p = run_lookup(["-dump", "-sequence", q, "-mers", db])
    assert p.returncode == 1 and "not part of this build" in p.stderr.decode()


@pytest.mark.gpu
def test_cli_filter_end_to_end(native_lib, oracle_lib, tmp_path):
    from meryl_amd import build
    k = 21
    reads = split_reads(oracle_lib.synth_reads(91, 40_000, 0, 2000, 150, 5000, 2000))
    (tmp_path / "db.fa").write_bytes(b"".join(b">r%d\n%s\n" % (j, r) for j, r in enumerate(reads)))
    subprocess.run([build.build_cli(), "-Q", "k=%d" % k, "memory=1", "count", str(tmp_path / "db.fa"), "output", str(tmp_path / "db.meryl")], check=True)
    hi, lo, cn, _ = oracle_lib.count_brute(b".".join(reads) + b".", k)
    tab, tab3 = table_dict(hi, lo, cn), table_dict(hi, lo, cn, 3)
    a, b = records_for(oracle_lib, 91, k, tab, tab3)
    r1, r2 = fmt_text(a, "fq", 1) + b"\n", fmt_text(b, "fq", 2)
    (tmp_path / "R1.fq").write_bytes(r1)
    with gzip.open(tmp_path / "R2.fq.gz", "wb") as f:
        f.write(r2)
    o1, o2 = tmp_path / "o1.fq", tmp_path / "o2.fq"
    kept_sets = []
    for flags, include, skip, table, tid in ((["-include"], True, 0, tab, "c0"), (["-exclude"], False, 0, tab, "c0"),
                                             (["-include", "-10x"], True, 23, tab, "c0"), (["-include", "-min", "3"], True, 0, tab3, "c3")):
        want, n, kept = restated_filter([r1, r2], k, table, tid, include, skip)
        p = run_lookup(flags + ["-sequence", tmp_path / "R1.fq", tmp_path / "R2.fq.gz", "-mers", tmp_path / "db.meryl", "-output", o1, o2],
                       {"MGC_LOOKUP_BATCH": "65536"})
        assert p.returncode == 0, p.stderr
        assert o1.read_bytes() == want[0] and o2.read_bytes() == want[1], flags
        assert ("Including %d reads (or read pairs) out of %d." % (kept, n)) in p.stderr.decode()
        kept_sets.append(want[0])
    assert kept_sets[0] != kept_sets[2] and kept_sets[0] != kept_sets[3]      # -10x and -min change the kept set
    # a single FASTA input; an empty input gives empty outputs
    fa = fmt_text(a, "fa60", 3)
    (tmp_path / "a.fa").write_bytes(fa)
    p = run_lookup(["-exclude", "-sequence", tmp_path / "a.fa", "-mers", tmp_path / "db.meryl", "-output", o1])
    assert p.returncode == 0, p.stderr
    assert o1.read_bytes() == restated_filter([fa], k, tab, "c0", False, 0)[0][0]
    (tmp_path / "none.fq").write_bytes(b"")
    p = run_lookup(["-include", "-sequence", tmp_path / "none.fq", "-mers", tmp_path / "db.meryl", "-output", o1])
    assert p.returncode == 0 and o1.read_bytes() == b"", p.stderr
    # 5 records against 4: exit status 1, both counts named
    (tmp_path / "five.fq").write_bytes(fmt_text(a[:5], "fq") + b"\n")
    (tmp_path / "four.fq").write_bytes(fmt_text(b[:4], "fq") + b"\n")
    p = run_lookup(["-include", "-sequence", tmp_path / "five.fq", tmp_path / "four.fq", "-mers", tmp_path / "db.meryl", "-output", o1, o2])
    assert p.returncode == 1 and "5 in" in p.stderr.decode() and "4 in" in p.stderr.decode(), p.stderr


def numpy_canonical(codes, k):
    """canonical k-mer of every window start (invalid where a code is 4), vectorised"""
    n = codes.size - k + 1
    f = np.zeros(n, dtype=np.uint64)
    r = np.zeros(n, dtype=np.uint64)
    c = np.where(codes > 3, 0, codes).astype(np.uint64)
    for j in range(k):
        f = (f << np.uint64(2)) | c[j:j + n]
        r = r | ((c[j:j + n] ^ np.uint64(2)) << np.uint64(2 * j))
    bad = np.concatenate([[0], np.cumsum(codes > 3)])
    ok = (bad[k:] - bad[:n]) == 0
    return np.minimum(f, r), ok


@pytest.mark.gpu
def test_cli_filter_large(native_lib, tmp_path):
    """A million read pairs of 150 bases through the CLI at its default batch size: the kept pairs and their nKmers against
    a vectorised restatement (include-exclude.C:64-93, 124-125), by digest of (pair index, nKmers)"""
    from meryl_amd import build
    k, L, npairs = 21, 150, 1_000_000
    rng = np.random.default_rng(17)
    lut = np.frombuffer(b"ACTG", dtype=np.uint8)
    genome = rng.integers(0, 4, 3_000_000, dtype=np.uint8)
    (tmp_path / "db.fa").write_bytes(b">g\n" + lut[genome].tobytes() + b"\n")
    subprocess.run([build.build_cli(), "-Q", "k=21", "memory=4", "count", str(tmp_path / "db.fa"), "output", str(tmp_path / "db.meryl")], check=True)
    gk, gok = numpy_canonical(genome, k)
    table = np.unique(gk[gok])
    def reads(own):                                                          # codes [npairs, L]; half from the genome with substitutions
        start = rng.integers(0, genome.size - L, npairs)
        c = genome[start[:, None] + np.arange(L)[None, :]]
        other = rng.integers(0, 4, c.shape, dtype=np.uint8)
        c = np.where((rng.random(c.shape, dtype=np.float32) < 0.01) | ~own[:, None], other, c)   # 1 % substitutions; foreign reads
        c[rng.random(c.shape, dtype=np.float32) < 0.0005] = 4                # N
        return c.astype(np.uint8)
    own = rng.random(npairs) < 0.5
    c1, c2 = reads(own), reads(own & (rng.random(npairs) < 0.9))
    def fastq(c, tag):
        body = np.where(c > 3, ord("N"), lut[np.minimum(c, 3)]).astype(np.uint8)
        return b"".join(b"@p%d/%s\n%s\n+\n%s\n" % (i, tag, body[i].tobytes(), b"I" * L) for i in range(npairs))
    (tmp_path / "R1.fq").write_bytes(fastq(c1, b"1"))
    (tmp_path / "R2.fq").write_bytes(fastq(c2, b"2"))
    found = np.zeros(npairs, dtype=np.int64)
    for c in (c1, c2):
        for lo in range(0, npairs, 100_000):                                 # (in slices: the k-mers of a slice are 8 B per base)
            part = c[lo:lo + 100_000]
            flat = np.concatenate([part, np.full((part.shape[0], 1), 4, dtype=np.uint8)], axis=1).reshape(-1)
            ck, ok = numpy_canonical(flat, k)
            hit = np.concatenate([ok & np.isin(ck, table), np.zeros(k - 1, dtype=bool)])
            found[lo:lo + 100_000] += hit.reshape(part.shape[0], L + 1).sum(axis=1)
    keep = np.nonzero(found > 0)[0]
    assert npairs / 4 < keep.size < 3 * npairs / 4
    want = np.stack([keep, found[keep]], axis=1).astype(np.int64)
    p = run_lookup(["-include", "-sequence", tmp_path / "R1.fq", tmp_path / "R2.fq", "-mers", tmp_path / "db.meryl",
                    "-output", tmp_path / "o1.fq", tmp_path / "o2.fq"])
    assert p.returncode == 0, p.stderr
    assert ("Including %d reads (or read pairs) out of %d." % (keep.size, npairs)) in p.stderr.decode()
    for name, tag, c in (("o1.fq", b"1", c1), ("o2.fq", b"2", c2)):
        lines = (tmp_path / name).read_bytes().split(b"\n")
        assert lines[-1] == b"" and len(lines) == 4 * keep.size + 1
        heads = lines[0:-1:4]
        got = np.array([(int(h[2:h.index(b"/")]), int(h[h.index(b"=") + 1:])) for h in heads], dtype=np.int64)
        assert hashlib.sha256(got.tobytes()).hexdigest() == hashlib.sha256(want.tobytes()).hexdigest()
        assert all(h.endswith(b"/" + tag + b" nKmers=%d" % f) for h, f in zip(heads[:50], want[:50, 1]))
        body = np.where(c[keep] > 3, ord("N"), lut[np.minimum(c[keep], 3)]).astype(np.uint8)
        assert hashlib.sha256(b"".join(lines[1:-1:4])).hexdigest() == hashlib.sha256(body.tobytes()).hexdigest()
        assert set(lines[2:-1:4]) == {b"+"} and set(lines[3:-1:4]) == {b"I" * L}
