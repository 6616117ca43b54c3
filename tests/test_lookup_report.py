"""meryl-lookup's position reports -bed, -bed-runs, -wig-count and -wig-depth (src/meryl-lookup/dump.C) through the C ABI
(mgc_lookup_positions / mgc_lookup_report), the Python API and the CLI, against a restatement of dump.C in this file: its own
rolling k-mers per sequence (kmerIterator), dictionaries for the tables, and the reference's output loops line for line."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

CODE = dict(zip("ACTGactg", (0, 1, 2, 3, 0, 1, 2, 3)))
M32 = 0xFFFFFFFF


# ---- restatement of src/meryl-lookup/dump.C ------------------------------------------------------------------------------
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


def process_sequence(seq, k, tables, what, labels_present):
    """dump.C:89-245: exist[t] (bed), count (wig-count) or depth (wig-depth), and maxP"""
    n, maxp = len(seq), 0
    if what == "presence":
        exist = [[False] * n for _ in tables]
        for p, f, r in windows(seq, k):                                     # :109-135
            for t, tab in enumerate(tables):
                if f in tab or r in tab:
                    exist[t if labels_present else 0][p] = True
                    maxp = p + 1
        return exist, maxp
    if what == "count":
        count = [0] * n
        for p, f, r in windows(seq, k):                                     # :146-164
            for tab in tables:
                fv, rv = tab.get(f, 0), tab.get(r, 0)
                count[p] = (count[p] + (fv if f == r else fv + rv)) & M32
                maxp = p + 1
        return count, maxp
    depth = [0] * (n + 1)
    for p, f, r in windows(seq, k):                                         # :222-233, table 0 only
        if f in tables[0] or r in tables[0]:
            depth[p] = (depth[p] + 1) & 0xFF
            depth[p + k] = (depth[p + k] - 1) & 0xFF
            maxp = p + k
    d = 0
    for pp in range(maxp + 1):                                              # :237-241
        d += depth[pp]
        depth[pp] = d & 0xFF
    return depth, maxp


def output_sequence(name, seq, k, tables, mode, labels):
    """outputBED (:251-298), outputBEDruns (:302-364), outputWIG (:368-405) of one sequence"""
    labels_present = max((len(l) for l in labels), default=0) > 0            # meryl-lookup.C:27-31
    out = []
    if mode in ("bed", "bed-runs"):
        exist, maxp = process_sequence(seq, k, tables, "presence", labels_present)
        lab = ["\t" + labels[t] if t < len(labels) else "" for t in range(len(tables))]
        if mode == "bed":
            for p in range(maxp):
                for t in range(len(tables)):
                    if exist[t][p]:
                        out.append("%s\t%d\t%d%s\n" % (name, p, p + k, lab[t]))
        else:
            bgn = [None] * len(tables)
            for p in range(maxp + 1):
                for t in range(len(tables)):
                    bit = exist[t][p] if p < maxp else False
                    if bit:
                        if bgn[t] is None:
                            bgn[t] = p
                        continue
                    if bgn[t] is None:
                        continue
                    out.append("%s\t%d\t%d%s\n" % (name, bgn[t], p + k, lab[t]))   # p + k: one past the last window's end
                    bgn[t] = None
    else:
        vals, maxp = process_sequence(seq, k, tables, "count" if mode == "wig-count" else "depth", False)
        out.append("variableStep chrom=%s\n" % name)
        for p in range(maxp):
            if vals[p]:
                out.append("%d\t%d\n" % (p + 1, vals[p]))
    return "".join(out)


def restated_report(names, seqs, k, tables, mode, labels=()):
    return "".join(output_sequence(n, s, k, tables, mode, list(labels)) for n, s in zip(names, seqs)).encode()


def restated_positions(seqs, k, tables, what):
    """per base of the stream the ABI gets (each sequence followed by '.')"""
    out = []
    for s in seqs:
        if what == "presence":
            v = [0] * (len(s) + 1)
            for p, f, r in windows(s, k):
                v[p] = sum(1 << t for t, tab in enumerate(tables) if f in tab or r in tab)
        else:
            v, _ = process_sequence(s, k, tables, what, True)
            v = (list(v) + [0] * (len(s) + 1))[:len(s) + 1]
        out.extend(v)
    return np.array(out, dtype=np.uint64).astype(np.uint32)


# ---- inputs ----------------------------------------------------------------------------------------------------------
def stream_of(seqs, breakers=True):
    text = "".join(s + "." if (breakers or s) else s for s in seqs)
    starts = np.zeros(len(seqs) + 1, dtype=np.uint64)
    o = 0
    for i, s in enumerate(seqs):
        o += len(s) + (1 if (breakers or s) else 0)
        starts[i + 1] = o
    return text, starts


def query_sequences(oracle_lib, seed, k):
    reads = [r for r in oracle_lib.synth_reads(seed, 40_000, 0, 400, 150, 5000, 2000).tobytes().decode().split(".") if r]
    rng = np.random.default_rng(seed)
    foreign = "".join(rng.choice(list("ACGT"), 300))
    lower = reads[5][:40] + reads[5][40:100].lower() + reads[5][100:]
    seqs = reads[:60] + [foreign, lower, "", reads[7][:k - 1], "N" * 30, reads[9] + "n" + reads[10], ""]
    return seqs


def table_dict(hi, lo, cn, vmin=0, vmax=M32):
    return {(int(h) << 64) | int(l): int(c) for h, l, c in zip(hi, lo, cn) if vmin <= int(c) <= vmax}


def device_keys(torch, hi, lo, k):
    order = np.lexsort((lo, hi))
    hi, lo = hi[order], lo[order]
    if k > 32:
        return torch.from_numpy(np.stack([lo, hi], axis=1).view(np.int64).copy()).cuda(), order
    return torch.from_numpy(lo.view(np.int64).copy()).cuda(), order


def make_tables(oracle_lib, seed, k):
    """(Lookups, dicts): a canonical table from a count, a non-canonical one of forward k-mers, and a -min 2 -max 5 filter"""
    import torch
    from meryl_amd import capi, count, lookup
    reads = oracle_lib.synth_reads(seed, 40_000, 0, 2000, 150, 5000, 2000)
    cfg = capi.configure(k, reads.size, 1 << 30)
    with count.Session(cfg, 0) as s:
        s.push_bases_device(torch.from_numpy(reads).cuda())
        s.count()
        keys, cnts = s.result_device()
        canon = lookup.Lookup.from_device(keys, cnts, k)
        filt = lookup.Lookup.from_device(keys, cnts, k, 2, 5)
    hi, lo, cn, _ = oracle_lib.count_brute(reads.tobytes(), k)
    fhi, flo, fcn, _ = oracle_lib.count_brute(oracle_lib.synth_reads(seed, 40_000, 2000, 1500).tobytes(), k, 1)   # forward
    fk, order = device_keys(torch, fhi, flo, k)
    fwd = lookup.Lookup.from_device(fk, torch.from_numpy(fcn[order].view(np.int32).copy()).cuda(), k)
    return [canon, fwd, filt], [table_dict(hi, lo, cn), table_dict(fhi, flo, fcn), table_dict(hi, lo, cn, 2, 5)]


# ---- positions -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("k", [21, 31, 51, 8])
def test_positions(native_lib, oracle_lib, k):
    import torch
    from meryl_amd import lookup
    lks, dicts = make_tables(oracle_lib, 60 + k, k)
    seqs = query_sequences(oracle_lib, 60 + k, k)
    text, _ = stream_of(seqs)
    bases = torch.from_numpy(np.frombuffer(text.encode(), dtype=np.uint8).copy()).cuda()
    for what in ("presence", "count", "depth"):
        got = lookup.positions(lks, what, bases).cpu().numpy().view(np.uint32)
        want = restated_positions(seqs, k, dicts, what)
        assert np.array_equal(got, want), (k, what, np.nonzero(got != want)[0][:10])
        assert want.any()
    # one table alone, and the filtered one first (depth reads table 0 only)
    for sub in ([2], [2, 0, 1]):
        t, d = [lks[i] for i in sub], [dicts[i] for i in sub]
        for what in ("presence", "depth"):
            got = lookup.positions(t, what, bases).cpu().numpy().view(np.uint32)
            assert np.array_equal(got, restated_positions(seqs, k, d, what)), (k, sub, what)
    for lk in lks:
        lk.close()


@pytest.mark.gpu
def test_count_wraps_mod_2_32(native_lib):
    """dump.C:154-160 sums uint32 values: 2^32 - 3 + 3 wraps to 0 (no WIG line), 2^32 - 1 + 10 to 9"""
    import torch
    from meryl_amd import lookup
    k = 21
    rng = np.random.default_rng(3)
    seq = "".join(rng.choice(list("ACGT"), 200))
    wins = list(windows(seq, k))
    _, fx, rx = wins[10]
    _, fy, ry = wins[50]
    a = {fx: M32 - 2, fy: M32}
    b = {fx: 3, fy: 10, ry: 0x80000000}
    lks = []
    for tab in (a, b):
        ks = sorted(tab)
        keys = torch.tensor([x if x < (1 << 63) else x - (1 << 64) for x in ks], dtype=torch.int64).cuda()
        vals = torch.from_numpy(np.array([tab[x] for x in ks], dtype=np.uint32).view(np.int32).copy()).cuda()
        lks.append(lookup.Lookup.from_device(keys, vals, k))
    text, starts = stream_of([seq])
    bases = torch.from_numpy(np.frombuffer(text.encode(), dtype=np.uint8).copy()).cuda()
    got = lookup.positions(lks, "count", bases).cpu().numpy().view(np.uint32)
    want = restated_positions([seq], k, [a, b], "count")
    assert np.array_equal(got, want)
    assert got[10] == 0 and got[50] == (M32 + 10 + 0x80000000) & M32
    rep = lookup.report(lks, "wig-count", ["s"], bases, starts)
    assert rep == restated_report(["s"], [seq], k, [a, b], "wig-count")
    assert b"\n11\t" not in rep and b"\n51\t" in rep
    for lk in lks:
        lk.close()


# ---- report bytes ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("k", [21, 8])
def test_report_bytes(native_lib, oracle_lib, k):
    import torch
    from meryl_amd import lookup
    lks, dicts = make_tables(oracle_lib, 90 + k, k)
    seqs = query_sequences(oracle_lib, 90 + k, k)
    names = ["seq%d" % i for i in range(len(seqs))]
    for breakers in (True, False):                                          # truly empty sequences: no byte at all
        text, starts = stream_of(seqs, breakers)
        bases = torch.from_numpy(np.frombuffer(text.encode(), dtype=np.uint8).copy()).cuda()
        for mode in ("bed", "bed-runs", "wig-count", "wig-depth"):
            for tabs in ([0], [0, 1, 2]):
                for labels in ([], ["alpha", "be"]):
                    if labels and mode.startswith("wig"):
                        continue
                    t, d = [lks[i] for i in tabs], [dicts[i] for i in tabs]
                    want = restated_report(names, seqs, k, d, mode, labels)
                    got = lookup.report(t, mode, names, bases, starts, labels=labels)
                    assert got == want, (k, mode, tabs, labels, breakers)
                    if breakers and len(tabs) == 3:
                        pieces = []
                        small = lookup.report(t, mode, names, bases, starts, labels=labels, chunk_bytes=200, pieces=pieces)
                        assert small == want and len(pieces) >= min(100, len(want) // 200) and max(map(len, pieces)) <= 200
    with pytest.raises(Exception, match="longest line"):
        lookup.report(lks, "bed", names, bases, starts, chunk_bytes=40)
    for lk in lks:
        lk.close()


@pytest.mark.gpu
def test_report_help_example_and_errors(native_lib):
    """meryl-lookup-help.C:55-69: two adjacent k = 21 hits -> -bed 0 21 / 1 22; -bed-runs writes 0 23 (the code, dump.C:350),
    where the help text shows 0 22"""
    import torch
    from meryl_amd import capi, lookup
    k = 21
    rng = np.random.default_rng(11)
    seq = "".join(rng.choice(list("ACGT"), 60))
    w = list(windows(seq, k))
    tab = {min(w[0][1], w[0][2]), min(w[1][1], w[1][2])}
    assert not any(min(f, r) in tab for _, f, r in w[2:])
    ks = sorted(tab)
    keys = torch.tensor(ks, dtype=torch.int64).cuda()
    lk = lookup.Lookup.from_device(keys, torch.ones(2, dtype=torch.int32).cuda(), k)
    text, starts = stream_of([seq])
    bases = torch.from_numpy(np.frombuffer(text.encode(), dtype=np.uint8).copy()).cuda()
    assert lookup.report([lk], "bed", ["sequence1"], bases, starts) == b"sequence1\t0\t21\nsequence1\t1\t22\n"
    assert lookup.report([lk], "bed-runs", ["sequence1"], bases, starts) == b"sequence1\t0\t23\n"
    assert lookup.report([lk, lk], "bed-runs", ["sequence1"], bases, starts, labels=["A", "B"]) == \
        b"sequence1\t0\t23\tA\nsequence1\t0\t23\tB\n"
    # MGC_EINVAL: different k, more than 32 tables, a window that could cross into the next sequence
    other = lookup.Lookup.from_device(keys, torch.ones(2, dtype=torch.int32).cuda(), 22)
    for bad in (lambda: lookup.report([lk, other], "bed", ["s"], bases, starts),
                lambda: lookup.positions([lk] * 33, "presence", bases),
                lambda: lookup.report([lk], "bed", ["a", "b"], bases, [0, 30, bases.numel()])):
        with pytest.raises(capi.MgcError) as e:
            bad()
        assert e.value.rc == capi.MGC_EINVAL
    lk.close()
    other.close()


# ---- CLI -------------------------------------------------------------------------------------------------------------
def run_lookup(args, env=None):
    from meryl_amd import build
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([build.build_lookup_cli()] + [str(a) for a in args], capture_output=True, env=e)


@pytest.mark.gpu
def test_cli_position_reports(native_lib, oracle_lib, tmp_path):
    from meryl_amd import build
    k = 21
    meryl = build.build_cli()
    dicts = []
    for i, seed in enumerate((31, 32)):
        reads = [r for r in oracle_lib.synth_reads(seed, 30_000, 0, 1500).tobytes().decode().split(".") if r]
        fa = tmp_path / ("r%d.fa" % i)
        fa.write_text("".join(">r%d\n%s\n" % (j, r) for j, r in enumerate(reads)))
        subprocess.run([meryl, "-Q", "k=%d" % k, "memory=1", "count", str(fa), "output", str(tmp_path / ("db%d.meryl" % i))], check=True)
        hi, lo, cn, _ = oracle_lib.count_brute(".".join(reads) + ".", k)
        dicts.append(table_dict(hi, lo, cn))
    genome = oracle_lib.synth_reads(31, 30_000, 0, 80, 150, 5000, 2000).tobytes().decode().split(".")
    long_seq = "".join(genome[:70])                                          # ~10 kbp: longer than a 4096-position range
    seqs = [long_seq, genome[70], "", genome[71][:15], "ACGTNacgtn" * 5, genome[72] + genome[73]]
    names = ["ctg%d" % i for i in range(len(seqs))]
    asm = tmp_path / "asm.fa"
    asm.write_text("".join(">%s desc\n%s\n" % (n, "\n".join(s[i:i + 60] for i in range(0, len(s), 60))) for n, s in zip(names, seqs)))
    dbs = [tmp_path / "db0.meryl", tmp_path / "db1.meryl"]
    env = {"MGC_LOOKUP_CHUNK": "4096"}
    for mode, labels in (("-bed", []), ("-bed-runs", ["A", "B"]), ("-wig-count", []), ("-wig-depth", [])):
        want = restated_report(names, seqs, k, dicts, mode[1:], labels)
        assert len(want) > 4096 or mode == "-bed-runs"
        lab = ["-labels"] + labels if labels else []
        p = run_lookup([mode, "-sequence", asm, "-mers"] + dbs + lab + ["-output", tmp_path / "o.txt"], env)
        assert p.returncode == 0, p.stderr
        assert (tmp_path / "o.txt").read_bytes() == want, mode
        p = run_lookup([mode, "-sequence", asm, "-mers"] + dbs + lab, env)
        assert p.returncode == 0 and p.stdout == want, mode
    # -existence is unchanged: name, k-mers, then per database (k-mers in it, found)
    p = run_lookup(["-existence", "-sequence", asm, "-mers"] + dbs)
    assert p.returncode == 0, p.stderr
    rows = []
    for n, s in zip(names, seqs):
        w = [min(f, r) for _, f, r in windows(s, k)]
        rows.append("\t".join([n, str(len(w))] + ["%d\t%d" % (len(d), sum(1 for x in w if x in d)) for d in dicts]) + "\n")
    assert p.stdout.decode() == "".join(rows)


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
def test_cli_wig_depth_large(native_lib, tmp_path):
    """-wig-depth of a 24 Mbp assembly against a database of a mutated 60 % of it: digest of (position, depth) against a
    vectorised restatement (dump.C:222-241, 384-405)"""
    from meryl_amd import build
    k = 21
    rng = np.random.default_rng(5)
    lut = np.frombuffer(b"ACTG", dtype=np.uint8)
    asm_codes = rng.integers(0, 4, 24_000_000, dtype=np.uint8)
    asm_codes[rng.integers(0, asm_codes.size, 2000)] = 4                    # N
    db_codes = asm_codes[:14_400_000].copy()
    mut = rng.integers(0, db_codes.size, 300_000)
    db_codes[mut] = (db_codes[mut] + 1) & 3
    def fasta(codes, name):
        b = np.where(codes > 3, ord("N"), lut[np.minimum(codes, 3)]).astype(np.uint8).tobytes()
        return b">" + name + b"\n" + b"\n".join(b[i:i + (1 << 20)] for i in range(0, len(b), 1 << 20)) + b"\n"
    (tmp_path / "asm.fa").write_bytes(fasta(asm_codes[:16_000_000], b"chrA") + fasta(asm_codes[16_000_000:], b"chrB"))
    (tmp_path / "db.fa").write_bytes(fasta(db_codes, b"reads"))
    subprocess.run([build.build_cli(), "-Q", "k=21", "memory=8", "count", str(tmp_path / "db.fa"), "output", str(tmp_path / "db.meryl")],
                   check=True)
    dbk, dbok = numpy_canonical(db_codes, k)
    table = np.unique(dbk[dbok])
    want_lines = []
    for part in (asm_codes[:16_000_000], asm_codes[16_000_000:]):
        ck, ok = numpy_canonical(part, k)
        hit = ok & np.isin(ck, table)
        cs = np.concatenate([[0], np.cumsum(hit.astype(np.int64))])
        i = np.arange(part.size)
        depth = cs[np.minimum(i + 1, hit.size)] - cs[np.clip(i - k + 1, 0, hit.size)]
        nz = np.nonzero(depth)[0]
        want_lines.append(np.stack([nz + 1, depth[nz]], axis=1))
    p = run_lookup(["-wig-depth", "-sequence", tmp_path / "asm.fa", "-mers", tmp_path / "db.meryl", "-output", tmp_path / "o.wig"])
    assert p.returncode == 0, p.stderr
    text = (tmp_path / "o.wig").read_bytes()
    head_a, rest = text.split(b"\n", 1)
    assert head_a == b"variableStep chrom=chrA"
    body_a, body_b = rest.split(b"variableStep chrom=chrB\n")
    for body, want in ((body_a, want_lines[0]), (body_b, want_lines[1])):
        got = np.fromstring(body.decode(), dtype=np.int64, sep=" ").reshape(-1, 2)
        assert hashlib.sha256(got.tobytes()).hexdigest() == hashlib.sha256(want.astype(np.int64).tobytes()).hexdigest()
    assert want_lines[0].shape[0] > 5_000_000


# ---- CLI checks before any device call (meryl-lookup.C:309-368) ----------------------------------------------------
def test_cli_option_checks(native_lib, tmp_path):
    q = tmp_path / "q.fa"
    q.write_text(">a\nACGT\n")
    db = tmp_path / "missing.meryl"
    cases = [
        (["-wig-count", "-labels", "A", "-sequence", q, "-mers", db], "Labels (-labels) not supported for -wig-count."),
        (["-wig-depth", "-sequence", q, "-mers", db, "-labels", "A", "B"], "Labels (-labels) not supported for -wig-depth."),
        (["-bed", "-sequence", q, q, "-mers", db], "Only one input sequence (-sequence) supported for -bed."),
        (["-sequence", q, "-mers", db], "No report-type (-bed, -wig-count, -wig-depth, -existence, -include, -exclude) supplied."),
        (["-wig-depth", "-sequence", q, "-mers", db, "-output", tmp_path / "o.wig.gz"], "compressed"),
    ]
    for args, msg in cases:
        p = run_lookup(args)
        assert p.returncode == 1 and msg in p.stderr.decode(), (args, p.stderr)
    assert not (tmp_path / "o.wig.gz").exists()
