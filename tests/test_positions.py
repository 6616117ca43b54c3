"""The k-mer position index and query painting (include/meryl_positions.h, meryl_amd/poslookup.py, bin/position-lookup) against a
restatement of src/meryl-lookup/position-lookup.C in this file: its own rolling k-mers (kmerIterator), a dict from canonical
k-mer to slot, Python lists of positions, and the reference's three loops of writeBatch (:241-328) written per hit and per
position -- with the length of a slot's list in place of the k-mer's value (the one documented divergence; the two are equal
when the database is the count of the reference).  Every comparison is exact."""
import functools
import os
import subprocess

import numpy as np
import pytest

CODE = dict(zip("ACTGactg", (0, 1, 2, 3, 0, 1, 2, 3)))
COMP = str.maketrans("ACGTacgt", "TGCAtgca")
M64 = (1 << 64) - 1
NONE = 0xFFFFFFFF


def revcomp(s):
    return s.translate(COMP)[::-1]


def random_seq(rng, n):
    return "".join(rng.choice(list("ACGT"), n)) if n else ""


# ---- restatement of src/meryl-lookup/position-lookup.C -----------------------------------------------------------------
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


def stream_of(seqs):
    """the base stream every entry point takes: '.' after each sequence; and the n + 1 offsets"""
    starts = np.zeros(len(seqs) + 1, dtype=np.int64)
    for i, s in enumerate(seqs):
        starts[i + 1] = starts[i] + len(s) + 1
    return "".join(s + "." for s in seqs), starts


class Restated:
    """merylExactLookup::load + loadPositions as position-lookup.C uses them: slot = rank in the table (index()), the list of
    a slot = the stream offsets of the reference windows whose canonical k-mer it is, ascending"""

    def __init__(self, k, table, ref_seqs):
        self.k, self.table = k, sorted(table)
        self.slot = {km: i for i, km in enumerate(self.table)}
        _, self.ref_start = stream_of(ref_seqs)
        self.n_ref = int(self.ref_start[-1])
        self.lists = [[] for _ in self.table]
        self.ref_slot = np.full(self.n_ref, NONE, dtype=np.uint32)
        for s, seq in enumerate(ref_seqs):
            off = int(self.ref_start[s])
            for p, f, r in windows(seq, k):
                i = self.slot.get(min(f, r))                   # :198: only the canonical k-mer
                if i is not None:
                    self.lists[i].append(off + p)
                    self.ref_slot[off + p] = i
        self.pos_start = np.concatenate([[0], np.cumsum([len(l) for l in self.lists])]).astype(np.int64)
        self.pos_data = np.array([p for l in self.lists for p in l], dtype=np.uint32)
        self.np_lists = [np.array(l, dtype=np.int64) for l in self.lists]

    def lookup_batch(self, queries):
        """lookupBatch (:189-208): (slot, query) per window whose canonical k-mer is in the table"""
        hits = []
        for qi, q in enumerate(queries):
            for _, f, r in windows(q, self.k):
                i = self.slot.get(min(f, r))
                if i is not None:
                    hits.append((i, qi))
        return hits

    def write_batch(self, queries, mers, qseqs):
        """writeBatch (:229-336) of one batch; mers / qseqs are nQmerPer / nQseqPer over the reference stream"""
        hits = self.lookup_batch(queries)
        t_cov = np.zeros(len(queries), dtype=np.uint32)
        n_per = np.zeros(len(queries), dtype=np.uint32)
        for i, qi in hits:                                     # :248-259 (uint32: they wrap)
            t_cov[qi] += np.uint32(1)
            n_per[qi] += np.uint32(len(self.lists[i]))
        for i, qi in hits:                                     # :272-288: over all the positions of the k-mer
            mers[self.np_lists[i]] += np.uint32(1)
        hits.sort()                                            # :299-302
        for pp, (i, qi) in enumerate(hits):                    # :307-327
            if pp != 0 and hits[pp - 1] == (i, qi):
                continue
            qseqs[self.np_lists[i]] += np.uint32(1)
        return n_per, t_cov

    def per_base_text(self, count, names):
        """saveMerPerBase / saveQueryPerBase (:340-364); with several sequences `# ident` before each one's lines"""
        out = []
        for s, name in enumerate(names):
            a, b = int(self.ref_start[s]), int(self.ref_start[s + 1])
            nz = [i for i in range(a, b) if count[i]]
            if nz and len(names) > 1:
                out.append("# %s\n" % name)
            out.extend("%d %d\n" % (i - a, count[i]) for i in nz)
        return "".join(out).encode()


def canonical_kmers(seqs, k):
    d = {}
    for s in seqs:
        for _, f, r in windows(s, k):
            c = min(f, r)
            d[c] = d.get(c, 0) + 1
    return d


# ---- inputs ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference():
    """four sequences of about 9,000 / 20 / 0 / 5,000 bases: N runs, lower-case stretches, a 600-base homopolymer run, a
    1,000-base AC repeat, one 300-base segment again as its reverse complement, and a 64-base reverse-complement palindrome"""
    rng = np.random.default_rng(71)
    a = random_seq(rng, 3000)
    seg = a[1200:1500]
    s0 = (a[:2000] + "NNNNN" + a[2000:] + "A" * 600 + random_seq(rng, 1400).lower() + "AC" * 500 + random_seq(rng, 1300) + "N"
          + revcomp(seg) + random_seq(rng, 1400) + "nn" + random_seq(rng, 95))
    half = random_seq(rng, 32)                                  # half + its reverse complement: a 64-mer equal to its own
    s3 = random_seq(rng, 2000) + "N" * 40 + random_seq(rng, 1500).lower() + half + revcomp(half) + random_seq(rng, 1396)
    return (s0, random_seq(rng, 20), "", s3)


@functools.lru_cache(maxsize=None)
def restated(k, which):
    """table 1: exactly the reference's k-mers; 2: a superset (k-mers of an unrelated sequence: empty lists); 3: the k-mers
    the reference holds at least twice (min_value = 2: some reference windows miss).  Returns (Restated, {kmer: value})."""
    ref = reference()
    counts = canonical_kmers(ref, k)
    if which == 2:
        for km in canonical_kmers([random_seq(np.random.default_rng(72), 3000)], k):
            counts.setdefault(km, 1)
    kept = {km: v for km, v in counts.items() if which != 3 or v >= 2}
    return Restated(k, kept.keys(), ref), counts


def device_table(torch, counts, k, min_value=0):
    from meryl_amd import lookup
    kms = sorted(counts)
    vals = torch.from_numpy(np.array([counts[km] for km in kms], dtype=np.int32)).cuda()
    return lookup.Lookup.from_device(device_kmers(torch, kms, k), vals, k, min_value)


def device_kmers(torch, kms, k):
    lo = np.array([km & M64 for km in kms], dtype=np.uint64)
    if k > 32:
        hi = np.array([km >> 64 for km in kms], dtype=np.uint64)
        return torch.from_numpy(np.stack([lo, hi], axis=1).view(np.int64).copy()).reshape(-1, 2).cuda()
    return torch.from_numpy(lo.view(np.int64).copy()).cuda()


def device_bases(torch, text):
    return torch.from_numpy(np.frombuffer(text.encode(), dtype=np.uint8).copy()).cuda()


def check_index(idx, R):
    ref_slot, pos_start, pos_data = idx.arrays()
    assert np.array_equal(ref_slot.cpu().numpy().view(np.uint32), R.ref_slot)
    assert np.array_equal(pos_start.cpu().numpy(), R.pos_start)
    assert np.array_equal(pos_data.cpu().numpy().view(np.uint32), R.pos_data)
    i = idx.info
    lens = [len(l) for l in R.lists]
    assert (i.k, i.n_kmers, i.n_ref_bases, i.n_placed) == (R.k, len(R.table), R.n_ref, len(R.pos_data))
    assert (i.n_slots_used, i.longest_list) == (sum(1 for n in lens if n), max(lens, default=0))
    assert i.device_bytes == 4 * R.n_ref + 8 * (len(R.table) + 1) + 4 * len(R.pos_data)


# ---- the index -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("which", [1, 2, 3])
@pytest.mark.parametrize("k", [6, 21, 33, 64])
def test_index_parity(native_lib, k, which):
    import torch
    from meryl_amd import poslookup
    R, counts = restated(k, which)
    lens = [len(l) for l in R.lists]
    if which == 1:
        assert min(lens) >= 1 and sorted(lens)[-2] > (250 if k > 6 else 100)   # two slots own hundreds of overlapping positions
        if k % 2 == 0:                                          # a k-mer that is its own reverse complement is placed
            assert any(f == r for s in reference() for _, f, r in windows(s, k))
    if which == 2:
        assert (k == 6) or 0 in lens
    if which == 3:
        assert len(R.pos_data) < sum(1 for s in reference() for _ in windows(s, k))   # some reference windows miss
    text, _ = stream_of(reference())
    with device_table(torch, counts, k, 2 if which == 3 else 0) as table:
        assert table.info.n_kmers == len(R.table)
        with poslookup.PositionIndex(table, device_bases(torch, text)) as idx:
            check_index(idx, R)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [21, 33])
def test_index_tile_edges(native_lib, k):
    """one workgroup of the slot pass covers LK_RUN = 16 x 256 = 4096 window starts, one of the pair compaction 8 x 256 = 2048
    stream positions: references with one less, exactly and one more window start than either, and with none and one"""
    import torch
    from meryl_amd import poslookup
    rng = np.random.default_rng(73)
    for n in (k - 1, k, 2047 + k, 2048 + k, 2049 + k, 4095 + k, 4096 + k, 4097 + k, 2047, 2048):
        ref = (random_seq(rng, n),)
        counts = canonical_kmers(ref, k) or {5: 1}
        R = Restated(k, counts.keys(), ref)
        with device_table(torch, counts, k) as table, poslookup.PositionIndex(table, device_bases(torch, stream_of(ref)[0])) as idx:
            check_index(idx, R)
            assert idx.info.n_placed == max(n - k + 1, 0)


@pytest.mark.gpu
def test_canonical_only(native_lib):
    """position-lookup.C:198 looks up min(fmer, rmer) alone: a table that holds only the non-canonical form of a k-mer places
    nothing and is hit by nothing, although Lookup.stream (value(fmer) || value(rmer)) finds it"""
    import torch
    from meryl_amd import poslookup
    k = 21
    rng = np.random.default_rng(74)
    seq = random_seq(rng, k)
    (_, f, r), = windows(seq, k)
    assert f != r
    ref = (random_seq(rng, 50) + seq + "N" + revcomp(seq) + random_seq(rng, 50),)
    text, starts = stream_of(ref)
    bases = device_bases(torch, text)
    with device_table(torch, {max(f, r): 3}, k) as table:
        assert sorted(table.stream(bases).cpu().numpy().nonzero()[0].tolist()) == [50, 50 + k + 1]
        with poslookup.PositionIndex(table, bases) as idx:
            assert idx.info.n_placed == 0 and idx.info.n_slots_used == 0
            assert (idx.arrays()[0].cpu().numpy().view(np.uint32) == NONE).all()
            with poslookup.Painter(idx) as p:
                n_per, t_cov = p.add(bases, starts)
                assert n_per.tolist() == [0] and t_cov.tolist() == [0]
                assert not p.mers().any() and not p.queries().any()
    with device_table(torch, {min(f, r): 3}, k) as table, poslookup.PositionIndex(table, bases) as idx:   # the canonical form: both strands
        assert idx.arrays()[2].cpu().numpy().tolist() == [50, 50 + k + 1]


@pytest.mark.gpu
@pytest.mark.parametrize("k", [21, 33])
def test_find(native_lib, k):
    import torch
    from meryl_amd import poslookup
    R, counts = restated(k, 2)
    rng = np.random.default_rng(75)
    empty = [km for km, l in zip(R.table, R.lists) if not l][:50]
    present = [R.table[i] for i in rng.choice(len(R.table), 200)] + [R.table[int(np.argmax([len(l) for l in R.lists]))]]
    absent = [km for km in (int(rng.integers(0, 1 << min(2 * k, 62))) for _ in range(50)) if km not in R.slot]
    if k < 32:
        absent.append((1 << 60) | 5)                           # bits above 2k: not a k-mer
    flipped = []                                               # the other strand of present k-mers: looked up as given -> absent
    for km in present[:20]:
        s = "".join("ACTG"[(km >> (2 * (k - 1 - j))) & 3] for j in range(k))
        (_, f, r), = windows(s, k)
        if max(f, r) not in R.slot:
            flipped.append(max(f, r))
    assert empty and absent and flipped
    asked = present + empty + absent + flipped
    text, _ = stream_of(reference())
    with device_table(torch, counts, k) as table, poslookup.PositionIndex(table, device_bases(torch, text)) as idx:
        begin, count = idx.find(device_kmers(torch, asked, k))
        pos_data = idx.arrays()[2].cpu().numpy().view(np.uint32)
    begin, count = begin.cpu().numpy(), count.cpu().numpy()
    for km, b, c in zip(asked, begin, count):
        want = R.lists[R.slot[km]] if km in R.slot else []
        assert pos_data[b:b + c].tolist() == want, km
        if km not in R.slot:
            assert (b, c) == (0, 0)


# ---- painting --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def queries(k):
    ref = reference()
    rng = np.random.default_rng(76)
    whole = ref[0] + ref[3]
    out = []
    for i in range(300):                                       # cut from both strands, ~2 % substitutions
        n = int(rng.integers(30, 401))
        a = int(rng.integers(0, len(whole) - n))
        q = list(whole[a:a + n])
        for j in np.nonzero(rng.random(n) < 0.02)[0]:
            q[j] = "ACGT"[("ACGT".find(q[j].upper()) + int(rng.integers(1, 4))) % 4] if q[j].upper() in "ACGT" else q[j]
        q = "".join(q)
        out.append(revcomp(q) if i % 2 else q)
    unique = ref[3][100:100 + k]
    out[7:7] = [random_seq(rng, 200), ref[0][:k - 1], "", "N".join([unique] * 5), "A" * 600, out[3], out[3], random_seq(rng, 90)]
    # two contigs: whole waves and workgroups of the slot pass lie inside one sequence (its sums are combined before they are added)
    out += [ref[3], random_seq(rng, 50), revcomp(ref[0])]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def restated_paint(k, which):
    R, _ = restated(k, which)
    mers, qseqs = np.zeros(R.n_ref, dtype=np.uint32), np.zeros(R.n_ref, dtype=np.uint32)
    n_per, t_cov = R.write_batch(list(queries(k)), mers, qseqs)
    return n_per, t_cov, mers, qseqs


def paint(torch, poslookup, idx, qs, cuts, what=7):
    """the queries in batches [cuts[i], cuts[i + 1]) -> (n_per, t_cov, mers, queries); None where not opened"""
    per, cov = [], []
    with poslookup.Painter(idx, what) as p:
        for a, b in zip(cuts[:-1], cuts[1:]):
            text, starts = stream_of(qs[a:b])
            n_per, t_cov = p.add(device_bases(torch, text), starts)
            if what & 1:
                per.append(n_per)
                cov.append(t_cov)
            else:
                assert n_per is None and t_cov is None
        got = [np.concatenate(per) if what & 1 else None, np.concatenate(cov) if what & 1 else None]
        for bit, get in ((2, p.mers), (4, p.queries)):
            if what & bit:
                got.append(get().cpu().numpy().view(np.uint32))
            else:
                with pytest.raises(Exception) as e:
                    get()
                assert e.value.rc == -1 and "not opened" in str(e.value)      # MGC_EINVAL
                got.append(None)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("which", [1, 2])
@pytest.mark.parametrize("k", [21, 33])
def test_paint_parity(native_lib, k, which):
    import torch
    from meryl_amd import poslookup
    R, counts = restated(k, which)
    qs = list(queries(k))
    want = restated_paint(k, which)
    n_per, t_cov, mers, qseqs = want
    # what the inputs are meant to exercise
    assert t_cov[7] == 0 and t_cov[8] == 0 and t_cov[9] == 0                   # random, shorter than k, empty
    assert t_cov[10] == 5 and n_per[10] == 5                                    # one k-mer five times
    assert t_cov[11] == 600 - k + 1 and n_per[11] == (600 - k + 1) * len(R.lists[R.slot[0]]) >= (600 - k + 1) ** 2   # the homopolymer run
    assert t_cov[-3] == sum(1 for _ in windows(reference()[3], k)) and t_cov[-1] == sum(1 for _ in windows(reference()[0], k)) > 8192
    assert mers.max() > qseqs.max() > 1 and (mers >= qseqs).all() and ((mers > 0) == (qseqs > 0)).all()
    text, _ = stream_of(reference())
    with device_table(torch, counts, k) as table, poslookup.PositionIndex(table, device_bases(torch, text)) as idx:
        n = len(qs)
        for cuts in ([0, n], [0, n // 3, n // 3, 2 * n // 3, n], list(range(41)) + [n]):
            got = paint(torch, poslookup, idx, qs, cuts)
            for g, w, name in zip(got, want, ("n_per", "t_cov", "mers", "queries")):
                assert np.array_equal(g, w), (name, cuts[:4])
        for what in range(1, 7):                               # every other subset of the outputs
            got = paint(torch, poslookup, idx, qs, [0, n], what)
            for g, w, bit in zip(got, want, (1, 1, 2, 4)):
                assert (g is None) if not what & bit else np.array_equal(g, w), what
        with poslookup.Painter(idx) as p:                      # zero sequences: a no-op
            a, b = p.add(torch.empty(0, dtype=torch.uint8, device="cuda"), [0])
            assert a.size == 0 and b.size == 0 and not p.mers().any() and not p.queries().any()
            with pytest.raises(Exception) as e:                # a seq_start that does not end at n_bases
                p.add(device_bases(torch, "ACGT."), [0, 4])
            assert e.value.rc == -1 and "seq_start does not end at n_bases" in str(e.value)


# ---- the front end -----------------------------------------------------------------------------------------------------
def fasta(names, seqs, width=70):
    return "".join(">%s some text\n%s\n" % (n, "\n".join(s[i:i + width] for i in range(0, len(s), width))) for n, s in zip(names, seqs))


def run_front_end(tmp, db, ref_fa, query_files, tag, env=None):
    from meryl_amd import build
    e = dict(os.environ)
    e.update(env or {})
    outs = [tmp / ("%s.%s" % (tag, x)) for x in ("hpq", "mpb", "qpb")]
    p = subprocess.run([build.build_position_lookup_cli(), "-m", str(db), "-s", str(ref_fa), "-hpq", str(outs[0]), "-mpb", str(outs[1]),
                        "-qpb", str(outs[2])] + [str(q) for q in query_files], capture_output=True, env=e)
    assert p.returncode == 0, p.stderr
    return [o.read_bytes() for o in outs]


@pytest.mark.gpu
@pytest.mark.parametrize("multi", [False, True])
def test_front_end(native_lib, tmp_path, multi):
    from meryl_amd import build
    k = 21
    ref = reference() if multi else (reference()[0],)
    ref_names = ["chr%d" % i for i in range(len(ref))]
    (tmp_path / "ref.fa").write_text(fasta(ref_names, ref))
    (tmp_path / "db.fa").write_text(fasta(["s%d" % i for i, s in enumerate(ref) if s], [s for s in ref if s]))
    subprocess.run([build.build_cli(), "-Q", "k=%d" % k, "memory=1", "count", str(tmp_path / "db.fa"), "output", str(tmp_path / "ref.meryl")],
                   check=True)
    R = Restated(k, canonical_kmers(ref, k).keys(), ref)        # the database is the count of the reference: value = list length
    qs = list(queries(k))
    names = ["q%d" % i for i in range(len(qs))]
    half = len(qs) // 2
    (tmp_path / "all.fa").write_text(fasta(names, qs))
    (tmp_path / "a.fa").write_text(fasta(names[:half], qs[:half]))
    (tmp_path / "b.fq").write_text("".join("@%s x\n%s\n+\n%s\n" % (n, s, "I" * len(s)) for n, s in zip(names[half:], qs[half:])))
    mers, qseqs = np.zeros(R.n_ref, dtype=np.uint32), np.zeros(R.n_ref, dtype=np.uint32)
    n_per, t_cov = R.write_batch(qs, mers, qseqs)
    want = ["".join("%d\t%d\t%d\t%s\n" % (n_per[i], t_cov[i], len(qs[i]), names[i]) for i in range(len(qs))).encode(),   # :262
            R.per_base_text(mers, ref_names), R.per_base_text(qseqs, ref_names)]
    assert (b"# chr3\n" in want[1] and b"# chr2\n" not in want[1]) if multi else b"#" not in want[1]
    assert want[1] != want[2] and len(want[1]) > 10000
    assert run_front_end(tmp_path, tmp_path / "ref.meryl", tmp_path / "ref.fa", [tmp_path / "all.fa"], "one") == want
    # two query files = their concatenation; batches of a few sequences each change nothing
    assert run_front_end(tmp_path, tmp_path / "ref.meryl", tmp_path / "ref.fa", [tmp_path / "a.fa", tmp_path / "b.fq"], "two",
                         {"MGC_POSLOOKUP_BATCH": "3000"}) == want
