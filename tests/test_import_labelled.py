"""meryl-import -labelwidth on the device: text `kmer value label` (the meryl 2 dialect) -> labelled database.

Expected results come from a model inside this file: a plain-Python line parser that restates the reference's
src/meryl2-import/meryl-import.C -- lines split at blanks, tabs and CR, empty lines skipped (:199-206); `value=<n>` /
`label=<n>` first words set the persistent value / label (:210-218); any other first word is a k-mer, its last k bases
(:222-223), with an optional value word (:225-228) and label word (:230-233); canonical / forward / reverse (:235-246) --
with numbers as decodeInteger reads them (documentation/source/reference.rst:615-617), the persistent value starting at 1
and the persistent label at 0.  Equal k-mers: values summed in uint32, labels summed modulo 2^lw
(`_labels[...] += getLabel()`, src/meryl2/merylCountArray.C:381-400, of which the writer stores the low lw bits).
For the bytes the expected result is the HOST writer meryl_amd.db.Writer(path, k, 6, label_size=lw) fed that model's blocks
(wPrefix = 6, meryl-import.C:158)."""
import os
import subprocess

import numpy as np
import pytest

import import_helpers
from import_helpers import assert_same_dirs, pick, prefixes, rand_kmer, with_batch

pytestmark = pytest.mark.gpu

W_PREFIX = 6
LETTERS = np.frombuffer(b"ACTG", dtype=np.uint8)          # code -> letter
M32 = 0xFFFFFFFF


# ---- the model -------------------------------------------------------------------------------------------------------
def decode_integer(word):
    """reference.rst:615-617: 123 / 123d, <hex>h, <octal>o, <binary>b; the last byte decides"""
    base = {"h": 16, "o": 8, "b": 2, "d": 10}.get(word[-1])
    return int(word, 10) if base is None else int(word[:-1], base)


def model_parse(text, k, mode, pval=1, plab=0):
    """-> ([(k-mer, value, label)] in input order, persistent value, persistent label after the text)"""
    out = []
    for line in text.split("\n"):
        words = [w for w in line.replace("\r", " ").replace("\t", " ").split(" ") if w]
        if not words:
            continue
        if words[0].startswith("value="):
            pval = decode_integer(words[0][6:])
            continue
        if words[0].startswith("label="):
            plab = decode_integer(words[0][6:])
            continue
        out.append((pick(words[0], k, mode), decode_integer(words[1]) if len(words) > 1 else pval,
                    decode_integer(words[2]) if len(words) > 2 else plab))
    return out, pval, plab


def model_sums(records, lw):
    """-> lo, hi, values (uint32), labels (uint64): k-mers ascending, values summed mod 2^32, labels mod 2^lw"""
    acc = {}
    for key, v, l in records:
        a = acc.get(key, (0, 0))
        acc[key] = ((a[0] + v) & M32, (a[1] + l) & ((1 << lw) - 1))
    keys = sorted(acc)
    lo = np.array([x & 0xFFFFFFFFFFFFFFFF for x in keys], dtype=np.uint64)
    hi = np.array([x >> 64 for x in keys], dtype=np.uint64)
    return lo, hi, np.array([acc[x][0] for x in keys], dtype=np.uint32), np.array([acc[x][1] for x in keys], dtype=np.uint64)


def host_write(path, lo, hi, cn, lab, k, lw):
    from meryl_amd import db
    w_data = 2 * k - W_PREFIX
    starts = np.searchsorted(prefixes(lo, hi, k, W_PREFIX), np.arange(0, (1 << W_PREFIX) + 1, dtype=np.uint64))
    mlo = np.uint64((1 << w_data) - 1) if w_data < 64 else np.uint64(0xFFFFFFFFFFFFFFFF)
    mhi = np.uint64((1 << (w_data - 64)) - 1) if w_data > 64 else np.uint64(0)
    w = db.Writer(path, k, W_PREFIX, label_size=lw)
    for p in range(1 << W_PREFIX):
        s, e = int(starts[p]), int(starts[p + 1])
        w.add_block(p, lo[s:e] & mlo, cn[s:e], (hi[s:e] & mhi) if w_data > 64 else None, labels=lab[s:e])
    w.close()


def read_db(path):
    return import_helpers.read_db(path, labels=True)


def assert_db_equals(path, lo, hi, cn, lab, k, lw):
    glo, ghi, gcn, glab, hv, ho, label_size = read_db(path)
    assert label_size == lw
    assert glo.size == lo.size, (glo.size, lo.size)
    assert np.array_equal(glo, lo) and np.array_equal(gcn, cn) and np.array_equal(glab, lab)
    if k > 32:
        assert np.array_equal(ghi, hi)
    wv, wo = np.unique(cn, return_counts=True)
    assert np.array_equal(hv, wv.astype(np.uint64)) and np.array_equal(ho, wo.astype(np.uint64))


# ---- inputs ----------------------------------------------------------------------------------------------------------
def number(rng, v):
    """v in one of the forms decodeInteger reads, now and then with leading zeros"""
    u = rng.random()
    zeros = "0" * int(rng.integers(1, 4)) if rng.random() < 0.25 else ""
    if u < 0.4:
        return zeros + "%d" % v
    if u < 0.5:
        return zeros + "%dd" % v
    if u < 0.7:
        return zeros + ("%xh" % v if rng.random() < 0.5 else "%Xh" % v)
    if u < 0.85:
        return zeros + "%oo" % v
    return zeros + "{:b}b".format(v)


def rand_label(rng, lw):
    return int(rng.integers(0, 1 << lw)) if lw < 63 else int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(0, 2))


def messy_text(rng, k, lw, n_records=1200, pool=350, assign_until=0.6):
    """Shuffled records over a small pool (well above 30 % repeats); lines of one, two, three and four words; `value=` and
    `label=` lines (only in the first `assign_until` of the lines, the first of each after some records that use the defaults);
    numbers in all four bases with leading zeros; blank lines, CRLF, tabs and runs of blanks, lower case, words longer than
    k; a k-mer whose values sum to 0; no final newline."""
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
        line = lead + w                                                   # one word: persistent value and label
        if u < 0.25:
            if rng.random() < 0.3:
                line += sep.replace("\t", " ")                           # trailing blanks, still no second word
        else:
            x = rng.random()
            v = 0 if x < 0.08 else int(rng.integers(1, 2000)) if x < 0.95 else int(rng.integers(2 ** 31, 2 ** 32))
            line += sep + number(rng, v)                                  # two words: persistent label
            if u >= 0.5:
                line += sep + number(rng, rand_label(rng, lw))            # three words
                if u >= 0.85:
                    line += sep + ["junk", "42", "label=1", "ACGT"][int(rng.integers(0, 4))]   # a fourth word is ignored
        lines.append(line)
    lines.append(zero_only + "\t0\t1")
    lines.append(zero_only.lower() + " 000 0b x")
    order = rng.permutation(len(lines))
    lines = [lines[i] for i in order]
    zone = max(8, int(len(lines) * assign_until))
    first = int(zone * 0.15)
    at = sorted(set([first, first + 3] + [int(x) for x in rng.integers(first, zone, 10)]), reverse=True)
    top = (1 << lw) - 1
    assigns = ["label=%s" % number(rng, top), "value=7", "value=0", " label=1 ", "value=4294967295", "label=0\tignored",
               "value=0005", "\tlabel=%s" % number(rng, rand_label(rng, lw)), "value=ffh more words", "label=1b", "value=21d",
               "label=%s" % number(rng, rand_label(rng, lw))]
    for j, pos in enumerate(at):
        lines.insert(pos, assigns[j % len(assigns)])
    for pos in sorted((int(x) for x in rng.integers(0, len(lines), 25)), reverse=True):
        lines.insert(pos, ["", "   ", "\t", " \t "][int(rng.integers(0, 4))])
    text = "\n".join(ln + ("\r" if rng.random() < 0.33 else "") for ln in lines)   # CRLF on a third; nothing after the last line
    assert not text.endswith("\n")
    return text


def check_messy(text):
    """the properties test 1 asks of its input"""
    counts = set()
    seen_assign = {"value=": False, "label=": False}
    defaults_before = {"value=": 0, "label=": 0}
    for line in text.split("\n"):
        words = line.replace("\r", " ").replace("\t", " ").split()
        if not words:
            continue
        for a in seen_assign:
            if words[0].startswith(a):
                seen_assign[a] = True
                break
        else:
            counts.add(min(len(words), 4))
            if len(words) < 2 and not seen_assign["value="]:
                defaults_before["value="] += 1
            if len(words) < 3 and not seen_assign["label="]:
                defaults_before["label="] += 1
    assert counts == {1, 2, 3, 4}
    assert all(seen_assign.values()) and all(defaults_before.values())
    body = text.replace("\t", " ")
    for suffix in ("h ", "o ", "b ", "d "):
        assert suffix in body
    assert "\r\n" in text and "\t" in text and "   " in text and " 00" in body


@pytest.fixture(scope="module")
def clis(native_lib):
    from meryl_amd import build
    return build.build_cli(), build.build_import_cli()


# ---- 1. bytes ----------------------------------------------------------------------------------------------------------
CASES = [(k, lw, (i + j) % 3) for i, k in enumerate((6, 21, 32, 33, 64)) for j, lw in enumerate((1, 8, 64))]


@pytest.mark.parametrize("k,lw,mode", CASES, ids=["k%d-lw%d-%s" % (k, lw, ("canonical", "forward", "reverse")[m]) for k, lw, m in CASES])
def test_bytes_equal_the_host_writers(native_lib, tmp_path, k, lw, mode):
    from meryl_amd import kmer_import
    rng = np.random.default_rng(1000 * k + lw)
    text = messy_text(rng, k, lw)
    check_messy(text)
    recs, _, _ = model_parse(text, k, mode)
    lo, hi, cn, lab = model_sums(recs, lw)
    assert len(recs) >= 1.3 * lo.size and (cn == 0).any() and len(recs) >= 1200
    assert lab.any() and int(lab.max()) < (1 << lw)
    host_write(str(tmp_path / "host"), lo, hi, cn, lab, k, lw)
    info = kmer_import.import_text(text, k, str(tmp_path / "dev"), mode=mode, host_threads=4, label_width=lw)
    assert info["n_records"] == len(recs) and info["n_distinct"] == lo.size and info["n_batches"] == 1
    assert info["n_lines"] == text.count("\n") + 1
    assert_same_dirs(str(tmp_path / "host"), str(tmp_path / "dev"))
    assert_db_equals(str(tmp_path / "dev"), lo, hi, cn, lab, k, lw)


# ---- 2. the parser alone, in chunks ------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,mode", [(21, 0), (51, 2)])
def test_parser_alone_in_four_chunks(native_lib, k, mode):
    """both persistent words and the record slots across chunk boundaries, records in input order"""
    import torch
    from meryl_amd import kmer_import
    lw = 8
    rng = np.random.default_rng(77 + k)
    # chunk 1 ends in a `label=` line, chunk 2 in a `value=` line: the records that depend on them open chunks 2 and 3
    parts = [messy_text(rng, k, lw, n_records=700) + "\nlabel=10100101b\n",
             "\n".join(rand_kmer(rng, k) + ["", " 5", "\t9 "][i % 3] for i in range(40)) + "\n" + messy_text(rng, k, lw, n_records=700, assign_until=0.0)
             .replace("label=", "value=") + "\nvalue=77o\n",
             "\n".join(rand_kmer(rng, k) + ["", "", " 5 1"][i % 3] for i in range(40)) + "\n" + messy_text(rng, k, lw, n_records=700) + "\n",
             messy_text(rng, k, lw, n_records=700, assign_until=0.0)]
    parser = kmer_import.Parser(k, mode, label_width=lw)
    pval, plab, lines = 1, 0, 0
    for i, part in enumerate(parts):
        want, pval_after, plab_after = model_parse(part, k, mode, pval, plab)
        if i == 1:                                   # the dependence is real: records of this chunk take the label of the last one
            assert plab == 0b10100101 and want[0][2] == plab and want[1][2] == plab
        if i == 2:
            assert pval == 0o77 and want[0][1] == pval and want[0][2] == plab
        keys, vals, labs, res = parser.parse(torch.frombuffer(bytearray(part.encode()), dtype=torch.uint8).cuda())
        assert res.bad_kind == 0
        lines += res.n_lines
        assert res.n_records == len(want)
        assert res.persistent_value == pval_after and parser.persistent_label == plab_after
        kk = keys.cpu().numpy().view(np.uint64)
        vv = vals.cpu().numpy().view(np.uint32)
        ll = labs.cpu().numpy().view(np.uint64)
        got = [((int(kk[j]) if k <= 32 else int(kk[j, 0]) | (int(kk[j, 1]) << 64)), int(vv[j]), int(ll[j])) for j in range(kk.shape[0])]
        assert got == want
        pval, plab = pval_after, plab_after
        # an empty chunk is MGC_OK, holds nothing and moves nothing
        keys, vals, labs, res = parser.parse(torch.empty(0, dtype=torch.uint8, device="cuda"))
        assert res.n_lines == 0 and res.n_records == 0 and keys.shape[0] == 0 and vals.numel() == 0 and labs.numel() == 0
        assert res.persistent_value == pval and parser.persistent_label == plab
    text = "".join(parts)
    assert lines == text.count("\n") + 1


# ---- 3. segments across workgroups, and both wraps ---------------------------------------------------------------------
def codes_to_keys(codes):
    """codes: uint8[n, k] (A0 C1 T2 G3), k <= 32 -> uint64 of the canonical k-mer"""
    return import_helpers.codes_to_keys(codes, 0)[0]


def fixed_width_text(codes, values, vdigits, labels, ldigits):
    """`KMER<TAB>value<TAB>label<LF>` rows of one width (zero-padded decimals), as a uint8 matrix (vectorised)"""
    n, k = codes.shape
    m = np.empty((n, k + 1 + vdigits + 1 + ldigits + 1), np.uint8)
    m[:, :k] = LETTERS[codes]
    m[:, k] = 9
    m[:, k + 1 + vdigits] = 9
    for col0, digits, x in ((k + 1, vdigits, values), (k + 2 + vdigits, ldigits, labels)):
        v = x.astype(np.uint64)
        for d in range(digits):
            m[:, col0 + digits - 1 - d] = (48 + (v % np.uint64(10))).astype(np.uint8)
            v = v // np.uint64(10)
    m[:, -1] = 10
    return m


@pytest.mark.parametrize("lw", [8, 64])
def test_long_segment_wraps_across_workgroups(native_lib, tmp_path, lw):
    from meryl_amd import kmer_import
    k, n_hot, n_other = 21, 200_000, 100_000
    rng = np.random.default_rng(3 + lw)
    others = rng.integers(0, 4, (n_other, k)).astype(np.uint8)
    hot = rng.integers(0, 4, (1, k)).astype(np.uint8)
    codes = np.concatenate([np.repeat(hot, n_hot, axis=0), others])
    values = np.concatenate([np.full(n_hot, 30_000, np.uint64), rng.integers(1000, 10000, n_other).astype(np.uint64)])
    if lw == 8:
        hot_labels = np.full(n_hot, 255, np.uint64)
        other_labels = rng.integers(0, 256, n_other).astype(np.uint64)
    else:
        hot_labels = (np.uint64(1 << 63) - rng.integers(0, 1000, n_hot).astype(np.uint64))
        other_labels = rng.integers(0, 1 << 63, n_other).astype(np.uint64) * np.uint64(2) + np.uint64(1)
    labels = np.concatenate([hot_labels, other_labels])
    order = rng.permutation(codes.shape[0])
    codes, values, labels = codes[order], values[order], labels[order]
    keys = codes_to_keys(codes)
    ulo, inv = np.unique(keys, return_inverse=True)
    sums = np.zeros(ulo.size, np.uint32)
    np.add.at(sums, inv, values.astype(np.uint32))
    lsum = np.zeros(ulo.size, np.uint64)
    np.add.at(lsum, inv, labels)                                     # uint64: wraps modulo 2^64
    if lw < 64:
        lsum &= np.uint64((1 << lw) - 1)
    # both wraps, in the model, before the device is asked
    at = int(np.searchsorted(ulo, codes_to_keys(hot)[0]))
    assert int(sums[at]) == (n_hot * 30_000) % (1 << 32) == 1705032704 and n_hot * 30_000 > 1 << 32
    want_l = sum(int(x) for x in hot_labels) % (1 << lw)
    assert int(lsum[at]) == want_l and sum(int(x) for x in hot_labels) >= (1 << lw) * 1000
    if lw == 8:
        assert want_l == (n_hot * 255) % 256 == 192
    text = fixed_width_text(codes, values, 5, labels, 20 if lw == 64 else 3).reshape(-1)
    info = kmer_import.import_text(text, k, str(tmp_path / "dev"), label_width=lw)
    assert info["n_records"] == n_hot + n_other and info["n_lines"] == n_hot + n_other and info["n_distinct"] == ulo.size
    assert_db_equals(str(tmp_path / "dev"), ulo, np.zeros(ulo.size, np.uint64), sums, lsum, k, lw)


# ---- 4. sort_triples alone ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,begin_bit,end_bit", [(1, 0, 64), (1, 3, 37), (2, 0, 128), (2, 5, 100)])
def test_sort_triples_alone(native_lib, kw, begin_bit, end_bit):
    """equal keys keep their input order: the labels number the records; a sub-range of the bits; numpy's stable argsort"""
    import torch
    from meryl_amd import kmer_import
    n, distinct = 50_000, 500
    rng = np.random.default_rng(kw * 1000 + end_bit)
    pool_lo = rng.integers(0, 1 << 64, distinct, dtype=np.uint64, endpoint=False)
    pool_hi = rng.integers(0, 1 << 64, distinct, dtype=np.uint64, endpoint=False) if kw == 2 else np.zeros(distinct, np.uint64)
    idx = rng.integers(0, distinct, n)
    lo, hi = pool_lo[idx], pool_hi[idx]
    vals = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    labs = np.arange(n, dtype=np.uint64)
    mask = (1 << (end_bit - begin_bit)) - 1
    digits = [(((int(a) | (int(b) << 64)) >> begin_bit) & mask) for a, b in zip(lo, hi)]
    dlo = np.array([d & 0xFFFFFFFFFFFFFFFF for d in digits], np.uint64)
    dhi = np.array([d >> 64 for d in digits], np.uint64)
    order = np.lexsort((dlo, dhi))                                   # stable
    host_keys = lo if kw == 1 else np.stack([lo, hi], axis=1)
    dk = torch.from_numpy(np.ascontiguousarray(host_keys).view(np.int64)).cuda()
    dv = torch.from_numpy(vals.view(np.int32)).cuda()
    dl = torch.from_numpy(labs.view(np.int64)).cuda()
    sk, sv, sl = kmer_import.sort_triples(dk, dv, dl, begin_bit, end_bit)
    assert np.array_equal(sl.cpu().numpy().view(np.uint64), labs[order])
    assert np.array_equal(sk.cpu().numpy().view(np.uint64), host_keys[order])
    assert np.array_equal(sv.cpu().numpy().view(np.uint32), vals[order])
    if begin_bit == 0:                                               # ... and reduce_triples over the fully sorted triples
        rk, rv, rl = kmer_import.reduce_triples(sk, sv, sl, 17)
        slo, shi = lo[order], hi[order]
        head = np.ones(n, bool)
        head[1:] = (slo[1:] != slo[:-1]) | (shi[1:] != shi[:-1])
        starts = np.flatnonzero(head)
        assert rk.shape[0] == starts.size <= distinct
        assert np.array_equal(rk.cpu().numpy().view(np.uint64), host_keys[order][starts])
        assert np.array_equal(rv.cpu().numpy().view(np.uint32), np.add.reduceat(vals[order], starts, dtype=np.uint32))
        assert np.array_equal(rl.cpu().numpy().view(np.uint64), np.add.reduceat(labs[order], starts) & np.uint64((1 << 17) - 1))


@pytest.mark.parametrize("lw", [1, 64])
@pytest.mark.parametrize("pattern", ["equal", "random"])
@pytest.mark.parametrize("kw", [1, 2])
@pytest.mark.parametrize("n", [1, 2047, 2048, 2049, 4097])
def test_reduce_triples_at_tile_edges(native_lib, n, kw, pattern, lw):
    """a reduce tile holds 2048 triples: one short of it, exactly it, one more, and two tiles and one; a segment over all of them
    (equal) and segments of about three; np.add.at in uint32 and in uint64 modulo 2^lw"""
    import torch
    from meryl_amd import kmer_import
    rng = np.random.default_rng(n * 7 + kw + lw)
    if pattern == "equal":
        lo, hi = np.full(n, 0x123456789ABCDEF, np.uint64), np.full(n, 0x2A if kw == 2 else 0, np.uint64)
    else:
        distinct = max(1, n // 3)
        pool_lo = rng.integers(0, 1 << 64, distinct, dtype=np.uint64, endpoint=False)
        pool_hi = rng.integers(0, 1 << 64, distinct, dtype=np.uint64, endpoint=False) if kw == 2 else np.zeros(distinct, np.uint64)
        idx = rng.integers(0, distinct, n)
        order = np.lexsort((pool_lo[idx], pool_hi[idx]))
        lo, hi = pool_lo[idx][order], pool_hi[idx][order]
    vals = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    labs = rng.integers(0, 1 << 64, n, dtype=np.uint64, endpoint=False)
    head = np.ones(n, bool)
    head[1:] = (lo[1:] != lo[:-1]) | (hi[1:] != hi[:-1])
    seg = np.cumsum(head) - 1
    want_v, want_l = np.zeros(int(seg[-1]) + 1, np.uint32), np.zeros(int(seg[-1]) + 1, np.uint64)
    np.add.at(want_v, seg, vals)
    np.add.at(want_l, seg, labs)                                     # uint64: wraps modulo 2^64
    if lw < 64:
        want_l &= np.uint64((1 << lw) - 1)
    host_keys = lo if kw == 1 else np.stack([lo, hi], axis=1)
    rk, rv, rl = kmer_import.reduce_triples(torch.from_numpy(np.ascontiguousarray(host_keys).view(np.int64)).cuda(),
                                            torch.from_numpy(vals.view(np.int32)).cuda(), torch.from_numpy(labs.view(np.int64)).cuda(), lw)
    assert rk.shape[0] == want_v.size
    assert np.array_equal(rk.cpu().numpy().view(np.uint64), host_keys[head])
    assert np.array_equal(rv.cpu().numpy().view(np.uint32), want_v) and np.array_equal(rl.cpu().numpy().view(np.uint64), want_l)


# ---- 5. batches --------------------------------------------------------------------------------------------------------
def test_batches(native_lib, tmp_path):
    from meryl_amd import kmer_import
    k, lw, mode, batch = 21, 8, 0, 4096
    rng = np.random.default_rng(1000 * k + lw)
    text = messy_text(rng, k, lw)                                    # the text of test 1
    # a `label=` line governs a label-less record more than a batch further on (a batch holds at most `batch` bytes)
    at, last_label, far = 0, None, 0
    for line in text.split("\n"):
        words = line.replace("\r", " ").replace("\t", " ").split()
        if words and words[0].startswith("label="):
            last_label = at
        elif words and not words[0].startswith("value=") and len(words) < 3 and last_label is not None and at - last_label > batch:
            far += 1
        at += len(line) + 1
    assert far > 20
    one = kmer_import.import_text(text, k, str(tmp_path / "one"), mode=mode, label_width=lw)
    assert one["n_batches"] == 1
    with with_batch(batch):
        many = kmer_import.import_text(text, k, str(tmp_path / "many"), mode=mode, label_width=lw)
    assert many["n_batches"] >= len(text) // batch > 5, many
    assert many["n_records"] == one["n_records"] and many["n_lines"] == one["n_lines"] and many["n_distinct"] == one["n_distinct"]
    assert_same_dirs(str(tmp_path / "one"), str(tmp_path / "many"))
    lo, hi, cn, lab = model_sums(model_parse(text, k, mode)[0], lw)
    assert_db_equals(str(tmp_path / "many"), lo, hi, cn, lab, k, lw)


# ---- 6. refusals -------------------------------------------------------------------------------------------------------
GOOD = "ACGTACGTACGTACGTACGTA"
REFUSALS = [
    ("label_bit_at_lw", 3, GOOD + " 4 8", "label"),
    ("label_12x", 8, GOOD + " 4 12x", "label"),
    ("label_2b", 8, GOOD + " 4 2b", "label"),
    ("label_123k", 64, GOOD + " 4 123k", "label"),
    ("value_2_32", 8, GOOD + " 4294967296 1", "value"),
    ("value_assign_empty", 8, "value=", "assign"),
    ("label_assign_zz", 8, "label=zz", "assign"),
    ("hash_line", 8, "#5", "base"),
    ("short", 8, GOOD[:-1] + " 4 1", "short"),
]


@pytest.mark.parametrize("name,lw,line,kind", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(native_lib, tmp_path, name, lw, line, kind):
    from meryl_amd import kmer_import
    rng = np.random.default_rng(len(name))
    good = ["%s %d %d" % (rand_kmer(rng, 21), int(rng.integers(1, 100)), int(rng.integers(0, 1 << min(lw, 3)))) for _ in range(3000)]
    good[5] = ""                                                     # blank, `value=` and `label=` lines count as lines
    good[9] = "label=1"
    good[11] = "value=3"
    # a second, later bad line of another kind must not be the one reported
    later = GOOD + " notanumber" if kind != "value" else GOOD + " 1 notanumber"
    for bad_at, batch in ((2, None), (400, None), (2500, 4096)):     # the first tile, beyond it, beyond the first batches
        lines = good[:bad_at] + [line] + good[bad_at:]
        lines.insert(bad_at + 300, later)
        text = "\n".join(lines) + "\n"
        offset = len("\n".join(lines[:bad_at])) + 1
        out = tmp_path / ("o_%d.meryl" % bad_at)
        with pytest.raises(kmer_import.ImportRefused) as e:
            if batch:
                assert offset > 5 * batch
                with with_batch(batch):
                    kmer_import.import_text(text, 21, str(out), label_width=lw)
            else:
                assert (offset > 4096) == (bad_at == 400)
                kmer_import.import_text(text, 21, str(out), label_width=lw)
        assert e.value.line == bad_at + 1 and e.value.kind == kind, (e.value.line, e.value.kind, str(e.value))
        assert ("line %d:" % (bad_at + 1)) in str(e.value)
        assert not os.path.exists(out)


def test_numbers_at_the_edges_are_accepted(native_lib, tmp_path):
    from meryl_amd import kmer_import
    text = "\n".join([GOOD + " 4294967295 18446744073709551615", GOOD + " 0000000000000000000001 1", GOOD + " ffffffffh FFFFFFFFFFFFFFFFh",
                      GOOD + " 37777777777o 1777777777777777777777o", GOOD + " " + "1" * 32 + "b " + "1" * 64 + "b", "label=18446744073709551615d",
                      "value=00d", GOOD])
    recs, pval, plab = model_parse(text, 21, 0)
    assert [r[1] for r in recs] == [M32, 1, M32, M32, M32, 0] and plab == (1 << 64) - 1 and pval == 0
    lo, hi, cn, lab = model_sums(recs, 64)
    info = kmer_import.import_text(text, 21, str(tmp_path / "o.meryl"), label_width=64)
    assert info["n_distinct"] == 1 and info["n_records"] == 6
    assert int(cn[0]) == (4 * M32 + 1) & M32 and int(lab[0]) == (5 * ((1 << 64) - 1) + 1) % (1 << 64)
    assert_db_equals(str(tmp_path / "o.meryl"), lo, hi, cn, lab, 21, 64)
    # one past either edge is refused
    for line, kind in ((GOOD + " 1 18446744073709551616", "label"), (GOOD + " 1 10000000000000000h", "label"),
                       (GOOD + " 100000000h", "value"), ("label=2000000000000000000000o", "assign"), ("value=4294967296", "assign"),
                       (GOOD + " 1 h", "label"), (GOOD + " d", "value"), (GOOD + " 1 1B", "label"), (GOOD + " 1 -1", "label")):
        with pytest.raises(kmer_import.ImportRefused) as e:
            kmer_import.import_text(GOOD + " 1 1\n" + line, 21, str(tmp_path / "r.meryl"), label_width=64)
        assert e.value.line == 2 and e.value.kind == kind, line
        assert not os.path.exists(tmp_path / "r.meryl")


# ---- 7. round trip through the tools -----------------------------------------------------------------------------------
def test_round_trip_print_import(clis, tmp_path):
    from meryl_amd import db
    meryl, importer = clis
    rng = np.random.default_rng(21)
    genome = rng.integers(0, 4, 60_000)
    for name, lo_, hi_ in (("a.fa", 0, 40_000), ("b.fa", 20_000, 60_000)):         # the middle third is in both samples
        with open(tmp_path / name, "w") as f:
            for i in range(2000):
                s = int(rng.integers(lo_, hi_ - 150))
                f.write(">r%d\n%s\n" % (i, "".join("ACGT"[c] for c in genome[s:s + 150])))
    ab, ab2 = str(tmp_path / "ab.meryl"), str(tmp_path / "ab2.meryl")
    subprocess.run([meryl, "-Q", "-l", "2", "k=21", "memory=1", "union-sum", "label=or", "[count", "label=#1", str(tmp_path / "a.fa") + "]",
                    "[count", "label=#2", str(tmp_path / "b.fa") + "]", "output", ab], check=True, timeout=600)
    text = subprocess.run([meryl, "-Q", "print", ab], check=True, stdout=subprocess.PIPE, timeout=600).stdout.decode()
    rows = [ln.split("\t") for ln in text.splitlines()]
    assert len(rows) > 50_000 and all(len(r) == 3 for r in rows)
    assert {r[2] for r in rows} == {"01", "10", "11"}
    stdin = "".join("%s\t%s\t%sb\n" % (r[0], r[1], r[2]) for r in rows).encode()
    p = subprocess.run([importer, "-k", "21", "-labelwidth", "2", "-kmers", "-", "-output", ab2], input=stdin, capture_output=True, timeout=600)
    err = p.stderr.decode()
    assert p.returncode == 0, err
    assert ("Added %d kmers; incorrectly added 0 kmers." % len(rows)) in err and err.rstrip().endswith("Bye."), err
    want, got = read_db(ab), read_db(ab2)
    assert want[0].size == len(rows) and want[2].max() > 1 and set(np.unique(want[3]).tolist()) == {1, 2, 3}
    for g, w in zip(got, want):                                      # k-mers, values, labels, histogram, label size
        assert np.array_equal(g, w)
    assert len(os.listdir(ab2)) == 129
    # the imported database is a working leaf of the trees: its labels XOR the original's are 0 everywhere.  The constant is
    # given: label=xor alone starts from all ones (mgc_label_default_constant, merylCommandBuilder-isAssign.C:124-156)
    seen = []
    db.evaluate_labelled(("intersect", ab2, ab, {"label": ("xor", 0)}),
                         on_slice=lambda ff, lo, hi, vals, labs: seen.append((lo.size, labs.copy())))
    assert sum(n for n, _ in seen) == len(rows)
    assert not np.concatenate([l for _, l in seen]).any()


# ---- 8. empty inputs ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lw", [1, 8, 64])
def test_empty_input_gives_an_empty_database(native_lib, tmp_path, lw):
    from meryl_amd import kmer_import
    none = np.zeros(0, np.uint64)
    host_write(str(tmp_path / "host"), none, none, np.zeros(0, np.uint32), none, 21, lw)
    for i, text in enumerate(("", "\n\n  \n", "label=1\n")):
        out = str(tmp_path / ("e%d.meryl" % i))
        info = kmer_import.import_text(text, 21, out, label_width=lw)
        assert info["n_records"] == 0 and info["n_distinct"] == 0
        got = read_db(out)
        assert got[0].size == 0 and got[6] == lw
        assert_same_dirs(str(tmp_path / "host"), out)
