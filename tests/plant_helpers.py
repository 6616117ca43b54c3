"""Planting sub-buckets of a known size next to filler reads, and comparing a device count with the oracle (shared by
test_count_structured_keys.py and test_count_huge_edges.py; the comparison needs a GPU, the rest is numpy)."""
import numpy as np

import structured_helpers as sh

# ---- the filler reads and what they leave free ----

_FILLER, _OCCUPIED, _SUFFIXES = {}, {}, {}


def filler(oracle_lib, k):
    """the stream-kernel test's reads: 4.5 Mbases at ~1x, so that the judged plan (fifteen-bit histogram, narrowed files) is on"""
    if k not in _FILLER:
        _FILLER[k] = oracle_lib.synth_reads(k, 4_000_000, 0, 30_000).tobytes().decode()
    return _FILLER[k]


def _ids(whi, wlo, low):
    """sub-bucket numbers (file bits included) of k-mers given as 64-bit halves: kmer >> low"""
    if low >= 64:
        return whi >> np.uint64(low - 64)
    return (whi << np.uint64(64 - low)) | (wlo >> np.uint64(low))


def occupied(oracle_lib, k, low, modes):
    """per mode: the sorted sub-bucket numbers of the filler's distinct k-mers and the running sum of their counts"""
    out = []
    for mode in modes:
        key = (k, low, mode)
        if key not in _OCCUPIED:
            whi, wlo, wcn, _ = oracle_lib.count_brute(filler(oracle_lib, k), k, mode)
            _OCCUPIED[key] = (_ids(whi, wlo, low), np.concatenate([[0], np.cumsum(wcn.astype(np.int64))]))   # (k-mers ascending: so are the numbers)
            if low < 32:
                _SUFFIXES[key] = (wlo & np.uint64((1 << low) - 1)).astype(np.uint32)
        out.append(_OCCUPIED[key])
    return out


def stray_suffixes(oracle_lib, k, low, mode, rng_ids):
    """the suffixes (below 32 bits) of the filler's k-mers inside the sub-buckets [first, end): a planted suffix must not be one of them"""
    ids, _ = occupied(oracle_lib, k, low, (mode,))[0]
    l, r = np.searchsorted(ids, np.uint64(rng_ids[0]), "left"), np.searchsorted(ids, np.uint64(rng_ids[1]), "left")
    return _SUFFIXES[(k, low, mode)][l:r].astype(np.int64)


def id_range(pre, min_top):
    """the sub-bucket numbers [first, end) whose k-mers begin with pre"""
    shift = (6 + min_top) - 2 * len(pre)
    v = sh.encode(pre)
    return (v << shift, (v + 1) << shift) if shift >= 0 else (v >> -shift, (v >> -shift) + 1)


def strays(occ, rng_ids):
    """filler k-mers (instances) inside the sub-buckets [first, end), the most over the modes"""
    worst = 0
    for ids, csum in occ:
        l, r = np.searchsorted(ids, np.uint64(rng_ids[0]), "left"), np.searchsorted(ids, np.uint64(rng_ids[1]), "left")
        worst = max(worst, int(csum[r] - csum[l]))
    return worst


def stray_kmers(occ_mode, rng_ids):
    """(instances, distinct k-mers) of the filler inside the sub-buckets [first, end) in ONE mode (an entry of occupied())"""
    ids, csum = occ_mode
    l, r = np.searchsorted(ids, np.uint64(rng_ids[0]), "left"), np.searchsorted(ids, np.uint64(rng_ids[1]), "left")
    return int(csum[r] - csum[l]), int(r - l)


def pick_prefix(head, n_bases, min_top, occ, rng, max_strays=0):
    """head + random bases (n_bases in all) such that the sub-buckets of k-mers beginning with it hold at most max_strays filler
    k-mers: a planted sub-bucket then has exactly the size -- and the table -- its case is built for.  Returns (prefix, strays)."""
    for _ in range(100_000):
        pre = head + "".join(sh.BASES[i] for i in rng.integers(0, 4, n_bases - len(head)))
        n = strays(occ, id_range(pre, min_top))
        if n <= max_strays:
            return pre, n
    raise AssertionError("no prefix %s... with at most %d filler k-mers" % (head, max_strays))


def plant(pre, tails, n_inst, rng):
    """n_inst reads of one k-mer each: every tail once, the rest drawn from them, shuffled"""
    m = len(tails)
    assert n_inst >= m
    picks = np.concatenate([np.arange(m), rng.integers(0, m, n_inst - m)])
    rng.shuffle(picks)
    return ".".join(pre + tails[int(i)] for i in picks) + "."


def count_and_compare(ops, oracle_lib, text, k, mode):
    """the device count of text against count_brute, exactly; returns (oracle k-mers hi, lo, counts, profile)"""
    from meryl_amd import capi
    cfg = capi.configure(k, len(text), 1 << 30, mode)
    cfg.use_simple = 0
    with ops.Session(cfg) as s:
        s.set_profiling(True)
        s.push_bases(text, end_of_sequence=False)
        s.count()
        klo, khi, counts, _ = s.result_wide()
        prof = s.profile()
    whi, wlo, wcn, _ = oracle_lib.count_brute(text, k, mode)
    print("mode %d: %d distinct k-mers on the device, %d in the oracle; stream_files %d, stream_retries %d"
          % (mode, len(klo), len(wlo), prof.stream_files, prof.stream_retries))
    assert len(klo) == len(wlo), "%d k-mers missing from the device result (%d against the oracle's %d)" % (len(wlo) - len(klo), len(klo), len(wlo))
    assert np.array_equal(klo, wlo) and np.array_equal(khi, whi) and np.array_equal(counts, wcn)
    return whi, wlo, wcn, prof


def subbucket(whi, wlo, wcn, low, ids):
    """(keys, distinct k-mers) of the sub-buckets [first, end) in the oracle's result"""
    got = _ids(whi, wlo, low)
    sel = (got >= np.uint64(ids[0])) & (got < np.uint64(ids[1]))
    return int(wcn[sel].sum()), int(sel.sum())
