"""A host model of the count stage's plan for GIGANTIC sub-buckets (pure numpy, no GPU).

A sub-bucket above 65536 keys does not go through the persistent count kernels but through launch_huge in
meryl_amd/csrc/mgc_finish.hip: huge_plan_kernel cuts it into equal slices, MODE 1 of hash_count_huge_kernel /
hash_count128_huge_kernel turns every slice into (suffix, count) pairs, MODE 2 merges the pairs, a slice with too many distinct
suffixes marks the sub-bucket dense and MODE 3 counts it by 64 quantile ranges of a sample; MODE 0 keeps the oversized sub-buckets
that are not cut.  Every function below is a copy of one line of that file, named in its comment.

What a test may CLAIM about the path a planted sub-bucket takes has to follow from its size n and the multiplicities of its
suffixes alone, in every order of the keys (the grouping passes keep input order only block by block) -- claims() derives exactly
those.  Two more claims are expected, not guaranteed; for them the module computes an upper bound of the probability that a
uniformly random order of the keys misses them (mode1_repass_log2_bound, empty_range_log2_bound).  A reordering that does not
look at the keys' values leaves a uniformly random order uniformly random.
"""
import math
from collections import namedtuple

import numpy as np

# constexpr u32 HUGE_SLICE = 32768, HUGE_SLICE_MIN = 65536, HUGE_WMAX = 8192, HUGE_RANGES = 64;
HUGE_SLICE, HUGE_SLICE_MIN, HUGE_WMAX, HUGE_RANGES = 32768, 65536, 8192, 64
HUGE_DENSE_DIV = 8                                # constexpr u32 HUGE_DENSE_DIV = 8;
HUGE_SAMPLE = 4096                                # constexpr u32 HUGE_SAMPLE = 4096;
# constexpr int HUGE_CAP32 = 4096 ...; HUGE_CAP64 = 2048 ...; HUGE_CAP128 = 2048 ...: the distinct suffixes one pass holds
HUGE_CAP32, HUGE_CAP64, HUGE_CAP128 = 4096, 2048, 2048

# The five families launch_oversized instantiates (kernel family, table capacity):
#   narrow32  NARROW32: launch_huge<Huge8<u32, u32>>                                 narrowed words, suffixes below 32 bits
#   whole32   WHOLE8, low_bits < 32: launch_huge<Huge8<u32, u64>>                    whole 8-byte keys, 32-bit entries
#   whole64   WHOLE8, low_bits >= 32: launch_huge<Huge8<u64, u64>>                   whole 8-byte keys, 64-bit entries
#   k96       K96: launch_huge<Huge16<wide, K96>>                                    12-byte records, suffixes up to / above 64 bits
#   k128      WHOLE16: launch_huge<Huge16<wide, K128>>                               16-byte keys
CAP = {"narrow32": HUGE_CAP32, "whole32": HUGE_CAP32, "whole64": HUGE_CAP64, "k96": HUGE_CAP128, "k128": HUGE_CAP128}


def huge_is_cut(n, huge_max=HUGE_SLICE_MIN):
    """return huge_max != 0 && n > huge_max && (n + HUGE_SLICE - 1) / HUGE_SLICE <= (u64)HUGE_WMAX;
    (huge_max = 0 -- MGC_HUGE_SLICES=0, or a file without a gigantic sub-bucket -- cuts nothing)"""
    return huge_max != 0 and n > huge_max and (n + HUGE_SLICE - 1) // HUGE_SLICE <= HUGE_WMAX


def huge_slices(n):
    """return (u32)((n + HUGE_SLICE - 1) / HUGE_SLICE);"""
    return (n + HUGE_SLICE - 1) // HUGE_SLICE


def huge_slice_len(n):
    """const u64 W = huge_slices(n); return (n + W - 1) / W;"""
    W = huge_slices(n)
    return (n + W - 1) // W


def slice_lengths(n):
    """MODE 1: off = slice_j * len; n64 = nall - off < len ? nall - off : len;   for slice_j = 0 .. W - 1"""
    W, ln = huge_slices(n), huge_slice_len(n)
    return [min(ln, n - j * ln) for j in range(W)]


def is_dense(distinct, n_slice):
    """MODE 1, after a slice's last pass: if (HUGE_DENSE_DIV * (out + D) > n64) -> gig_fail[cq] = 1"""
    return HUGE_DENSE_DIV * distinct > n_slice


def overflows(distinct, cap):
    """if (old == EMPTY && atomicAdd(&s_st[0], 1u) >= (u32)CAP) -> overflow: the insert that finds CAP suffixes already counted, so a pass
    holds exactly CAP distinct suffixes without one"""
    return distinct > cap


def sample_index(i, n):
    """huge_split_kernel: const u64 idx = (u64)(((u128)i * n) / HUGE_SAMPLE);"""
    return (i * n) // HUGE_SAMPLE


def splitters(sample_sorted, low_mask):
    """huge_split_kernel: range r ends at sorted sample[(r + 1) * (HUGE_SAMPLE / HUGE_RANGES) - 1]; the last one at low_mask"""
    step = HUGE_SAMPLE // HUGE_RANGES
    return [int(sample_sorted[(r + 1) * step - 1]) for r in range(HUGE_RANGES - 1)] + [low_mask]


def huge_range(split, r):
    """huge_range: hi = split[r]; if (r == 0) { lo = 0; return true; } if (prev >= hi) return false; lo = prev + 1; return true;
    Returns (lo, hi), or None for an empty range."""
    hi = split[r]
    if r == 0:
        return 0, hi
    if split[r - 1] >= hi:
        return None
    return split[r - 1] + 1, hi


# ---- the plan of a whole text, from the oracle's result ----

def subbucket_ids(whi, wlo, low):
    """sub-bucket numbers (file bits included) of k-mers given as 64-bit halves: kmer >> low"""
    whi, wlo = np.asarray(whi, dtype=np.uint64), np.asarray(wlo, dtype=np.uint64)
    if low >= 64:
        return whi >> np.uint64(low - 64)
    if low == 0:
        return wlo
    return (whi << np.uint64(64 - low)) | (wlo >> np.uint64(low))


Plan = namedtuple("Plan", "cut slices groups")      # groups: {sub-bucket number: (keys, distinct k-mers)} of those above HUGE_SLICE_MIN / 2


def expected_plan(whi, wlo, wcn, k, min_top, sliced=True):
    """huge_cut and huge_slices of a count whose files are grouped by 6 + min_top bits (low = 2k - 6 - min_top bits below the
    sub-bucket): the k-mers of the oracle's result (ascending) grouped by kmer >> low; a group is cut when huge_is_cut says so."""
    low = 2 * k - 6 - min_top
    ids = subbucket_ids(whi, wlo, low)
    assert np.all(ids[1:] >= ids[:-1])
    first = np.concatenate([[0], np.nonzero(ids[1:] != ids[:-1])[0] + 1, [len(ids)]])
    csum = np.concatenate([[0], np.cumsum(np.asarray(wcn, dtype=np.int64))])
    sizes = csum[first[1:]] - csum[first[:-1]]
    cut = slices = 0
    groups = {}
    for i in np.nonzero(sizes > HUGE_SLICE_MIN // 2)[0]:
        n = int(sizes[i])
        groups[int(ids[first[i]])] = (n, int(first[i + 1] - first[i]))
        if sliced and huge_is_cut(n):
            cut += 1
            slices += huge_slices(n)
    return Plan(cut, slices, groups)


# ---- what follows from (n, multiplicities) in every order of the keys ----

Claims = namedtuple("Claims", "n distinct cut slices cannot_be_dense must_be_dense mode0_must_repass mode1_must_repass "
                              "mode1_cannot_repass mode2_must_repass mode2_cannot_repass mode3_must_repass why")


def fewest_distinct(mults_desc, length):
    """the fewest distinct suffixes `length` keys can have: the heaviest suffixes first"""
    c = np.cumsum(mults_desc)
    return int(np.searchsorted(c, length, "left")) + 1


def claims(mults, cap, sliced=True):
    """mults: how often each distinct suffix of the sub-bucket occurs; cap: its family's table capacity."""
    m = np.sort(np.asarray(mults, dtype=np.int64))[::-1]
    n, d = int(m.sum()), len(m)
    cut = bool(sliced and huge_is_cut(n))
    why = []
    if not cut:
        why.append("n = %d %s: not cut, MODE 0" % (n, "<= %d" % HUGE_SLICE_MIN if n <= HUGE_SLICE_MIN else "with MGC_HUGE_SLICES=0"))
        m0 = overflows(d, cap)
        why.append("MODE 0 %s re-pass: %d distinct %s CAP = %d" % ("must" if m0 else "cannot", d, ">" if m0 else "<=", cap))
        return Claims(n, d, False, 0, True, False, m0, False, True, False, True, False, why)
    lens = slice_lengths(n)
    why.append("n = %d > %d: cut into %d slices of %s keys" % (n, HUGE_SLICE_MIN, len(lens), sorted(set(lens), reverse=True)))
    # cannot be dense: a slice sees at most all d distinct suffixes, and HUGE_DENSE_DIV * d <= its length for the shortest one
    cannot = not is_dense(d, min(lens))
    # must be dense: (a) if no slice were dense, d <= sum of the slices' distinct <= sum(len_j / 8) = n / 8;
    #                (b) a slice of len_j keys holds at least fewest_distinct(len_j) suffixes
    must = is_dense(d, n) or any(is_dense(fewest_distinct(m, ln), ln) for ln in lens)
    assert not (cannot and must)
    if cannot:
        why.append("cannot be dense: %d * %d distinct <= %d, the shortest slice" % (HUGE_DENSE_DIV, d, min(lens)))
    if must:
        why.append("must be dense: " + ("%d * %d distinct > n = %d, so some slice holds more than 1/%d of its keys distinct"
                                        % (HUGE_DENSE_DIV, d, n, HUGE_DENSE_DIV) if is_dense(d, n) else
                                        "a slice of %d keys holds at least %d distinct suffixes" % (lens[0], fewest_distinct(m, lens[0]))))
    if not cannot and not must:
        why.append("dense or merged: depends on the order of the keys (%d distinct)" % d)
    # a slice's passes: no more than d suffixes anywhere; a slice of len_j keys holds at least fewest_distinct(len_j)
    m1 = any(overflows(fewest_distinct(m, ln), cap) for ln in lens)
    m1no = not overflows(d, cap)
    if m1 or m1no:
        why.append("MODE 1 %s re-pass: %s" % ("must" if m1 else "cannot", "a slice of %d keys holds at least %d distinct suffixes > CAP = %d"
                                              % (lens[0], fewest_distinct(m, lens[0]), cap) if m1 else "%d distinct <= CAP = %d" % (d, cap)))
    m2 = cannot and overflows(d, cap)
    m2no = not overflows(d, cap)
    m3 = must and overflows(d, HUGE_RANGES * cap)
    if cannot:
        why.append("MODE 2 %s re-pass: the pairs hold %d distinct suffixes %s CAP = %d" % ("must" if m2 else "cannot", d, ">" if m2 else "<=", cap))
    if must:
        why.append("MODE 3 %s: %d distinct %s %d ranges * CAP = %d" % ("must re-pass in some range" if m3 else "may count every range in one pass",
                                                                         d, ">" if m3 else "<=", HUGE_RANGES, HUGE_RANGES * cap))
    return Claims(n, d, True, len(lens), cannot, must, False, m1, m1no, m2, m2no, m3, why)


# ---- expected, not guaranteed: how unlikely a uniformly random order misses them ----

def _log2_binom(n, k):
    return (math.lgamma(n + 1) - math.lgamma(k + 1) - math.lgamma(n - k + 1)) / math.log(2)


def mode1_repass_log2_bound(mults, cap):
    """log2 of an upper bound of P(NO slice of the sub-bucket sees more than cap distinct suffixes) under a uniformly random order.
    Slice 0 (length L of n keys) sees at most cap distinct only if some set T of t = d - cap suffixes is absent from it.  The keys
    of T, M_T of them, all miss the slice with probability C(n - M_T, L) / C(n, L) <= (1 - L / n)^M_T, and M_T >= M, the sum of the
    t smallest multiplicities; there are C(d, t) sets: P <= C(d, t) (1 - L / n)^M.  (No slice re-passing implies slice 0 not.)"""
    m = np.sort(np.asarray(mults, dtype=np.int64))
    n, d = int(m.sum()), len(m)
    t = d - cap
    if t <= 0:
        return 0.0
    L = slice_lengths(n)[0]
    M = int(m[:t].sum())
    return min(0.0, _log2_binom(d, t) + M * math.log2(1.0 - L / n))


def empty_range_log2_bound(n, heavy):
    """log2 of an upper bound of P(no range of a dense sub-bucket is empty) when one suffix holds `heavy` of its n keys, under a
    uniformly random order.  The sample is then HUGE_SAMPLE keys drawn without replacement; X of them are the heavy suffix, a run
    of X equal entries in the sorted sample.  A run of 3 * (HUGE_SAMPLE / HUGE_RANGES) entries covers three positions 63 mod 64
    wherever it lies; at most one of them is the sample's last entry, which is no splitter (the last range ends at the mask), so
    two neighbouring splitters are equal and huge_range finds prev >= hi.  Hoeffding's bound holds for sampling without
    replacement: P(X <= mu - s) <= exp(-2 s^2 / HUGE_SAMPLE)."""
    need = 3 * (HUGE_SAMPLE // HUGE_RANGES)
    mu = HUGE_SAMPLE * heavy / n
    s = mu - need
    if s <= 0:
        return 0.0
    return -2.0 * s * s / HUGE_SAMPLE / math.log(2)


# ---- the rows of tests/test_count_huge_edges.py: (n, multiplicities) of every planted sub-bucket ----

def even_mults(n, d):
    """d suffixes, n keys, as even as it goes"""
    return [n // d + (1 if i < n % d else 0) for i in range(d)]


def drawn_mults(n, d, seed):
    """every suffix once, the other n - d keys drawn uniformly (test_count_huge_edges.plant_drawn draws the same picks)"""
    picks = drawn_picks(n, d, seed)
    return np.bincount(picks, minlength=d).tolist()


def drawn_picks(n, d, seed):
    rng = np.random.default_rng(seed)
    picks = np.concatenate([np.arange(d), rng.integers(0, d, n - d)])
    rng.shuffle(picks)
    return picks


def heavy_mults(n, heavy):
    return [heavy] + [1] * (n - heavy)


EDGE_N = 3 * HUGE_SLICE                            # 98304: three slices of exactly HUGE_SLICE keys


def rows(cap):
    """name -> list of multiplicity lists (one per planted sub-bucket) for a family whose tables hold cap suffixes; the 4096-suffix
    rows of the 2048 families carry `_4096` in their name"""
    r = {
        "cut_edge": [even_mults(HUGE_SLICE_MIN, 300), even_mults(HUGE_SLICE_MIN + 1, 300)],
        "equal_slices": [even_mults(EDGE_N, 20), even_mults(EDGE_N + 1, 20)],
        "full_table": [even_mults(EDGE_N, cap)],
        "one_over": [even_mults(EDGE_N, cap + 1)],
        "dense_wide": [[1] * (400_000 if cap == HUGE_CAP32 else 200_000)],
        "clustered_dense": [[1] * 200_000],
        "heavy_in_dense": [heavy_mults(200_000, 100_000)],
        "uncut_passes": [[1] * HUGE_SLICE_MIN],
        "neighbours": [[1] * 70_000, even_mults(70_000, 20), even_mults(40_000, 700)],
    }
    if cap == HUGE_CAP64:
        r["full_table_4096"] = [even_mults(EDGE_N, 4096)]
        r["slice_repass"] = [drawn_mults(EDGE_N, 3000, 3000)]
    return r


def want(cut=None, slices=None, cannot_dense=None, must_dense=None, m0=None, m1=None, m1no=None, m2=None, m2no=None, m3=None):
    return dict(cut=cut, slices=slices, cannot_be_dense=cannot_dense, must_be_dense=must_dense, mode0_must_repass=m0,
                mode1_must_repass=m1, mode1_cannot_repass=m1no, mode2_must_repass=m2, mode2_cannot_repass=m2no, mode3_must_repass=m3)


# what test_count_huge_edges.py asserts of each planted sub-bucket (None: the row says nothing about it); test_huge_model_host.py checks
# that claims() derives every one of them from the row's multiplicities.  one_over is not here: it differs by family.
ROW_CLAIMS = {
    "cut_edge": [want(cut=False, m0=False), want(cut=True, slices=3, cannot_dense=True, m1no=True, m2no=True)],
    "equal_slices": [want(cut=True, slices=3, cannot_dense=True, m1no=True, m2no=True), want(cut=True, slices=4, cannot_dense=True, m1no=True, m2no=True)],
    "full_table": [want(cut=True, slices=3, cannot_dense=True, m1no=True, m2=False, m2no=True)],
    "full_table_4096": [want(cut=True, slices=3, cannot_dense=True, m2=True)],
    "slice_repass": [want(cut=True, slices=3, cannot_dense=True, m2=True)],
    "dense_wide": [want(cut=True, must_dense=True, m1=True, m3=True)],
    "clustered_dense": [want(cut=True, must_dense=True, m1=True)],
    "heavy_in_dense": [want(cut=True, must_dense=True)],
    "uncut_passes": [want(cut=False, m0=True)],
    "neighbours": [want(cut=True, slices=3, must_dense=True), want(cut=True, slices=3, cannot_dense=True, m1no=True, m2no=True), want(cut=False, m0=False)],
}
