"""Host checks of tests/huge_model.py: the slice arithmetic of huge_plan_kernel over every size, and -- for every row the GPU module
(test_count_huge_edges.py) plants -- that the path it claims follows from the planted (n, multiplicities) alone.  No GPU; the
output (-s) lists every row's claims and the reason each holds."""
import numpy as np
import pytest

import huge_model as hm


def test_slice_arithmetic_every_size():
    """65537 .. 2^22: the slices sum to n, none exceeds HUGE_SLICE, the last one is not empty and at most W - 1 shorter"""
    n = np.arange(hm.HUGE_SLICE_MIN + 1, (1 << 22) + 1, dtype=np.int64)
    W = (n + hm.HUGE_SLICE - 1) // hm.HUGE_SLICE
    ln = (n + W - 1) // W
    last = n - (W - 1) * ln
    assert (ln <= hm.HUGE_SLICE).all()
    assert (last >= 1).all() and (ln - last <= W - 1).all() and (last <= ln).all()
    assert ((W - 1) * ln + last == n).all()
    assert (W <= hm.HUGE_WMAX).all()
    # the scalar statements agree with the vector ones
    for x in (65537, 98304, 98305, 131072, 131073, 1 << 22, 1234567):
        i = x - (hm.HUGE_SLICE_MIN + 1)
        assert hm.huge_slices(x) == W[i] and hm.huge_slice_len(x) == ln[i]
        assert hm.slice_lengths(x) == [int(ln[i])] * (int(W[i]) - 1) + [int(last[i])] and sum(hm.slice_lengths(x)) == x


def test_slice_arithmetic_spot_values():
    assert not hm.huge_is_cut(65536)
    assert hm.huge_is_cut(65537) and hm.slice_lengths(65537) == [21846, 21846, 21845]
    assert hm.huge_is_cut(98304) and hm.slice_lengths(98304) == [32768, 32768, 32768]
    assert hm.huge_is_cut(98305) and hm.slice_lengths(98305) == [24577, 24577, 24577, 24574]
    assert hm.huge_is_cut(hm.HUGE_WMAX * hm.HUGE_SLICE) and not hm.huge_is_cut(hm.HUGE_WMAX * hm.HUGE_SLICE + 1)     # (more slices than the plan holds: MODE 0)
    assert not hm.huge_is_cut(1 << 20, 0)                                   # MGC_HUGE_SLICES=0


def test_dense_and_overflow_edges():
    assert not hm.is_dense(4096, 32768) and hm.is_dense(4097, 32768)        # 8 D = the slice's length / one more
    assert not hm.overflows(2048, 2048) and hm.overflows(2049, 2048)        # D = CAP exactly: the table is half full, no overflow
    assert hm.sample_index(0, 200_000) == 0 and hm.sample_index(hm.HUGE_SAMPLE - 1, 200_000) == 199_951
    assert hm.sample_index(hm.HUGE_SAMPLE - 1, hm.HUGE_SLICE_MIN + 1) == 65520
    # equal splitters make empty ranges; the first range is never empty, the last one ends at the mask
    split = [5, 5, 5, 9] + list(range(10, 10 + hm.HUGE_RANGES - 5)) + [1023]
    assert len(split) == hm.HUGE_RANGES
    assert hm.huge_range(split, 0) == (0, 5) and hm.huge_range(split, 1) is None and hm.huge_range(split, 2) is None
    assert hm.huge_range(split, 3) == (6, 9) and hm.huge_range(split, hm.HUGE_RANGES - 1) == (split[-2] + 1, 1023)
    assert hm.huge_range([0] * 63 + [1023], 1) is None and hm.huge_range([1023] * 64, 63) is None
    s = np.sort(np.random.default_rng(1).integers(0, 1 << 20, hm.HUGE_SAMPLE))
    sp = hm.splitters(s, (1 << 20) - 1)
    assert len(sp) == hm.HUGE_RANGES and sp[0] == s[63] and sp[62] == s[4031] and sp[63] == (1 << 20) - 1


def test_expected_plan_from_an_oracle_result():
    """three sub-buckets of a k = 21, min_top = 16 result (20 bits below the sub-bucket): 65536 keys, 65537 keys, 98305 keys"""
    low = 20
    kmers, counts = [], []
    for g, (n, d) in ((5, (65536, 300)), (6, (65537, 300)), (1 << 21, (98305, 20))):
        m = hm.even_mults(n, d)
        kmers += [(g << low) | (i * 7) for i in range(d)]
        counts += m
    wlo = np.array(kmers, dtype=np.uint64)
    plan = hm.expected_plan(np.zeros(len(wlo), dtype=np.uint64), wlo, np.array(counts, dtype=np.uint32), 21, 16)
    assert (plan.cut, plan.slices) == (2, 3 + 4)
    assert plan.groups == {5: (65536, 300), 6: (65537, 300), 1 << 21: (98305, 20)}
    assert hm.expected_plan(np.zeros(len(wlo), dtype=np.uint64), wlo, np.array(counts, dtype=np.uint32), 21, 16, sliced=False)[:2] == (0, 0)
    # 16-byte k-mers: the sub-bucket number comes from the high half
    whi = np.array([(1 << 46) | 5, (1 << 46) | 9, 2 << 46], dtype=np.uint64)
    p = hm.expected_plan(whi, np.array([1, 2, 3], dtype=np.uint64), np.array([40000, 40000, 70000], dtype=np.uint32), 64, 12)    # low = 110
    assert hm.subbucket_ids(whi, whi, 110).tolist() == [1, 1, 2] and (p.cut, p.slices) == (2, 3 + 3) and p.groups == {1: (80000, 2), 2: (70000, 1)}


_ROW_CLAIMS = hm.ROW_CLAIMS


@pytest.mark.parametrize("cap", [hm.HUGE_CAP32, hm.HUGE_CAP64])
def test_every_row_claims_only_what_follows(cap):
    rows = hm.rows(cap)
    assert set(rows) - {"one_over"} <= set(_ROW_CLAIMS)
    for name, subs in sorted(rows.items()):
        for i, mults in enumerate(subs):
            c = hm.claims(mults, cap)
            print("CAP %d, row %s, sub-bucket %d: %d keys, %d distinct" % (cap, name, i, c.n, c.distinct))
            for w in c.why:
                print("    " + w)
            if name == "one_over":
                continue
            for field, want in _ROW_CLAIMS[name][i].items():
                if want is not None:
                    assert getattr(c, field) == want, (name, i, field, getattr(c, field), want)
    # one over: the 4096 family may go either way (the row asserts the result only), the 2048 families cannot be dense and must re-pass
    c = hm.claims(rows["one_over"][0], cap)
    if cap == hm.HUGE_CAP32:
        assert c.distinct == 4097 and not c.cannot_be_dense and not c.must_be_dense
    else:
        assert c.distinct == 2049 and c.cannot_be_dense and c.mode2_must_repass
    # full table: every suffix at least 8 times
    assert min(rows["full_table"][0]) >= 8 and len(rows["full_table"][0]) == cap


def test_claims_hold_under_adversarial_orders():
    """the claims against a direct simulation of the dense rule on orders built to break them: sorted by suffix (a slice sees the
    fewest suffixes), round-robin (every slice sees the most), and a random one"""
    rng = np.random.default_rng(7)
    for cap in (hm.HUGE_CAP32, hm.HUGE_CAP64):
        for name, subs in hm.rows(cap).items():
            for mults in subs:
                c = hm.claims(mults, cap)
                if not c.cut:
                    continue
                keys = np.repeat(np.arange(len(mults)), mults)
                rr = np.argsort(np.concatenate([np.arange(m) for m in mults]), kind="stable")
                for order in (keys, keys[rr], rng.permutation(keys)):
                    dense, at = False, 0
                    for ln in hm.slice_lengths(c.n):
                        dense = dense or hm.is_dense(len(np.unique(order[at:at + ln])), ln)
                        at += ln
                    assert not (c.cannot_be_dense and dense) and not (c.must_be_dense and not dense), name


def test_expected_claims_are_astronomically_likely():
    """the two claims that are expected, not guaranteed: the probability that a uniformly random order of the keys misses them"""
    mults = hm.rows(hm.HUGE_CAP64)["slice_repass"][0]
    assert sum(mults) == hm.EDGE_N and len(mults) == 3000 and min(mults) >= 1
    b1 = hm.mode1_repass_log2_bound(mults, hm.HUGE_CAP64)
    print("slice re-pass: 3000 suffixes over %d keys, %d .. %d times each; P(no slice sees more than %d) <= 2^%.0f"
          % (hm.EDGE_N, min(mults), max(mults), hm.HUGE_CAP64, b1))
    assert b1 < -1000
    assert hm.mode1_repass_log2_bound(hm.even_mults(hm.EDGE_N, 2048), hm.HUGE_CAP64) == 0.0       # (nothing to expect at D = CAP)
    b2 = hm.empty_range_log2_bound(200_000, 100_000)
    print("heavy in dense: 100000 of 200000 keys are one suffix; P(no empty range) <= 2^%.0f" % b2)
    assert b2 < -1000
    assert hm.empty_range_log2_bound(200_000, 5_000) == 0.0                                       # (a suffix of 2.5 %: no claim)
