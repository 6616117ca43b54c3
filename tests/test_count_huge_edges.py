"""Count stage, GIGANTIC sub-buckets: the slice, merge and range edges of launch_huge (run with -m gpu on an MI355X).

A sub-bucket above 65536 keys is cut into slices (huge_plan_kernel), the slices become (suffix, count) pairs (MODE 1), the pairs
are merged (MODE 2), a dense sub-bucket is counted by 64 quantile ranges stitched by a chain (MODE 3), and MODE 0 keeps the
oversized sub-buckets that are not cut.  The neighbouring parity test plants random clusters that reach only the interior of each
mode: no pass of MODE 1, 2 or 3 ever overflowed its table there, no range was ever empty, no size sat on an edge, and nothing
asserted which path had run.  The sub-buckets planted here sit ON the edges (65536 / 65537 keys, 3 * 32768 / one more, CAP / CAP + 1
distinct suffixes, 8 D = the slice's length, more than 64 * CAP distinct, a heavy suffix at either end of the suffix space), in all
five key/table families, next to the structured-keys tests' filler reads.  Every case asserts
  - klo, khi and the counts equal the oracle's brute-force count, exactly;
  - huge_cut and huge_slices of the profile equal what huge_model.expected_plan derives from the oracle's result;
  - the path claims of its row (huge_model.ROW_CLAIMS), which huge_model.claims derives from the sub-bucket the ORACLE found --
    its size and the multiplicities of its suffixes, whatever the order of the keys -- against the profile's path counters
    (huge_dense, huge_repasses[MODE], huge_empty_ranges).  test_huge_model_host.py checks the model without a GPU.
A planted sub-bucket has exactly the size of its row: its prefix is chosen where the filler has no k-mer (min_top >= 14) or few
(min_top = 12: 2^18 sub-buckets for 4.5 M filler k-mers), and those few are taken off what is planted.  MGC_HASH_STREAM=0 keeps the
grouping at 6 + min_top bits (the judged plan may coarsen a file; the gigantic path is the same under both).

What the cases found: no wrong or missing k-mer -- every row is exact in every family.  What they pin, tried on scratch builds:
the dense rule with `>=` for `>` sends the 8 D = 32768 sub-buckets of test_full_table to MODE 3 (huge_dense 1, not 0); the overflow
test one insert early (`>= CAP - 1`) re-passes in test_full_table, where no pass may be repeated; the chain published on a range's
FIRST pass instead of its last loses about 210 000 k-mers in every case of test_dense_wide_and_clustered_ranges."""
import zlib

import numpy as np
import pytest

import huge_model as hm
import plant_helpers as ph
import structured_helpers as sh

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "the -m gpu tests need a GPU"
    torch.cuda.set_device(0)
    return torch


@pytest.fixture(scope="module")
def ops(native_lib, torch_cuda):
    from meryl_amd import count
    return count


# family: k, MGC_FINISH_MIN_TOP, further switches, the tables' capacity (huge_model.CAP)
FAMILY = {
    "narrow32_k21": (21, 16, {}, hm.CAP["narrow32"]),                  # launch_huge<Huge8<u32, u32>>, 20-bit suffixes
    "narrow32_k16": (16, 12, {}, hm.CAP["narrow32"]),                  # ... 14-bit suffixes
    "whole32_k21": (21, 16, {"MGC_NARROW": "0"}, hm.CAP["whole32"]),   # launch_huge<Huge8<u32, u64>>
    "whole64_k26": (26, 14, {}, hm.CAP["whole64"]),                    # launch_huge<Huge8<u64, u64>>, 32-bit suffixes
    "whole64_k31": (31, 16, {}, hm.CAP["whole64"]),                    # ... 40-bit suffixes
    "k96_k40": (40, 12, {}, hm.CAP["k96"]),                            # launch_huge<Huge16<false, K96>>, 62-bit suffixes
    "k96w_k51": (51, 12, {}, hm.CAP["k96"]),                           # launch_huge<Huge16<true, K96>>, 84-bit suffixes
    "k128w_k64": (64, 12, {}, hm.CAP["k128"]),                         # launch_huge<Huge16<true, K128>>, 110-bit suffixes
    "k128_k40": (40, 12, {"MGC_K96": "0"}, hm.CAP["k128"]),            # launch_huge<Huge16<false, K128>>
}
FORWARD, CANONICAL = 1, 0
_LUT = np.frombuffer(b"ACTG", dtype=np.uint8)                          # base codes A0 C1 T2 G3 (structured_helpers.BASES)


def S(row, i=0, head="AAC", heavy=None, shared=0):
    """one planted sub-bucket: multiplicities of huge_model.rows(cap)[row][i]; heavy: where the heaviest suffix lies ("zero", "ones",
    "mid"); shared: leading tail bases all its suffixes share"""
    return dict(row=row, i=i, head=head, heavy=heavy, shared=shared)


def _tails(n, tlen, rng, shared=0, avoid=()):
    """n distinct tails (base codes, [n, tlen]) that do not end in T: with a head that begins with A the forward k-mer is the canonical
    one.  avoid: suffixes the filler has in the sub-bucket (a short tail could meet one; a long one will not)"""
    if tlen <= 11:
        v = np.arange(1 << (2 * tlen), dtype=np.int64)
        v = rng.permutation(v[((v & 3) != 2) & ~np.isin(v, avoid)])[:n]
        assert len(v) == n, "the suffix space holds only %d such tails" % len(v)
        return ((v[:, None] >> (2 * (tlen - 1 - np.arange(tlen)))) & 3).astype(np.uint8)
    t = rng.integers(0, 4, (n + n // 64 + 16, tlen), dtype=np.uint8)
    t[:, :shared] = rng.integers(0, 4, shared, dtype=np.uint8)
    t[:, -1] = np.array([0, 1, 3], dtype=np.uint8)[rng.integers(0, 3, len(t))]
    t = rng.permutation(np.unique(t, axis=0))[:n]
    assert len(t) == n
    return t


_HEAVY = {"zero": lambda tlen: np.zeros(tlen, dtype=np.uint8),                       # suffix 0
          "ones": lambda tlen: np.full(tlen, 3, dtype=np.uint8),                     # the all-ones suffix: low_mask, the last range's fixed end
          "mid": lambda tlen: np.array(([2, 1, 0, 3] * tlen)[:tlen - 1] + [1], dtype=np.uint8)}


def _planted_mults(mults, stray_n, stray_d):
    """the row's multiplicities less what the filler already has in the sub-bucket: stray_d suffixes fewer, stray_n keys fewer"""
    m = list(mults)
    target = sum(m) - stray_n
    if stray_d:
        del m[-stray_d:]
    while sum(m) > target:
        m.pop()
    m[0] += target - sum(m)
    return m


def _block(pre, k, mults, rng, heavy, shared, avoid=()):
    """reads of one k-mer each, a '.' behind every one: suffix i mults[i] times, in a uniformly random order"""
    tlen = k - len(pre)
    tails = _tails(len(mults), tlen, rng, shared, avoid)
    if heavy:
        h = _HEAVY[heavy](tlen)
        tails = tails[~(tails == h).all(axis=1)]
        tails = np.concatenate([h[None, :], tails])[:len(mults)]
        assert len(tails) == len(mults) and mults[0] == max(mults)
    picks = rng.permutation(np.repeat(np.arange(len(mults)), mults))
    mat = np.empty((len(picks), k + 1), dtype=np.uint8)
    mat[:, :len(pre)] = np.frombuffer(pre.encode(), dtype=np.uint8)
    mat[:, len(pre):k] = _LUT[tails[picks]]
    mat[:, k] = ord(".")
    return mat.tobytes().decode("ascii")


def _prefixes(subs, plen, min_top, occ, rng, adjacent):
    """a prefix per sub-bucket with no filler k-mer inside (min_top = 12: few); adjacent: consecutive sub-bucket numbers"""
    per = 0 if min_top >= 14 else 12
    if adjacent:
        stem, _ = ph.pick_prefix(subs[0]["head"], plen - 1, min_top, occ, rng, max_strays=4 * per)
        return [stem + sh.BASES[i] for i in range(len(subs))]
    out = []
    for s in subs:
        while True:
            pre, _ = ph.pick_prefix(s["head"], plen, min_top, occ, rng, max_strays=per)
            if pre not in out:
                out.append(pre)
                break
    return out


def _run(ops, oracle_lib, monkeypatch, family, subs, modes=(FORWARD,), env=None, adjacent=False, expect_slice_repass=False):
    k, min_top, fam_env, cap = FAMILY[family]
    env = dict(fam_env, **(env or {}))
    sliced = env.get("MGC_HUGE_SLICES", "1") != "0"
    monkeypatch.setenv("MGC_FINISH_MIN_TOP", str(min_top))
    monkeypatch.setenv("MGC_HASH_STREAM", "0")
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    assert (6 + min_top) % 2 == 0
    plen, low = (6 + min_top) // 2, 2 * k - 6 - min_top
    rows = hm.rows(cap)
    rng = np.random.default_rng(zlib.crc32(repr((family, [(s["row"], s["i"], s["heavy"], s["head"]) for s in subs])).encode()))
    occ = ph.occupied(oracle_lib, k, low, modes)
    pres = _prefixes(subs, plen, min_top, occ, rng, adjacent)
    for mode, occ_mode in zip(modes, occ):
        text = ""
        for s, pre in zip(subs, pres):
            stray_n, stray_d = ph.stray_kmers(occ_mode, ph.id_range(pre, min_top))
            avoid = ph.stray_suffixes(oracle_lib, k, low, mode, ph.id_range(pre, min_top)) if low < 32 else ()
            text += _block(pre, k, _planted_mults(rows[s["row"]][s["i"]], stray_n, stray_d), rng, s["heavy"], s["shared"], avoid)
        text += ph.filler(oracle_lib, k)
        whi, wlo, wcn, prof = ph.count_and_compare(ops, oracle_lib, text, k, mode)
        rp = list(prof.huge_repasses)
        print("%s mode %d: huge_cut %d, huge_slices %d, huge_dense %d, huge_repasses %s, huge_empty_ranges %d"
              % (family, mode, prof.huge_cut, prof.huge_slices, prof.huge_dense, rp, prof.huge_empty_ranges))
        # the plan, from the oracle's result
        plan = hm.expected_plan(whi, wlo, wcn, k, min_top, sliced)
        assert (prof.huge_cut, prof.huge_slices) == (plan.cut, plan.slices), (prof.huge_cut, prof.huge_slices, plan)
        # every planted sub-bucket as the oracle found it: the size of its row, and the claims of its row follow from it
        ids = hm.subbucket_ids(whi, wlo, low)
        cs = []
        for s, pre in zip(subs, pres):
            first, end = ph.id_range(pre, min_top)
            mults = wcn[(ids >= np.uint64(first)) & (ids < np.uint64(end))].astype(np.int64)
            c = hm.claims(mults, cap, sliced)
            print("  %s[%d] at %s: %d keys, %d distinct: %s" % (s["row"], s["i"], pre, c.n, c.distinct, "; ".join(c.why)))
            row = rows[s["row"]][s["i"]]
            assert c.n == sum(row) and plan.groups[first] == (c.n, c.distinct)
            # (singletons: a filler k-mer that comes twice takes two of them away)
            assert c.distinct == len(row) or (min(row) == 1 and 0 < len(row) - c.distinct <= 12), (c.distinct, len(row))
            if s["row"] == "one_over":
                assert c.distinct == cap + 1
                if cap == hm.HUGE_CAP64:
                    assert c.cannot_be_dense and c.mode2_must_repass
            elif sliced:
                for field, want in hm.ROW_CLAIMS[s["row"]][s["i"]].items():
                    assert want is None or getattr(c, field) == want, (s["row"], s["i"], field, getattr(c, field), want)
            if s["heavy"]:
                assert int(mults.max()) == max(row) and int({"zero": mults[0], "ones": mults[-1], "mid": mults.max()}[s["heavy"]]) == max(row)
            cs.append(c)
        assert plan.cut == sum(c.cut for c in cs)
        # the paths that ran, against what follows from those sub-buckets
        cut = [c for c in cs if c.cut]
        assert sum(c.must_be_dense for c in cut) <= prof.huge_dense <= sum(not c.cannot_be_dense for c in cut), prof.huge_dense
        assert rp[0] >= sum(c.mode0_must_repass for c in cs)
        if not any(c.mode0_must_repass for c in cs):
            assert rp[0] == 0                                # (an uncut planted sub-bucket of at most CAP suffixes; the filler's are small)
        assert rp[1] >= max(sum(c.mode1_must_repass for c in cut), 1 if expect_slice_repass else 0)
        if all(c.mode1_cannot_repass for c in cut):
            assert rp[1] == 0
        assert rp[2] >= sum(c.mode2_must_repass for c in cut)
        if all(c.mode2_cannot_repass or c.must_be_dense for c in cut):
            assert rp[2] == 0
        assert rp[3] >= sum(c.mode3_must_repass for c in cut)
        assert prof.huge_empty_ranges >= sum(1 for s, c in zip(subs, cs) if s["heavy"] and c.cut)
        if all(c.cannot_be_dense for c in cut):
            assert rp[3] == 0 and prof.huge_empty_ranges == 0
        if not sliced:
            assert (prof.huge_cut, prof.huge_slices, prof.huge_dense, rp[1], rp[2], rp[3]) == (0, 0, 0, 0, 0, 0)
    return prof


def _modes(family):
    """forward and canonical mode for a narrowed and a 12-byte family (the filler's k-mers differ between the modes, the planted ones do
    not: heads begin with A, tails do not end in T); the count stage itself does not see the mode"""
    return (FORWARD, CANONICAL) if family in ("narrow32_k21", "k96w_k51") else (FORWARD,)


@pytest.mark.parametrize("family", sorted(FAMILY))
def test_cut_edge_and_equal_slices(ops, oracle_lib, torch_cuda, monkeypatch, family):
    """Four sub-buckets of one file: 65536 keys (not cut: MODE 0) and 65537 (three slices of 21846 / 21846 / 21845), 300 distinct
    each; 98304 keys (three slices of exactly 32768) and 98305 (four of 24577 / .. / 24574), 20 distinct each.  Never dense."""
    prof = _run(ops, oracle_lib, monkeypatch, family, [S("cut_edge", 0), S("cut_edge", 1), S("equal_slices", 0), S("equal_slices", 1)], _modes(family))
    assert (prof.huge_cut, prof.huge_slices, prof.huge_dense) == (3, 3 + 3 + 4, 0)


@pytest.mark.parametrize("family,row", [("narrow32_k21", "full_table"), ("whole32_k21", "full_table"), ("whole64_k31", "full_table"),
                                        ("k96_k40", "full_table"), ("k96w_k51", "full_table"), ("k128w_k64", "full_table"),
                                        ("whole64_k31", "full_table_4096"), ("k96w_k51", "full_table_4096")])
def test_full_table(ops, oracle_lib, torch_cuda, monkeypatch, family, row):
    """98304 keys with exactly CAP distinct suffixes, every one at least 8 times: 8 D = the slice's length at most (never dense), a
    slice and the merge hold exactly CAP suffixes -- the table exactly half full, `>= CAP` must not fire: no pass is repeated.
    The 2048 families with 4096 suffixes: still never dense (8 * 4096 = 32768), the merge must re-pass."""
    prof = _run(ops, oracle_lib, monkeypatch, family, [S(row)], _modes(family))
    assert prof.huge_dense == 0
    if row == "full_table":
        assert list(prof.huge_repasses) == [0, 0, 0, 0]
    else:
        assert prof.huge_repasses[2] >= 1


@pytest.mark.parametrize("family", ["narrow32_k21", "whole64_k26", "k96_k40", "k128_k40"])
def test_one_over_the_table(ops, oracle_lib, torch_cuda, monkeypatch, family):
    """98304 keys with CAP + 1 distinct suffixes.  4096 family: dense or merged depends on the order of the keys -- the result only.
    2048 families: never dense, the merge must re-pass."""
    prof = _run(ops, oracle_lib, monkeypatch, family, [S("one_over")])
    if FAMILY[family][3] == hm.HUGE_CAP64:
        assert prof.huge_dense == 0 and prof.huge_repasses[2] >= 1


@pytest.mark.parametrize("family", ["whole64_k31", "k96w_k51", "k128_k40"])
def test_slice_repass(ops, oracle_lib, torch_cuda, monkeypatch, family):
    """98304 keys, 3000 suffixes drawn uniformly: never dense, the merge must re-pass, and every slice is expected to see more than
    CAP = 2048 of them (huge_model.mode1_repass_log2_bound: missed with probability below 2^-1000): MODE 1 re-passes too."""
    assert hm.mode1_repass_log2_bound(hm.rows(hm.HUGE_CAP64)["slice_repass"][0], hm.HUGE_CAP64) < -1000
    prof = _run(ops, oracle_lib, monkeypatch, family, [S("slice_repass")], expect_slice_repass=True)
    assert prof.huge_dense == 0 and prof.huge_repasses[1] >= 1 and prof.huge_repasses[2] >= 1


@pytest.mark.parametrize("family", ["narrow32_k21", "whole64_k31", "k96_k40", "k96w_k51", "k128w_k64"])
def test_dense_wide_and_clustered_ranges(ops, oracle_lib, torch_cuda, monkeypatch, family):
    """All distinct: more than 64 * CAP suffixes, so some range of MODE 3 must take several passes (chain_wait before the first emit,
    chain_sent on the last pass only, emit_at = chain_base + out).  Next to it (not at k = 21: ten tail bases) the same with every
    tail sharing its first 8 bases: all suffixes in a sliver of the space, the quantile ranges have to find them."""
    subs = [S("dense_wide")] + ([S("clustered_dense", shared=8)] if family != "narrow32_k21" else [])
    prof = _run(ops, oracle_lib, monkeypatch, family, subs, _modes(family))
    assert prof.huge_dense == len(subs) and prof.huge_repasses[3] >= len(subs)


@pytest.mark.parametrize("family", ["narrow32_k21", "whole64_k31", "k96w_k51", "k128w_k64"])
def test_heavy_suffix_in_dense(ops, oracle_lib, torch_cuda, monkeypatch, family):
    """Three dense sub-buckets of 200 000 keys: 100 000 instances of one suffix H and 100 000 singletons, shuffled; H = suffix 0,
    H = the all-ones suffix (the last range's fixed end), H in the middle.  Half the sample is H: equal splitters, empty ranges
    (huge_model.empty_range_log2_bound) that still have to pass the chain on -- the last one has to write the sub-bucket's total."""
    assert hm.empty_range_log2_bound(200_000, 100_000) < -1000
    subs = [S("heavy_in_dense", heavy="zero"), S("heavy_in_dense", heavy="ones"), S("heavy_in_dense", heavy="mid")]
    prof = _run(ops, oracle_lib, monkeypatch, family, subs, _modes(family))
    assert prof.huge_dense == 3 and prof.huge_empty_ranges >= 3


@pytest.mark.parametrize("family", ["narrow32_k21", "whole64_k26", "k128w_k64"])
def test_uncut_many_passes(ops, oracle_lib, torch_cuda, monkeypatch, family):
    """65536 keys, all distinct: the largest sub-bucket that is not cut, sixteen (4096) or thirty-two (2048) tables full: MODE 0 re-passes"""
    prof = _run(ops, oracle_lib, monkeypatch, family, [S("uncut_passes")])
    assert prof.huge_cut == 0 and prof.huge_repasses[0] >= 1


@pytest.mark.parametrize("family,env", [("narrow32_k21", {}), ("whole64_k31", {}), ("k96w_k51", {}), ("k96w_k51", {"MGC_HUGE_SLICES": "0"})])
def test_neighbours(ops, oracle_lib, torch_cuda, monkeypatch, family, env):
    """A dense (70 000 all distinct), a sliced (70 000 / 20) and an oversized uncut (40 000 / 700) sub-bucket with consecutive numbers:
    each by its own rule, nothing of one in the other (the result is exact).  MGC_HUGE_SLICES=0: round 5's form, nothing is cut."""
    prof = _run(ops, oracle_lib, monkeypatch, family, [S("neighbours", 0), S("neighbours", 1), S("neighbours", 2)], env=env, adjacent=True)
    if not env:
        assert (prof.huge_cut, prof.huge_slices, prof.huge_dense) == (2, 6, 1)


@pytest.mark.parametrize("streams", [None, "1"])
def test_many_files(ops, oracle_lib, torch_cuda, monkeypatch, streams):
    """A sliced and a dense sub-bucket in each of six files: more sliced files than streaming streams (four by default, one with
    MGC_HUGE_STREAMS=1), so a workspace and a second buffer are used again; the counters are sums over the files."""
    subs = []
    for head in ("AAC", "ACA", "ATT", "AGC", "ACC", "AGG"):
        subs += [S("neighbours", 1, head=head), S("neighbours", 0, head=head)]
    prof = _run(ops, oracle_lib, monkeypatch, "narrow32_k21", subs, env={"MGC_HUGE_STREAMS": streams} if streams else None)
    assert (prof.huge_cut, prof.huge_slices, prof.huge_dense) == (12, 36, 6)


def test_round5_form_dense(ops, oracle_lib, torch_cuda, monkeypatch):
    """MGC_HUGE_SLICES=0: the 400 000 all-distinct keys through ONE workgroup (MODE 0, a hundred passes); cut = slices = dense = 0"""
    prof = _run(ops, oracle_lib, monkeypatch, "narrow32_k21", [S("dense_wide")], env={"MGC_HUGE_SLICES": "0"})
    assert (prof.huge_cut, prof.huge_slices, prof.huge_dense) == (0, 0, 0) and prof.huge_repasses[0] >= 1
