"""Count stage on hash-STRUCTURED sub-buckets (run with -m gpu on an MI355X).

Every other parity test draws its k-mers at random, and a multiplicative hash spreads random keys evenly: no test had put many
distinct suffixes of one sub-bucket on ONE home slot of a count kernel's LDS table.  The sub-buckets planted here are searched
for exactly that (structured_helpers.colliding_tails; test_structured_helpers_host.py proves on the host that every case forces
the probe chains it claims, through the wrap at the table's last slot as well), next to the neighbouring tests' filler reads, and
every result is compared with the oracle's brute-force count of the same text: klo, khi and counts, exactly.

What the cases found: hash_count_stream_kernel gives a key up after 64 probe steps and sends the sub-bucket to the retry launch;
the retry launch sized its table by the same key count, met the same chain, and -- having nowhere to send the sub-bucket -- wrote a
distinct count of 0: every k-mer of the sub-bucket was missing from the result, without an error (stream cases a, b, c, e; d
reached the retry launch through the probe bound alone and was lost there the same way).  The retry instantiation now probes up
to one full turn of its table, which is never more than half full."""
import numpy as np
import pytest

import structured_helpers as sh
from plant_helpers import (filler as _filler, occupied as _occupied, id_range as _id_range, pick_prefix as _pick_prefix, plant as _plant,
                           count_and_compare as _count_and_compare, subbucket as _subbucket)

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


# ---- hash_count_stream_kernel<u32> ----

# case: keys in the sub-bucket, distinct ones, MGC_FINISH_NOLIST, modes, slots of the first / the retry launch
_STREAM = {
    "a": (128, 100, "1", (1, 0), 256, 256),
    "b": (128, 100, "0", (1,), 256, 256),
    "c": (2500, 2500, "1", (1,), 2048, 8192),
    "d": (3000, 1000, "0", (1,), 2048, 8192),
    "e": (128, 100, "0", (1,), 256, 256),
}


@pytest.mark.parametrize("case", sorted(_STREAM))
def test_stream_kernel_u32_crowded_home_slots(ops, oracle_lib, torch_cuda, monkeypatch, case):
    """hash_count_stream_kernel<u32> (MGC_HASH_STREAM=1), one planted sub-bucket per run, nothing else that could retry:
      a  128 keys, 100 distinct 20-bit suffixes on ONE home slot of the 256-slot table both launches give it: the first launch
         trips PROBE_MAX, the retry launch met the same chain and dropped the sub-bucket (forward and canonical mode);
      b  the same on the table's LAST slot: the chain wraps to slot 0;
      c  2500 distinct 18-bit suffixes (above DCAP: retry), 110 of them in eight slots of the retry launch's 8192-slot table;
      d  3000 keys, 1000 distinct (below DCAP), 90 on one slot of the first launch's 2048-slot table: only the probe bound sends it
         to the retry launch, where the ninety lie in four neighbouring slots (the 8192-slot home is the same hash two bits finer);
      e  12-bit suffixes, the narrowest width at which a window of the 256-slot table still holds enough of them: 100 in twenty
         slots.  (The plan gives this kernel at most 18 grouping bits: twelve bits below them is k = 15, not k = 21.)
    Without the fix a, b, c, d and e all fail with the planted k-mers missing, e.g. case a:
      AssertionError: 100 k-mers missing from the device result (3234814 against the oracle's 3234914)
    (b the same, c 2500 missing, d 1000, e 109: the planted k-mers and the filler's in that sub-bucket.)"""
    keys, distinct, nolist, modes, slots_first, slots_retry = _STREAM[case]
    c = sh.CASE["stream_" + case]
    low = 2 * c.k - 6 - c.min_top
    monkeypatch.setenv("MGC_FINISH_MIN_TOP", str(c.min_top))
    monkeypatch.setenv("MGC_FINISH_NOLIST", nolist)
    monkeypatch.setenv("MGC_HASH_STREAM", "1")
    rng = np.random.default_rng(c.k * 100 + c.min_top)
    occ = _occupied(oracle_lib, c.k, low, modes)
    pre, strays = _pick_prefix("AAC", sh.case_plen(c), c.min_top, occ, rng, max_strays=20 if case == "e" else 0)
    tails, homes = sh.case_tails(c, pre)
    assert sh.linear_probe_max_steps(homes, c.slots) > sh.PROBE_MAX
    rest = sh.random_tails(distinct - c.m, c.k - len(pre), 7, exclude=tails) if distinct > c.m else []
    text = _plant(pre, tails + rest, keys - strays, rng) + _filler(oracle_lib, c.k)
    for mode in modes:
        whi, wlo, wcn, prof = _count_and_compare(ops, oracle_lib, text, c.k, mode)
        n, d = _subbucket(whi, wlo, wcn, low, _id_range(pre, c.min_top))
        # the sub-bucket is what the case is built for: its size gives it the tables the colliding suffixes were searched in
        assert n == keys and distinct <= d <= distinct + strays, (n, d, strays)
        assert sh.slots_stream(n, 2048) == slots_first and sh.slots_stream(n, 8192) == slots_retry
        assert c.slots in (slots_first, slots_retry)
        assert (d > sh.DCAP_STREAM) == (case == "c")
        assert prof.stream_files > 0, prof.stream_files
        assert prof.stream_retries >= 1, prof.stream_retries


@pytest.mark.parametrize("k,min_top", [(31, 16), (28, 17)])
def test_stream_kernel_u64_crowded_home_slots(ops, oracle_lib, torch_cuda, monkeypatch, k, min_top):
    """hash_count_stream_kernel<u64> (whole 8-byte k-mers, 40- and 33-bit suffixes, the two-multiply W64 hash): cases a and b in two
    sub-buckets of one run.  Both trip PROBE_MAX; the retry list goes through launch_huge_mode<Huge8<...>, 0>, another table under
    another hash."""
    monkeypatch.setenv("MGC_FINISH_MIN_TOP", str(min_top))
    monkeypatch.setenv("MGC_FINISH_NOLIST", "1")
    monkeypatch.setenv("MGC_HASH_STREAM", "1")
    low = 2 * k - 6 - min_top
    rng = np.random.default_rng(k * 100 + min_top)
    occ = _occupied(oracle_lib, k, low, (1, 0))
    planted, text = [], ""
    for name, head in (("a", "AAC"), ("b", "ACA")):
        c = sh.CASE["stream64_k%d_%s" % (k, name)]
        pre, _ = _pick_prefix(head, sh.case_plen(c), min_top, occ, rng)
        tails, homes = sh.case_tails(c, pre)
        assert sh.linear_probe_max_steps(homes, c.slots) > sh.PROBE_MAX
        text += _plant(pre, tails, 128, rng)
        planted.append(pre)
    text += _filler(oracle_lib, k)
    for mode in (1, 0):
        whi, wlo, wcn, prof = _count_and_compare(ops, oracle_lib, text, k, mode)
        for pre in planted:
            assert _subbucket(whi, wlo, wcn, low, _id_range(pre, min_top)) == (128, 100)          # (128 keys: the 256-slot table)
        assert prof.stream_files > 0, prof.stream_files
        assert prof.stream_retries >= 2, prof.stream_retries


def test_stream_kernel_extreme_entries(ops, oracle_lib, torch_cuda, monkeypatch):
    """The packed entry suffix << 12 | count at its ends: the all-ones 20-bit suffix 4094 times is 0xFFFFFFFE, one below EMPTY,
    and the zero suffix 4094 times; each in a sub-bucket of exactly 4094 keys (FIN_CAP_STREAM), forward mode."""
    k, min_top, low = 21, 16, 20
    monkeypatch.setenv("MGC_FINISH_MIN_TOP", str(min_top))
    monkeypatch.setenv("MGC_FINISH_NOLIST", "1")
    monkeypatch.setenv("MGC_HASH_STREAM", "1")
    rng = np.random.default_rng(4094)
    occ = _occupied(oracle_lib, k, low, (1,))
    ones, _ = _pick_prefix("AAC", 11, min_top, occ, rng)
    zero, _ = _pick_prefix("ACA", 11, min_top, occ, rng)
    text = (ones + "G" * 10 + ".") * sh.CAP_STREAM + (zero + "A" * 10 + ".") * sh.CAP_STREAM + _filler(oracle_lib, k)
    whi, wlo, wcn, prof = _count_and_compare(ops, oracle_lib, text, k, 1)
    for pre, sfx in ((ones, (1 << low) - 1), (zero, 0)):
        assert _subbucket(whi, wlo, wcn, low, _id_range(pre, min_top)) == (sh.CAP_STREAM, 1)
        i = int(np.searchsorted(wlo, np.uint64((sh.encode(pre) << low) | sfx)))
        assert int(wlo[i]) & ((1 << low) - 1) == sfx and int(wcn[i]) == sh.CAP_STREAM
    assert prof.stream_files > 0, prof.stream_files


# ---- the kernels without a probe bound: the chains are long, the result has to be right ----

@pytest.mark.parametrize("R", [1, 2, 4])
def test_multi_kernel_crowded_home_slots(ops, oracle_lib, torch_cuda, monkeypatch, R):
    """hash_count_multi_kernel<R> (MGC_HASH_MULTI=R on the dense grid): cases a and b.  The 100 colliding suffixes lie in the first
    sub-bucket of a range (tag 0) and, the same ones, in its neighbour (tag 1: the tag moves all their homes by one constant, they
    crowd two slots there); 120 keys each, so R = 1 counts each in 256 slots and R = 2 / 4 the range's 240 in 512.  And the
    largest composite the table holds -- tag R - 1, suffix all ones -- 1536 times, the table's capacity."""
    k, min_top, low = 21, 18, 18
    monkeypatch.setenv("MGC_FINISH_MIN_TOP", str(min_top))
    monkeypatch.setenv("MGC_FINISH_NOLIST", "1")
    monkeypatch.setenv("MGC_HASH_MULTI", str(R))
    monkeypatch.setenv("MGC_HASH_STREAM", "0")
    rng = np.random.default_rng(2118 + R)
    occ = _occupied(oracle_lib, k, low, (1, 0))
    planted, text = [], ""
    for name, head in (("a", "AAC"), ("b", "ACA")):
        c = sh.CASE["multi%s_%s" % ("1" if R == 1 else "24", name)]
        pre11, _ = _pick_prefix(head, 11, min_top, occ, rng)               # four sub-buckets free of filler: ranges of every R
        tails, _ = sh.case_tails(c, pre11 + "A")
        text += _plant(pre11 + "A", tails, 120, rng) + _plant(pre11 + "C", tails, 120, rng)
        planted.append((pre11, c))
    top11, _ = _pick_prefix("ATT", 11, min_top, occ, rng)
    text += (top11 + "G" + "G" * 9 + ".") * sh.CAP_HASH + _filler(oracle_lib, k)
    for mode in (1, 0):
        whi, wlo, wcn, _ = _count_and_compare(ops, oracle_lib, text, k, mode)
        for pre11, c in planted:
            assert _subbucket(whi, wlo, wcn, low, _id_range(pre11 + "A", min_top)) == (120, 100)
            n, _ = _subbucket(whi, wlo, wcn, low, _id_range(pre11 if R > 1 else pre11 + "A", min_top))
            assert n == (120 if R == 1 else 240) and sh.slots_quarter(n) == c.slots
        assert _subbucket(whi, wlo, wcn, low, _id_range(top11, min_top)) == (sh.CAP_HASH, 1)


def test_hash_count_kernel_crowded_home_slots(ops, oracle_lib, torch_cuda, monkeypatch):
    """hash_count_kernel (MGC_HASH_MULTI=0, MGC_HASH_STREAM=0), 20-bit suffixes: cases a and b in 128-key sub-buckets (256 slots) and
    a 600-key sub-bucket with 300 distinct suffixes on one home slot of its 1024."""
    k, min_top, low = 21, 16, 20
    monkeypatch.setenv("MGC_FINISH_MIN_TOP", str(min_top))
    monkeypatch.setenv("MGC_FINISH_NOLIST", "0")
    monkeypatch.setenv("MGC_HASH_MULTI", "0")
    monkeypatch.setenv("MGC_HASH_STREAM", "0")
    rng = np.random.default_rng(2116)
    occ = _occupied(oracle_lib, k, low, (1, 0))
    planted, text = [], ""
    for name, head, keys in (("a", "AAC", 128), ("b", "ACA", 128), ("600", "ATT", 600)):
        c = sh.CASE["hash_" + name]
        pre, _ = _pick_prefix(head, sh.case_plen(c), min_top, occ, rng)
        tails, _ = sh.case_tails(c, pre)
        text += _plant(pre, tails, keys, rng)
        planted.append((pre, c, keys))
    text += _filler(oracle_lib, k)
    for mode in (1, 0):
        whi, wlo, wcn, prof = _count_and_compare(ops, oracle_lib, text, k, mode)
        assert prof.stream_files == 0
        if mode == 1:                                       # (the 600-key case's tails do not all end in G: forward mode keeps it together)
            for pre, c, keys in planted:
                assert _subbucket(whi, wlo, wcn, low, _id_range(pre, min_top)) == (keys, c.m)
                assert sh.slots_quarter(keys) == c.slots


@pytest.mark.parametrize("k,min_top", [(31, 16), (51, 12)])
def test_countw_kernel_crowded_home_slots(ops, oracle_lib, torch_cuda, monkeypatch, k, min_top):
    """hash_countw_kernel (the index-claimed table; EMPTY = 0x0000FFFF): 8-byte keys with 40-bit suffixes (k = 31) and K96 records with
    84-bit ones, the high word part of the mix (k = 51): cases a and b in 128-key sub-buckets, 300 suffixes on the last slot of
    a 600-key sub-bucket's 1024.  (k = 51: sixteen filler k-mers per sub-bucket on average -- the sizes leave room for them.)"""
    monkeypatch.setenv("MGC_FINISH_MIN_TOP", str(min_top))
    monkeypatch.setenv("MGC_FINISH_NOLIST", "0")
    monkeypatch.setenv("MGC_HASH_STREAM", "0")
    low = 2 * k - 6 - min_top
    rng = np.random.default_rng(k * 100 + min_top)
    occ = _occupied(oracle_lib, k, low, (1, 0)) if k <= 32 else None
    planted, text = [], ""
    for name, head, keys in (("a", "AAC", 128), ("b", "ACA", 128), ("600", "ATT", 600)):
        c = sh.CASE["countw_k%d_%s" % (k, name)]
        if occ is not None:
            pre, _ = _pick_prefix(head, sh.case_plen(c), min_top, occ, rng)
        else:
            pre = head + "".join(sh.BASES[i] for i in rng.integers(0, 4, sh.case_plen(c) - len(head)))
        tails, _ = sh.case_tails(c, pre)
        text += _plant(pre, tails, keys, rng)
        planted.append((pre, c, keys))
    text += _filler(oracle_lib, k)
    for mode in (1, 0):
        whi, wlo, wcn, prof = _count_and_compare(ops, oracle_lib, text, k, mode)
        assert prof.stream_files == 0
        for pre, c, keys in planted:
            n, d = _subbucket(whi, wlo, wcn, low, _id_range(pre, min_top))
            assert keys <= n <= keys + 60 and d >= c.m and sh.slots_quarter(n) == c.slots, (n, d)


@pytest.mark.parametrize("k,min_top,modes", [(21, 16, (1,)), (40, 12, (1, 0))])
def test_oversized_subbucket_crowded_home_slots(ops, oracle_lib, torch_cuda, monkeypatch, k, min_top, modes):
    """The streaming kernels of oversized sub-buckets (hash_count_huge_body, 8192 slots; hash_count128_huge_body on K96 records, 4096):
    one sub-bucket of 20 000 keys whose 5000 distinct suffixes have their homes in 64 slots of the table."""
    monkeypatch.setenv("MGC_FINISH_MIN_TOP", str(min_top))
    low = 2 * k - 6 - min_top
    c = sh.CASE["huge_k%d" % k]
    rng = np.random.default_rng(k * 100 + min_top)
    pre = "AAC" + "".join(sh.BASES[i] for i in rng.integers(0, 4, sh.case_plen(c) - 3))
    tails, _ = sh.case_tails(c, pre)
    text = _plant(pre, tails, 20_000, rng) + _filler(oracle_lib, k)
    for mode in modes:
        whi, wlo, wcn, _ = _count_and_compare(ops, oracle_lib, text, k, mode)
        n, d = _subbucket(whi, wlo, wcn, low, _id_range(pre, min_top))
        assert 20_000 <= n <= 20_100 and d >= c.m, (n, d)
