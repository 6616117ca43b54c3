"""The whole-key grouping passes (mgc_sort.hip, launch_group_wide: radix_group_kernel on u64 keys, 12-byte K96 records and K128
keys, with 256 and 512 counters, the first pass counting the low digit as it goes, the `compress` forms with the rank table in
LDS) at their tile, region and digit edges.  tests/wide_edge_helpers.py builds the inputs -- integer k-mers first, one file, the
digits where the plan puts them -- and tests/test_wide_edge_helpers_host.py checks without a GPU that the edges are in them.

Every case counts a whole input in a session and compares the whole result, keys and counts, with two references: the sorted
distinct integer keys the input was written from (nothing of the oracle in it), and the threaded port (`compress`: the oracle's
compression + its brute-force count).  Every case asserts its plan from the profile -- the file took the high-digit-first passes
on whole keys, with the digit widths the case is about (wide_digit_widths) and as the key kind the case is about (k96_files) --
rather than presuming it: mgc_group_route.hpp maps (key kind, widths, hpc) to one instantiation, tests/test_group_route_host.py
pins that map.

    widths 8 + 8 (and 7 + 7)      256 counters in both passes
    widths 9 + 8, 9 + 9           512 counters in both passes (t = 17: 256 of them in use in the first pass)
    `compress`, 10 + 10           dense ranks in both passes, off the rank table in LDS (u64, K128)
    `compress`, 10 + 8 (mixed)    a dense rank off the table, then 256 counters on the plain eight bits of four bases
    MGC_WIDE_MSD=0                the low digit first off a histogram read: the same result"""
import numpy as np
import pytest

import wide_edge_helpers as wh

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


_INPUT = {}                                                         # the latest input, its text and both references: cases that share one stand together


def _input(oracle_lib, inp, compress):
    """(keys, text, np.unique reference, oracle reference) of an input, computed once and left unchanged"""
    if inp not in _INPUT:
        _INPUT.clear()
        x = wh.build(inp)
        text = wh.text_of(x.k, x.hi, x.lo)
        assert text.size >= 1 << 22                                 # the fifteen-bit histogram, and with it the high digit first
        mine = wh.unique_ref(x.hi, x.lo)
        if compress:
            stream = oracle_lib.compress_stream(text.tobytes())
            assert stream == text.tobytes()                         # (nothing to compress)
            theirs = oracle_lib.count_brute(stream, x.k, wh.FORWARD)
        else:
            theirs = oracle_lib.count_threaded(text.tobytes(), x.k, _w_prefix(x.k, text.size), wh.FORWARD, threads=16)
        _INPUT[inp] = (x, text, mine, theirs)
    return _INPUT[inp]


def _w_prefix(k, n_bases):
    from meryl_amd import capi
    return capi.configure(k, n_bases, 4 << 30, wh.FORWARD).w_prefix


@pytest.mark.parametrize("c", wh.CASES, ids=[c.name for c in wh.CASES])
def test_whole_key_passes_at_their_edges(ops, oracle_lib, torch_cuda, monkeypatch, c):
    from meryl_amd import capi
    for name, value in c.environ().items():
        monkeypatch.setenv(name, value)
    x, text, (mhi, mlo, mcn), (whi, wlo, wcn, wni) = _input(oracle_lib, c.inp, c.compress)
    k, n = x.k, c.inp.n
    cfg = capi.configure(k, text.size, 4 << 30, wh.FORWARD, homopoly_compress=1) if c.compress else capi.configure(k, text.size, 4 << 30, wh.FORWARD)
    cfg.use_simple = 0
    with ops.Session(cfg) as s:
        s.set_profiling(True)
        s.push_bases_device(torch_cuda.from_numpy(text).cuda())
        s.count()
        klo, khi, counts, _ = s.result_wide()
        prof = s.profile()
        info = s.info()
    plan = wh.PLANS[c.plan]
    print("%s: wide_msd_files %d, wide_digit_widths %#x, k96_files %d, stream_files %d, hpc_mixed_files %d, pass_launches %s, pass_keys %s, distinct %d"
          % (c.name, prof.wide_msd_files, prof.wide_digit_widths, prof.k96_files, prof.stream_files, prof.hpc_mixed_files,
             list(prof.pass_launches), list(prof.pass_keys), info.n_distinct))
    # the integer keys the text was written from
    assert info.n_instances == n and info.n_distinct == len(mlo)
    assert np.array_equal(klo, mlo) and np.array_equal(khi, mhi) and np.array_equal(counts, mcn)
    # the oracle
    assert wni == n and len(wlo) == info.n_distinct
    assert np.array_equal(klo, wlo) and np.array_equal(khi, whi) and np.array_equal(counts, wcn)
    # which passes ran
    assert prof.pass_launches[1] > 0
    if c.msd:
        assert prof.wide_msd_files == 1
        assert prof.pass_keys[0] == n
        assert prof.wide_digit_widths == plan.widths, hex(prof.wide_digit_widths)
    else:
        assert prof.wide_msd_files == 0 and prof.wide_digit_widths == 0
    assert prof.k96_files == (1 if c.k96 else 0)
    assert prof.narrow_digit_widths == 0
    assert prof.stream_files == (1 if c.stream else 0)
    assert prof.hpc_mixed_files == (1 if c.plan == "mixed" else 0)
