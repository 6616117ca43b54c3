"""Host checks of tests/structured_helpers.py: every case the GPU module (test_count_structured_keys.py) plants really is a set of
distinct k-mers of ONE sub-bucket whose suffixes crowd a few home slots -- checked here without a GPU, so that an edit of the
helper (or of a hash it mirrors) cannot leave the GPU cases passing on ordinary, well-spread keys."""
import numpy as np
import pytest

import structured_helpers as sh


def _prefix(c, head="AAC", seed=1):
    rng = np.random.default_rng(seed)
    return head + "".join(sh.BASES[i] for i in rng.integers(0, 4, sh.case_plen(c) - len(head)))


@pytest.mark.parametrize("c", sh.CASES, ids=[c.name for c in sh.CASES])
def test_case_construction_bites(c):
    pre = _prefix(c)
    tails, homes = sh.case_tails(c, pre)
    low = 2 * c.k - 6 - c.min_top
    # m distinct tails of the right length, all in one sub-bucket, with m distinct suffixes
    assert len(tails) == c.m and len(set(tails)) == c.m
    assert all(len(t) == c.k - len(pre) for t in tails)
    if c.last:
        assert all(t[-1] == c.last for t in tails)
    kmers = [sh.encode(pre + t) for t in tails]
    assert len({x >> low for x in kmers}) == 1
    assert len({x & ((1 << low) - 1) for x in kmers}) == c.m
    # the homes, stated a second time on Python integers, lie in the window the case asks for
    again = sh.suffix_homes(c.k, c.min_top, pre, tails, c.slots, c.hash)
    assert np.array_equal(again, homes)
    start, width = sh.window_of(homes, c.slots)
    assert width <= c.width
    assert ((homes - sh.case_home(c)) % c.slots < c.width).all()
    # the pigeonhole bound and the simulation: more steps than the case has to force, in every order / in this one
    m = min(c.m, c.slots // 2) if c.kernel == "huge" else c.m        # (the streaming kernels: what ONE pass puts into the table)
    assert sh.pigeonhole_steps(m, c.width) >= c.steps
    for order in (homes, homes[::-1], np.random.default_rng(2).permutation(homes)):
        assert sh.linear_probe_max_steps(order[:m], c.slots) >= max(c.steps, sh.pigeonhole_steps(m, c.width))
    if c.kernel == "stream":
        assert c.m - c.width >= 70 and sh.linear_probe_max_steps(homes, c.slots) > sh.PROBE_MAX


@pytest.mark.parametrize("name", ["stream_b", "stream64_k31_b", "stream64_k28_b", "multi1_b", "multi24_b", "hash_b", "countw_k31_b", "countw_k51_b"])
def test_chain_wraps_past_the_last_slot(name):
    c = sh.CASE[name]
    _, homes = sh.case_tails(c, _prefix(c))
    assert (homes == c.slots - 1).all()
    # all but the first key wrap to slot 0 and go on from there: key i ends i steps from its home, at slot i - 1
    assert sh.linear_probe_max_steps(homes, c.slots) == c.m - 1


def test_stream_case_d_crowds_the_retry_table_too():
    """The home slot of a 2^11-entry table is the top eleven bits of the hash, that of the 2^13-entry retry table its top thirteen:
    ninety suffixes on one slot of the first lie in four neighbouring slots of the second, still more than PROBE_MAX steps deep."""
    c = sh.CASE["stream_d"]
    pre = _prefix(c)
    tails, homes = sh.case_tails(c, pre)
    retry = sh.suffix_homes(c.k, c.min_top, pre, tails, 8192, c.hash)
    assert (retry >> 2 == homes).all()
    assert sh.pigeonhole_steps(c.m, 4) > sh.PROBE_MAX and sh.linear_probe_max_steps(retry, 8192) > sh.PROBE_MAX


@pytest.mark.parametrize("R,tag", [(2, 1), (4, 1), (4, 3)])
def test_multi_tag_moves_all_homes_together(R, tag):
    """hash_count_multi_kernel hashes  suffix | tag << low_bits: the tag adds one constant to every product, so suffixes that
    share a home slot under tag 0 lie in two neighbouring slots under any other tag -- the neighbour sub-bucket of the range,
    planted with the same suffixes, crowds as well."""
    c = sh.CASE["multi24_a"]
    pre = _prefix(c)
    tails, _ = sh.case_tails(c, pre)
    low = 2 * c.k - 6 - c.min_top
    sfx = np.array([sh.encode(pre + t) & ((1 << low) - 1) for t in tails], dtype=np.uint64)
    h = sh.home_fib32(sfx, 0, c.slots, tag, low).astype(np.int64)
    assert sh.window_of(h, c.slots)[1] <= 2
    assert all(int(x) == sh.home_scalar("fib32", int(s), 0, c.slots, tag, low) for x, s in zip(h, sfx))


def test_slots_for_mirrors():
    assert [sh.slots_stream(n, 2048) for n in (1, 128, 129, 256, 257, 1024, 1025, 4094)] == [256, 256, 512, 512, 1024, 2048, 2048, 2048]
    assert [sh.slots_stream(n, 8192) for n in (128, 2500, 3000, 4094)] == [256, 8192, 8192, 8192]
    assert all(sh.slots_stream(n, 8192) >= 2 * n for n in range(1, sh.CAP_STREAM + 1))      # the retry table is at most half full
    assert [sh.slots_quarter(n) for n in (1, 205, 206, 240, 410, 411, 600, 819, 820, 1536)] == [256, 256, 512, 512, 512, 1024, 1024, 1024, 2048, 2048]


def test_linear_probe_simulation():
    assert sh.linear_probe_max_steps([0, 1, 2, 3], 8) == 0
    assert sh.linear_probe_max_steps([5, 5, 5], 8) == 2
    assert sh.linear_probe_max_steps([7, 7, 7], 8) == 2                  # 7, then 0 and 1: through the wrap
    assert sh.linear_probe_max_steps([6, 7, 6, 6], 8) == 3
    assert sh.window_of([7, 0, 1], 8) == (7, 3) and sh.window_of([3, 3], 8) == (3, 1)
    # the smallest suffixes on the last home slot of 256 are multiples of Fibonacci numbers
    s = np.arange(1, 1000, dtype=np.uint64)
    assert s[sh.home_fib32(s, 0, 256) == 255][:4].tolist() == [144, 377, 754, 987]
