"""Host checks of tests/wide_edge_helpers.py: the edges that tests/test_group_wide_edges.py is about really are in its inputs -- the
region sizes, the region starts off a 16-byte boundary, the tile remainders, the digit extremes, the dense ranks -- read back from
the integer keys at the digit positions of the plan each case asserts, without a GPU.  An edit of the helper cannot leave the GPU
cases passing on ordinary keys."""
import numpy as np
import pytest

import wide_edge_helpers as wh

_BUILT = {}


def _built(inp):
    """one input at a time (the cases that share one stand together)"""
    if inp not in _BUILT:
        _BUILT.clear()
        _BUILT[inp] = wh.build(inp)
    return _BUILT[inp]


def _hist(a, size):
    return np.bincount(a.astype(np.int64), minlength=size)


@pytest.mark.parametrize("c", wh.CASES, ids=[c.name for c in wh.CASES])
def test_the_edge_is_in_the_input(c):
    kind, plan, inp = c.kind, wh.PLANS[c.plan], c.inp
    tile = wh.TILE[kind.layout]
    x = _built(inp)
    k, n = kind.k, inp.n
    assert x.k == k and x.hi.size == n and x.lo.size == n
    # one file, and nothing above the 2k bits
    assert (wh.field(x.hi, x.lo, 2 * k - 6, 6) == wh.FILE).all()
    if 2 * k < 128:
        assert not (x.hi >> np.uint64(max(2 * k - 64, 0))).any()
    assert 2 * k - 6 - plan.t >= 32                                 # whole keys: 32 bits or more below the digits
    assert n * k >= 1 << 22                                         # the fifteen-bit histogram is in play
    a, b = wh.digits_of(k, x.hi, x.lo, c.plan)
    top = 242 if c.compress else (1 << plan.hi_bits) - 1
    ha = _hist(a, 512)
    hb = _hist(b, 1024)
    assert ha[top + 1:].sum() == 0
    # k-mers seen more than once are plenty, and so are k-mers seen once.  (The fewest repeats: n / 4 keys with random digits of
    # eighteen bits and one of two values below them -- 49152 keys in 2^19 cells, about 4400 of them not alone)
    _, _, cn = wh.unique_ref(x.hi, x.lo)
    assert cn[cn > 1].sum() >= 2000 and (cn == 1).sum() > 1000 and cn.sum() == n
    if inp.shape in ("planted", "hpc_planted"):
        want = wh.planted_sizes(tile)
        assert sorted(want.values()) == [0, 0, 1, tile - 1, tile, tile + 1, 2 * tile + 3]
        for v, size in want.items():
            assert ha[v] == size, (v, ha[v], size)
        assert ha[0] > 0 and ha[top] > 0 and ha[8:top].min() >= 0 and (ha[8:top] > 0).sum() > (top - 8) // 2
        # an empty region between occupied ones
        assert ha[1] > 0 and ha[2] == 0 and ha[3] > 0
        # where the regions start: the keys of all lower digits lie ahead
        start = np.concatenate(([0], np.cumsum(ha)))
        assert {v: int(start[v]) for v in want} == wh.planted_starts(tile)
        for v, size in want.items():
            if size in (tile - 1, tile + 1):
                assert start[v] % 2 == 1 and start[v] % 4 != 0, (v, start[v])   # off a 16-byte boundary as 8-byte and as 12-byte keys
        assert (start[4] * 12) % 16 and (start[4] * 8) % 16 and (start[1] * 12) % 16 and (start[1] * 8) % 16
    elif inp.shape == "ones_hi":
        assert ha[top] == n and top == (1 << plan.hi_bits) - 1
        assert (hb[:1 << plan.lo_bits] > 0).all()
    elif inp.shape == "one_lo":
        assert (hb > 0).sum() == 1 and (ha[:top + 1] > 0).all()
    elif inp.shape == "alt_hi":
        assert ha[0] == (n + 1) // 2 and ha[top] == n // 2
        assert (a[:6] == [0, top, 0, top, 0, top]).all()
    elif inp.shape == "ninth_hi":
        assert plan.hi_bits == 9 and sorted(np.flatnonzero(ha)) == [256, 384, 511]
    elif inp.shape == "ninth_lo":
        assert plan.lo_bits == 9 and sorted(np.flatnonzero(hb)) == [256, 384, 511]
    else:
        assert inp.shape in ("random", "hpc_random")
        assert (ha[:top + 1] > 0).all()                             # every high digit value, 0 and the highest included
    if c.compress:
        codes = wh.codes_of(k, x.hi, x.lo)
        assert (codes[:, 1:] != codes[:, :-1]).all()                # no base repeats the one before it
        assert ha[0] > 0 and ha[242] > 0 and ha[243:].sum() == 0
        if c.plan == "hpc1":
            assert hb[0] > 0 and hb[242] > 0 and hb[243:].sum() == 0
        else:
            assert hb[256:].sum() == 0 and 0 < (hb > 0).sum() <= 108   # four bases that repeat none, after any base: 4 * 27 patterns at most
    # the text is these keys
    text = wh.text_of(k, x.hi, x.lo)
    assert text.size == n * (k + 1)
    hi2, lo2 = wh.keys_of_text(k, text)
    assert np.array_equal(hi2, x.hi) and np.array_equal(lo2, x.lo)


@pytest.mark.parametrize("layout", ["u64", "k96", "k128"])
def test_edge_sizes_are_tile_edges(layout):
    tile = wh.TILE[layout]
    assert [n % tile for n in wh.N_EDGES] == [tile - 1, 0, 1]
    assert wh.N_ODD % tile == 1
    # the tail branch of a lane's fetch: a valid count that is no multiple of the vector
    assert layout == "k128" or (wh.N_ODD % tile) % wh.VEC[layout] != 0
    used = {c.inp.n for c in wh.CASES if c.kind.layout == layout and c.group == "edge"}
    assert used >= set(wh.N_EDGES)


def test_every_kind_and_plan_is_used():
    seen = {(c.kind.layout, c.plan) for c in wh.CASES if c.msd and not c.compress}
    for layout in ("u64", "k96", "k128"):
        assert {(layout, "t16"), (layout, "t18")} <= seen
    assert ("u64", "t17") in seen and ("u64", "t14") in seen
    assert {(c.inp.kind, c.plan) for c in wh.CASES if c.compress} == {("u64", "hpc1"), ("u64", "mixed"), ("k128", "hpc1"), ("k96", "hpc1")}
    assert {c.inp.kind for c in wh.CASES if not c.msd} == {"u64", "k96", "k96_k40", "k128", "k128_k51"}
    assert len({c.name for c in wh.CASES}) == len(wh.CASES)
    # cases that share an input stand together
    order = [c.inp for c in wh.CASES]
    runs = [x for i, x in enumerate(order) if i == 0 or order[i - 1] != x]
    assert len(runs) == len(set(runs))


def test_hpc_digit_is_the_dense_rank():
    """the rule restated in the helper against a plain enumeration: the 3^5 sequences that repeat no base after a given one, in order"""
    for prev in range(4):
        seqs = []
        for x in range(1024):
            c = [(x >> (8 - 2 * i)) & 3 for i in range(5)]
            if all(p != q for p, q in zip([prev] + c[:-1], c)):
                seqs.append(x)
        assert len(seqs) == 243
        got = wh.hpc_digit(np.array([(prev << 10) | x for x in seqs], dtype=np.uint64))
        assert np.array_equal(got, np.arange(243, dtype=np.uint64))


def test_unique_ref_and_fields_on_python_integers():
    rng = np.random.default_rng(5)
    for k in (26, 31, 40, 51, 64):
        top = rng.integers(0, 1 << 24, size=300, dtype=np.uint64)
        hi, lo = wh.compose(k, top, 24, rng, np.arange(300) % 3 == 0)
        big = [(int(h) << 64) | int(l) for h, l in zip(hi, lo)]
        assert all(x >> (2 * k - 24) == int(t) for x, t in zip(big, top)) and all(x >> (2 * k) == 0 for x in big)
        for shift, width in ((0, 9), (2 * k - 24, 9), (60, 9), (2 * k - 15, 9), (2 * k - 12, 12)):
            want = [(x >> shift) & ((1 << width) - 1) for x in big]
            assert [int(v) for v in wh.field(hi, lo, shift, width)] == want
        dup_hi, dup_lo = np.concatenate([hi, hi[:50]]), np.concatenate([lo, lo[:50]])
        uh, ul, cn = wh.unique_ref(dup_hi, dup_lo)
        from collections import Counter
        cnt = Counter(big + big[:50])
        keys = sorted(cnt)
        assert [(int(h) << 64) | int(l) for h, l in zip(uh, ul)] == keys and [int(v) for v in cn] == [cnt[x] for x in keys]
        text = wh.text_of(k, hi, lo).tobytes().decode()
        seqs = text.split(".")[:-1]
        assert all(len(s) == k for s in seqs)
        assert [sum("ACTG".index(ch) << (2 * (k - 1 - i)) for i, ch in enumerate(s)) for s in seqs] == big
