"""mgc_dev_merge_many_* (mgc_merge_many.hip): 2..32 sorted (k-mer, value) streams merged in one count pass and one emit
pass, against a Python statement of the reference's k-way step (src/meryl/merylOp-nextMer.C:559-612 with
findMin/Max/SumCount and subtractCount, :23-62; a sum that wraps to 0 is kept, as the two-input merge keeps it) and
against the left fold of the two-input merge (mgc_dev_merge_*) over the same tensors."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

M32 = 0xFFFFFFFF
OP_WORDS = ["union-sum", "union-min", "union-max", "intersect-sum", "intersect-min", "intersect-max", "intersect", "subtract",
            "difference", "symmetric-difference", "union"]


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


def make_pool(rng, n_pool, kw):
    """distinct ascending keys as rows (lo, hi), drawn like test_device_merge_matches_numpy draws them: for 16-byte keys runs
    that share the high word (the low word decides) and a run that shares the low word (the high word decides)"""
    n_pool = max(n_pool, 1)
    lo = rng.integers(0, 1 << 62, n_pool, dtype=np.uint64)
    hi = rng.integers(0, 1 << 30, n_pool, dtype=np.uint64) if kw == 2 else np.zeros(n_pool, np.uint64)
    if kw == 2 and n_pool > 100:
        hi[: n_pool // 2] = hi[0]
        lo[n_pool // 2: n_pool // 2 + 50] = lo[n_pool // 2]
    order = np.lexsort((lo, hi))
    pool = np.stack([lo[order], hi[order]], axis=1)
    keep = np.ones(pool.shape[0], bool)
    keep[1:] = np.any(pool[1:] != pool[:-1], axis=1)
    return pool[keep]


def draw(rng, pool, n):
    n = min(n, pool.shape[0])
    idx = np.sort(rng.choice(pool.shape[0], n, replace=False)) if n else np.zeros(0, np.int64)
    return pool[idx]


def shapes(N, T):
    """name -> builder(rng, kw) of the list of key arrays"""
    def sizes_summing_to(total):
        s = [total // N] * N
        s[0] += total - sum(s)
        return s

    def overlapping(sizes, share=0.5):
        def b(rng, kw):
            pool = make_pool(rng, int(max(sizes) + sum(sizes) * (1.0 - share) / 2) + 64, kw)
            return [draw(rng, pool, n) for n in sizes]
        return b

    def identical(rng, kw):
        a = make_pool(rng, 700, kw)
        return [a.copy() for _ in range(N)]

    def disjoint(rng, kw):
        pool = make_pool(rng, 300 * N, kw)
        which = rng.integers(0, N, pool.shape[0])
        return [pool[which == i] for i in range(N)]

    def group_at(pos):
        """a k-mer held by all N inputs whose group begins at merged position `pos`"""
        def b(rng, kw):
            pool = make_pool(rng, pos + 1 + T + 64, kw)
            below, x, above = pool[:pos], pool[pos:pos + 1], pool[pos + 1:]
            assert below.shape[0] == pos
            which = rng.integers(0, N, pos)                          # every smaller k-mer in exactly one input: pos elements before the group
            return [np.concatenate([below[which == i], x, draw(rng, above, above.shape[0] // 2)]) for i in range(N)]
        return b

    def single_elements(rng, kw):
        pool = make_pool(rng, 3, kw)
        return [draw(rng, pool, 1) for _ in range(N)]

    return {
        "all-empty": overlapping([0] * N),
        "one-empty": overlapping([700 if i != N // 2 else 0 for i in range(N)]),
        "single-elements": single_elements,
        "sum-T-1": overlapping(sizes_summing_to(T - 1)),
        "sum-T": overlapping(sizes_summing_to(T)),
        "sum-T+1": overlapping(sizes_summing_to(T + 1)),
        "sum-3T+17": overlapping(sizes_summing_to(3 * T + 17)),
        "identical": identical,
        "disjoint": disjoint,
        "one-large": overlapping([100_000] + [10] * (N - 1), share=1.0),
        "group-at-T-1": group_at(T - 1),
        "group-at-T": group_at(T),
        "group-at-T+1": group_at(T + 1),
    }


SHAPE_NAMES = sorted(shapes(2, 64))


def key_ints(a):
    return [(int(h) << 64) | int(l) for l, h in zip(a[:, 0].tolist(), a[:, 1].tolist())]


def special_values(N):
    """values of the k-mers every input holds: sums that wrap past 2^32 and to exactly 0; subtract with the first value above,
    equal to and below the sum of the others, and above the second but not above what is left for the third"""
    rows = [[M32] * N]                                                             # wraps past 2^32 (for N >= 2)
    rest = [0x40000000 + 17 * i for i in range(N - 1)]
    rows.append(rest + [(-sum(rest)) & M32])                                        # wraps to exactly 0
    rows.append([1000 * N] + [1] * (N - 1))                                         # a above the sum of the others
    rows.append([N - 1] + [1] * (N - 1))                                            # a equal to it
    rows.append([1] + [5] * (N - 1))                                                # a below
    rows.append(([10, 4, 6] + [1] * N)[:N])                                         # a > b, a - b <= c
    assert all(v > 0 for r in rows for v in r)
    return rows


def model(groups, N, op):
    """merylOp-nextMer.C:559-612 over groups = [(k-mer, [(input, value), ...] in input order)] in k-mer order; zero sums kept"""
    out = []
    for key, act in groups:
        idx0, vals = act[0][0], [v for _, v in act]
        n = len(act)
        if op == 10:
            v = n
        elif op in (0, 3):
            v = sum(vals) & M32
        elif op in (1, 4):
            v = min(vals)
        elif op in (2, 5):
            v = max(vals)
        else:
            v = vals[0]
        if op in (3, 4, 5, 6) and n != N:
            continue
        if op == 7:
            if idx0 != 0:
                continue
            dropped = False
            for c in vals[1:]:                                                      # subtractCount, :51-62
                if v > c:
                    v -= c
                else:
                    dropped = True
                    break
            if dropped:
                continue
        if op == 8 and not (n == 1 and idx0 == 0):
            continue
        if op == 9 and n != 1:
            continue
        out.append((key, v))
    return out


def fold(ops, torch, dk, dc, op):
    """the left fold of the two-input merge, as mgc_db_merge runs it: symmetric-difference over more than two inputs is the
    union-sum of the values where the union-sum of ones is 1"""
    word = OP_WORDS[op]
    if op == 9 and len(dk) > 2:
        k, c = dk[0], dc[0]
        m = torch.ones_like(dc[0])
        for i in range(1, len(dk)):
            k2, c = ops.dev_merge(k, c, dk[i], dc[i], "union-sum")
            _, m = ops.dev_merge(k, m, dk[i], torch.ones_like(dc[i]), "union-sum")
            k = k2
        sel = m == 1
        return k[sel], c[sel]
    k, c = dk[0], dc[0]
    for i in range(1, len(dk)):
        k, c = ops.dev_merge(k, c, dk[i], dc[i], word)
    return k, c


@pytest.mark.parametrize("shape", SHAPE_NAMES)
@pytest.mark.parametrize("kw", [1, 2])
@pytest.mark.parametrize("N", [2, 3, 5, 32])
def test_merge_many_matches_the_reference_step_and_the_left_fold(ops, torch_cuda, native_lib, N, kw, shape):
    torch = torch_cuda
    T = native_lib.mgc_dev_merge_many_tile(kw)
    assert 64 <= T <= 1 << 16
    rng = np.random.default_rng(1000 * N + 10 * kw + SHAPE_NAMES.index(shape))
    keys = shapes(N, T)[shape](rng, kw)
    assert len(keys) == N
    vals = [rng.integers(1, 1000, a.shape[0]).astype(np.uint32) for a in keys]
    for v in vals[::2]:
        v[::3] = rng.integers(1, M32, v[::3].size, dtype=np.uint64).astype(np.uint32)
    ints = [key_ints(a) for a in keys]
    where = [dict(zip(ki, range(len(ki)))) for ki in ints]
    everywhere = sorted(set(ints[0]).intersection(*[set(k) for k in ints[1:]]))
    for key, row in zip(everywhere, special_values(N)):
        for i in range(N):
            vals[i][where[i][key]] = row[i]
    if shape.startswith("group-at"):                                                 # the group does begin where the case says
        pos = {"group-at-T-1": T - 1, "group-at-T": T, "group-at-T+1": T + 1}[shape]
        assert len(everywhere) >= 1 and sum(sum(1 for k in ki if k < everywhere[0]) for ki in ints) == pos
    if shape.startswith("sum-"):
        assert sum(len(k) for k in ints) == {"sum-T-1": T - 1, "sum-T": T, "sum-T+1": T + 1, "sum-3T+17": 3 * T + 17}[shape]
    act = {}
    for i in range(N):
        for key, v in zip(ints[i], vals[i].tolist()):
            act.setdefault(key, []).append((i, v))
    groups = sorted(act.items())

    def dev(a, c):
        if kw == 2:
            k_ = torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy()).cuda().view(-1, 2)
        else:
            k_ = torch.from_numpy(np.ascontiguousarray(a[:, 0]).view(np.int64).copy()).cuda()
        return k_, torch.from_numpy(c.view(np.int32).copy()).cuda()
    dk, dc = zip(*[dev(a, c) for a, c in zip(keys, vals)])

    def host(k, c):
        gk = k.cpu().numpy().view(np.uint64)
        got = [(int(r[1]) << 64) | int(r[0]) for r in gk.reshape(-1, 2).tolist()] if kw == 2 else [int(x) for x in gk.tolist()]
        return got, c.cpu().numpy().view(np.uint32).tolist()

    for op in range(11):
        ok, oc = ops.dev_merge_many(list(dk), list(dc), op)
        want = model(groups, N, op)
        got_k, got_c = host(ok, oc)
        assert got_k == [k for k, _ in want], (OP_WORDS[op], len(got_k), len(want))
        assert got_c == [v for _, v in want], OP_WORDS[op]
        if op == 10:
            continue                                                                 # the two-input merge has no `union`
        fk, fc = fold(ops, torch, dk, dc, op)
        assert torch.equal(fk, ok) and torch.equal(fc, oc), OP_WORDS[op]


def test_merge_many_refuses_bad_arguments(ops, torch_cuda, native_lib):
    from meryl_amd import capi
    torch = torch_cuda
    L = native_lib
    k = torch.arange(1, 9, dtype=torch.int64, device="cuda")
    c = torch.ones(8, dtype=torch.int32, device="cuda")
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    n_out = ctypes.c_uint64(0)

    def call(n_inputs, op):
        kp = (ctypes.c_void_p * n_inputs)(*[k.data_ptr()] * n_inputs)
        cp = (ctypes.c_void_p * n_inputs)(*[c.data_ptr()] * n_inputs)
        ns = (ctypes.c_uint64 * n_inputs)(*[8] * n_inputs)
        rc = L.mgc_dev_merge_many_count(kp, cp, ns, n_inputs, 1, op, ws.data_ptr(), ws.numel(), ctypes.byref(n_out), None)
        rc2 = L.mgc_dev_merge_many_emit(kp, cp, ns, n_inputs, 1, op, ws.data_ptr(), ws.numel(), k.data_ptr(), c.data_ptr(), None)
        return rc, rc2
    assert call(1, 0) == (capi.MGC_EINVAL, capi.MGC_EINVAL)
    assert call(33, 0) == (capi.MGC_EINVAL, capi.MGC_EINVAL)
    assert call(2, 11) == (capi.MGC_EINVAL, capi.MGC_EINVAL)
    assert call(2, -1) == (capi.MGC_EINVAL, capi.MGC_EINVAL)
    assert L.mgc_dev_merge_many_count(None, None, None, 2, 1, 0, ws.data_ptr(), ws.numel(), ctypes.byref(n_out), None) == capi.MGC_EINVAL
    torch.cuda.synchronize()
