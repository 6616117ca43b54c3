"""K-mer text lists formatted on the device: mgc_list_kmers (db.format_kmers), lists of operation-tree nodes (mgc_db_eval_listed) and
the command line's print of an operation.  The expected text is written here, line by line, from the key bits, str(value)
and the label's bits; nothing of it comes from the library."""
import os
import subprocess

import numpy as np
import pytest

import eval_helpers as H
import label_helpers as LH
from test_labels import dir_bytes

pytestmark = pytest.mark.gpu

MGC_EINVAL, MGC_ESTATE = -1, -4
KS = (1, 16, 31, 32, 33, 64)
LABEL_SIZES = (0, 1, 63, 64)
SPECIAL_VALUES = (0, 9, 10, 999999999, 1000000000, 4294967295)


@pytest.fixture(scope="module")
def torch_cuda(native_lib):
    import torch
    from meryl_amd import capi
    assert torch.cuda.is_available(), "the -m gpu tests need a GPU"
    torch.cuda.set_device(0)
    assert (capi.MGC_EINVAL, capi.MGC_ESTATE) == (MGC_EINVAL, MGC_ESTATE)
    return torch


def line(key, value, label, k, label_size):
    """one line as printKmer writes it; key: the k-mer's 2k bits as a Python int"""
    text = "".join("ACTG"[(key >> (2 * (k - 1 - b))) & 3] for b in range(k)) + "\t" + str(value)
    if label_size:
        text += "\t" + format(label & ((1 << label_size) - 1), "0%db" % label_size)
    return (text + "\n").encode()


def sample(k, label_size, n, seed=0):
    """n k-mers (any order: the lister does not care), values of every decimal length, labels of 64 random bits
    -> (keys as Python ints, values, labels, the expected lines)"""
    rng = np.random.default_rng(1000 * k + label_size + seed)
    bits = 2 * k
    keys = [int.from_bytes(rng.bytes(16), "little") & ((1 << bits) - 1) for _ in range(n)]
    keys[1 % n], keys[2 % n] = 0, (1 << bits) - 1
    digits = rng.integers(1, 11, n)
    values = [int(rng.integers(0 if d == 1 else 10 ** (d - 1), min(10 ** d, 1 << 32))) for d in digits.tolist()]
    for i, v in enumerate(SPECIAL_VALUES):
        values[(3 + 2 * i) % n] = v
    labels = [int.from_bytes(rng.bytes(8), "little") for _ in range(n)]
    labels[0], labels[4 % n] = 0, (1 << 64) - 1
    return keys, values, labels, [line(a, v, l, k, label_size) for a, v, l in zip(keys, values, labels)]


def on_device(torch, keys, values, labels, k):
    m64 = (1 << 64) - 1
    words = [[a & m64, a >> 64] for a in keys] if k > 32 else [a & m64 for a in keys]
    to = lambda a, dt, view: torch.from_numpy(np.ascontiguousarray(np.array(a, dtype=dt)).view(view)).cuda()    # noqa: E731
    return to(words, np.uint64, np.int64), to(values, np.uint32, np.int32), to(labels, np.uint64, np.int64)


@pytest.mark.parametrize("label_size", LABEL_SIZES)
@pytest.mark.parametrize("k", KS)
def test_format_kmers_over_the_grid(torch_cuda, k, label_size):
    from meryl_amd import db
    max_line, T = db.list_geometry(k, label_size)
    assert T in (256, 512, 1024)
    keys, values, labels, lines = sample(k, label_size, 3 * T + 5)
    assert {len(str(v)) for v in values} == set(range(1, 11))
    assert {len(x) for x in lines} == {max_line - (0 if label_size else 1) - 10 + d for d in range(1, 11)}
    dk, dv, dl = on_device(torch_cuda, keys, values, labels, k)

    def fmt(s, e):
        return db.format_kmers(dk[s:e], dv[s:e], dl[s:e] if label_size else None, k=k, label_size=label_size)
    for n in (0, 1, T - 1, T, T + 1, 3 * T + 5):
        assert fmt(0, n) == b"".join(lines[:n]), (k, label_size, n)
    # a second tile that starts at every alignment of the 16-byte stores (head and tail bytes): the line lengths vary, so the text
    # of the T k-mers from s on has every length modulo 16 for some s
    starts = np.cumsum([0] + [len(x) for x in lines])
    first_s = {}
    for s in range(2 * T):
        first_s.setdefault(int(starts[s + T] - starts[s]) % 16, s)
    assert sorted(first_s) == list(range(16))
    for s in first_s.values():
        assert fmt(s, s + T + 3) == b"".join(lines[s:s + T + 3]), (k, label_size, s)
    # the two passes on their own: the whole text, left on the device
    text = db.format_kmers_device(dk, dv, dl if label_size else None, k=k, label_size=label_size)
    assert text.is_cuda and bytes(text.cpu().numpy()) == b"".join(lines)
    if label_size:                                                  # no labels given: zeros
        got = db.format_kmers(dk[:5], dv[:5], None, k=k, label_size=label_size)
        assert got == b"".join(line(a, v, 0, k, label_size) for a, v in zip(keys[:5], values[:5]))


@pytest.mark.parametrize("k,label_size", [(21, 0), (33, 5), (64, 64)])
def test_pieces_hold_whole_lines_and_at_most_chunk_bytes(torch_cuda, k, label_size):
    from meryl_amd import capi, db
    max_line, T = db.list_geometry(k, label_size)
    n = 3 * T + 5
    keys, values, labels, lines = sample(k, label_size, n, seed=7)
    want = b"".join(lines)
    dk, dv, dl = on_device(torch_cuda, keys, values, labels, k)
    tile_text = sum(len(x) for x in lines[:T])
    for chunk in (max_line, max_line + 1, tile_text - 1, tile_text, 2 * tile_text + 17, 1 << 30):
        pieces = []
        got = db.format_kmers(dk, dv, dl, k=k, label_size=label_size, chunk_bytes=chunk, on_piece=lambda p: pieces.append(p) and False)
        assert got == want == b"".join(pieces), chunk
        assert all(0 < len(p) <= chunk and p.endswith(b"\n") for p in pieces), chunk
        assert len(pieces) >= -(-len(want) // chunk)
    with pytest.raises(capi.MgcError) as e:
        db.format_kmers(dk, dv, dl, k=k, label_size=label_size, chunk_bytes=max_line - 1)
    assert e.value.code == MGC_EINVAL and "shorter than the longest line" in str(e.value)
    # a callback that says stop on its second call: MGC_ESTATE, and no third call
    calls = []
    with pytest.raises(capi.MgcError) as e:
        db.format_kmers(dk, dv, dl, k=k, label_size=label_size, chunk_bytes=max_line + 40, on_piece=lambda p: calls.append(p) or len(calls) == 2)
    assert e.value.code == MGC_ESTATE and len(calls) == 2 and b"".join(calls) == want[:sum(map(len, calls))]
    # the lister is whole again afterwards
    assert db.format_kmers(dk[:9], dv[:9], dl[:9], k=k, label_size=label_size) == b"".join(lines[:9])


# ---- lists of the nodes of a tree ----------------------------------------------------------------------------------------------------
def small_db(path, k, wp, n, seed, label_size=0):
    """a database of about n random k-mers with values 1..6 (and labels of label_size random bits) -> {key: (value, label)}"""
    rng = np.random.default_rng(seed)
    lo, hi = H.random_kmers(rng, k, n)
    cn = rng.integers(1, 7, lo.size).astype(np.uint32)
    cn[::11] = np.uint32(4294967295 - 3)
    lab = rng.integers(0, 1 << label_size, lo.size, dtype=np.uint64) if label_size else np.zeros(lo.size, np.uint64)
    if label_size:
        LH.write_labelled_db(str(path), lo, hi, cn, lab, k, wp, label_size)
    else:
        H.write_db(str(path), lo, hi, cn, k, wp)
    return {(int(h) << 64) | int(l): (int(c), int(b)) for l, h, c, b in zip(lo.tolist(), hi.tolist(), cn.tolist(), lab.tolist())}


def pool_db(path, k, wp, pool, take, seed):
    """a database of some of the k-mers of `pool` (so that databases share k-mers)"""
    rng = np.random.default_rng(seed)
    lo, hi = pool
    idx = np.sort(rng.choice(lo.size, take, replace=False))
    cn = rng.integers(1, 7, idx.size).astype(np.uint32)
    H.write_db(str(path), lo[idx], hi[idx], cn, k, wp)
    return {(int(h) << 64) | int(l): int(c) for l, h, c in zip(lo[idx].tolist(), hi[idx].tolist(), cn.tolist())}


def text_of(kmers, k, label_size=0):
    """{key: value} or {key: (value, label)} -> the list, ascending by k-mer (= files ascending, k-mers ascending inside a file)"""
    out = []
    for key in sorted(kmers):
        v = kmers[key]
        out.append(line(key, v[0], v[1], k, label_size) if isinstance(v, tuple) else line(key, v, 0, k, 0))
    return b"".join(out)


def collect(tree, **kw):
    """evaluate_listed -> {node: text}, {node: [files in call order]}; every piece holds whole lines of its file"""
    from meryl_amd import db
    texts, files = {}, {}

    def on_text(node, ff, piece):
        assert piece and piece.endswith(b"\n")
        texts[node] = texts.get(node, b"") + piece
        files.setdefault(node, []).append((ff, piece))
    hists = db.evaluate_listed(tree, on_text, **kw)
    return texts, files, hists


def check_files(pieces, k):
    """the file arguments ascend, and every k-mer handed over for file f has f as its top six bits"""
    ffs = [ff for ff, _ in pieces]
    assert ffs == sorted(ffs) and len(set(ffs)) > 1
    code = {"A": 0, "C": 1, "T": 2, "G": 3}
    for ff, piece in pieces:
        for ln in piece.split(b"\n")[:-1]:
            first = ln.decode()[:3]
            assert (code[first[0]] << 4 | code[first[1]] << 2 | code[first[2]]) == ff, (ff, ln)


@pytest.mark.parametrize("k", [21, 51])
def test_root_inner_node_and_leaf_lists(torch_cuda, tmp_path, k):
    wp = H.CONFIGS[k]
    pool = H.random_kmers(np.random.default_rng(k), k, 900)
    a, b = pool_db(tmp_path / "a", k, wp, pool, 600, 1), pool_db(tmp_path / "b", k, wp, pool, 500, 2)
    inner = {key: v for key, v in a.items() if v >= 2}
    root = dict(b)
    for key, v in inner.items():
        root[key] = (root.get(key, 0) + v) & 0xFFFFFFFF
    assert 0 < len(inner) < len(a) and len(root) > len(b) and len(set(inner) & set(b)) > 50
    tree = ("union-sum", ("at-least", 2, str(tmp_path / "a"), {"list": True}), {"database": str(tmp_path / "b"), "list": True},
            {"list": True, "histogram": True, "output": str(tmp_path / "u")})
    texts, files, hists = collect(tree)
    # node indices: children before their parent -- a (0), at-least (1), b (2), union-sum (3)
    assert sorted(texts) == [1, 2, 3]
    assert texts[1] == text_of(inner, k) and texts[2] == text_of(b, k) and texts[3] == text_of(root, k)
    for node in (1, 2, 3):
        check_files(files[node], k)
    assert len(hists) == 1 and int((hists[0][0] * hists[0][1]).sum()) == sum(root.values())
    # what the root listed is what its output holds
    from meryl_amd import db
    r = db.Reader(str(tmp_path / "u"))
    lo, hi, cn = r.read_all()
    r.close()
    assert text_of({(int(h) << 64) | int(l): int(c) for l, h, c in zip(lo.tolist(), hi.tolist(), cn.tolist())}, k) == texts[3]
    # small pieces: the same text, MGC_LIST_CHUNK being what the evaluation reads
    os.environ["MGC_LIST_CHUNK"] = "1"                              # (raised to one line)
    try:
        small, _, _ = collect(("union-sum", ("at-least", 2, str(tmp_path / "a")), str(tmp_path / "b"), {"list": True}))
    finally:
        del os.environ["MGC_LIST_CHUNK"]
    assert small[3] == texts[3]


def test_a_labelled_tree_lists_the_label_column(torch_cuda, tmp_path):
    k, wp, L = 21, 10, 5
    a, b = small_db(tmp_path / "a", k, wp, 700, 3, label_size=L), small_db(tmp_path / "b", k, wp, 700, 4, label_size=3)
    some = sorted(a)[::2]
    lo = np.array([key & ((1 << 64) - 1) for key in some], dtype=np.uint64)
    shared = {key: (3, 0b10001) for key in some}
    LH.write_labelled_db(str(tmp_path / "c"), lo, np.zeros(lo.size, np.uint64), np.full(lo.size, 3, np.uint32), np.full(lo.size, 0b10001, np.uint64), k, wp, L)
    want = {}
    for d in (a, b, shared):
        for key, (v, lab) in d.items():
            pv, pl = want.get(key, (0, 0))
            want[key] = ((pv + v) & 0xFFFFFFFF, pl | lab)
    tree = ("union-sum", str(tmp_path / "a"), str(tmp_path / "b"), str(tmp_path / "c"), {"label": "or", "list": True})
    texts, files, _ = collect(tree, with_labels=True)
    assert texts[3] == text_of(want, k, L) and texts[3].count(b"\t") == 2 * len(want)
    check_files(files[3], k)
    # -l style: the label column takes label_size bits
    texts, _, _ = collect(tree, with_labels=True, label_size=9)
    assert texts[3] == text_of(want, k, 9)
    # a database whose root is a leaf: how `print <db>` arrives
    texts, _, _ = collect({"database": str(tmp_path / "a"), "list": True}, with_labels=True)
    assert texts[0] == text_of(a, k, L)


def test_nothing_flagged_writes_the_bytes_of_the_reported_evaluation(torch_cuda, tmp_path):
    from meryl_amd import db
    k, wp = 21, 10
    pool = H.random_kmers(np.random.default_rng(5), k, 900)
    for name, seed in (("a", 1), ("b", 2), ("c", 3)):
        pool_db(tmp_path / name, k, wp, pool, 500, seed)
    p = lambda n: str(tmp_path / n)                                # noqa: E731
    tree = lambda d: ("subtract", ("union-sum", p("a"), p("b"), p("c"), {"select": ["value:>=3"], "output": str(tmp_path / d / "inner")}),   # noqa: E731
                      ("at-most", 4, p("b"), {"value": "mul#3"}), {"output": str(tmp_path / d / "root"), "histogram": True})
    for d in ("rep", "lst"):
        os.makedirs(tmp_path / d)
    rep = db.evaluate_reported(tree("rep"))
    called = []
    lst = db.evaluate_listed(tree("lst"), lambda *a: called.append(a))
    assert called == [] and len(rep) == len(lst) == 1 and all((x == y).all() for x, y in zip(rep[0], lst[0]))
    for name in ("inner", "root"):
        assert dir_bytes(str(tmp_path / "lst" / name)) == dir_bytes(str(tmp_path / "rep" / name)), name
    assert len(dir_bytes(str(tmp_path / "lst" / "root"))) == 129


def test_a_callback_that_fails_stops_the_evaluation(torch_cuda, tmp_path):
    from meryl_amd import db
    pool = H.random_kmers(np.random.default_rng(9), 21, 400)
    pool_db(tmp_path / "a", 21, 10, pool, 300, 1)
    seen = []

    def on_text(node, ff, piece):
        seen.append(ff)
        if len(seen) == 3:
            raise KeyError("stop")
    with pytest.raises(KeyError):
        db.evaluate_listed(("at-least", 1, str(tmp_path / "a"), {"list": True}), on_text)
    assert len(seen) == 3


# ---- the command line ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def meryl(native_lib):
    from meryl_amd import build
    path = build.build_cli()
    assert os.path.exists(path)
    return path


@pytest.fixture(scope="module")
def cli_world(tmp_path_factory):
    d = tmp_path_factory.mktemp("list_cli")
    k, wp = 21, 10
    pool = H.random_kmers(np.random.default_rng(21), k, 3000)
    a, b = pool_db(d / "a", k, wp, pool, 2000, 1), pool_db(d / "b", k, wp, pool, 1500, 2)
    union = dict(b)
    for key, v in a.items():
        union[key] = union.get(key, 0) + v
    return d, k, a, b, union


def run(meryl, *args, env=None):
    r = subprocess.run([meryl, "-Q"] + [str(x) for x in args], capture_output=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr.decode()
    return r.stdout


def test_cli_print_of_an_operation_and_small_pieces(torch_cuda, meryl, native_lib, cli_world, tmp_path):
    d, k, a, b, union = cli_world
    want = text_of(union, k)
    tree = ["[union-sum", d / "a", str(d / "b") + "]"]
    assert run(meryl, "print", *tree) == want
    # the tree's root written as a database and printed from it by the host reader: the same bytes
    assert run(meryl, "print", "[union-sum", d / "a", d / "b", "output", str(tmp_path / "u.meryl") + "]") == want
    assert run(meryl, "print", tmp_path / "u.meryl") == want
    # pieces of one line: the same bytes again
    env = dict(os.environ, MGC_LIST_CHUNK=str(native_lib.mgc_list_max_line(k, 0)))
    assert run(meryl, "print", *tree, env=env) == want
    assert run(meryl, "print", "[at-least", "3", str(d / "a") + "]", env=env) == text_of({key: v for key, v in a.items() if v >= 3}, k)
    # a tree that also reports keeps its path: the same k-mers, the report after them
    both = run(meryl, "print", "[union-sum", "output:histogram", d / "a", str(d / "b") + "]")
    assert both.startswith(want) and len(both) > len(want)
    assert run(meryl, "print", d / "a", env=env) == text_of(a, k)
