"""Labels through the operation trees (meryl2; merylOpCompute::findOutputLabel, src/meryl2/merylOpCompute.C:286-395), on the
device: the labelled merge_many and select emits against the Python statement of the label table in label_helpers.py (beside
the value rules tests/test_merge_many.py states), the device decoder and encoder against the host codec for labelled
databases, whole trees through evaluate_labelled read back with the host reader, and the command line.  Everything is exact."""
import os
import subprocess
import sys

import numpy as np
import pytest

import label_helpers as LH
import test_merge_many as TM

pytestmark = pytest.mark.gpu

M32, M64 = LH.M32, LH.M64
SELECT_TILE = 2048                               # SL_TILE of mgc_merge.hip


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


def u64_tensor(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64).copy()).cuda()


def key_tensor(torch, a, kw):
    if kw == 2:
        return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy()).cuda().view(-1, 2)
    return torch.from_numpy(np.ascontiguousarray(a[:, 0]).view(np.int64).copy()).cuda()


def host_keys(k, kw):
    gk = k.cpu().numpy().view(np.uint64)
    return [(int(r[1]) << 64) | int(r[0]) for r in gk.reshape(-1, 2).tolist()] if kw == 2 else [int(x) for x in gk.tolist()]


def random_labels(rng, n):
    """over the full 64 bits"""
    return rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n, dtype=np.uint64)


class Inputs:
    """N sorted streams with values and labels on the device, and their groups for the model; input `null_input` is passed
    without a label buffer (its labels are zeros)"""

    def __init__(self, torch, rng, keys, kw, null_input):
        self.N, self.kw = len(keys), kw
        self.keys = keys
        self.ints = [TM.key_ints(a) for a in keys]
        self.vals = [rng.integers(1, 1000, a.shape[0]).astype(np.uint32) for a in keys]
        for v in self.vals[::2]:
            v[::3] = rng.integers(1, M32, v[::3].size, dtype=np.uint64).astype(np.uint32)
        self.labs = [random_labels(rng, a.shape[0]) for a in keys]
        if null_input is not None:
            self.labs[null_input][:] = 0
        self.null_input = null_input
        self.where = [dict(zip(ki, range(len(ki)))) for ki in self.ints]
        self.everywhere = sorted(set(self.ints[0]).intersection(*[set(k) for k in self.ints[1:]])) if self.N > 1 else list(self.ints[0])
        self.torch = torch

    def set_row(self, key, vals=None, labs=None):
        for i in range(self.N):
            if vals is not None:
                self.vals[i][self.where[i][key]] = vals[i]
            if labs is not None and i != self.null_input:
                self.labs[i][self.where[i][key]] = labs[i]

    def upload(self):
        t = self.torch
        self.dk = [key_tensor(t, a, self.kw) for a in self.keys]
        self.dc = [t.from_numpy(c.view(np.int32).copy()).cuda() for c in self.vals]
        self.dl = [None if i == self.null_input else u64_tensor(t, l) for i, l in enumerate(self.labs)]
        act = {}
        for i in range(self.N):
            for key, v, l in zip(self.ints[i], self.vals[i].tolist(), self.labs[i].tolist()):
                act.setdefault(key, []).append((i, v, l))
        self.act = act
        self.groups = sorted((key, [(i, v) for i, v, _ in a]) for key, a in act.items())

    def want(self, op, word, c):
        """[(k-mer, value, label)]: the value rules of test_merge_many.model, the label table of label_helpers.label_of"""
        out = []
        for key, v in TM.model(self.groups, self.N, op):
            a = self.act[key]
            out.append((key, v, LH.label_of(word, c, [l for _, _, l in a], [vv for _, vv, _ in a], merge_op=op)))
        return out

    def check(self, ops, op, word, c=None):
        cc = LH.DEFAULT_CONSTANT.get(word, 0) if c is None else c
        ok, oc, ol = ops.dev_merge_many_labelled(self.dk, self.dc, self.dl, op, word, c)
        want = self.want(op, word, cc)
        what = (TM.OP_WORDS[op], word, c)
        assert host_keys(ok, self.kw) == [k for k, _, _ in want], what
        assert oc.cpu().numpy().view(np.uint32).tolist() == [v for _, v, _ in want], what
        assert ol.cpu().numpy().view(np.uint64).tolist() == [l for _, _, l in want], what
        return len(want)


def special_rows(inp):
    """rows of the k-mers every input holds: a value of 2^32-1 everywhere and in input 0 only (MIN), labels of equal popcount
    (LIGHTEST / HEAVIEST ties), and a lighter / heavier label in a later input"""
    N = inp.N
    ev = inp.everywhere
    rows = [
        dict(vals=[M32] * N),                                                         # MIN: nobody wins, the constant stays
        dict(vals=[M32] + [7] * (N - 1)),                                             # MIN: input 0 never wins
        dict(vals=[9] * N),                                                           # equal values: the first input wins
        dict(labs=[(0b0011 << (i % 60)) for i in range(N)]),                          # popcount ties among the inputs: the first stays
        dict(labs=[0b1001] * N),                                                      # ... and with the constant 0b1001
        dict(labs=[0xFF] * (N - 1) + [0x1]),                                          # the lightest comes last
        dict(labs=[0x1] * (N - 1) + [0xFFFF]),                                        # the heaviest comes last
    ]
    used = 0
    for key, row in zip(ev, rows):
        inp.set_row(key, **row)
        used += 1
    return used


@pytest.mark.parametrize("shape", ["sum-3T+17", "group-at-T"])
@pytest.mark.parametrize("kw", [1, 2])
@pytest.mark.parametrize("N", [2, 32])
def test_every_label_operation(ops, torch_cuda, native_lib, N, kw, shape):
    from meryl_amd import capi
    T = native_lib.mgc_dev_merge_many_tile(kw)
    rng = np.random.default_rng(7000 + 100 * N + 10 * kw + len(shape))
    keys = TM.shapes(N, T)[shape](rng, kw)
    inp = Inputs(torch_cuda, rng, keys, kw, null_input=1)
    if shape == "group-at-T":
        assert len(inp.everywhere) >= 1
    special_rows(inp)
    inp.upload()
    # a k-mer only in a later input: FIRST is not input 0
    assert any(a[0][0] > 0 for a in inp.act.values())
    n_checked = 0
    for word in LH.LABEL_WORDS:
        if word == "invert":
            with pytest.raises(capi.MgcError):
                ops.dev_merge_many_labelled(inp.dk, inp.dc, inp.dl, 0, word)
            continue
        merge_ops = range(11) if word in ("default", "selected") else (0,)
        for op in merge_ops:
            n_checked += inp.check(ops, op, word)
        if word in ("set", "min", "max", "and", "or", "xor", "difference", "lightest", "heaviest"):
            n_checked += inp.check(ops, 0, word, 0b1001)                             # an explicit constant
            n_checked += inp.check(ops, 3, word, 0xF0F0F0F0F0F0F0F0)                  # ... under intersect-sum: every input active
    assert n_checked > 0


BORDER_SHAPES = [s for s in TM.SHAPE_NAMES if s != "one-large"]


@pytest.mark.parametrize("shape", BORDER_SHAPES)
@pytest.mark.parametrize("kw", [1, 2])
def test_labels_at_every_shape(ops, torch_cuda, native_lib, kw, shape):
    N = 3
    T = native_lib.mgc_dev_merge_many_tile(kw)
    rng = np.random.default_rng(9000 + 10 * kw + BORDER_SHAPES.index(shape))
    keys = TM.shapes(N, T)[shape](rng, kw)
    inp = Inputs(torch_cuda, rng, keys, kw, null_input=2)
    if len(inp.everywhere) >= 7:
        special_rows(inp)
    inp.upload()
    n = 0
    for op, word in ((0, "or"), (7, "difference"), (1, "min"), (2, "selected"), (4, "selected")):
        n += inp.check(ops, op, word)
    if shape != "all-empty":
        assert n > 0


@pytest.mark.parametrize("kw", [1, 2])
def test_one_input(ops, torch_cuda, native_lib, kw):
    T = native_lib.mgc_dev_merge_many_tile(kw)
    rng = np.random.default_rng(50 + kw)
    for n in (0, 1, T, 3 * T + 17):
        keys = [TM.draw(rng, TM.make_pool(rng, n + 64, kw), n)]
        for null_input in (None, 0):
            inp = Inputs(torch_cuda, rng, keys, kw, null_input=null_input)
            inp.upload()
            for op, word in ((0, "default"), (0, "invert"), (6, "first"), (7, "min"), (9, "xor"), (10, "set"), (2, "selected")):
                assert inp.check(ops, op, word) == keys[0].shape[0]


@pytest.mark.parametrize("kw", [1, 2])
@pytest.mark.parametrize("n", [0, 1, SELECT_TILE - 1, SELECT_TILE, SELECT_TILE + 1, 3 * SELECT_TILE + 17])
def test_select_carries_the_labels(ops, torch_cuda, native_lib, n, kw):
    torch = torch_cuda
    rng = np.random.default_rng(300 + n + kw)
    keys = TM.draw(rng, TM.make_pool(rng, n + 64, kw), n)
    assert keys.shape[0] == n
    vals = rng.integers(1, 20, n).astype(np.uint32)
    vals[::5] = rng.integers(1, M32, vals[::5].size, dtype=np.uint64).astype(np.uint32)
    vals[1::7] = M32
    labs = random_labels(rng, n)
    dk, dc, dl = key_tensor(torch, keys, kw), torch.from_numpy(vals.view(np.int32).copy()).cuda(), u64_tensor(torch, labs)
    ints = TM.key_ints(keys)
    kept_any = 0
    for fop in range(12):
        for c, word, lc in ((7, "default", None), (3, "invert", None), (0, "min", 0x55), (1 << 33, "and", 0x0F0F), (7, "lightest", None)):
            if c > M32 and fop == 10:
                continue                                             # (divide-round's float rounding is not what is under test)
            ok, oc, ol = ops.dev_select_labelled(dk, dc, dl if fop % 2 == 0 or word != "default" else None, fop, c, word, lc)
            null = not (fop % 2 == 0 or word != "default")
            cc = LH.DEFAULT_CONSTANT.get(word, 0) if lc is None else lc
            want = []
            for key, v, l in zip(ints, vals.tolist(), labs.tolist()):
                nv = LH.sel_value(fop, v, c)
                if nv:
                    want.append((key, nv, LH.label_of(word, cc, [0 if null else l], [v])))
            what = (fop, c, word)
            assert host_keys(ok, kw) == [k for k, _, _ in want], what
            assert oc.cpu().numpy().view(np.uint32).tolist() == [v for _, v, _ in want], what
            assert ol.cpu().numpy().view(np.uint64).tolist() == [l for _, _, l in want], what
            kept_any += len(want)
    assert kept_any > 0 or n == 0


# ---- decode and encode against the host codec -------------------------------------------------------------------------------
def dir_bytes(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d))}


def check_codec_round_trip(torch, ops, base, lo, hi, cn, lab, k, wp, label_size):
    """host-written database: device decode == host reader, file by file; the same arrays through the device encoder give
    the host writer's files byte for byte"""
    from meryl_amd import db
    kw = 2 if k > 32 else 1
    host_dir, dev_dir = os.path.join(base, "host"), os.path.join(base, "dev")
    LH.write_labelled_db(host_dir, lo, hi, cn, lab, k, wp, label_size)
    r = db.Reader(host_dir)
    assert r.info.label_size == label_size
    total = 0
    for ff in range(64):
        wlo, whi, wcn, wlb = r.read_file(ff, labels=True)
        dk, dc, dl = ops.dev_decode_file(r, ff)
        gk = dk.cpu().numpy().view(np.uint64)
        glo, ghi = (gk.reshape(-1, 2)[:, 0], gk.reshape(-1, 2)[:, 1]) if kw == 2 else (gk, np.zeros(gk.size, np.uint64))
        assert np.array_equal(glo, wlo) and np.array_equal(ghi, whi), ff
        assert np.array_equal(dc.cpu().numpy().view(np.uint32), wcn), ff
        assert np.array_equal(dl.cpu().numpy().view(np.uint64), wlb), ff
        total += wlo.size
    r.close()
    assert total == lo.size
    mask = np.uint64(M64 if label_size == 64 else (1 << label_size) - 1)
    # (what the host reader gave above is the masked labels: the writer keeps the low label_size bits)
    keys = np.stack([lo, hi], axis=1)
    s = ops.DbStream(dev_dir, k, wp, label_size=label_size, label=0)
    s.write(key_tensor(torch, keys, kw), torch.from_numpy(cn.view(np.int32).copy()).cuda(), 0, 1 << wp, labels=u64_tensor(torch, lab))
    s.close()
    a, b = dir_bytes(dev_dir), dir_bytes(host_dir)
    assert sorted(a) == sorted(b) and len(a) == 129
    assert all(a[n] == b[n] for n in a), [n for n in a if a[n] != b[n]][:5]
    return mask


@pytest.mark.parametrize("k", [21, 51])
@pytest.mark.parametrize("label_size", [1, 7, 33, 63, 64])
def test_labelled_databases_round_trip_through_the_device_codec(ops, torch_cuda, native_lib, tmp_path, label_size, k):
    import eval_helpers as H
    wp = {21: 9, 51: 10}[k]
    rng = np.random.default_rng(1000 * k + label_size)
    lo, hi = H.random_kmers(rng, k, 9000)
    pre = H.prefixes(lo, hi, k, wp)
    # empty blocks (prefixes 5..20 and the last one) and one-k-mer blocks (prefixes 30..40 keep their first k-mer only)
    first = np.ones(lo.size, bool)
    first[1:] = pre[1:] != pre[:-1]
    keep = ~(((pre >= 5) & (pre <= 20)) | (pre == (1 << wp) - 1)) & ~(((pre >= 30) & (pre <= 40)) & ~first)
    lo, hi, pre = lo[keep], hi[keep], pre[keep]
    sizes = np.bincount(pre.astype(np.int64), minlength=1 << wp)
    assert (sizes == 0).sum() >= 17 and (sizes[30:41] <= 1).all() and (sizes == 1).sum() >= 1 and sizes.max() > 8
    cn = rng.integers(1, 1 << 20, lo.size).astype(np.uint32)
    cn[::11] = M32
    lab = random_labels(rng, lo.size)
    lab[::13] = M64
    lab[1::13] = 0
    check_codec_round_trip(torch_cuda, ops, str(tmp_path), lo, hi, cn, lab, k, wp, label_size)


def test_a_label_section_across_the_16_MiB_border(ops, torch_cuda, native_lib, tmp_path):
    """one block of 1.25 M 21-mers with 64-bit labels at w_prefix 6: its stuffedBits object is longer than one 16 MiB
    sub-block and the border falls inside the label section"""
    k, wp, n = 21, 6, 1_250_000
    rng = np.random.default_rng(16)
    suffix = np.unique(rng.integers(0, 1 << 36, n + 4000, dtype=np.uint64))[:n]
    assert suffix.size == n
    lo = (np.uint64(37) << np.uint64(36)) | suffix                    # everything in prefix 37
    small = np.array([(3 << 36) | 5, (50 << 36) | 9], dtype=np.uint64)
    lo = np.sort(np.concatenate([lo, small]))
    hi = np.zeros(lo.size, np.uint64)
    cn = rng.integers(1, 500, lo.size).astype(np.uint32)
    lab = random_labels(rng, lo.size)
    check_codec_round_trip(torch_cuda, ops, str(tmp_path), lo, hi, cn, lab, k, wp, 64)
    size = os.path.getsize(os.path.join(str(tmp_path), "host", "0x100101.merylData"))
    assert size > (16 << 20) + 4096, size                             # more than one sub-block ...
    assert size - 8 * n < (16 << 20), size                            # ... and the label section begins in the first


# ---- trees -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=sorted(LH.TREE_K))
def tree_world(request, native_lib, torch_cuda, tmp_path_factory):
    k = request.param
    base = str(tmp_path_factory.mktemp("labels_k%d" % k))
    wdir = os.path.join(base, "world")
    os.makedirs(wdir)
    LH.make_tree_world(wdir, k)
    out = os.path.join(base, "out")
    got = LH.run_tree(wdir, out)
    return {"k": k, "base": base, "dir": wdir, "out": out, "got": got}


def tree_model(wdir):
    """-> (inner, root): {k-mer: (value, label)}; labels as full 64-bit values"""
    dbs = {n: LH.read_db(os.path.join(wdir, n))[0] for n in ("a", "b", "c", "d")}
    inner = {}
    for key in sorted(set(dbs["a"]) | set(dbs["b"]) | set(dbs["c"])):
        act = [dbs[n][key] for n in ("a", "b", "c") if key in dbs[n]]
        inner[key] = (sum(v for v, _ in act) & M32, LH.label_of("or", 0, [l for _, l in act], [v for v, _ in act], merge_op=0))
    d2 = {key: (v, LH.label_of("default", 0, [l], [v])) for key, (v, l) in dbs["d"].items() if v >= 2}
    root = {}
    for key, (v, l) in inner.items():
        if key in d2:
            if v <= d2[key][0]:
                continue
            root[key] = (v - d2[key][0], LH.label_of("default", 0, [l, d2[key][1]], [v, d2[key][0]], merge_op=7))
        else:
            root[key] = (v, LH.label_of("default", 0, [l], [v], merge_op=7))
    return inner, root


def test_tree_outputs_and_callback_equal_the_model(tree_world):
    inner, root = tree_model(tree_world["dir"])
    assert len(root) > 1000 and len(inner) > len(root)
    ls = max(LH.TREE_LABEL_SIZES.values())
    mask = (1 << ls) - 1
    for name, want in (("inner", inner), ("root", root)):
        got, got_ls = LH.read_db(os.path.join(tree_world["out"], name))
        assert got_ls == ls                                             # the largest label size among the leaves
        assert got == {key: (v, l & mask) for key, (v, l) in want.items()}, name
        assert any(l & mask for _, l in want.values())
    assert sorted(os.listdir(tree_world["out"])) == ["inner", "root"]
    lo, hi, v, lab = tree_world["got"]
    keys = [(int(h) << 64) | int(l) for l, h in zip(lo.tolist(), hi.tolist())]
    assert keys == sorted(root)
    assert v.tolist() == [root[key][0] for key in keys]
    assert lab.tolist() == [root[key][1] for key in keys]                # the callback's labels are the file's (no bit above 12 arises here)
    assert all(l <= mask for l in lab.tolist())


def test_tree_with_a_label_size_and_label_words(tree_world, tmp_path):
    """-l 5 on the outputs; SET, INVERT on a value node and MIN with a constant between the nodes as full 64-bit values"""
    from meryl_amd import db
    p = lambda n: os.path.join(tree_world["dir"], n)                     # noqa: E731
    tree = ("union-min", ("increase", 1, p("a"), {"label": "invert"}), p("b"), ("at-least", 1, p("c"), {"label": ("set", 0x1F3)}),
            {"label": ("min", 0x15), "output": str(tmp_path / "o")})
    db.evaluate_labelled(tree, label_size=5)
    dbs = {n: LH.read_db(p(n))[0] for n in ("a", "b", "c")}
    a2 = {key: ((v + 1) & M32, ~l & M64) for key, (v, l) in dbs["a"].items()}
    c2 = {key: (v, 0x1F3) for key, (v, _) in dbs["c"].items()}
    want = {}
    for key in set(a2) | set(dbs["b"]) | set(c2):
        act = [s[key] for s in (a2, dbs["b"], c2) if key in s]
        want[key] = (min(v for v, _ in act), LH.label_of("min", 0x15, [l for _, l in act], [v for v, _ in act], merge_op=1) & 0x1F)
    got, ls = LH.read_db(tmp_path / "o")
    assert ls == 5 and got == want


def test_host_decode_gives_identical_files(tree_world):
    """MGC_DECODE_HOST=1 (labels from mdb_reader_read_file_ex) in a fresh process"""
    out = os.path.join(tree_world["base"], "out_host_decode")
    env = dict(os.environ, MGC_DECODE_HOST="1")
    p = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "label_helpers.py"), tree_world["dir"], out],
                       capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    for name in ("inner", "root"):
        assert dir_bytes(os.path.join(out, name)) == dir_bytes(os.path.join(tree_world["out"], name)), name
    z = np.load(os.path.join(out, "callback.npz"))
    for got, want in zip((z["lo"], z["hi"], z["v"], z["lab"]), tree_world["got"]):
        assert np.array_equal(got, want)


def test_unlabelled_leaves_give_the_files_of_the_unlabelled_evaluation(tree_world, tmp_path):
    from meryl_amd import db
    p = lambda n: os.path.join(tree_world["dir"], n)                     # noqa: E731

    def tree(out_dir):
        return ("subtract", ("union-sum", p("c"), p("e"), {"output": os.path.join(out_dir, "inner")}), ("at-least", 2, p("f")),
                {"output": os.path.join(out_dir, "root")})
    plain, labelled = str(tmp_path / "plain"), str(tmp_path / "labelled")
    os.makedirs(plain)
    os.makedirs(labelled)
    want = []
    db.evaluate(tree(plain), lambda ff, lo, hi, v: want.append((ff, lo, v)))
    got = []
    db.evaluate_labelled(tree(labelled), lambda ff, lo, hi, v, lab: got.append((ff, lo, v, lab)))
    for name in ("inner", "root"):
        a, b = dir_bytes(os.path.join(labelled, name)), dir_bytes(os.path.join(plain, name))
        assert sorted(a) == sorted(b) and len(a) == 129 and all(a[n] == b[n] for n in a), name
    assert len(got) == len(want) == 64 and sum(g[1].size for g in got) > 1000
    for g, w in zip(got, want):
        assert g[0] == w[0] and np.array_equal(g[1], w[1]) and np.array_equal(g[2], w[2]) and not g[3].any()


# ---- command line ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def meryl(native_lib):
    from meryl_amd import build
    path = build.build_cli()
    assert os.path.exists(path)
    return path


def run(meryl, *args):
    p = subprocess.run([meryl] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    return p


def canonical_kmers(seq, k):
    """{canonical k-mer: occurrences}; meryl orders the bases A < C < T < G (the 2-bit code of its k-mers)"""
    code = {"A": 0, "C": 1, "T": 2, "G": 3}
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    out = {}
    for i in range(len(seq) - k + 1):
        f = seq[i:i + k]
        r = "".join(comp[b] for b in reversed(f))
        m = min(f, r, key=lambda s: [code[b] for b in s])
        out[m] = out.get(m, 0) + 1
    return out


def test_cli_labels_say_which_sample_holds_a_kmer(meryl, torch_cuda, tmp_path):
    k = 15
    rng = np.random.default_rng(15)
    bases = "".join(rng.choice(list("ACGT"), 3000))
    sa, sb = bases[:2000], bases[1000:]                                  # the middle third is in both samples
    (tmp_path / "a.fa").write_text(">a\n%s\n" % sa)
    (tmp_path / "b.fa").write_text(">b\n%s\n" % sb)
    ka, kb = canonical_kmers(sa, k), canonical_kmers(sb, k)
    want = {m: (ka.get(m, 0) + kb.get(m, 0), (1 if m in ka else 0) | (2 if m in kb else 0)) for m in set(ka) | set(kb)}
    assert {l for _, l in want.values()} == {1, 2, 3}

    def parse(text):
        rows = [line.split("\t") for line in text.splitlines()]
        assert all(len(r) == 3 and len(r[2]) == 2 for r in rows), rows[:3]
        return {r[0]: (int(r[1]), int(r[2], 2)) for r in rows}
    # the example of the README: one bit per sample, OR over the samples that hold the k-mer
    before = set(os.listdir(tmp_path))
    run(meryl, "-Q", "-l", "2", "k=%d" % k, "memory=2", "union-sum", "label=or", "[count", "label=#1", str(tmp_path / "a.fa") + "]",
        "[count", "label=#2", str(tmp_path / "b.fa") + "]", "output", tmp_path / "ab.meryl")
    assert set(os.listdir(tmp_path)) - before == {"ab.meryl"}            # the counts' databases were temporary
    assert parse(run(meryl, "-Q", "print", tmp_path / "ab.meryl").stdout) == want
    # labelled databases as inputs, no label= and no -l: refused before, the labels are the OR (union-sum's default)
    run(meryl, "-Q", "-l", "2", "k=%d" % k, "memory=2", "count", "label=#1", tmp_path / "a.fa", "output", tmp_path / "a.lab")
    run(meryl, "-Q", "-l", "2", "k=%d" % k, "memory=2", "count", "label=#2", tmp_path / "b.fa", "output", tmp_path / "b.lab")
    assert parse(run(meryl, "-Q", "print", "union-sum", tmp_path / "a.lab", tmp_path / "b.lab").stdout) == want
    # ... and a label word on the tree under print: the k-mers of both samples keep 01 & 10 = 00 under AND
    got = parse(run(meryl, "-Q", "print", "intersect-sum", "label=and", tmp_path / "a.lab", tmp_path / "b.lab").stdout)
    assert got == {m: (v, 0) for m, (v, l) in want.items() if l == 3} and len(got) > 100
