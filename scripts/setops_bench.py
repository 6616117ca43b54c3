#!/usr/bin/env python3
"""Timing of the set operations over more than two inputs on one GPU.  One JSON object per line:

  * kernel (leg a): N sorted inputs of KEYS_M million 8-byte k-mers each in HBM, `disjoint` (no k-mer in two inputs) and
    `shared50` (half of every input is held by all N).  merge_many (mgc_dev_merge_many_*, one count pass and one emit pass
    over all inputs) beside the left fold of the two-input merge (mgc_dev_merge_*) over the same device arrays, as
    mgc_db_merge folds: N - 1 steps, and for symmetric-difference over more than two inputs a second fold over ones plus a
    selection (here a torch mask).  Both sides pay their host synchronisation per count pass and the output allocations.
    HIP events, a warm-up, the median of 5 with the samples kept; a device-to-device copy of the inputs' bytes is the floor.
  * cli (leg b): three counts of READS_M million reads each written to DIR (tmpfs), then
    `meryl union-sum [greater-than 1 A] [greater-than 1 B] [greater-than 1 C] output U` as one tree beside the same command
    staged with three intermediate databases (`--staged-meryl PATH`: the front end of another build, e.g. the parent
    commit's; default: this build's), wall clock per command, median of 3 after a warm-up.  `start`: a filter of a database
    of a handful of k-mers -- what a process pays before it touches data.
  * labels (leg c): merge_many with labels (mgc_dev_merge_many_count + mgc_dev_merge_many_emit_labelled, label=or, every input
    labelled) beside the unlabelled pair over the same keys and values, union-sum over the `shared50` mix, N = 2, 8 and 32,
    8- and 16-byte keys.  `expected_ratio` is the ratio of the bytes the two move: per input element the count pass reads the
    key and the emit pass the key and the value (4 B), per kept k-mer the emit writes key and value; labels add 8 B per element
    read and 8 B per kept k-mer written.
  * selectors (leg s): merge_many with a selector program (`input:2-all value:ge2`, mgc_dev_merge_many_*_selected, no labels)
    beside the same union-sum without one (mgc_dev_merge_many_*) over the `shared50` mix, N = 3 and 8, 8-byte keys.  No ratio
    is fixed in advance; the line holds the bytes each pair moves: the plain count pass reads the keys and the emit pass keys and
    values and writes what is kept; with a VALUE term the selected count pass reads the values too (4 B more per element), and
    the selected emit writes fewer k-mers.
  * values (leg v): merge_many with a value assignment (mgc_dev_merge_many_*_assigned, no program, no labels) -- `value=sub` and
    `value=divzero`, whose count passes read the values (a zero result is not written), under `union` presence -- beside the same
    run's `union-sum` (the count pass reads keys only) and `subtract` (the existing case whose count pass reads the values) through
    mgc_dev_merge_many_*, over the `shared50` mix, N = 3 and 32, 8-byte keys.  No threshold is fixed in advance.
  * histogram (leg h): the value histogram of HIST_M million uint32 values in one device buffer (--hist-m, default 64), four
    distributions -- all ones; geometric (p = 0.4, typical of counts); uniform in [1, 1000]; uniform in [1, 2^31] -- two ways over
    the same buffer: the accumulator's add (mgc_value_hist_add and mgc_value_hist_get on one accumulator, its buffers grown by the
    warm-up as the evaluator's are after its first slice), which is also the database writer's pass; a device copy of the buffer, the
    floor.  The median of 5 after a warm-up.  `equal`: the accumulator's pairs equal torch.unique's.  (Lines recorded with a `writer`
    leg timed the pass the database writer had before it took the accumulator; that code is gone.)

usage: python scripts/setops_bench.py [KEYS_M] [READS_M] [--dir DIR] [--legs a,b,c,s,v,h] [--hist-m HIST_M] [--staged-meryl PATH] >> profiles/setops_bench.jsonl"""
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

sys.path.insert(0, '.')
import torch  # noqa: E402
from meryl_amd import build, capi, count, db  # noqa: E402


def option(name, default=None):
    if name in sys.argv:
        i = sys.argv.index(name)
        v = sys.argv[i + 1]
        del sys.argv[i:i + 2]
        return v
    return default


work = option("--dir")
legs = option("--legs", "a,b").split(",")
staged_meryl = option("--staged-meryl", build.CLI)
hist_m = float(option("--hist-m", "64"))
args = sys.argv[1:]
keys_m = float(args[0]) if args else 8.0
reads_m = float(args[1]) if len(args) > 1 else 0.25
own_dir = work is None
if own_dir:
    work = tempfile.mkdtemp(prefix="setops_bench_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
dev = torch.device("cuda")


def emit(**kv):
    print(json.dumps(kv), flush=True)


def timed(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), [round(x, 3) for x in ms]


def sorted_unique(n, g):
    """about n distinct ascending 56-bit values"""
    return torch.unique(torch.randint(0, 1 << 56, (n,), generator=g, device=dev, dtype=torch.int64))


def make_inputs(n_inputs, n, mix, g):
    """keys = value << 6 | tag: tag = the input's index for its own k-mers, 32 for the k-mers every input holds"""
    shared = (sorted_unique(n // 2, g) << 6) | 32 if mix == "shared50" else None
    ks, vs = [], []
    for i in range(n_inputs):
        own = (sorted_unique(n if shared is None else n - n // 2, g) << 6) | i
        k = own if shared is None else torch.sort(torch.cat([own, shared])).values
        ks.append(k.contiguous())
        vs.append(torch.randint(1, 100, (k.shape[0],), generator=g, device=dev, dtype=torch.int32))
    return ks, vs


def fold(ks, vs, op):
    if op == "symmetric-difference" and len(ks) > 2:
        k, c, m = ks[0], vs[0], torch.ones_like(vs[0])
        for i in range(1, len(ks)):
            k2, c = count.dev_merge(k, c, ks[i], vs[i], "union-sum")
            _, m = count.dev_merge(k, m, ks[i], torch.ones_like(vs[i]), "union-sum")
            k = k2
        sel = m == 1
        return k[sel], c[sel]
    k, c = ks[0], vs[0]
    for i in range(1, len(ks)):
        k, c = count.dev_merge(k, c, ks[i], vs[i], op)
    return k, c


def kernel_leg():
    n = int(keys_m * 1_000_000)
    g = torch.Generator(device=dev)
    g.manual_seed(20261018)
    for n_inputs in (3, 4, 8, 16, 32):
        for mix in ("disjoint", "shared50"):
            ks, vs = make_inputs(n_inputs, n, mix, g)
            total = sum(int(k.shape[0]) for k in ks)
            k2 = [torch.empty_like(k) for k in ks]
            v2 = [torch.empty_like(v) for v in vs]

            def copy():
                for a, b in zip(k2, ks):
                    a.copy_(b)
                for a, b in zip(v2, vs):
                    a.copy_(b)
            copy_ms, copy_samples = timed(copy)
            del k2, v2
            for op in ("union-sum", "symmetric-difference"):
                out = {}

                def many():
                    out["many"] = count.dev_merge_many(ks, vs, op)

                def folded():
                    out["fold"] = fold(ks, vs, op)
                many_ms, many_samples = timed(many)
                fold_ms, fold_samples = timed(folded)
                same = torch.equal(out["many"][0], out["fold"][0]) and torch.equal(out["many"][1], out["fold"][1])
                n_out = int(out["many"][0].shape[0])
                out.clear()
                emit(what="kernel", n_inputs=n_inputs, mix=mix, op=op, keys_per_input=n, total=total, n_out=n_out, equal=bool(same),
                     merge_many_ms=round(many_ms, 3), fold_ms=round(fold_ms, 3), fold_over_many=round(fold_ms / many_ms, 3),
                     copy_ms=round(copy_ms, 3), many_over_copy=round(many_ms / copy_ms, 3),
                     many_gkeys_per_s=round(total / many_ms / 1e6, 2), copy_gb_per_s=round(2 * 12 * total / copy_ms / 1e6, 1),
                     samples_many_ms=many_samples, samples_fold_ms=fold_samples, samples_copy_ms=copy_samples)
            del ks, vs
            torch.cuda.empty_cache()


def labels_leg():
    n = int(keys_m * 1_000_000)
    g = torch.Generator(device=dev)
    g.manual_seed(20261019)
    for kw in (1, 2):
        for n_inputs in (2, 8, 32):
            ks, vs = make_inputs(n_inputs, n, "shared50", g)
            if kw == 2:                                              # 16-byte keys (lo, hi): the same order with hi = 0
                ks = [torch.stack([k, torch.zeros_like(k)], dim=1).contiguous() for k in ks]
            ls = [torch.randint(0, 1 << 62, (k.shape[0],), generator=g, device=dev, dtype=torch.int64) for k in ks]
            total = sum(int(k.shape[0]) for k in ks)
            out = {}

            def plain():
                out["plain"] = count.dev_merge_many(ks, vs, "union-sum")

            def labelled():
                out["lab"] = count.dev_merge_many_labelled(ks, vs, ls, "union-sum", "or")
            plain_ms, plain_samples = timed(plain)
            lab_ms, lab_samples = timed(labelled)
            same = torch.equal(out["plain"][0], out["lab"][0]) and torch.equal(out["plain"][1], out["lab"][1])
            n_out = int(out["plain"][0].shape[0])
            out.clear()
            kb = 8 * kw
            plain_bytes = total * kb + total * (kb + 4) + n_out * (kb + 4)
            lab_bytes = plain_bytes + 8 * total + 8 * n_out
            emit(what="labels", n_inputs=n_inputs, key_bytes=kb, mix="shared50", op="union-sum", label_op="or", keys_per_input=n, total=total,
                 n_out=n_out, equal=bool(same), merge_many_ms=round(plain_ms, 3), labelled_ms=round(lab_ms, 3),
                 labelled_over_plain=round(lab_ms / plain_ms, 3), expected_ratio=round(lab_bytes / plain_bytes, 3),
                 samples_plain_ms=plain_samples, samples_labelled_ms=lab_samples)
            del ks, vs, ls
            torch.cuda.empty_cache()


def selectors_leg():
    n = int(keys_m * 1_000_000)
    g = torch.Generator(device=dev)
    g.manual_seed(20261020)
    words = ["input:2-all", "value:ge2"]
    for n_inputs in (3, 8):
        ks, vs = make_inputs(n_inputs, n, "shared50", g)
        terms = db.parse_selector(words, n_inputs)
        total = sum(int(k.shape[0]) for k in ks)
        out = {}

        def plain():
            out["plain"] = count.dev_merge_many(ks, vs, "union-sum")

        def selected():
            out["sel"] = count.dev_merge_many_selected(ks, vs, None, 28, "union-sum", terms, with_labels=False)
        plain_ms, plain_samples = timed(plain)
        sel_ms, sel_samples = timed(selected)
        n_plain, n_sel = int(out["plain"][0].shape[0]), int(out["sel"][0].shape[0])
        pk, pc = out["plain"]
        # what the program keeps, from the plain result: the shared k-mers (tag 32, held by every input; their sums are >= 2)
        keep = (pk & 63) == 32
        same = torch.equal(pk[keep], out["sel"][0]) and torch.equal(pc[keep], out["sel"][1])
        out.clear()
        plain_bytes = total * 8 + total * 12 + n_plain * 12
        sel_bytes = total * 12 + total * 12 + n_sel * 12
        emit(what="selectors", n_inputs=n_inputs, key_bytes=8, mix="shared50", op="union-sum", select=words, keys_per_input=n, total=total,
             n_out_plain=n_plain, n_out_selected=n_sel, equal=bool(same), merge_many_ms=round(plain_ms, 3), selected_ms=round(sel_ms, 3),
             selected_over_plain=round(sel_ms / plain_ms, 3), plain_bytes=plain_bytes, selected_bytes=sel_bytes,
             bytes_ratio=round(sel_bytes / plain_bytes, 3), samples_plain_ms=plain_samples, samples_selected_ms=sel_samples)
        del ks, vs
        torch.cuda.empty_cache()


def values_leg():
    n = int(keys_m * 1_000_000)
    g = torch.Generator(device=dev)
    g.manual_seed(20261021)
    for n_inputs in (3, 32):
        ks, vs = make_inputs(n_inputs, n, "shared50", g)
        total = sum(int(k.shape[0]) for k in ks)
        out, line = {}, {}
        for name, fn in (("union-sum", lambda: count.dev_merge_many(ks, vs, "union-sum")),
                         ("subtract", lambda: count.dev_merge_many(ks, vs, "subtract")),
                         ("value=sub", lambda: count.dev_merge_many_assigned(ks, vs, None, 28, "union", "sub", with_labels=False)),
                         ("value=divzero", lambda: count.dev_merge_many_assigned(ks, vs, None, 28, "union", "divzero", with_labels=False))):
            def run():
                out[name] = fn()
            ms, samples = timed(run)
            line[name] = dict(ms=round(ms, 3), n_out=int(out[name][0].shape[0]), samples_ms=samples)
        # own k-mers keep their value under both rules; a shared k-mer stays under value=sub exactly where subtract keeps it
        sk, sc = out["subtract"][:2]
        ak, ac = out["value=sub"][:2]
        shared = (ak & 63) == 32
        same = torch.equal(ak[shared], sk[(sk & 63) == 32]) and torch.equal(ac[shared], sc[(sk & 63) == 32])
        same = same and line["value=divzero"]["n_out"] == line["union-sum"]["n_out"]          # divzero of positive values is never 0
        out.clear()
        base, sub = line["union-sum"]["ms"], line["subtract"]["ms"]
        emit(what="values", n_inputs=n_inputs, key_bytes=8, mix="shared50", presence="union", keys_per_input=n, total=total, equal=bool(same),
             legs=line, sub_over_union_sum=round(line["value=sub"]["ms"] / base, 3), sub_over_subtract=round(line["value=sub"]["ms"] / sub, 3),
             divzero_over_union_sum=round(line["value=divzero"]["ms"] / base, 3), divzero_over_subtract=round(line["value=divzero"]["ms"] / sub, 3))
        del ks, vs
        torch.cuda.empty_cache()


def histogram_leg():
    import numpy as np
    n = int(hist_m * 1_000_000)
    g = torch.Generator(device=dev)
    g.manual_seed(20261019)
    copy_to = torch.empty(n, dtype=torch.int32, device=dev)
    dense, _ = db.ValueHistogram.geometry()

    def geometric():
        u = torch.rand(n, generator=g, device=dev, dtype=torch.float64).clamp_(min=1e-300)
        return (torch.floor(torch.log(u) / np.log(1.0 - 0.4)) + 1).to(torch.int32)
    dists = (("ones", lambda: torch.ones(n, dtype=torch.int32, device=dev)), ("geometric-0.4", geometric),
             ("uniform-1-1000", lambda: torch.randint(1, 1001, (n,), generator=g, device=dev, dtype=torch.int32)),
             ("uniform-1-2^31", lambda: torch.randint(1, (1 << 31) + 1, (n,), generator=g, device=dev, dtype=torch.int64).to(torch.int32)))
    for name, make in dists:
        v = make().contiguous()
        got = {}

        fresh = db.ValueHistogram()                              # what is compared: one add into an empty accumulator
        fresh.add(v)
        got["new"] = fresh.get()
        fresh.close()
        acc = db.ValueHistogram()                                # what is timed: add + read on an accumulator whose buffers have grown

        def new_add(t=v):
            acc.add(t)
            got["pairs"] = acc.get()[0].size

        line = {}
        ms, samples = timed(lambda: copy_to.copy_(v))
        line["copy"] = dict(ms=round(ms, 3), samples_ms=samples)
        ms, samples = timed(new_add)
        line["add"] = dict(ms=round(ms, 3), samples_ms=samples, pairs=int(got["pairs"]))
        acc.close()
        uv, uc = torch.unique(v.to(torch.int64) & 0xFFFFFFFF, return_counts=True)
        same = got["new"][0].size == int(uv.numel()) and np.array_equal(got["new"][0].astype(np.int64), uv.cpu().numpy()) \
            and np.array_equal(got["new"][1].astype(np.int64), uc.cpu().numpy())
        emit(what="histogram", distribution=name, values=n, dense_limit=dense, above_dense_limit=int((uv >= dense).sum()),
             equal=bool(same), legs=line,
             add_over_copy=round(line["add"]["ms"] / line["copy"]["ms"], 2), gbytes_per_s_add=round(4e-6 * n / line["add"]["ms"], 1))
        del v, uv, uc
        torch.cuda.empty_cache()


def wall(cmd, env=None):
    t0 = time.perf_counter()
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, env=env)
    return time.perf_counter() - t0


def cli_leg():
    meryl = build.CLI
    names = []
    n_kmers = []
    for i, name in enumerate("ABC"):
        reads = int(reads_m * 1_000_000)
        bases = count.dev_synth_reads(2, 333_333_334, i * (reads // 2), reads, 150, 5000, 100)   # neighbours share half their reads
        cfg = capi.configure(21, bases.numel(), 128 << 30)
        db = os.path.join(work, name + ".meryl")
        with count.Session(cfg, 0) as s:
            s.push_bases_device(bases)
            s.count()
            n_kmers.append(int(s.info().n_distinct))
            s.write_database(db, 16)
        names.append(db)
        del bases
    torch.cuda.empty_cache()
    tiny = os.path.join(work, "tiny.meryl")
    subprocess.run([meryl, "-Q", "equal-to", "987654321", names[0], "output", tiny], check=True)

    def clean(*ns):
        for n_ in ns:
            shutil.rmtree(os.path.join(work, n_), ignore_errors=True)
    U, mids = os.path.join(work, "U.meryl"), [os.path.join(work, "g%s.meryl" % c) for c in "ABC"]

    def tree():
        clean("U.meryl")
        cmd = [meryl, "-Q", "union-sum"]
        for n_ in names:
            cmd += ["[greater-than", "1", n_ + "]"]
        return wall(cmd + ["output", U])

    def staged(binary):
        clean("U.meryl", *[os.path.basename(m) for m in mids])
        parts = [wall([binary, "-Q", "greater-than", "1", n_, "output", m]) for n_, m in zip(names, mids)]
        parts.append(wall([binary, "-Q", "union-sum"] + mids + ["output", U]))
        return parts

    def start():
        clean("tiny2.meryl")
        return wall([meryl, "-Q", "at-least", "1", tiny, "output", os.path.join(work, "tiny2.meryl")])
    tree(); staged(staged_meryl); start()                                            # warm-up: page cache, code objects
    t_tree = [tree() for _ in range(3)]
    t_staged = [staged(staged_meryl) for _ in range(3)]
    t_start = [start() for _ in range(3)]
    fold_env = dict(os.environ, MGC_MERGE_MANY="0")
    clean("U.meryl")
    cmd = [meryl, "-Q", "union-sum"]
    for n_ in names:
        cmd += ["[greater-than", "1", n_ + "]"]
    t_tree_fold = []
    for _ in range(3):
        clean("U.meryl")
        t_tree_fold.append(wall(cmd + ["output", U], env=fold_env))
    sums = [sum(p) for p in t_staged]
    emit(what="cli", k=21, kmers=n_kmers, dir=work, staged_meryl=staged_meryl,
         tree_s=round(statistics.median(t_tree), 3), staged_s=round(statistics.median(sums), 3),
         tree_fold_s=round(statistics.median(t_tree_fold), 3), start_s=round(statistics.median(t_start), 3),
         staged_over_tree=round(statistics.median(sums) / statistics.median(t_tree), 3),
         samples_tree_s=[round(x, 3) for x in t_tree], samples_staged_s=[[round(x, 3) for x in p] for p in t_staged],
         samples_tree_fold_s=[round(x, 3) for x in t_tree_fold], samples_start_s=[round(x, 3) for x in t_start])


emit(what="setup", device=torch.cuda.get_device_name(0), keys_m=keys_m, reads_m=reads_m, dir=work,
     tile=[int(capi.lib().mgc_dev_merge_many_tile(1)), int(capi.lib().mgc_dev_merge_many_tile(2))])
if "a" in legs:
    kernel_leg()
if "b" in legs:
    cli_leg()
if "c" in legs:
    labels_leg()
if "v" in legs:
    values_leg()
if "s" in legs:
    selectors_leg()
if "h" in legs:
    histogram_leg()
if own_dir:
    shutil.rmtree(work, ignore_errors=True)
