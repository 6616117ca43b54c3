#!/usr/bin/env python3
"""Timing of the k-mer text lists (include/meryl_list.h) on one GPU.  One JSON object per line:

  * format: mgc_dev_list_format of n (k-mer, value[, label]) records against a device-to-device copy of the same number of output
    bytes, in the same process (HIP events, a warm-up, median of 5, the samples kept); the length pass + scan beside it.
  * list_kmers: mgc_list_kmers end to end -- device arrays -> pieces in pinned memory -> a callback that discards them (wall
    clock, median of 5).
  * print / print_tree: `meryl print <db> > /dev/null` and `meryl print [at-least 1 <db>] > /dev/null` of one database (a slice
    of the benchmark's reads, READS_M million 150-base reads, counted at k = 21), this build's CLI and, with --parent-meryl PATH,
    the CLI of the commit before, in alternation (wall clock of the whole process, median of REPS each).  The first prints from
    the host reader in both builds; the second is where the device formats the text.

usage: python scripts/list_bench.py [READS_M] [KMERS_M] [--dir DIR] [--parent-meryl PATH] [--reps N] >> profiles/list_bench.jsonl"""
import ctypes
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

args = [a for a in sys.argv[1:] if not a.startswith("--")]


def opt(name, default):
    if name in sys.argv:
        v = sys.argv[sys.argv.index(name) + 1]
        args.remove(v)
        return v
    return default


work = opt("--dir", None)
parent = opt("--parent-meryl", None)
reps = int(opt("--reps", 5))
reads = int((float(args[0]) if args else 2) * 1_000_000)
kmers = int((float(args[1]) if len(args) > 1 else 100) * 1_000_000)
own_dir = work is None
if own_dir:
    work = tempfile.mkdtemp(prefix="list_bench_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
dev = torch.device("cuda")
L_ = capi.lib()
sp = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
g = torch.Generator(device=dev)
g.manual_seed(20261020)


def emit(**kv):
    print(json.dumps(kv), flush=True)


def timed(fn, n=5):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), [round(x, 3) for x in ms]


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


emit(what="setup", device=torch.cuda.get_device_name(0), reads=reads, kmers=kmers)

# ---- (a) the format pass against a copy of its output, (b) mgc_list_kmers end to end --------------------------------------------------
for k, label_size, n in ((21, 0, kmers), (51, 0, kmers // 2), (21, 8, kmers // 2)):
    kw = 2 if k > 32 else 1
    keys = torch.randint(0, 1 << 62, (n,) if kw == 1 else (n, 2), generator=g, device=dev, dtype=torch.int64)
    # count-like values: mostly one or two digits, a tail up to ten
    vals = (torch.randint(1, 60, (n,), generator=g, device=dev, dtype=torch.int64) *
            torch.where(torch.rand(n, generator=g, device=dev) < 0.02, torch.randint(1, 1 << 25, (n,), generator=g, device=dev, dtype=torch.int64), 1)).to(torch.int32)
    labs = torch.randint(0, 1 << 62, (n,), generator=g, device=dev, dtype=torch.int64) if label_size else None
    ws = torch.empty(L_.mgc_dev_list_workspace_bytes(n, k, label_size), dtype=torch.uint8, device=dev)
    total = ctypes.c_uint64(0)
    capi.check(L_.mgc_dev_list_lengths(ptr(vals), n, k, label_size, ptr(ws), ws.numel(), ctypes.byref(total), sp), "list_lengths")
    text, other = torch.empty(total.value, dtype=torch.uint8, device=dev), torch.empty(total.value, dtype=torch.uint8, device=dev)
    med_l, ms_l = timed(lambda: capi.check(L_.mgc_dev_list_lengths(ptr(vals), n, k, label_size, ptr(ws), ws.numel(), None, sp), "list_lengths"))
    med_f, ms_f = timed(lambda: capi.check(L_.mgc_dev_list_format(ptr(keys), ptr(vals), ptr(labs), n, k, label_size, ptr(ws), ws.numel(), ptr(text), sp), "list_format"))
    med_c, ms_c = timed(lambda: other.copy_(text))
    in_bytes = n * (8 * kw + 4 + (8 if label_size else 0))
    emit(what="format", k=k, label_size=label_size, n=n, text_bytes=total.value, bytes_per_kmer=round(total.value / n, 2), format_ms=round(med_f, 3),
         copy_ms=round(med_c, 3), format_over_copy=round(med_f / med_c, 2), lengths_ms=round(med_l, 3), text_GBps=round(total.value / med_f / 1e6, 1),
         traffic_GBps=round((total.value + in_bytes) / med_f / 1e6, 1), kmers_per_s=round(n / med_f * 1e3), format_samples_ms=ms_f, copy_samples_ms=ms_c,
         lengths_samples_ms=ms_l)
    del text, other
    seen = [0]

    def discard(p, nbytes, user):
        seen[0] += nbytes
        return 0
    cb = capi.LIST_WRITE_CB(discard)
    wall = []
    for i in range(6):
        seen[0] = 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        capi.check(L_.mgc_list_kmers(ptr(keys), ptr(vals), ptr(labs), n, k, label_size, db.LIST_CHUNK, cb, None, sp), "mgc_list_kmers")
        wall.append((time.perf_counter() - t0) * 1e3)
        assert seen[0] == total.value
    wall = wall[1:]
    med_w = statistics.median(wall)
    emit(what="list_kmers", k=k, label_size=label_size, n=n, text_bytes=total.value, chunk_bytes=db.LIST_CHUNK, ms=round(med_w, 3),
         text_GBps=round(total.value / med_w / 1e6, 2), kmers_per_s=round(n / med_w * 1e3), over_format=round(med_w / (med_f + med_l), 2),
         samples_ms=[round(x, 3) for x in wall])
    del keys, vals, labs, ws
    torch.cuda.empty_cache()

# ---- (c) `meryl print <db> > /dev/null`, this build and the one before ----------------------------------------------------------------
K = 21
bases = count.dev_synth_reads(2, 333_333_334, 0, reads, 150, 5000, 100)
cfg = capi.configure(K, bases.numel(), 128 << 30)
db_a = os.path.join(work, "a.meryl")
with count.Session(cfg, 0) as s:
    s.push_bases_device(bases)
    s.count()
    n_distinct = s.info().n_distinct
    s.write_database(db_a, 16)
del bases
torch.cuda.empty_cache()
clis = [("this", build.build_cli())] + ([("parent", parent)] if parent else [])
for what, words in (("print", [db_a]), ("print_tree", ["[at-least", "1", db_a + "]"])):
    sizes = {}
    for name, cli in clis:                                       # the bytes once, and a warm-up of the page cache
        out = subprocess.run([cli, "-Q", "print"] + words, check=True, stdout=subprocess.PIPE).stdout
        sizes[name] = (len(out), hash(out))
    assert len(set(sizes.values())) == 1, sizes
    wall = {name: [] for name, _ in clis}
    for _ in range(reps):
        for name, cli in clis:
            with open(os.devnull, "wb") as f:
                t0 = time.perf_counter()
                subprocess.run([cli, "-Q", "print"] + words, check=True, stdout=f)
                wall[name].append(time.perf_counter() - t0)
    med = {name: statistics.median(w) for name, w in wall.items()}
    text_bytes = sizes["this"][0]
    emit(what=what, k=K, kmers=n_distinct, text_bytes=text_bytes, this_s=round(med["this"], 3), this_samples_s=[round(x, 3) for x in wall["this"]],
         this_text_MBps=round(text_bytes / med["this"] / 1e6, 1),
         **({"parent_s": round(med["parent"], 3), "parent_samples_s": [round(x, 3) for x in wall["parent"]],
             "this_over_parent": round(med["this"] / med["parent"], 3), "same_bytes": True} if parent else {}))
if own_dir:
    shutil.rmtree(work, ignore_errors=True)
