#!/usr/bin/env python3
"""Timing of meryl-analyze (include/meryl_analyze.h) on one GPU.  One JSON object per line:

  * kernel: a slice of the benchmark's reads (bench.py's generator, READS_M million 150-base reads) is counted at k = 21; its
    distinct k-mers and values stay in HBM.  mgc_analyze_add_device of them for -gc / -ga / -gt (HIP events, a warm-up, median
    of 5, the samples kept) beside a device-to-device copy of the same 12 bytes per k-mer in the same process -- the traffic
    floor (the copy also writes what it reads; the histogram only reads).  `values=poisson30` repeats the leg with values drawn
    like a 30x count on the same k-mers (the slice itself is counted at about 1x, most of its values are 1 or 2).
    `k=51` repeats -gc / -ga on a k = 51 count (20 bytes per k-mer).
  * tier: the same input with MGC_ANALYZE_DENSE=0 -- no dense tier, everything through the overflow list and its sort.
  * database: the count written to DIR (tmpfs); mgc_analyze_add_database of it in wall clock with the read / decode /
    histogram split of its info, beside mgc_db_filter of the same database with a filter every k-mer passes (at-least 1) to
    DIR: the existing operation that also reads, uploads and decodes all 64 files (and then encodes and writes them).

usage: python scripts/analyze_bench.py [READS_M] [--dir DIR] >> profiles/analyze_bench.jsonl"""
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

sys.path.insert(0, '.')
import torch  # noqa: E402
from meryl_amd import analyze, capi, count  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
work = None
if "--dir" in sys.argv:
    work = sys.argv[sys.argv.index("--dir") + 1]
    args.remove(work)
reads = int((float(args[0]) if args else 2.0) * 1_000_000)
own_dir = work is None
if own_dir:
    work = tempfile.mkdtemp(prefix="analyze_bench_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
dev = torch.device("cuda")
NAMES = {analyze.GC: "gc", analyze.GA: "ga", analyze.GT: "gt"}


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


def counted(k, db=None):
    bases = count.dev_synth_reads(2, 333_333_334, 0, reads, 150, 5000, 100)
    cfg = capi.configure(k, bases.numel(), 128 << 30)
    with count.Session(cfg, 0) as s:
        s.push_bases_device(bases)
        s.count()
        keys, vals = s.result_device()
        if db:
            s.write_database(db, 16)
    del bases
    torch.cuda.empty_cache()
    return keys, vals


def kernel_leg(keys, vals, k, types, tag, dense=True):
    n = int(keys.shape[0])
    kb = 8 * (2 if k > 32 else 1)
    k2, v2 = torch.empty_like(keys), torch.empty_like(vals)

    def copy():
        k2.copy_(keys)
        v2.copy_(vals)

    copy_ms, copy_samples = timed(copy)
    if dense:
        os.environ.pop("MGC_ANALYZE_DENSE", None)
    else:
        os.environ["MGC_ANALYZE_DENSE"] = "0"
    for t in types:
        infos = []

        def run():
            with analyze.Analyzer(k, t) as a:               # (a fresh accumulator: opening it costs two small allocations)
                a.add_device(keys, vals)
                infos.append(a.info())

        ms, samples = timed(run)
        i = infos[-1]
        emit(what="tier" if not dense else "kernel", type=NAMES[t], k=k, values=tag, n=n, bytes_per_kmer=kb + 4, add_device_ms=round(ms, 3),
             hist_ms=round(i["hist_ms"], 3), overflow_ms=round(i["overflow_ms"], 3), overflow_kmers=i["n_overflow_kmers"],
             overflow_share=round(i["n_overflow_kmers"] / max(1, n), 5), retries=i["n_overflow_retries"],
             copy_ms=round(copy_ms, 3), ratio_to_copy=round(ms / copy_ms, 3), hist_ratio_to_copy=round(i["hist_ms"] / copy_ms, 3),
             kmers_per_s=round(n / ms * 1e3), read_gb_per_s=round(n * (kb + 4) / ms / 1e6, 1),
             copy_gb_per_s=round(2 * n * (kb + 4) / copy_ms / 1e6, 1), samples_ms=samples, copy_samples_ms=copy_samples)
    os.environ.pop("MGC_ANALYZE_DENSE", None)


emit(what="setup", device=torch.cuda.get_device_name(0), reads=reads, dense_values=analyze.DENSE_VALUES, dir=work)
ALL = (analyze.GC, analyze.GA, analyze.GT)

# ---- k = 21 -------------------------------------------------------------------------------------------------------------
K = 21
db = os.path.join(work, "a.meryl")
keys, vals = counted(K, db)
n = int(keys.shape[0])
emit(what="input", k=K, kmers=n, share_above_dense=round(float((vals >= analyze.DENSE_VALUES).float().mean()), 6),
     share_ones=round(float((vals == 1).float().mean()), 4))
kernel_leg(keys, vals, K, ALL, "count")
g = torch.Generator(device=dev)
g.manual_seed(20261017)
v30 = torch.poisson(torch.full((n,), 30.0, device=dev), generator=g).to(torch.int32)
u = torch.rand(n, generator=g, device=dev)
v30[u < 0.10] = 1
tail = u > 0.99
v30[tail] = torch.floor(10 ** (2.0 + 4.0 * torch.rand(int(tail.sum()), generator=g, device=dev))).to(torch.int32)
kernel_leg(keys, v30, K, ALL, "poisson30")
kernel_leg(keys, v30, K, ALL, "poisson30", dense=False)
del v30, u, tail

# ---- the database of that count -------------------------------------------------------------------------------------------
for t in (analyze.GC, analyze.GA):
    runs = []
    for rep in range(4):                                     # the first is the warm-up (code objects, page cache)
        t0 = time.perf_counter()
        with analyze.Analyzer(K, t) as a:
            a.add_database(db, 16)
            info = a.info()
        info["wall_s"] = time.perf_counter() - t0
        if rep:
            runs.append(info)
    med = sorted(runs, key=lambda r: r["wall_s"])[len(runs) // 2]
    emit(what="database", type=NAMES[t], k=K, kmers=med["n_kmers"], wall_s=round(med["wall_s"], 3), kmers_per_s=round(med["n_kmers"] / med["wall_s"]),
         read_s=round(med["read_s"], 3), decode_ms=round(med["decode_ms"], 3), hist_ms=round(med["hist_ms"], 3),
         overflow_ms=round(med["overflow_ms"], 3), samples_wall_s=[round(r["wall_s"], 3) for r in runs])
times = []
for rep in range(4):
    out = os.path.join(work, "f.meryl")
    shutil.rmtree(out, ignore_errors=True)
    t0 = time.perf_counter()
    capi.check(capi.lib().mgc_db_filter(db.encode(), 2, 1, out.encode(), -1, 16), "mgc_db_filter")      # MGC_VALUE_AT_LEAST 1
    if rep:
        times.append(time.perf_counter() - t0)
shutil.rmtree(os.path.join(work, "f.meryl"), ignore_errors=True)
emit(what="database_filter", k=K, kmers=n, wall_s=round(statistics.median(times), 3), samples_wall_s=[round(x, 3) for x in times])
del keys, vals
torch.cuda.empty_cache()
shutil.rmtree(db, ignore_errors=True)

# ---- k = 51: 20 bytes per k-mer ---------------------------------------------------------------------------------------------
keys, vals = counted(51)
kernel_leg(keys, vals, 51, (analyze.GC, analyze.GA), "count")
if own_dir:
    shutil.rmtree(work, ignore_errors=True)
