#!/usr/bin/env python3
"""Timing of meryl-import (include/meryl_import.h) on one GPU.  One JSON object per line:

  * pair_sort: mgc_dev_sort_pairs of n (key, value) pairs against mgc_dev_radix_sort of the same n bare keys over the same
    bits, in the same process (HIP events, a warm-up, median of 5, the samples kept; the input is copied back before every
    repetition, outside the timed region).  The payload adds 4 bytes to 8 (16), so traffic alone allows x1.5 (x1.25).
  * reduce: mgc_dev_reduce_pairs_count + _emit over the sorted pairs.
  * import: a slice of the benchmark's reads (bench.py's generator, READS_M million 150-base reads) is counted at k = 21,
    written as a database and printed with `meryl print` into DIR; mgc_import_file then turns that text back into a
    database: wall clock, text GB/s, and per run the time the text took to arrive over the host link (upload_ms) next to the
    device stages (parse + sort + reduce) -- the design wants the second to hide behind the first.  Once with the default
    batch size and once with MGC_IMPORT_BATCH = BATCH_MB so that the run store and its merge are in the path; and once through the CLI.
  * the labelled leg (include/meryl_import_labelled.h), over the same k-mers: triple_sort / reduce_triples -- mgc_dev_sort_triples
    and mgc_dev_reduce_triples_* over the keys and values of pair_sort / reduce plus a uint64 label each, with the pair times
    beside them; import_labelled -- the same printed text with a third column (an 8-bit label) through mgc_import_labelled_file,
    and import_labelled_vs_pairs -- the device times of parse, sort and reduce, triples against pairs, from the default runs.

usage: python scripts/import_bench.py [READS_M] [PAIRS_M] [--dir DIR] [--batch-mb N] >> profiles/import_bench.jsonl
       (profiles/import_bench_labelled.jsonl holds a run of this script beside one of the commit before the labelled leg)"""
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
from meryl_amd import build, capi, count, kmer_import  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]


def opt(name, default):
    if name in sys.argv:
        v = sys.argv[sys.argv.index(name) + 1]
        args.remove(v)
        return v
    return default


work = opt("--dir", None)
batch_mb = int(opt("--batch-mb", 128))
reads = int((float(args[0]) if args else 0.3) * 1_000_000)
pairs = int((float(args[1]) if len(args) > 1 else 40) * 1_000_000)
own_dir = work is None
if own_dir:
    work = tempfile.mkdtemp(prefix="import_bench_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
dev = torch.device("cuda")
L_ = capi.lib()
sp = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
g = torch.Generator(device=dev)
g.manual_seed(20261016)


def emit(**kv):
    print(json.dumps(kv), flush=True)


def timed(fn, prepare=None, reps=5):
    if prepare:
        prepare()
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        if prepare:
            prepare()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), [round(x, 3) for x in ms]


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


emit(what="setup", device=torch.cuda.get_device_name(0), reads=reads, pairs=pairs, batch_mb=batch_mb)

# ---- the pair sort against the bare-key sort --------------------------------------------------------------------------
for kw, bits, n in ((1, 42, pairs), (2, 102, pairs // 2)):
    shape = (n,) if kw == 1 else (n, 2)
    src = torch.randint(0, 1 << 62, shape, generator=g, device=dev, dtype=torch.int64)
    if kw == 1:
        src &= (1 << bits) - 1
    else:
        src[:, 1] &= (1 << (bits - 64)) - 1
    vals = torch.randint(0, 1 << 31, (n,), generator=g, device=dev, dtype=torch.int32)
    keys, alt, v, av = torch.empty_like(src), torch.empty_like(src), torch.empty_like(vals), torch.empty_like(vals)
    ws_p = torch.empty(L_.mgc_dev_sort_pairs_workspace_bytes(n), dtype=torch.uint8, device=dev)
    ws_k = torch.empty(L_.mgc_dev_sort_workspace_bytes(n), dtype=torch.uint8, device=dev)
    ia = ctypes.c_int(0)

    def refill():
        keys.copy_(src)
        v.copy_(vals)

    med_p, ms_p = timed(lambda: capi.check(L_.mgc_dev_sort_pairs(ptr(keys), ptr(v), ptr(alt), ptr(av), n, kw, 0, bits, ptr(ws_p), ws_p.numel(),
                                                                 ctypes.byref(ia), sp), "sort_pairs"), refill)
    med_k, ms_k = timed(lambda: capi.check(L_.mgc_dev_radix_sort(ptr(keys), ptr(alt), n, kw, 0, bits, ptr(ws_k), ws_k.numel(),
                                                                 ctypes.byref(ia), sp), "radix_sort"), refill)
    emit(what="pair_sort", key_bytes=8 * kw, bits=bits, n=n, pairs_ms=round(med_p, 3), keys_ms=round(med_k, 3), ratio=round(med_p / med_k, 3),
         traffic_ratio=round((8 * kw + 4) / (8 * kw), 3), pairs_per_s=round(n / med_p * 1e3), pairs_samples_ms=ms_p, keys_samples_ms=ms_k)
    # the reduction over the sorted pairs (a third of the keys repeated)
    refill()
    (keys if kw == 1 else keys[:, 0]).div_(3, rounding_mode="floor")
    capi.check(L_.mgc_dev_sort_pairs(ptr(keys), ptr(v), ptr(alt), ptr(av), n, kw, 0, bits, ptr(ws_p), ws_p.numel(), ctypes.byref(ia), sp), "sort_pairs")
    sk, sv = (alt, av) if ia.value else (keys, v)
    ok, ov = (keys, v) if ia.value else (alt, av)
    ws_r = torch.empty(L_.mgc_dev_reduce_pairs_workspace_bytes(n), dtype=torch.uint8, device=dev)
    nd = ctypes.c_uint64(0)

    def reduce_step():
        capi.check(L_.mgc_dev_reduce_pairs_count(ptr(sk), ptr(sv), n, kw, ptr(ws_r), ws_r.numel(), ctypes.byref(nd), sp), "reduce_count")
        capi.check(L_.mgc_dev_reduce_pairs_emit(ptr(sk), ptr(sv), n, kw, ptr(ws_r), ws_r.numel(), ptr(ok), ptr(ov), sp), "reduce_emit")

    med_r, ms_r = timed(reduce_step)
    emit(what="reduce", key_bytes=8 * kw, n=n, distinct=nd.value, ms=round(med_r, 3), pairs_per_s=round(n / med_r * 1e3), samples_ms=ms_r)
    # the labelled leg: the same keys and values with a uint64 label each
    labs = torch.randint(0, 1 << 62, (n,), generator=g, device=dev, dtype=torch.int64)
    lb, alb = torch.empty_like(labs), torch.empty_like(labs)
    ws_t = torch.empty(L_.mgc_dev_sort_triples_workspace_bytes(n), dtype=torch.uint8, device=dev)

    def refill3():
        refill()
        lb.copy_(labs)

    def sort3():
        capi.check(L_.mgc_dev_sort_triples(ptr(keys), ptr(v), ptr(lb), ptr(alt), ptr(av), ptr(alb), n, kw, 0, bits, ptr(ws_t), ws_t.numel(),
                                           ctypes.byref(ia), sp), "sort_triples")

    med_t, ms_t = timed(sort3, refill3)
    emit(what="triple_sort", key_bytes=8 * kw, bits=bits, n=n, triples_ms=round(med_t, 3), pairs_ms=round(med_p, 3), ratio=round(med_t / med_p, 3),
         triples_per_s=round(n / med_t * 1e3), triples_samples_ms=ms_t)
    refill3()
    (keys if kw == 1 else keys[:, 0]).div_(3, rounding_mode="floor")
    sort3()
    sk, sv, sl = (alt, av, alb) if ia.value else (keys, v, lb)
    ok, ov, ol = (keys, v, lb) if ia.value else (alt, av, alb)
    ws_r3 = torch.empty(L_.mgc_dev_reduce_triples_workspace_bytes(n), dtype=torch.uint8, device=dev)

    def reduce3():
        capi.check(L_.mgc_dev_reduce_triples_count(ptr(sk), ptr(sv), ptr(sl), n, kw, ptr(ws_r3), ws_r3.numel(), ctypes.byref(nd), sp), "reduce3_count")
        capi.check(L_.mgc_dev_reduce_triples_emit(ptr(sk), ptr(sv), ptr(sl), n, kw, 64, ptr(ws_r3), ws_r3.numel(), ptr(ok), ptr(ov), ptr(ol), sp),
                   "reduce3_emit")

    med_r3, ms_r3 = timed(reduce3)
    emit(what="reduce_triples", key_bytes=8 * kw, n=n, distinct=nd.value, triples_ms=round(med_r3, 3), pairs_ms=round(med_r, 3),
         ratio=round(med_r3 / med_r, 3), triples_per_s=round(n / med_r3 * 1e3), samples_ms=ms_r3)
    del src, vals, keys, alt, v, av, ws_p, ws_k, ws_r, labs, lb, alb, ws_t, ws_r3
    torch.cuda.empty_cache()

# ---- `meryl print` of a k = 21 count -> database ------------------------------------------------------------------------
K = 21
bases = count.dev_synth_reads(2, 333_333_334, 0, reads, 150, 5000, 100)
cfg = capi.configure(K, bases.numel(), 128 << 30)
db_a, txt = os.path.join(work, "a.meryl"), os.path.join(work, "a.txt")
with count.Session(cfg, 0) as s:
    s.push_bases_device(bases)
    s.count()
    n_distinct = s.info().n_distinct
    s.write_database(db_a, 16)
del bases
torch.cuda.empty_cache()
with open(txt, "wb") as f:
    subprocess.run([build.build_cli(), "-Q", "print", db_a], check=True, stdout=f)
text_bytes = os.path.getsize(txt)
emit(what="import_input", k=K, kmers=n_distinct, text_bytes=text_bytes, bytes_per_record=round(text_bytes / max(1, n_distinct), 2), dir=work)


def import_runs(tag, env_batch, path=None, label_width=0):
    path = path or txt
    n_bytes = os.path.getsize(path)
    if env_batch:
        os.environ["MGC_IMPORT_BATCH"] = str(env_batch)
    else:
        os.environ.pop("MGC_IMPORT_BATCH", None)
    runs = []
    for rep in range(4):                                     # the first is the warm-up (code objects, page cache)
        out = os.path.join(work, "b.meryl")
        shutil.rmtree(out, ignore_errors=True)
        t0 = time.perf_counter()
        info = kmer_import.import_file(path, K, out, host_threads=16, **({"label_width": label_width} if label_width else {}))
        info["wall_s"] = time.perf_counter() - t0
        if rep:
            runs.append(info)
    med = sorted(runs, key=lambda r: r["wall_s"])[len(runs) // 2]
    device_ms = med["parse_ms"] + med["sort_ms"] + med["reduce_ms"]
    emit(what="import_labelled" if label_width else "import", mode=tag, batches=med["n_batches"], records=med["n_records"], distinct=med["n_distinct"],
         wall_s=round(med["wall_s"], 3), text_gb_per_s=round(n_bytes / med["wall_s"] / 1e9, 3),
         upload_ms=round(med["upload_ms"], 3), upload_gb_per_s=round(n_bytes / max(med["upload_ms"], 1e-9) / 1e6, 2),
         parse_ms=round(med["parse_ms"], 3), sort_ms=round(med["sort_ms"], 3), reduce_ms=round(med["reduce_ms"], 3),
         device_ms=round(device_ms, 3), device_over_upload=round(device_ms / max(med["upload_ms"], 1e-9), 3),
         read_s=round(med["read_s"], 3), write_s=round(med["write_s"], 3), samples_wall_s=[round(r["wall_s"], 3) for r in runs])
    return med


pairs_run = import_runs("default", 0)
import_runs("batches", batch_mb << 20)
# the labelled leg: the same lines with a third column, the line number modulo 256 as an 8-bit label
txt3 = os.path.join(work, "a3.txt")
with open(txt3, "wb") as f:
    subprocess.run(["awk", '{print $0 "\t" (NR % 256)}', txt], check=True, stdout=f)
triples_run = import_runs("default", 0, txt3, 8)
import_runs("batches", batch_mb << 20, txt3, 8)
emit(what="import_labelled_vs_pairs", k=K, records=triples_run["n_records"], label_width=8,
     **{"%s_ms" % stage: {"triples": round(triples_run["%s_ms" % stage], 3), "pairs": round(pairs_run["%s_ms" % stage], 3),
                          "ratio": round(triples_run["%s_ms" % stage] / max(pairs_run["%s_ms" % stage], 1e-9), 3)}
        for stage in ("parse", "sort", "reduce")})
os.environ.pop("MGC_IMPORT_BATCH", None)
times = []
for rep in range(3):
    out = os.path.join(work, "c.meryl")
    shutil.rmtree(out, ignore_errors=True)
    t0 = time.perf_counter()
    subprocess.run([build.build_import_cli(), "-k", str(K), "-kmers", txt, "-output", out], check=True, capture_output=True)
    times.append(time.perf_counter() - t0)
emit(what="import_cli", seconds=round(statistics.median(times), 3), text_gb_per_s=round(text_bytes / statistics.median(times) / 1e9, 3),
     samples_s=[round(x, 3) for x in times])
if own_dir:
    shutil.rmtree(work, ignore_errors=True)
