#!/usr/bin/env python3
"""Timing of meryl-lookup's per-position lookups and reports (include/meryl_lookup.h) on one GPU.

A synthetic genome (GENOME_MBP Mbp, default 300, cut into 50 Mbp "chromosomes" with a few N) is read at ~10x coverage
(150-base reads, 0.5 % substitutions, made on the device), the reads are counted in-process at k = 21, and the genome is
looked up in the counted table:
  * mgc_lookup_positions for presence / count / depth, in windows per second (HIP events, median of 5 after a warm-up);
  * mgc_lookup_existence on the same stream and table -- presence with one table costs the same lookups per window;
  * Lookup.load of the counted table written to a database (min_value 2), in seconds (median of 3 after a warm-up);
  * mgc_lookup_report end to end for every mode into a sink callback, in GB of text per second.
usage: python scripts/lookup_bench.py [GENOME_MBP] > profiles/lookup_bench.json   (one JSON object per line)"""
import ctypes
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

sys.path.insert(0, '.')
import numpy as np  # noqa: E402
import torch  # noqa: E402
from meryl_amd import capi, count, db, lookup  # noqa: E402

K = 21
genome_mbp = int(sys.argv[1]) if len(sys.argv) > 1 else 300
n = genome_mbp * 1_000_000
dev = torch.device("cuda")
g = torch.Generator(device=dev)
g.manual_seed(20261016)
lut = torch.tensor(list(b"ACTG"), dtype=torch.uint8, device=dev)
codes = torch.randint(0, 4, (n,), generator=g, device=dev, dtype=torch.uint8)
genome = lut[codes.long()]
del codes

# reads: 10x, 150 bases + '.', 0.5 % substitutions
read_len, n_reads = 150, n * 10 // 150
reads_parts = []
for lo in range(0, n_reads, 4_000_000):
    m = min(4_000_000, n_reads - lo)
    start = torch.randint(0, n - read_len, (m, 1), generator=g, device=dev)
    r = genome[start + torch.arange(read_len, device=dev)]
    sub = torch.rand(r.shape, generator=g, device=dev) < 0.005
    r = torch.where(sub, lut[torch.randint(0, 4, r.shape, generator=g, device=dev).long()], r)
    reads_parts.append(torch.cat([r, torch.full((m, 1), ord("."), dtype=torch.uint8, device=dev)], dim=1).reshape(-1))
reads = torch.cat(reads_parts)
del reads_parts
torch.cuda.synchronize()
cfg = capi.configure(K, reads.numel(), 128 << 30)
with count.Session(cfg, 0) as s:
    s.push_bases_device(reads)
    s.count()
    keys, cnts = s.result_device()
    table = lookup.Lookup.from_device(keys, cnts, K)
    work = tempfile.mkdtemp(prefix="lookup_bench.")
    db.write_database(s, os.path.join(work, "reads.meryl"))
del reads, keys, cnts
torch.cuda.empty_cache()

# the query: the genome in 50 Mbp sequences, each ending with '.', and a few N
chrom = 50_000_000
stream = genome.clone()
stream[torch.randint(0, n, (n // 100_000,), generator=g, device=dev)] = ord("N")
stream[chrom - 1::chrom] = ord(".")
stream[-1] = ord(".")
seq_start = list(range(0, n, chrom)) + [n]
names = ["chr%d" % i for i in range(len(seq_start) - 1)]
torch.cuda.synchronize()
L = capi.lib()
stream_ptr = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


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
    return statistics.median(ms), ms


def emit(**kv):
    print(json.dumps(kv), flush=True)


emit(what="setup", genome_bases=n, k=K, table_kmers=int(table.info.n_kmers), index_bits=int(table.info.index_bits),
     read_coverage=10, sequences=len(names))
# the table loaded from its database: 64 data files read by host threads, decoded and value-filtered on the device
load_s = []
for rep in range(4):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    loaded = lookup.Lookup.load(os.path.join(work, "reads.meryl"), min_value=2)
    load_s.append(time.perf_counter() - t0)
    load_kmers = int(loaded.info.n_kmers)
    loaded.close()
shutil.rmtree(work)
emit(what="load", min_value=2, seconds=round(statistics.median(load_s[1:]), 4), table_kmers=load_kmers,
     kmers_in_db_per_s=round(int(table.info.n_kmers) / statistics.median(load_s[1:])), samples_s=[round(x, 4) for x in load_s[1:]])
out = torch.empty(n, dtype=torch.int32, device=dev)
arr = (ctypes.c_void_p * 1)(table._h)
res = {}
for what, code in lookup.WHAT.items():
    med, ms = timed(lambda: capi.check(L.mgc_lookup_positions(arr, 1, code, ctypes.c_void_p(stream.data_ptr()), n,
                                                              ctypes.c_void_p(out.data_ptr()), stream_ptr), "positions"))
    res[what] = med
    emit(what="positions", kind=what, tables=1, ms=round(med, 3), windows_per_s=round(n / med * 1e3), samples_ms=[round(x, 3) for x in ms])
ss = torch.tensor(seq_start, dtype=torch.int64, device=dev)
tot = torch.empty(len(names), dtype=torch.int64, device=dev)
fnd = torch.empty(len(names), dtype=torch.int64, device=dev)
med, ms = timed(lambda: capi.check(L.mgc_lookup_existence(table._h, ctypes.c_void_p(stream.data_ptr()), n, ctypes.c_void_p(ss.data_ptr()),
                                                          len(names), ctypes.c_void_p(tot.data_ptr()), ctypes.c_void_p(fnd.data_ptr()),
                                                          stream_ptr), "existence"))
emit(what="existence", ms=round(med, 3), windows_per_s=round(n / med * 1e3), samples_ms=[round(x, 3) for x in ms],
     found_fraction=round(float(fnd.sum()) / max(1, float(tot.sum())), 4),
     presence_over_existence=round(res["presence"] / med, 3))

# reports end to end: the text goes to a callback that only counts it
sink = {"bytes": 0, "pieces": 0}


def _sink(_data, nbytes, _user):
    sink["bytes"] += nbytes
    sink["pieces"] += 1
    return 0


cb = capi.LOOKUP_WRITE_CB(_sink)
c_names = (ctypes.c_char_p * len(names))(*[x.encode() for x in names])
c_ss = np.array(seq_start, dtype=np.uint64)
for mode, code in lookup.MODES.items():
    times = []
    for rep in range(3):
        sink["bytes"] = sink["pieces"] = 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        capi.check(L.mgc_lookup_report(arr, 1, code, None, 0, ctypes.c_void_p(stream.data_ptr()), n,
                                       c_ss.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), c_names, len(names), 64 << 20, cb, None),
                   "report")
        times.append(time.perf_counter() - t0)
    t = statistics.median(times[1:])
    emit(what="report", mode=mode, seconds=round(t, 4), text_bytes=sink["bytes"], pieces=sink["pieces"],
         text_gb_per_s=round(sink["bytes"] / t / 1e9, 3), bases_per_s=round(n / t), samples_s=[round(x, 4) for x in times])
table.close()
