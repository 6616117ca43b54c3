#!/usr/bin/env python3
"""Timing of the k-mer position index and of query painting (include/meryl_positions.h) on one GPU.

A synthetic reference (GENOME_MBP Mbp, default 100, cut into 50 Mbp "chromosomes" with a few N) is counted in-process at
k = 21 into the lookup table; reads of it (150 bases, 0.5 % substitutions, COVERAGE x, default 2, made on the device) are the
queries.  Timed, each as the median of 5 after a warm-up:
  * mgc_posidx_build (wall clock: it sizes its lists on the host);
  * mgc_paint_add of all the reads in one batch with all three outputs, with MERS alone and with HITS alone (wall clock: the
    call returns when the batch is done), in seconds per Gbp of query;
  * the yardstick: Lookup.stream over the same query bases with the same table -- the same lookups and nothing else (HIP events);
  * the two gathers, mgc_paint_get of MERS and of QUERIES (HIP events).
usage: python scripts/positions_bench.py [GENOME_MBP [COVERAGE]] > profiles/positions_bench.jsonl   (one JSON object per line)"""
import ctypes
import json
import statistics
import sys
import time

sys.path.insert(0, '.')
import torch  # noqa: E402
from meryl_amd import capi, count, lookup, poslookup  # noqa: E402

K = 21
genome_mbp = int(sys.argv[1]) if len(sys.argv) > 1 else 100
coverage = int(sys.argv[2]) if len(sys.argv) > 2 else 2
n = genome_mbp * 1_000_000
dev = torch.device("cuda")
g = torch.Generator(device=dev)
g.manual_seed(20261019)
lut = torch.tensor(list(b"ACTG"), dtype=torch.uint8, device=dev)
codes = torch.randint(0, 4, (n,), generator=g, device=dev, dtype=torch.uint8)
genome = lut[codes.long()]
del codes

# the reference: the genome in 50 Mbp sequences, each ending with '.', and a few N
chrom = 50_000_000
ref = genome.clone()
ref[torch.randint(0, n, (n // 100_000,), generator=g, device=dev)] = ord("N")
ref[chrom - 1::chrom] = ord(".")
ref[-1] = ord(".")

# the queries: 150 bases + '.', 0.5 % substitutions
read_len, n_reads = 150, n * coverage // 150
parts = []
for lo in range(0, n_reads, 4_000_000):
    m = min(4_000_000, n_reads - lo)
    start = torch.randint(0, n - read_len, (m, 1), generator=g, device=dev)
    r = genome[start + torch.arange(read_len, device=dev)]
    sub = torch.rand(r.shape, generator=g, device=dev) < 0.005
    r = torch.where(sub, lut[torch.randint(0, 4, r.shape, generator=g, device=dev).long()], r)
    parts.append(torch.cat([r, torch.full((m, 1), ord("."), dtype=torch.uint8, device=dev)], dim=1).reshape(-1))
reads = torch.cat(parts)
del parts, genome
seq_start = torch.arange(0, n_reads + 1, device=dev, dtype=torch.int64) * (read_len + 1)
torch.cuda.synchronize()

cfg = capi.configure(K, n, 128 << 30)
with count.Session(cfg, 0) as s:
    s.push_bases_device(ref)
    s.count()
    keys, cnts = s.result_device()
    table = lookup.Lookup.from_device(keys, cnts, K)
del keys, cnts
torch.cuda.empty_cache()
L = capi.lib()
stream_ptr = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def emit(**kv):
    print(json.dumps(kv), flush=True)


def wall(fn, reps=5):
    fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), out


def events(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out), out


def rounded(ms):
    return [round(x, 3) for x in ms]


def build_once():
    poslookup.PositionIndex(table, ref).close()


med, ms = wall(build_once, 3)
index = poslookup.PositionIndex(table, ref)
emit(what="setup", reference_bases=n, table_kmers=int(table.info.n_kmers), query_bases=int(reads.numel()), queries=n_reads,
     **index.info.as_dict())
emit(what="index_build", ms=round(med, 3), ref_bases_per_s=round(n / med * 1e3), samples_ms=rounded(ms))

gbp = reads.numel() / 1e9
sv = torch.empty(reads.numel(), dtype=torch.int32, device=dev)
base_ms, ms = events(lambda: capi.check(L.mgc_lookup_stream(table._h, ctypes.c_void_p(reads.data_ptr()), reads.numel(),
                                                            ctypes.c_void_p(sv.data_ptr()), stream_ptr), "stream"))
emit(what="lookup_stream", ms=round(base_ms, 3), s_per_gbp=round(base_ms / 1e3 / gbp, 4), hit_fraction=round(float((sv != 0).float().mean()), 4),
     samples_ms=rounded(ms))
del sv

per = torch.empty(n_reads, dtype=torch.int32, device=dev)
cov = torch.empty(n_reads, dtype=torch.int32, device=dev)
for name, what in (("hits+mers+queries", 7), ("mers", poslookup.MERS), ("hits", poslookup.HITS)):
    with poslookup.Painter(index, what) as p:
        med, ms = wall(lambda: poslookup._check(L.mgc_paint_add(p._h, ctypes.c_void_p(reads.data_ptr()), reads.numel(),
                                                                ctypes.c_void_p(seq_start.data_ptr()), n_reads, ctypes.c_void_p(per.data_ptr()),
                                                                ctypes.c_void_p(cov.data_ptr()), stream_ptr), "paint_add"))
        emit(what="paint_add", outputs=name, ms=round(med, 3), s_per_gbp=round(med / 1e3 / gbp, 4), over_lookup_stream=round(med / base_ms, 3),
             samples_ms=rounded(ms))
        if what == 7:
            out = torch.empty(index.info.n_ref_bases, dtype=torch.int32, device=dev)
            for gname, which in (("mers", poslookup.MERS), ("queries", poslookup.QUERIES)):
                gmed, gms = events(lambda: poslookup._check(L.mgc_paint_get(p._h, which, ctypes.c_void_p(out.data_ptr()), stream_ptr), "paint_get"))
                emit(what="paint_get", output=gname, ms=round(gmed, 3), ref_bases_per_s=round(n / gmed * 1e3),
                     gb_per_s=round(12.0 * n / gmed / 1e6, 1), painted_fraction=round(float((out != 0).float().mean()), 4), samples_ms=rounded(gms))
            del out
index.close()
table.close()
