#!/usr/bin/env python3
"""Timing of meryl-lookup -include / -exclude (mgc_lookup_filter_text, include/meryl_lookup.h) on one GPU.

A synthetic genome (GENOME_MBP Mbp, default 100) is read at ~10x coverage and counted in-process at k = 21 (the table of
scripts/lookup_bench.py).  The query: PAIRS_M million pairs (default 4) of 150-base reads as four-line FASTQ text resident
in HBM, half of the pairs from the genome and half random, so about half are kept.  One JSON object per line:
  * mgc_lookup_filter_text (-include, both inputs): ms per step, GB/s of input text, windows/s (HIP events, a warm-up,
    median of 5, the samples kept);
  * mgc_lookup_existence on the same reads as a base stream with the same table, and a device-to-device copy of as many
    bytes as the text, in the same process: the filter step should cost about the existence call plus a small multiple of
    the copy;
  * with --cli DIR: file -> files through the CLI under DIR (a tmpfs), plain and BGZF-or-gzip input, wall clock.
The split between index, found-count and emit kernels comes from a run of its own:
  rocprofv3 --kernel-trace --stats -d filter_prof -- python scripts/lookup_filter_bench.py 100 2
usage: python scripts/lookup_filter_bench.py [GENOME_MBP] [PAIRS_M] [--cli DIR] >> profiles/lookup_filter_bench.jsonl"""
import ctypes
import gzip
import json
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, '.')
import numpy as np  # noqa: E402
import torch  # noqa: E402
from meryl_amd import build, capi, count, lookup  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
cli_dir = sys.argv[sys.argv.index("--cli") + 1] if "--cli" in sys.argv else None
if cli_dir:
    args.remove(cli_dir)
K, L = 21, 150
n = (int(args[0]) if args else 100) * 1_000_000
pairs = int((float(args[1]) if len(args) > 1 else 4) * 1_000_000)
dev = torch.device("cuda")
g = torch.Generator(device=dev)
g.manual_seed(20261016)
lut = torch.tensor(list(b"ACTG"), dtype=torch.uint8, device=dev)
genome = lut[torch.randint(0, 4, (n,), generator=g, device=dev, dtype=torch.uint8).long()]


def sample_reads(m, own):
    """[m, L] bases: from the genome with 0.5 % substitutions where own, random elsewhere"""
    out = torch.empty((m, L), dtype=torch.uint8, device=dev)
    for lo in range(0, m, 2_000_000):
        hi = min(m, lo + 2_000_000)
        start = torch.randint(0, n - L, (hi - lo, 1), generator=g, device=dev)
        r = genome[start + torch.arange(L, device=dev)]
        rnd = lut[torch.randint(0, 4, r.shape, generator=g, device=dev).long()]
        sub = torch.rand(r.shape, generator=g, device=dev) < 0.005
        out[lo:hi] = torch.where(sub | ~own[lo:hi, None], rnd, r)
    return out


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


# the table: 10x reads of the genome, counted in process
n_reads = n * 10 // L
all_own = torch.ones(n_reads, dtype=torch.bool, device=dev)
reads = torch.cat([sample_reads(n_reads, all_own), torch.full((n_reads, 1), ord("."), dtype=torch.uint8, device=dev)], dim=1).reshape(-1)
cfg = capi.configure(K, reads.numel(), 128 << 30)
with count.Session(cfg, 0) as s:
    s.push_bases_device(reads)
    s.count()
    keys, cnts = s.result_device()
    table = lookup.Lookup.from_device(keys, cnts, K)
del reads, keys, cnts, all_own
torch.cuda.empty_cache()


def fastq(bases, tag):
    """four-line FASTQ text of [m, L] bases on the device: @p<9 digits>/<tag> \\n bases \\n + \\n I*L \\n"""
    m = bases.shape[0]
    idx = torch.arange(m, device=dev)
    digits = torch.stack([(idx // 10 ** (8 - j)) % 10 + ord("0") for j in range(9)], dim=1).to(torch.uint8)
    col = lambda s: torch.tensor(list(s), dtype=torch.uint8, device=dev).expand(m, len(s))
    return torch.cat([col(b"@p"), digits, col(b"/" + tag + b"\n"), bases, col(b"\n+\n" + b"I" * L + b"\n")], dim=1).reshape(-1)


own = torch.rand(pairs, generator=g, device=dev) < 0.5
b1, b2 = sample_reads(pairs, own), sample_reads(pairs, own)
texts = [fastq(b1, b"1"), fastq(b2, b"2")]
text_bytes = sum(t.numel() for t in texts)
outs = [torch.empty(t.numel() + t.numel() // 4, dtype=torch.uint8, device=dev) for t in texts]
L_ = capi.lib()
sp = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
res = capi.FilterResult()
c_text = (ctypes.c_void_p * 2)(*[t.data_ptr() for t in texts])
c_n = (ctypes.c_uint64 * 2)(*[t.numel() for t in texts])
c_out = (ctypes.c_void_p * 2)(*[o.data_ptr() for o in outs])
c_cap = (ctypes.c_uint64 * 2)(*[o.numel() for o in outs])
windows = 2 * pairs * (L - K + 1)
emit(what="setup", genome_bases=n, k=K, table_kmers=int(table.info.n_kmers), pairs=pairs, text_bytes=text_bytes, windows=windows)


def step():
    capi.check(L_.mgc_lookup_filter_text(table._h, 0, 0, 2, c_text, c_n, 1, c_out, c_cap, ctypes.byref(res), sp), "filter_text")


med_f, ms = timed(step)
emit(what="filter_text", mode="include", ms=round(med_f, 3), text_gb_per_s=round(text_bytes / med_f / 1e6, 3),
     windows_per_s=round(windows / med_f * 1e3), kept_fraction=round(res.n_kept / max(1, res.n_records), 4),
     out_bytes=list(res.out_bytes), samples_ms=ms)

# the same reads as a base stream ('.' after each) through mgc_lookup_existence, and a copy of as many bytes as the text
stream = torch.cat([torch.cat([b, torch.full((pairs, 1), ord("."), dtype=torch.uint8, device=dev)], dim=1).reshape(-1) for b in (b1, b2)])
ss = torch.arange(0, stream.numel() + 1, L + 1, dtype=torch.int64, device=dev)
tot = torch.empty(2 * pairs, dtype=torch.int64, device=dev)
fnd = torch.empty(2 * pairs, dtype=torch.int64, device=dev)
med_e, ms = timed(lambda: capi.check(L_.mgc_lookup_existence(table._h, ctypes.c_void_p(stream.data_ptr()), stream.numel(),
                                                             ctypes.c_void_p(ss.data_ptr()), 2 * pairs, ctypes.c_void_p(tot.data_ptr()),
                                                             ctypes.c_void_p(fnd.data_ptr()), sp), "existence"))
emit(what="existence", ms=round(med_e, 3), windows_per_s=round(windows / med_e * 1e3), samples_ms=ms)
src = torch.cat(texts)
dst = torch.empty_like(src)
med_c, ms = timed(lambda: dst.copy_(src))
emit(what="copy", bytes=text_bytes, ms=round(med_c, 3), gb_per_s=round(text_bytes / med_c / 1e6, 1), samples_ms=ms)
emit(what="summary", filter_ms=round(med_f, 3), existence_ms=round(med_e, 3), copy_ms=round(med_c, 3),
     filter_minus_existence_in_copies=round((med_f - med_e) / med_c, 2))
table.close()

if cli_dir:                                                   # file -> files through the CLI (read, device and write are one wall clock)
    r1, r2 = texts[0].cpu().numpy().tobytes(), texts[1].cpu().numpy().tobytes()
    gen = lut[torch.randint(0, 4, (1,), device=dev).long()]  # (keeps the generator state out of the files)
    del gen
    open(os.path.join(cli_dir, "db.fa"), "wb").write(b">g\n" + genome.cpu().numpy().tobytes() + b"\n")
    subprocess.run([build.build_cli(), "-Q", "k=21", "memory=16", "count", os.path.join(cli_dir, "db.fa"), "output",
                    os.path.join(cli_dir, "db.meryl")], check=True)
    for kind in ("plain", "gzip"):
        names = []
        for tag, body in (("R1", r1), ("R2", r2)):
            names.append(os.path.join(cli_dir, tag + (".fq" if kind == "plain" else ".fq.gz")))
            (open if kind == "plain" else lambda p, m: gzip.open(p, m, compresslevel=1))(names[-1], "wb").write(body)
        times = []
        for rep in range(3):
            t0 = time.perf_counter()
            subprocess.run([build.build_lookup_cli(), "-include", "-sequence"] + names + ["-mers", os.path.join(cli_dir, "db.meryl"), "-output",
                            os.path.join(cli_dir, "o1.fq"), os.path.join(cli_dir, "o2.fq")], check=True, capture_output=True)
            times.append(time.perf_counter() - t0)
        emit(what="cli", input=kind, seconds=round(statistics.median(times), 3), text_gb_per_s=round(text_bytes / statistics.median(times) / 1e9, 3),
             samples_s=[round(x, 3) for x in times])
