#!/usr/bin/env python
"""BAM input decoded on the device: what the decode kernel costs against the upload it hides behind, and file -> database
runs of the CLI over the new route, the host reader and (optionally) another build's binary.

    python scripts/bam_bench.py kernel [--iters 20]
        mgc_dev_bam_decode on a 32 MiB piece of 150-base records and on one of 15 kb records (qualities, 2 KB of aux each),
        against a device-to-device copy with the same traffic (half of what the decode reads plus writes, read and written), and
        against the upload of the piece (and its segment table) from pinned memory.  Timed with events in this process, a window
        of twelve launches over twelve sets of buffers (more than the last-level cache holds) at a time.  One JSON line per piece;
        "hides_behind_upload" is decode_ms < upload_ms.

    python scripts/bam_bench.py e2e [--dir /tmp/bam_bench] [--other-meryl PATH] [--runs 3] [--short-reads 4000000] [--long-bases 1000000000]
        writes a short-read BAM (reads of 150 bases) and a long-read BAM (reads of 15 kb, with qualities) and the same reads as
        bgzip'd FASTQ, then counts each with the CLI (threads=16, k=21), the routes taken in turn, --runs times: this build's
        default route, this build with MERYL_HOST_PARSER=1, PATH's default route.  One JSON line per run with the read phase of
        the -V TIMING line and the [io] line of MGC_IO_TRACE, and a summary line per file."""
import argparse
import ctypes
import json
import os
import re
import shutil
import struct
import subprocess
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NT16 = b"=ACMGRSVTWYHKDBN"
SEG = np.dtype([("src_off", "<u4"), ("nbf", "<u4"), ("out_off", "<u8")])
DOT = 1 << 31


def records(rows, qual_bytes, aux_bytes):
    """rows: uint8[reads, L] of ACGT letters (L even) -> uint8[reads, record bytes]: fixed-shape BAM records, name "r" """
    reads, L = rows.shape
    lut = np.zeros(256, dtype=np.uint8)
    for i, ch in enumerate(NT16):
        lut[ch] = i
    codes = lut[rows]
    packed = (codes[:, 0::2] << 4) | codes[:, 1::2]
    fixed = struct.pack("<iiBBHHHiiii", -1, -1, 2, 0, 4680, 0, 4, L, -1, -1, 0) + b"r\0"
    body = len(fixed) + L // 2 + qual_bytes + aux_bytes
    rec = np.empty((reads, 4 + body), dtype=np.uint8)
    rec[:, :4] = np.frombuffer(struct.pack("<i", body), dtype=np.uint8)
    rec[:, 4:4 + len(fixed)] = np.frombuffer(fixed, dtype=np.uint8)
    rec[:, 4 + len(fixed):4 + len(fixed) + L // 2] = packed
    rec[:, 4 + len(fixed) + L // 2:4 + len(fixed) + L // 2 + qual_bytes] = 0x28
    if aux_bytes:
        rec[:, 4 + len(fixed) + L // 2 + qual_bytes:] = np.frombuffer((b"ZZZ" + b"x" * 60 + b"\0") * (aux_bytes // 64 + 1), dtype=np.uint8)[:aux_bytes]
    return rec, 4 + len(fixed)


def random_rows(rng, reads, L):
    genome = rng.integers(0, 4, 5_000_000 + L, dtype=np.uint8)
    starts = rng.integers(0, 5_000_000, reads)
    out = np.empty((reads, L), dtype=np.uint8)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    slab = max(1, (16 << 20) // L)                            # in slabs: the index array of a whole file would not fit
    for a in range(0, reads, slab):
        s = starts[a:a + slab]
        out[a:a + s.size] = letters[genome[s[:, None] + np.arange(L)[None, :]]]
    return out


def bgzf_fast(data, block=0xff00):
    out = []
    for i in range(0, len(data), block):
        d = data[i:i + block]
        c = zlib.compressobj(1, zlib.DEFLATED, -15)
        cd = c.compress(d) + c.flush()
        bs = 12 + 6 + len(cd) + 8
        out.append(struct.pack("<BBBBIBBH", 0x1f, 0x8b, 8, 4, 0, 0, 0xff, 6) + b"BC" + struct.pack("<HH", 2, bs - 1) + cd +
                   struct.pack("<II", zlib.crc32(d) & 0xffffffff, len(d)))
    return b"".join(out) + bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")     # the EOF marker (SAMv1 4.1.2)


# ---- the kernel ---------------------------------------------------------------------------------------------------------
def kernel_leg(name, L, qual, aux, iters):
    import torch
    from meryl_amd import capi
    L_ = capi.lib()
    rng = np.random.default_rng(7)
    rec_bytes = records(np.full((1, L), ord("A"), dtype=np.uint8), qual, aux)[0].shape[1]
    reads = ((32 << 20) - 12) // rec_bytes
    rec, seq_at = records(random_rows(rng, reads, L), qual, aux)
    piece = np.concatenate([np.frombuffer(b"BAM\x01" + struct.pack("<ii", 0, 0), dtype=np.uint8), rec.reshape(-1)])
    table = np.zeros(reads, dtype=SEG)
    table["src_off"] = 12 + np.arange(reads, dtype=np.uint64) * rec_bytes + seq_at
    table["nbf"] = L | DOT
    table["out_off"] = np.arange(reads, dtype=np.uint64) * (L + 1)
    out_bytes = reads * (L + 1)
    h_piece = torch.from_numpy(piece).pin_memory()
    h_tab = torch.from_numpy(np.frombuffer(table.tobytes(), dtype=np.uint8).copy()).pin_memory()
    read_bytes = reads * (L // 2) + h_tab.numel()             # what the decode reads: the packed SEQ fields and the table
    moved = read_bytes + out_bytes
    # SETS sets of buffers, taken in turn, one launch on each per timed window: a set is ~85 MB, the sets together are several
    # times the 256 MiB of last-level cache, so that no launch finds its piece or its output there from the launch before
    SETS = 12
    d_piece = [torch.from_numpy(piece).cuda() for _ in range(SETS)]
    d_tab = [h_tab.cuda() for _ in range(SETS)]
    d_out = [torch.empty(out_bytes + 64, dtype=torch.uint8, device="cuda") for _ in range(SETS)]
    # the copy reads moved / 2 bytes and writes as many: the decode's traffic
    d_src = [torch.empty(moved // 2, dtype=torch.uint8, device="cuda") for _ in range(SETS)]
    d_dst = [torch.empty(moved // 2, dtype=torch.uint8, device="cuda") for _ in range(SETS)]
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def upload(i):
        d_piece[i].copy_(h_piece, non_blocking=True)
        d_tab[i].copy_(h_tab, non_blocking=True)

    def decode(i):
        capi.check(L_.mgc_dev_bam_decode(ctypes.c_void_p(d_piece[i].data_ptr()), piece.size, ctypes.c_void_p(d_tab[i].data_ptr()), reads, out_bytes,
                                         ctypes.c_void_p(d_out[i].data_ptr() + 5), st), "mgc_dev_bam_decode")

    def copy(i):
        d_dst[i].copy_(d_src[i], non_blocking=True)

    def timed(f):
        """ms per call: `iters` windows of SETS calls each, one per buffer set -> (median, min, max)"""
        for i in range(SETS):
            f(i)
        torch.cuda.synchronize()
        ms = []
        for _ in range(iters):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for i in range(SETS):
                f(i)
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b) / SETS)
        return float(np.median(ms)), float(min(ms)), float(max(ms))

    up, dec, cp = timed(upload), timed(decode), timed(copy)
    # the result, once, against numpy
    want = np.empty((reads, L + 1), dtype=np.uint8)
    codes = np.empty((reads, L), dtype=np.uint8)
    packed = rec[:, seq_at:seq_at + L // 2]
    codes[:, 0::2] = packed >> 4
    codes[:, 1::2] = packed & 15
    want[:, :L] = np.frombuffer(NT16, dtype=np.uint8)[codes]
    want[:, L] = ord(".")
    ok = all(bool(np.array_equal(d_out[i][5:5 + out_bytes].cpu().numpy(), want.reshape(-1))) for i in (0, SETS - 1))
    print(json.dumps({"leg": "kernel", "piece": name, "piece_bytes": int(piece.size), "records": int(reads), "out_bytes": int(out_bytes),
                      "decode_reads_plus_writes": int(moved), "buffer_sets": SETS, "decode_ms": dec[0], "decode_ms_min_max": dec[1:], "copy_ms": cp[0], "copy_ms_min_max": cp[1:],
                      "decode_over_copy": dec[0] / cp[0], "upload_ms": up[0], "upload_ms_min_max": up[1:], "upload_GBps": (piece.size + h_tab.numel()) / up[0] / 1e6,
                      "decode_GBps_out": out_bytes / dec[0] / 1e6, "hides_behind_upload": dec[0] < up[0], "correct": ok}), flush=True)
    return ok and dec[0] < up[0]


# ---- end to end ---------------------------------------------------------------------------------------------------------
def write_inputs(d, short_reads, long_bases):
    os.makedirs(d, exist_ok=True)
    rng = np.random.default_rng(3)
    files = {}
    for name, L, reads in (("short", 150, short_reads), ("long", 15000, long_bases // 15000)):
        bam, fq = os.path.join(d, name + ".bam"), os.path.join(d, name + ".fastq.gz")
        files[name] = (bam, fq, reads * L)
        if os.path.exists(bam) and os.path.exists(fq):
            continue
        t0 = time.time()
        with open(bam + ".tmp", "wb") as fb, open(fq + ".tmp", "wb") as ff:
            fb.write(bgzf_fast(b"BAM\x01" + struct.pack("<ii", 0, 0))[:-28])
            slab = max(1, (256 << 20) // (L * 3))
            for a in range(0, reads, slab):
                rows = random_rows(rng, min(slab, reads - a), L)
                fb.write(bgzf_fast(records(rows, L, 0)[0].tobytes())[:-28])
                q = np.empty((rows.shape[0], 3 + L + 3 + L + 1), dtype=np.uint8)
                q[:, :3] = np.frombuffer(b"@r\n", dtype=np.uint8)
                q[:, 3:3 + L] = rows
                q[:, 3 + L:6 + L] = np.frombuffer(b"\n+\n", dtype=np.uint8)
                q[:, 6 + L:6 + 2 * L] = ord("I")
                q[:, 6 + 2 * L] = 10
                ff.write(bgzf_fast(q.tobytes())[:-28])
            fb.write(bgzf_fast(b""))
            ff.write(bgzf_fast(b""))
        os.replace(bam + ".tmp", bam)
        os.replace(fq + ".tmp", fq)
        print(json.dumps({"leg": "e2e", "wrote": name, "seconds": time.time() - t0, "bam_MB": os.path.getsize(bam) >> 20, "fastq_gz_MB": os.path.getsize(fq) >> 20}), flush=True)
    return files


def run_cli(meryl, src, out, env_extra):
    shutil.rmtree(out, ignore_errors=True)
    env = dict(os.environ, MGC_IO_TRACE="1", **env_extra)
    t0 = time.time()
    p = subprocess.run([meryl, "-V", "-V", "k=21", "memory=32", "threads=16", "count", src, "output", out], capture_output=True, text=True, env=env)
    wall = time.time() - t0
    m = re.search(r"TIMING\s+read\+parse\+stage=([0-9.]+) s\s+count=([0-9.]+) s", p.stderr)
    io = [l for l in p.stderr.splitlines() if l.startswith("[io] BAM file") or l.startswith("[io] BGZF file")]
    distinct = re.findall(r"([0-9]+) distinct", p.stderr)
    return {"rc": p.returncode, "wall_s": wall, "read_s": float(m.group(1)) if m else None, "count_s": float(m.group(2)) if m else None,
            "io": io[-1] if io else None, "distinct": distinct[-1] if distinct else None, "err": p.stderr[-300:] if p.returncode else None}


def e2e(args):
    from meryl_amd import build
    mine = build.build_cli()
    files = write_inputs(args.dir, args.short_reads, args.long_bases)
    out = os.path.join(args.dir, "out.meryl")
    ok = True
    for name, (bam, fq, bases) in files.items():
        routes = [("default", mine, bam, {}), ("host_parser", mine, bam, {"MERYL_HOST_PARSER": "1"}), ("fastq_bgzf", mine, fq, {})]
        if args.other_meryl:
            routes.insert(0, ("other", args.other_meryl, bam, {}))
        reads = {r[0]: [] for r in routes}
        for run in range(args.runs):
            for route, meryl, src, env in routes:
                r = run_cli(meryl, src, out, env)
                r.update(leg="e2e", file=name, route=route, run=run)
                print(json.dumps(r), flush=True)
                if r["read_s"] is not None:
                    reads[route].append(r["read_s"])
        s = {"leg": "e2e_summary", "file": name, "bases": bases, "read_s": {k: sorted(v) for k, v in reads.items()}}
        med = {k: float(np.median(v)) for k, v in reads.items() if v}
        s["Gbase_per_s"] = {k: bases / v / 1e9 for k, v in med.items()}
        if "other" in med and "default" in med:
            s["default_over_other"] = med["default"] / med["other"]
            s["not_slower_than_other"] = min(reads["default"]) <= max(reads["other"])          # within the spread of the runs
            ok = ok and s["not_slower_than_other"]
        if "fastq_bgzf" in med and "default" in med:
            s["bam_rate_over_fastq_rate"] = med["fastq_bgzf"] / med["default"]
        print(json.dumps(s), flush=True)
    shutil.rmtree(out, ignore_errors=True)
    return ok


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("leg", choices=["kernel", "e2e"])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--dir", default="/tmp/bam_bench")
    ap.add_argument("--other-meryl", default=None)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--short-reads", type=int, default=4_000_000)
    ap.add_argument("--long-bases", type=int, default=1_000_000_000)
    args = ap.parse_args()
    if args.leg == "kernel":
        from meryl_amd import build
        build.build()
        ok = kernel_leg("150 bp records", 150, 150, 0, args.iters)
        ok = kernel_leg("15 kb records, qualities, 2 KB aux", 15000, 15000, 2048, args.iters) and ok
    else:
        ok = e2e(args)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
