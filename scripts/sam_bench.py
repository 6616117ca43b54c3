#!/usr/bin/env python
"""SAM input parsed on the device: what the parse kernels cost against the upload they hide behind, and file -> database runs of
the CLI over the new route, the host reader and another build's binary.

    python scripts/sam_bench.py kernel [--iters 10]
        mgc_dev_text_parse (MGC_TEXT_SAM) on a 32 MiB piece of short-read SAM (150 bases, 11 columns and a few aux tags) and on one
        of long-read SAM (records of 15 .. 25 kb), against a device-to-device copy of the piece and against the piece's upload
        from pinned memory.  Timed with events in this process, a window of eight launches over eight sets of buffers (more than
        the last-level cache holds) at a time.  One JSON line per piece; "hides_behind_upload" is parse_ms < upload_ms.

    python scripts/sam_bench.py e2e [--dir /tmp/sam_bench] [--other-meryl PATH] [--runs 3] [--short-reads 3000000] [--long-bases 600000000]
        writes a short-read .sam, a long-read .sam and the short reads as a BGZF .sam.gz, then counts each with the CLI
        (threads=16, k=21), the variants taken in turn, --runs times: this build's default route, this build with
        MERYL_HOST_PARSER=1, and --other-meryl's default route (the parent commit's binary: the yardstick).  One JSON line per run
        with the read phase of the -V TIMING line and the [io] line of MGC_IO_TRACE, and a summary line per file with medians and
        the spread.

Every line is also appended to --out (default profiles/sam_bench.jsonl)."""
import argparse
import ctypes
import json
import os
import re
import shutil
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from bam_bench import bgzf_fast, random_rows  # noqa: E402

OUT = None


def say(obj):
    line = json.dumps(obj)
    print(line, flush=True)
    if OUT:
        with open(OUT, "a") as f:
            f.write(line + "\n")


def sam_rows(rows, aux):
    """rows: uint8[reads, L] of ACGT letters -> uint8[reads, line bytes]: alignment lines of one shape, QUAL of 'I', `aux` behind"""
    reads, L = rows.shape
    head = b"read/000000\t0\tchr1\t1000000\t60\t%dM\t*\t0\t0\t" % L
    line = np.empty((reads, len(head) + L + 1 + L + len(aux) + 1), dtype=np.uint8)
    line[:, :len(head)] = np.frombuffer(head, dtype=np.uint8)
    digits = np.frombuffer(b"0123456789", dtype=np.uint8)
    n = np.arange(reads)
    for d in range(6):
        line[:, 10 - d] = digits[(n // 10 ** d) % 10]
    at = len(head)
    line[:, at:at + L] = rows
    line[:, at + L] = 9
    line[:, at + L + 1:at + 2 * L + 1] = ord("I")
    line[:, at + 2 * L + 1:-1] = np.frombuffer(aux, dtype=np.uint8)
    line[:, -1] = 10
    return line


SHORT_AUX = b"\tNM:i:1\tMD:Z:75A74\tAS:i:145\tXS:i:20\tRG:Z:lane1"
LONG_AUX = b"\trq:f:0.999\tnp:i:12\tRG:Z:cell1"
HEADER = b"@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:chr1\tLN:248956422\n@RG\tID:lane1\n"


def long_lines(rng, total_bytes):
    """lines of 15, 17.5, 20, 22.5 and 25 kb reads in turn, up to total_bytes"""
    out, at, i = [], 0, 0
    while True:
        L = 15000 + 2500 * (i % 5)
        if at + 2 * L + 120 > total_bytes:
            return b"".join(out)
        out.append(sam_rows(random_rows(rng, 1, L), LONG_AUX).tobytes())
        at += len(out[-1])
        i += 1


# ---- the kernel ---------------------------------------------------------------------------------------------------------
def kernel_leg(name, piece, iters):
    import torch
    from meryl_amd import capi
    L_ = capi.lib()
    piece = np.frombuffer(piece, dtype=np.uint8)
    n = int(piece.size)
    h_piece = torch.from_numpy(piece.copy()).pin_memory()
    ws_bytes = int(L_.mgc_dev_text_parse_workspace_bytes(n))
    SETS = 8                                                  # 8 x (32 + 32 + 32 MiB): several times the last-level cache
    d_piece = [torch.from_numpy(piece.copy()).cuda() for _ in range(SETS)]
    d_out = [torch.empty(n + 64, dtype=torch.uint8, device="cuda") for _ in range(SETS)]
    d_ws = [torch.empty(ws_bytes, dtype=torch.uint8, device="cuda") for _ in range(SETS)]
    d_dst = [torch.empty(n, dtype=torch.uint8, device="cuda") for _ in range(SETS)]
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def upload(i):
        d_piece[i].copy_(h_piece, non_blocking=True)

    def parse(i):
        capi.check(L_.mgc_dev_text_parse(ctypes.c_void_p(d_piece[i].data_ptr()), n, capi.TEXT_SAM, ctypes.c_void_p(d_ws[i].data_ptr()),
                                         ctypes.c_void_p(d_out[i].data_ptr()), st), "mgc_dev_text_parse")

    def copy(i):
        d_dst[i].copy_(d_piece[i], non_blocking=True)

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

    up, par, cp = timed(upload), timed(parse), timed(copy)
    # the result, once, against numpy: column 9 of every line and a '.'
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import sam_model
    want = sam_model.model(piece.tobytes())[0][:-1]
    state = d_ws[SETS - 1][:32].cpu().numpy()
    out_len, err = int(state[:8].view(np.uint64)[0]), int(state[24:28].view(np.uint32)[0])
    ok = out_len == len(want) and err == 0 and d_out[SETS - 1][:out_len].cpu().numpy().tobytes() == want
    say({"leg": "kernel", "piece": name, "piece_bytes": n, "out_bytes": out_len, "buffer_sets": SETS, "parse_ms": par[0], "parse_ms_min_max": par[1:],
         "copy_ms": cp[0], "copy_ms_min_max": cp[1:], "parse_over_copy": par[0] / cp[0], "upload_ms": up[0], "upload_ms_min_max": up[1:],
         "upload_GBps": n / up[0] / 1e6, "parse_GBps_in": n / par[0] / 1e6, "hides_behind_upload": par[0] < up[0], "correct": ok})
    return ok


# ---- end to end ---------------------------------------------------------------------------------------------------------
def write_inputs(d, short_reads, long_bases):
    os.makedirs(d, exist_ok=True)
    rng = np.random.default_rng(3)
    short, long_, bgz = os.path.join(d, "short.sam"), os.path.join(d, "long.sam"), os.path.join(d, "short.sam.gz")
    files = {"short.sam": (short, short_reads * 150), "long.sam": (long_, 0), "short.sam.gz": (bgz, short_reads * 150)}
    t0 = time.time()
    if not (os.path.exists(short) and os.path.exists(bgz)):
        with open(short + ".tmp", "wb") as f, open(bgz + ".tmp", "wb") as g:
            f.write(HEADER)
            g.write(bgzf_fast(HEADER)[:-28])
            for a in range(0, short_reads, 250_000):
                text = sam_rows(random_rows(rng, min(250_000, short_reads - a), 150), SHORT_AUX).tobytes()
                f.write(text)
                g.write(bgzf_fast(text)[:-28])
            g.write(bgzf_fast(b""))
        os.replace(short + ".tmp", short)
        os.replace(bgz + ".tmp", bgz)
    if not os.path.exists(long_):
        with open(long_ + ".tmp", "wb") as f:
            f.write(HEADER)
            left = 2 * long_bases
            while left > 100_000:
                text = long_lines(rng, min(left, 64 << 20))
                f.write(text)
                left -= len(text)
        os.replace(long_ + ".tmp", long_)
    files["long.sam"] = (long_, os.path.getsize(long_) // 2)
    say({"leg": "e2e", "wrote": sorted(files), "seconds": time.time() - t0, "MB": {k: os.path.getsize(v[0]) >> 20 for k, v in files.items()}})
    return files


def run_cli(meryl, src, out, env_extra):
    shutil.rmtree(out, ignore_errors=True)
    env = dict(os.environ, MGC_IO_TRACE="1", **env_extra)
    t0 = time.time()
    p = subprocess.run([meryl, "-V", "-V", "k=21", "memory=32", "threads=16", "count", src, "output", out], capture_output=True, text=True, env=env)
    wall = time.time() - t0
    m = re.search(r"TIMING\s+read\+parse\+stage=([0-9.]+) s\s+count=([0-9.]+) s", p.stderr)
    io = [l for l in p.stderr.splitlines() if l.startswith("[io] ") and "SAM file" in l]    # the reader's line, not the database writer's
    distinct = re.findall(r"([0-9]+) distinct", p.stderr)
    return {"rc": p.returncode, "wall_s": wall, "read_s": float(m.group(1)) if m else None, "count_s": float(m.group(2)) if m else None,
            "io": io[-1][:400] if io else None, "distinct": distinct[-1] if distinct else None, "err": p.stderr[-300:] if p.returncode else None}


def e2e(args):
    from meryl_amd import build
    mine = build.build_cli()
    files = write_inputs(args.dir, args.short_reads, args.long_bases)
    out = os.path.join(args.dir, "out.meryl")
    ok = True
    for name, (src, bases) in files.items():
        variants = [("device", mine, {}), ("host_parser", mine, {"MERYL_HOST_PARSER": "1"})]
        if args.other_meryl:
            variants.append(("other", args.other_meryl, {}))
        reads, walls, distinct = {v[0]: [] for v in variants}, {v[0]: [] for v in variants}, set()
        for run in range(args.runs):
            for variant, meryl, env in variants:
                r = run_cli(meryl, src, out, env)
                r.update(leg="e2e", file=name, variant=variant, run=run)
                say(r)
                ok = ok and r["rc"] == 0
                distinct.add(r["distinct"])
                if r["read_s"] is not None:
                    reads[variant].append(r["read_s"])
                    walls[variant].append(r["wall_s"])
        s = {"leg": "e2e_summary", "file": name, "bases": bases, "read_s": {k: sorted(v) for k, v in reads.items()}, "wall_s": {k: sorted(v) for k, v in walls.items()},
             "same_distinct_everywhere": len(distinct) == 1}
        med = {k: float(np.median(v)) for k, v in reads.items() if v}
        s["read_s_median"] = med
        s["Gbase_per_s"] = {k: bases / v / 1e9 for k, v in med.items() if v}
        for base in ("other", "host_parser"):
            if base in med and "device" in med and med["device"]:
                s["%s_over_device" % base] = med[base] / med["device"]
                s["device_faster_than_%s_beyond_spread" % base] = max(reads["device"]) < min(reads[base])
        say(s)
    shutil.rmtree(out, ignore_errors=True)
    return ok


def main():
    global OUT
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("leg", choices=["kernel", "e2e"])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--dir", default="/tmp/sam_bench")
    ap.add_argument("--other-meryl", default=None)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--short-reads", type=int, default=3_000_000)
    ap.add_argument("--long-bases", type=int, default=600_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sam_bench.jsonl"))
    args = ap.parse_args()
    OUT = args.out
    if args.leg == "kernel":
        from meryl_amd import build
        build.build()
        rng = np.random.default_rng(7)
        reads = ((32 << 20) - len(HEADER)) // sam_rows(np.full((1, 150), 65, dtype=np.uint8), SHORT_AUX).shape[1]
        ok = kernel_leg("short reads: 150 bases, 11 columns, 5 aux tags", HEADER + sam_rows(random_rows(rng, reads, 150), SHORT_AUX).tobytes(), args.iters)
        ok = kernel_leg("long reads: 15 .. 25 kb", HEADER + long_lines(rng, (32 << 20) - len(HEADER)), args.iters) and ok
    else:
        ok = e2e(args)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
