#!/usr/bin/env python
"""Plain gzip input inflated in parallel and resolved on the device: what the three kernels cost against the upload they hide
behind, and file -> database runs of the CLI over the new route, the one-thread reader and (optionally) another build's binary.

    python scripts/gzip_bench.py kernel [--iters 10]
        mgc_dev_gzip_resolve (resolve + window) and mgc_dev_crc32_pieces on a 32 MiB piece of FASTQ-shaped text -- once with an
        unresolved prefix of 64 KiB, once with the whole piece unresolved (a tenth of the symbols markers: what a FASTQ file
        gives, whose headers are copied on from record to record) -- against a device-to-device copy of the piece and against
        the upload of the piece, its symbols and its CRC table from pinned memory.  Timed with events in this process, a window
        of launches over several sets of buffers (more than the last-level cache holds) at a time.  One JSON line per case;
        "hides_behind_upload" is kernels_ms < upload_ms.

    python scripts/gzip_bench.py e2e [--dir /tmp/gzip_bench] [--other-meryl PATH] [--runs 3] [--reads 1000000]
        writes reads of 150 bases as single-member .fastq.gz at levels 1 and 6 and as BGZF, then counts each with the CLI
        (threads=16, k=21), the routes taken in turn, --runs times: this build's default route, this build with
        MERYL_GZIP_GENERIC=1, PATH's default route, the BGZF file.  One JSON line per run with the read phase of the -V TIMING
        line and the [io] line of MGC_IO_TRACE, and a summary line per level."""
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
WIN = 32768
PIECE = 32 << 20


def fastq_rows(rng, reads, L=150):
    """uint8[reads, record bytes]: '@r<8 digits>\\n' + L bases + '\\n+\\n' + L qualities + '\\n'"""
    genome = rng.integers(0, 4, 5_000_000 + L, dtype=np.uint8)
    starts = rng.integers(0, 5_000_000, reads)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    rec = np.empty((reads, 11 + L + 3 + L + 1), dtype=np.uint8)
    rec[:, :2] = np.frombuffer(b"@r", dtype=np.uint8)
    ids = rng.integers(0, 10, (reads, 8), dtype=np.uint8) + ord("0")
    rec[:, 2:10] = ids
    rec[:, 10] = 10
    slab = 100_000
    for a in range(0, reads, slab):
        s = starts[a:a + slab]
        rec[a:a + s.size, 11:11 + L] = letters[genome[s[:, None] + np.arange(L)[None, :]]]
    rec[:, 11 + L:14 + L] = np.frombuffer(b"\n+\n", dtype=np.uint8)
    rec[:, 14 + L:14 + 2 * L] = rng.choice(np.frombuffer(b"FFFFFFFF:,#", dtype=np.uint8), size=(reads, L))
    rec[:, 14 + 2 * L] = 10
    return rec


# ---- the kernels --------------------------------------------------------------------------------------------------------
def kernel_case(name, n_symbols, iters):
    import torch
    from meryl_amd import capi
    L_ = capi.lib()
    rng = np.random.default_rng(7)
    rec = fastq_rows(rng, PIECE // 315 + 1)
    text = rec.reshape(-1)[:PIECE].copy()
    window = rng.integers(33, 127, WIN, dtype=np.uint8)
    sym = text[:n_symbols].astype(np.uint16)
    marks = rng.random(n_symbols) < 0.1
    sym[marks] = 0x8000 + rng.integers(0, WIN, int(marks.sum()))
    want = text.copy()
    want[:n_symbols][marks] = window[sym[marks] - 0x8000]
    text[:n_symbols][marks] = 0
    begins = np.arange(0, PIECE, 4096, dtype=np.int64)
    lens = np.full(begins.size, 4096, dtype=np.int32)
    h_text, h_sym = torch.from_numpy(text).pin_memory(), torch.from_numpy(sym.view(np.int16)).pin_memory()
    h_begin, h_len = torch.from_numpy(begins).pin_memory(), torch.from_numpy(lens).pin_memory()
    SETS = 8                                                   # 32 MiB of text + up to 64 MiB of symbols each: beyond the last-level cache
    d_text = [torch.from_numpy(text).cuda() for _ in range(SETS)]
    d_sym = [torch.from_numpy(sym.view(np.int16)).cuda() for _ in range(SETS)]
    d_begin, d_len = [h_begin.cuda() for _ in range(SETS)], [h_len.cuda() for _ in range(SETS)]
    d_crc = [torch.zeros(begins.size, dtype=torch.int32, device="cuda") for _ in range(SETS)]
    d_win = [torch.from_numpy(window).cuda() for _ in range(SETS)]
    d_wout = [torch.zeros(WIN, dtype=torch.uint8, device="cuda") for _ in range(SETS)]
    d_copy = [torch.empty(PIECE, dtype=torch.uint8, device="cuda") for _ in range(SETS)]
    d_err = torch.zeros(1, dtype=torch.int32, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    vp = ctypes.c_void_p

    def upload(i):
        d_text[i].copy_(h_text, non_blocking=True)
        d_sym[i].copy_(h_sym, non_blocking=True)
        d_begin[i].copy_(h_begin, non_blocking=True)
        d_len[i].copy_(h_len, non_blocking=True)

    def resolve(i):
        capi.check(L_.mgc_dev_gzip_resolve(vp(d_text[i].data_ptr()), PIECE, vp(d_sym[i].data_ptr()), n_symbols, vp(d_win[i].data_ptr()), WIN,
                                           vp(d_wout[i].data_ptr()), vp(d_err.data_ptr()), st), "mgc_dev_gzip_resolve")

    def crc(i):
        capi.check(L_.mgc_dev_crc32_pieces(vp(d_text[i].data_ptr()), vp(d_begin[i].data_ptr()), vp(d_len[i].data_ptr()), begins.size,
                                           vp(d_crc[i].data_ptr()), st), "mgc_dev_crc32_pieces")

    def kernels(i):
        resolve(i)
        crc(i)

    def copy(i):
        d_copy[i].copy_(d_text[i], non_blocking=True)

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

    up = timed(upload)                                         # (leaves the unresolved text in every set)
    res, c, both, cp = timed(resolve), timed(crc), timed(kernels), timed(copy)
    ok = bool(np.array_equal(d_text[SETS - 1].cpu().numpy(), want)) and int(d_err.item()) == 0
    z = zlib.crc32(want[:4096].tobytes()) & 0xffffffff
    ok = ok and int(d_crc[SETS - 1].cpu().numpy().view(np.uint32)[0]) == z
    ok = ok and bool(np.array_equal(d_wout[0].cpu().numpy(), want[-WIN:]))
    up_bytes = PIECE + 2 * n_symbols + 12 * begins.size
    print(json.dumps({"leg": "kernel", "case": name, "piece_bytes": PIECE, "n_symbols": int(n_symbols), "buffer_sets": SETS,
                      "resolve_window_ms": res[0], "resolve_window_ms_min_max": res[1:], "crc_ms": c[0], "crc_ms_min_max": c[1:],
                      "kernels_ms": both[0], "kernels_ms_min_max": both[1:], "copy_ms": cp[0], "copy_ms_min_max": cp[1:],
                      "upload_ms": up[0], "upload_ms_min_max": up[1:], "upload_bytes": int(up_bytes), "upload_GBps": up_bytes / up[0] / 1e6,
                      "kernels_over_copy": both[0] / cp[0], "hides_behind_upload": both[0] < up[0], "correct": ok}), flush=True)
    return ok and both[0] < up[0]


# ---- end to end ---------------------------------------------------------------------------------------------------------
def bgzf_fast(data, block=0xff00):
    out = []
    for i in range(0, len(data), block):
        d = data[i:i + block]
        c = zlib.compressobj(1, zlib.DEFLATED, -15)
        cd = c.compress(d) + c.flush()
        bs = 12 + 6 + len(cd) + 8
        out.append(struct.pack("<BBBBIBBH", 0x1f, 0x8b, 8, 4, 0, 0, 0xff, 6) + b"BC" + struct.pack("<HH", 2, bs - 1) + cd +
                   struct.pack("<II", zlib.crc32(d) & 0xffffffff, len(d)))
    return b"".join(out)


def write_inputs(d, reads):
    os.makedirs(d, exist_ok=True)
    names = {"level1": os.path.join(d, "reads.l1.fastq.gz"), "level6": os.path.join(d, "reads.l6.fastq.gz"), "bgzf": os.path.join(d, "reads.bgzf.fastq.gz")}
    if all(os.path.exists(p) for p in names.values()):
        return names
    t0 = time.time()
    rng = np.random.default_rng(3)
    z1, z6 = zlib.compressobj(1, zlib.DEFLATED, 31), zlib.compressobj(6, zlib.DEFLATED, 31)
    with open(names["level1"], "wb") as f1, open(names["level6"], "wb") as f6, open(names["bgzf"], "wb") as fb:
        for a in range(0, reads, 200_000):
            text = fastq_rows(rng, min(200_000, reads - a)).tobytes()
            f1.write(z1.compress(text))
            f6.write(z6.compress(text))
            fb.write(bgzf_fast(text))
        f1.write(z1.flush())
        f6.write(z6.flush())
        fb.write(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"))
    print(json.dumps({"leg": "e2e", "wrote": {k: os.path.getsize(p) >> 20 for k, p in names.items()}, "text_MB": reads * 315 >> 20, "seconds": time.time() - t0}), flush=True)
    return names


def run_cli(meryl, src, out, env_extra):
    shutil.rmtree(out, ignore_errors=True)
    env = dict(os.environ, MGC_IO_TRACE="1", **env_extra)
    t0 = time.time()
    p = subprocess.run([meryl, "-V", "-V", "k=21", "memory=32", "threads=16", "count", src, "output", out], capture_output=True, text=True, env=env, timeout=600)
    wall = time.time() - t0
    m = re.search(r"TIMING\s+read\+parse\+stage=([0-9.]+) s\s+count=([0-9.]+) s", p.stderr)
    io = [l for l in p.stderr.splitlines() if l.startswith("[io] gzip file") or l.startswith("[io] BGZF file")]
    distinct = re.findall(r"([0-9]+) distinct", p.stderr)
    return {"rc": p.returncode, "wall_s": wall, "read_s": float(m.group(1)) if m else None, "count_s": float(m.group(2)) if m else None,
            "io": io[-1] if io else None, "distinct": distinct[-1] if distinct else None, "err": p.stderr[-300:] if p.returncode else None}


def e2e(args):
    from meryl_amd import build
    mine = build.build_cli()
    names = write_inputs(args.dir, args.reads)
    out = os.path.join(args.dir, "out.meryl")
    text_bytes = args.reads * 315
    ok = True
    for level in ("level1", "level6"):
        routes = [("default", mine, names[level], {}), ("generic", mine, names[level], {"MERYL_GZIP_GENERIC": "1"}), ("bgzf", mine, names["bgzf"], {})]
        if args.other_meryl:
            routes.insert(0, ("other", args.other_meryl, names[level], {}))
        reads = {r[0]: [] for r in routes}
        distinct = set()
        for run in range(args.runs):
            for route, meryl, src, env in routes:
                r = run_cli(meryl, src, out, env)
                r.update(leg="e2e", file=level, route=route, run=run)
                print(json.dumps(r), flush=True)
                distinct.add(r["distinct"])
                if r["read_s"] is not None:
                    reads[route].append(r["read_s"])
        s = {"leg": "e2e_summary", "file": level, "text_bytes": text_bytes, "read_s": {k: sorted(v) for k, v in reads.items()}, "same_result": len(distinct) == 1}
        med = {k: float(np.median(v)) for k, v in reads.items() if v}
        s["text_GBps"] = {k: text_bytes / v / 1e9 for k, v in med.items()}
        for other in ("other", "generic", "bgzf"):
            if other in med and "default" in med:
                s["default_over_" + other] = med["default"] / med[other]
        if "other" in med and "default" in med:
            s["faster_than_other"] = max(reads["default"]) < min(reads["other"])
            ok = ok and s["faster_than_other"]
        ok = ok and s["same_result"]
        print(json.dumps(s), flush=True)
    shutil.rmtree(out, ignore_errors=True)
    return ok


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("leg", choices=["kernel", "e2e"])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--dir", default="/tmp/gzip_bench")
    ap.add_argument("--other-meryl", default=None)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reads", type=int, default=1_000_000)
    args = ap.parse_args()
    if args.leg == "kernel":
        ok = kernel_case("prefix of 64 KiB", 65536, args.iters)
        ok = kernel_case("the whole piece unresolved", PIECE, args.iters) and ok
    else:
        ok = e2e(args)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
