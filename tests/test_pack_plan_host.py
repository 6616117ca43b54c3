"""Whether the files of a count may be packed while later files are still being counted, and how many k-mers the packed result
gets room for before the first packing launch is queued (meryl_amd/csrc/mgc_pack_plan.hpp), pinned on a machine without a GPU: a
stand-alone host program built with the address and undefined-behaviour sanitizers walks
  - the eligibility over every vector of up to three files of nine kinds (empty, plain, a sub-bucket exactly at and one above the
    count kernels' capacity, an oversized list that is streamed -- up to and exactly at MGC_STREAM_MAX --, one above it, which the
    host asks a probe launch about, one that nothing streams, a file already finished by the stable sort) with the switch on and
    off, no file at all, and 64 files of which ten have a streamed list and then one a list nothing streams;
  - the estimate over instances x probe ratios (none, tiny, the benchmarked 0.1369, the plan's threshold 0.30, 1 and above) x
    margins (below -1000, negative, 0, the default, huge): never above the instances, nothing without a probe, never short of
    ratio x instances with a margin of zero or more, short by construction with a negative one, monotone in the margin;
  - what the arena is asked to grow to and the capacity the gate is given: caller buffers (their size, never grown), no probe
    (what is there), zero existing capacity (the serial path), an arena that refuses to grow (what it holds then, which may be
    nothing), key and count buffers of different sizes;
  - the chain for every first deferred file q of every m up to 66 files: the early files are a prefix one step behind the scans,
    the launch thresholds say the same as the host's rule, the serial loop starts at the first file that did not run."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ELIGIBILITY = 9 * 10 * 10 * 2 + 3                         # pack_plan_host.cpp: the vectors x the switch, and the three named cases
CAPACITY = 9 * 9 * 9 + 6 * 6 * 6 * 2 * 3                 # instances x ratios x margins; estimate x arena x caller size x caller x outcome of the growth
CHAIN = sum(m + 1 for m in range(1, 67))


def test_pack_plan_over_files_estimates_and_chains(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "pack_plan_host")
    c = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        os.path.join(ROOT, "tests", "host", "pack_plan_host.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert c.returncode == 0, c.stderr
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    tag, elig, cap, chain = p.stdout.split()
    assert tag == "ok"
    assert (int(elig), int(cap), int(chain)) == (ELIGIBILITY, CAPACITY, CHAIN)
