#!/usr/bin/env python3
"""Register / scratch / LDS use of the kernels whose mangled name contains PATTERN (developer tool).
Usage: python scripts/kres.py PATTERN [FILE.hip ...]   (only the named sources of meryl_amd/csrc when given)"""
import re, subprocess, sys, os
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
out = ""
names = ("mgc_kmer.hip", "mgc_sort.hip", "mgc_scan.hip", "mgc_finish.hip", "mgc_misc.hip", "mgc_parse.hip", "mgc_merge.hip", "mgc_merge_many.hip", "mgc_decode.hip", "mgc_encode.hip", "mgc_value_hist.hip",
         "mgc_lookup.hip", "mgc_filter.hip", "mgc_import.hip", "mgc_analyze.hip", "mgc_positions.hip", "mgc_list.hip", "mgc_gzip.hip")
for name in (sys.argv[2:] or names):
    src = os.path.join(root, "meryl_amd", "csrc", name)
    out += subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", "-Rpass-analysis=kernel-resource-usage",
                           "-o", "/tmp/kres.o", src], capture_output=True, text=True).stderr
cur = None
for line in out.splitlines():
    if "error:" in line:
        print(line)
    m = re.search(r"Function Name: (\S+)", line)
    if m:
        cur = m.group(1)
        continue
    if cur and sys.argv[1] in cur:
        m = re.search(r"remark:\s+(TotalSGPRs|SGPRs|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m:
            print(cur[:70], m.group(1), m.group(2))
