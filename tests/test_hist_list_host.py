"""The host merge of the histograms' one list tier (meryl_amd/csrc/mgc_hist_list.hpp), on a machine without a GPU: a stand-alone host
program built with the address and undefined-behaviour sanitizers (tests/host/hist_list_host.cpp, no HIP) merges a few thousand
generated passes -- empty on either side or both, disjoint, interleaved and identical key sets, the keys 0, 2^32 - 1 and a 40-bit key
as meryl-analyze packs it, counts whose sum passes 2^32, many passes into one vector -- and checks the vector against a std::map after
every merge: strictly ascending, every count summed."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_list_tier_merge_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "hist_list_host")
    c = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-DMGC_HIST_LIST_HOST_ONLY", os.path.join(ROOT, "tests", "host", "hist_list_host.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=600)
    assert c.returncode == 0, c.stderr[-4000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout + p.stderr)[-4000:]
    tag, cases, checks = p.stdout.split()
    assert tag == "ok" and int(cases) > 2000 and int(checks) > 10000
