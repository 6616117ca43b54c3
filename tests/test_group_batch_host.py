"""Which narrowed files share the launches of their grouping passes, and where each file's words lie in the pass buffer meanwhile
(meryl_amd/csrc/mgc_group_batch.hpp), pinned on a machine without a GPU: a stand-alone host program built with the address and
undefined-behaviour sanitizers runs the planner over a grid of file-size vectors (empty files, files of one key, files of one key
below, at and above the tile sizes of both passes, ineligible files, three launch keys interleaved), budgets (none, below one slice,
exactly one and two tiles' words, 8 GiB, everything) and file caps, and asserts for every plan: every eligible file in exactly one
batch and no other file in any; slices of the buffer disjoint, aligned and inside the budget; tile prefixes strictly increasing;
a budget below two files' words, or a cap of one, gives one file per batch; no batch mixes instantiations."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VECTORS = 1 + 17 + 3                                      # group_batch_host.cpp: none, each edge size alone, the three mixed vectors
BUDGETS, CAPS = 12, 5


def test_batch_plans_over_sizes_budgets_and_caps(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "group_batch_host")
    c = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        os.path.join(ROOT, "tests", "host", "group_batch_host.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert c.returncode == 0, c.stderr
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    tag, plans, batches = p.stdout.split()
    assert tag == "ok"
    assert int(plans) == VECTORS * BUDGETS * CAPS
    assert int(batches) > int(plans)                       # (most plans hold several batches)
