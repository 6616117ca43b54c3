"""The geometry hash_count_stream_kernel takes once per sub-bucket (meryl_amd/csrc/mgc_stream_geom.hpp: chunk size, table slots, the
per-wave queue of pending keys), on a machine without a GPU: a stand-alone host program built with the address and
undefined-behaviour sanitizers walks every sub-bucket size 1 .. 4094 at both table sizes with the kernel's own chunk loop -- one to
three chunks of whole 256-key rows, none above 1536 keys, every key exactly once; a power-of-two table of at least 2n slots wherever
the table allows, the retry table never more than half full -- and every fill of a wave's queue against every row size."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 4094                                                # FIN_CAP_STREAM
MAX_SIZES = (4094, 2304, 1536, 300)                       # stream_geom_host.cpp: the capacities walked
QCAP = 128                                                # STREAM_QCAP


def test_stream_geometry_of_every_subbucket_size(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "stream_geom_host")
    c = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        os.path.join(ROOT, "tests", "host", "stream_geom_host.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert c.returncode == 0, c.stderr
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    tag, sizes, states = p.stdout.split()
    assert tag == "ok"
    assert int(sizes) == 2 * sum(min(m, CAP) for m in MAX_SIZES)
    assert int(states) == 4 * (QCAP + 1) * 65
