"""The read half of the one database-file loader (meryl_amd/csrc/mgc_dbfile.cpp), on a machine without a GPU: a stand-alone host
program built with the address and undefined-behaviour sanitizers (tests/host/dbfile_host.cpp, no HIP) writes small databases of
three shapes -- k = 4 with empty files and blocks of a handful, k = 16, and k = 40 with two key words and labels -- makes chosen data
files of a copy readable by the host decoder only, and checks every file's record against mdb_reader_read_file_ex: raw where the
framing is canonical, host-decoded where it is not or where host decoding is asked for, labels only when asked for and stored, and a
truncated file reported as that file's error with nothing leaked."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "meryl_amd", "csrc")


def test_read_half_of_the_loader_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "dbfile_host")
    c = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-DMGC_DBFILE_HOST_ONLY", os.path.join(ROOT, "tests", "host", "dbfile_host.cpp"),
                        os.path.join(CSRC, "mgc_dbfile.cpp"), os.path.join(CSRC, "meryl_db.cpp"), "-pthread", "-o", exe],
                       capture_output=True, text=True, timeout=600)
    assert c.returncode == 0, c.stderr[-4000:]
    work = tmp_path / "work"
    work.mkdir()
    env = {k: v for k, v in os.environ.items() if k != "MGC_DECODE_HOST"}
    p = subprocess.run([exe, str(work)], capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0, (p.stdout + p.stderr)[-4000:]
    tag, checks = p.stdout.split()
    assert tag == "ok" and int(checks) > 10000
