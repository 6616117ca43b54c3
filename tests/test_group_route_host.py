"""Which instantiation of radix_group_kernel a grouping pass runs (meryl_amd/csrc/mgc_group_route.hpp), pinned on a machine without
a GPU: a stand-alone host program built with the address and undefined-behaviour sanitizers runs the picking functions over the
full grids of a narrowed file (high digit first x 5-byte layout x fetch a tile ahead x instrumented x digit widths), of a whole-key
file (key kind x plan) and of the grouping mode of the stable sort's launcher, and the answers are compared with the rules written
out here.  An instantiation is (key, RB, KPT, DBG, NARROW, HIST2, SOA, PIPE, HPCD); BLOCK is 1024 everywhere."""
import itertools
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64, U32, K128, K96 = 0, 1, 2, 3
NAMES = {U64: "u64", U32: "u32", K128: "K128", K96: "K96"}
KPT_WIDE = {U64: 16, K128: 8, K96: 12}
KEY_BYTES = {U64: 8, U32: 4, K128: 16, K96: 12}
LDS_MAX = 160 * 1024

# the 29 instantiations the library holds
NARROW_FIRST = {
    (U64, 9, 16, 0, 1, 0, 0, 0, 0),       # low digit first
    (U64, 9, 16, 0, 1, 1, 0, 0, 0),       # high digit first, whole keys
    (U64, 9, 16, 0, 1, 1, 1, 0, 0),       # 5-byte layout, the fetch inside the look-back
    (U64, 9, 24, 0, 1, 1, 1, 2, 0),       # 5-byte layout, the fetch a tile ahead
    (U64, 8, 24, 0, 1, 1, 1, 2, 0),       # ... a first digit of at most eight bits
    (U64, 9, 16, 1, 1, 1, 0, 0, 0),       # instrumented
    (U64, 9, 16, 1, 1, 1, 1, 0, 0),
    (U64, 9, 24, 1, 1, 1, 1, 2, 0),
}
NARROW_SECOND = {(U32, 9, 24, 0, 0, 0, 0, 0, 0), (U32, 8, 24, 0, 0, 0, 0, 0, 0), (U32, 9, 24, 1, 0, 0, 0, 0, 0)}
WIDE = ({(K, rb, KPT_WIDE[K], 0, 0, h2, 0, 0, 0) for K in (U64, K128, K96) for rb in (8, 9) for h2 in (0, 1)} |
        {(K, 9, KPT_WIDE[K], 0, 0, h2, 0, 0, hpcd) for K in (U64, K128) for h2, hpcd in ((1, 1), (0, 1), (1, 2))})
ALL = NARROW_FIRST | NARROW_SECOND | WIDE


def lds_bytes(inst):
    """the tile (a narrowing pass: 32-bit words + one or two bytes of digit) + five counter arrays + 288 bytes + the rank table"""
    key, rb, kpt, _, narrow, _, _, _, hpcd = inst
    per_key = (5 if rb <= 8 else 6) if narrow else KEY_BYTES[key]
    return 1024 * kpt * per_key + 20 * (1 << rb) + 288 + (8192 if hpcd else 0)


def want_narrow(msd, soa, pipe, dbg, b_first, b_second):
    """(first, second, keys per tile of each, granules per tile of the second)"""
    dbg = dbg and msd                                           # instrumented: only high digit first
    if not msd:
        first = (U64, 9, 16, 0, 1, 0, 0, 0, 0)
    elif soa and pipe:                                          # 24576-key tiles; eight-bit digits: RB 8, but not instrumented
        first = (U64, 9, 24, 1, 1, 1, 1, 2, 0) if dbg else (U64, 8 if b_first <= 8 else 9, 24, 0, 1, 1, 1, 2, 0)
    elif soa:
        first = (U64, 9, 16, dbg, 1, 1, 1, 0, 0)
    else:
        first = (U64, 9, 16, dbg, 1, 1, 0, 0, 0)
    if dbg:
        second, granules = (U32, 9, 24, 1, 0, 0, 0, 0, 0), 256
    elif b_second <= 8:
        second, granules = (U32, 8, 24, 0, 0, 0, 0, 0, 0), 128
    else:
        second, granules = (U32, 9, 24, 0, 0, 0, 0, 0, 0), 256
    return first, second, 24576 if (msd and soa and pipe) else 16384, 24576, granules


def want_wide(key, hpc, b_lo, b_hi):
    kpt = KPT_WIDE[key]
    tab = key != K96                                            # 8 KiB for the rank table behind the tile: not beside 144 KiB
    if hpc == 1 and tab:
        first, second, granules = (key, 9, kpt, 0, 0, 1, 0, 0, 1), (key, 9, kpt, 0, 0, 0, 0, 0, 1), 256
    elif hpc == 2 and tab and b_lo <= 8:
        first, second, granules = (key, 9, kpt, 0, 0, 1, 0, 0, 2), (key, 8, kpt, 0, 0, 0, 0, 0, 0), 128
    else:
        rb = 8 if (not hpc and b_lo <= 8 and b_hi <= 8) else 9
        first, second, granules = (key, rb, kpt, 0, 0, 1, 0, 0, 0), (key, rb, kpt, 0, 0, 0, 0, 0, 0), (1 << rb) // 2
    return first, second, 1024 * kpt, 1024 * kpt, granules


def show(inst):
    return "%s %d %d %d %d %d %d %d %d %d" % ((NAMES[inst[0]],) + tuple(int(x) for x in inst[1:]) + (lds_bytes(inst),))


def test_group_instantiation_rules_on_the_host(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "group_route_host")
    c = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        os.path.join(ROOT, "tests", "host", "group_route_host.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert c.returncode == 0, c.stderr
    # what validation refuses is left out: the 5-byte layout without the high-digit-first form (asked once below)
    narrow = [c for c in itertools.product((0, 1), (0, 1), (0, 1), (0, 1), (7, 8, 9), (7, 8, 9)) if not (c[1] and not c[0])]
    plans = [(0, lo, hi) for lo in (8, 9) for hi in (8, 9)] + [(1, 10, 10), (2, 8, 10)]
    wide = [(key,) + p for key in (U64, K128, K96) for p in plans]
    assert len(narrow) == 3 * 4 * 9 and len(wide) == 3 * 6
    lines = (["N %d %d %d %d %d %d" % c for c in narrow] + ["W %d %d %d %d 0 0" % c for c in wide] +
             ["S %d 0 0 0 0 0" % key for key in (U64, K128)] + ["N 0 1 1 0 9 9"])
    p = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    got = p.stdout.split("\n")[:-1]
    assert len(got) == len(lines)
    reached = set()
    wants = [want_narrow(*c) for c in narrow] + [want_wide(*c) for c in wide]
    for case, want, g in zip(narrow + wide, wants, got):
        first, second, tile0, tile1, granules = want
        assert g == "%s | %s | %d %d %d" % (show(first), show(second), tile0, tile1, granules), (case, g)
        reached |= {first, second}
    for key, g in zip((U64, K128), got[len(wants):]):
        inst = (key, 9, KPT_WIDE[key], 0, 0, 0, 0, 0, 0)
        assert g == show(inst), (key, g)
        reached.add(inst)
    assert got[-1] == "refused"
    assert reached == ALL and len(ALL) == 29
    assert not any(i[0] == K96 and i[8] for i in reached)       # K96 never gets the rank table: its tile leaves no 8 KiB
    assert lds_bytes((K96, 9, 12, 0, 0, 0, 0, 0, 0)) + 8192 > LDS_MAX
    # every tile is above half the LDS (one workgroup per CU whatever the instantiation), and fits it beside the 2 KiB of HIST2 counters
    assert all(LDS_MAX // 2 < lds_bytes(i) <= LDS_MAX - (2048 if i[5] else 0) for i in reached)
