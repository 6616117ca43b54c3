"""The grouping passes of narrowed files over a BATCH of files: one launch per pass over the tiles of all files of the batch
(mgc_sort.hip, radix_group_batch_kernel; the batches: mgc_group_batch.hpp; Count::group_batches).  Every case counts a whole input in
a session, compares the WHOLE result with the threaded port, and asserts from the profile which launches ran: pass_launches[] counts
one per file and pass whatever shared a launch, pass_kernel_launches[] the kernel launches themselves.

The inputs are small, so a first-pass tile (24576 keys) is a good part of a file: with ~81 K k-mers per file every workgroup of a
batched launch crosses file boundaries and every file's first and last tile lie beside another file's in the ticket sequence.

Which files share a launch: narrowed files of the judged form (high digit first off the 5-byte layout, fetched a tile ahead) whose
plans have the same digits -- shifts and widths are arguments of the launch.  The probe file goes first and alone; a file that is
alone with its digits keeps its per-file launches.  (A non-empty file that takes no grouping passes at all cannot lie beside batched
ones: CountPlan::soa_mask gives the 5-byte layout only where EVERY non-empty file takes the narrowed passes, and without that layout
nothing is batched -- the file "the plan does not batch" of test_uneven_files is therefore one whose digits differ.)"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FORWARD = 1


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "the -m gpu tests need a GPU"
    torch.cuda.set_device(0)
    return torch


@pytest.fixture(scope="module")
def ops(native_lib, torch_cuda):
    from meryl_amd import count
    return count


_ORACLE = {}
_READS = {}


def _reads(oracle_lib):
    """the reads of every many-files case (one input, made once)"""
    if "r" not in _READS:
        _READS["r"] = oracle_lib.synth_reads(521, 300_000, 0, 40_000)
    return _READS["r"]


def _oracle(oracle_lib, key, bases, k, w_prefix, mode):
    """the threaded port's result of an input, computed once per module run and left unchanged"""
    if key not in _ORACLE:
        _ORACLE[key] = oracle_lib.count_threaded(bases.tobytes(), k, w_prefix, mode, threads=16)
    return _ORACLE[key]


def _count(ops, torch_cuda, bases, k, mode):
    from meryl_amd import capi
    cfg = capi.configure(k, bases.size, 1 << 30, mode)
    cfg.use_simple = 0
    with ops.Session(cfg) as s:
        s.set_profiling(True)
        s.push_bases_device(torch_cuda.from_numpy(bases).cuda())
        s.count()
        klo, khi, counts, _ = s.result_wide()
        prof = s.profile()
        info = s.info()
    return cfg, (klo, khi, counts), prof, info


def _count_and_check(ops, oracle_lib, torch_cuda, key, bases, k, mode):
    cfg, (klo, khi, counts), prof, info = _count(ops, torch_cuda, bases, k, mode)
    whi, wlo, wcn, wni = _oracle(oracle_lib, key, bases, k, cfg.w_prefix, mode)
    assert info.n_instances == wni and info.n_distinct == len(wlo)
    assert np.array_equal(klo, wlo) and np.array_equal(khi, whi) and np.array_equal(counts, wcn)
    assert prof.pass_launches[1] == prof.pass_launches[0] > 0       # two digits really
    return prof, (klo, khi, counts)


def _launches(prof):
    return (prof.pass_launches[0], prof.pass_launches[1]), (prof.pass_kernel_launches[0], prof.pass_kernel_launches[1])


# ~81 K canonical k-mers in each of the 64 files, ~3.3 first-pass tiles: target 1 gives sixteen top bits (eight-bit first digits, the
# 256-counter kernels); MGC_FINISH_MIN_TOP=18 two nine-bit digits (the 512-counter kernels: the first pass with the tight LDS).
# k = 23: 40 bits below the file, 32-bit words with no spare bit.  There the eight-bit case asks for MGC_FINISH_MIN_TOP=16: left to
# itself the plan gives the smallest files fifteen top bits, 25 bits stay below them, a word cannot hold them beside an eight-bit digit
# (sort_plan_narrows), and ONE file that does not narrow takes the 5-byte layout -- and with it the batched form -- from the whole count.
@pytest.mark.parametrize("k,min_top,width", [(21, None, 8), (21, 18, 9), (23, 16, 8), (23, 18, 9)])
def test_many_small_files_in_one_launch(ops, oracle_lib, torch_cuda, monkeypatch, k, min_top, width):
    monkeypatch.setenv("MGC_FINISH_TARGET", "1")
    if min_top is not None:
        monkeypatch.setenv("MGC_FINISH_MIN_TOP", str(min_top))
    prof, _ = _count_and_check(ops, oracle_lib, torch_cuda, ("reads", k), _reads(oracle_lib), k, 0)
    files, kernels = _launches(prof)
    print("k=%d min_top=%s: launches per file %s, kernel launches %s" % (k, min_top, files, kernels))
    assert prof.narrow_digit_widths & (1 << width)
    assert files[0] > 50
    assert kernels[0] < files[0] and kernels[1] < files[1]


# the budget: one file per batch (the parent's launch sequence), two, all.  MGC_GROUP_BATCH_BYTES is the bytes of the pass buffer a batch
# may fill -- 1: no two files fit; MGC_GROUP_BATCH_FILES caps the files of a batch whatever fits.
def test_budget_edges_identical_results(ops, oracle_lib, torch_cuda, monkeypatch):
    monkeypatch.setenv("MGC_FINISH_TARGET", "1")
    got = {}
    for name, env in (("one", {"MGC_GROUP_BATCH_BYTES": "1"}), ("two", {"MGC_GROUP_BATCH_FILES": "2"}),
                      ("all", {"MGC_GROUP_BATCH_BYTES": str(1 << 40)})):
        with monkeypatch.context() as m:
            for n, v in env.items():
                m.setenv(n, v)
            prof, arrays = _count_and_check(ops, oracle_lib, torch_cuda, ("reads", 21), _reads(oracle_lib), 21, 0)
        got[name] = (arrays, _launches(prof))
        print("budget %s: launches per file %s, kernel launches %s" % ((name,) + got[name][1]))
    for name in ("two", "all"):
        for a, b in zip(got["one"][0], got[name][0]):
            assert np.array_equal(a, b)
    files = got["one"][1][0]
    assert files[0] > 50
    assert got["two"][1][0] == files and got["all"][1][0] == files   # one per file and pass, whatever shared a launch
    assert got["one"][1][1] == files                                 # one file per batch: every file its own kernel launches
    for p in (0, 1):
        # batches of two: at least half as many launches as files, fewer than files; everything: fewer again
        assert (files[p] + 1) // 2 <= got["two"][1][1][p] < files[p]
        assert got["all"][1][1][p] < got["two"][1][1][p]


def _file_input(rng, first3, n, prefixes=("",)):
    """n separate 21-base sequences first3 + prefix + random bases, joined by `.`: n forward 21-mers of the file first3 names"""
    a = np.full((n, 22), ord("."), dtype=np.uint8)
    a[:, :3] = np.frombuffer(first3.encode("ascii"), dtype=np.uint8)
    a[:, 3:21] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=(n, 18))]
    for i, p in enumerate(prefixes):
        if p:
            a[i::len(prefixes), 3:3 + len(p)] = np.frombuffer(p.encode("ascii"), dtype=np.uint8)
    return a.reshape(-1)


# Uneven files in ONE count, forward k-mers.  MGC_FINISH_TARGET=3 and MGC_FINISH_MIN_TOP=16: every file of up to 262143 k-mers takes
# sixteen top bits (two eight-bit digits) and shares the batch; the file of 270000 takes seventeen (nine + eight) and is alone with
# its digits: per-file launches.  The high digit of a k-mer is the four bases behind the file's three: `GGGG` = 255 in every key
# (every tile one run, a histogram of one counter), `AAAA` / `GGGG` = 0 and 255.
_UNEVEN = [
    ("AAA", 196609, ("",)),                                          # eight tiles and one key
    ("AAC", 24576, ("",)),                                           # exactly one full tile
    ("AAT", 24577, ("",)),                                           # a full tile and a one-key last tile
    # AAG: empty, between two non-empty files
    ("ACA", 40000, ("GGGG",)),
    ("ACC", 30000, ("",)),
    ("ACT", 40000, ("AAAA", "GGGG")),
    ("ACG", 270000, ("",)),                                          # other digits: not batched
    ("ATA", 20000, ("",)),
]


def test_uneven_files(ops, oracle_lib, torch_cuda, monkeypatch):
    monkeypatch.setenv("MGC_FINISH_TARGET", "3")
    monkeypatch.setenv("MGC_FINISH_MIN_TOP", "16")
    rng = np.random.default_rng(77)
    bases = np.concatenate([_file_input(rng, f, n, p) for f, n, p in _UNEVEN])
    assert bases.size >= 1 << 22                                    # (the high-digit-first path)
    prof, _ = _count_and_check(ops, oracle_lib, torch_cuda, ("uneven",), bases, 21, FORWARD)
    files, kernels = _launches(prof)
    print("uneven: launches per file %s, kernel launches %s, digit widths %x" % (files, kernels, prof.narrow_digit_widths))
    assert prof.pass_keys[0] == sum(n for _, n, _ in _UNEVEN)
    assert files == (len(_UNEVEN), len(_UNEVEN))
    # the batch, the file with other digits, and the probe file where the plan has one
    assert 2 <= kernels[0] <= 3 and kernels[0] == kernels[1]


# the forms that keep their per-file launches: every forced form still gives the exact result, one kernel launch per file and pass
@pytest.mark.parametrize("env", [{"MGC_PASS_STAGGER": "8"}, {"MGC_GROUP_DBG": "1"}, {"MGC_GROUP_PIPE": "0"}, {"MGC_SOA5": "0"}, {"MGC_FINE_HIST": "0"}],
                         ids=lambda e: ",".join("%s=%s" % kv for kv in e.items()))
def test_forms_that_stay_per_file(ops, oracle_lib, torch_cuda, monkeypatch, capfd, env):
    monkeypatch.setenv("MGC_FINISH_TARGET", "1")
    for n, v in env.items():
        monkeypatch.setenv(n, v)
    prof, _ = _count_and_check(ops, oracle_lib, torch_cuda, ("reads", 21), _reads(oracle_lib), 21, 0)
    files, kernels = _launches(prof)
    assert files[0] > 50 and kernels == files
    assert ("[groupdbg]" in capfd.readouterr().err) == ("MGC_GROUP_DBG" in env)


# whole keys (k = 31: launch_group_wide): per-file launches
def test_whole_key_files_stay_per_file(ops, oracle_lib, torch_cuda, monkeypatch):
    monkeypatch.setenv("MGC_FINISH_TARGET", "1")
    cfg, (klo, khi, counts), prof, info = _count(ops, torch_cuda, _reads(oracle_lib), 31, 0)
    whi, wlo, wcn, wni = _oracle(oracle_lib, ("reads", 31), _reads(oracle_lib), 31, cfg.w_prefix, 0)
    assert info.n_instances == wni and info.n_distinct == len(wlo)
    assert np.array_equal(klo, wlo) and np.array_equal(khi, whi) and np.array_equal(counts, wcn)
    files, kernels = _launches(prof)
    assert files[0] > 50 and kernels == files
