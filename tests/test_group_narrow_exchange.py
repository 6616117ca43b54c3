"""The first grouping pass of a narrowed file exchanges what it writes (mgc_sort.hip, radix_group_kernel<..., NARROW>): a k-mer goes
through LDS as its 32-bit narrowed word plus its digit of the pass (one byte for digits of up to eight bits, 16 bits for nine-bit
digits), and the pipelined 5-byte form runs on 24576-key tiles.  Every case counts a whole input in a session and compares the
whole result with the threaded port, and asserts from the profile that the narrowed two-digit passes really ran.

The plans (CountPlan::plan_top, make_sort_plan): a file of n k-mers takes the smallest t with (n >> t) <= MGC_FINISH_TARGET top
bits, split into a low digit of ceil(t / 2) and a high digit of floor(t / 2) bits; with the fifteen-bit histogram at hand the HIGH
digit goes first.  t = 16 / 17: an eight-bit first digit (the 256-counter kernel, byte digits); t = 18: nine bits (the 512-counter
kernel, 16-bit digits)."""
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


def _one_file_input(n, seed, prefixes=("",)):
    """n separate 21-base sequences `AAA` + prefix + random bases, joined by `.`: forward 21-mers, all of file 0, exactly n of them.
    Sequence i takes prefixes[i % len(prefixes)]."""
    rng = np.random.default_rng(seed)
    a = np.full((n, 22), ord("."), dtype=np.uint8)
    a[:, :3] = ord("A")
    a[:, 3:21] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=(n, 18))]
    for i, p in enumerate(prefixes):
        if p:
            a[i::len(prefixes), 3:3 + len(p)] = np.frombuffer(p.encode("ascii"), dtype=np.uint8)
    return a.reshape(-1)


_ORACLE = {}


def _oracle(oracle_lib, key, bases, k, w_prefix, mode):
    """the threaded port's result of an input, computed once per module run and left unchanged"""
    if key not in _ORACLE:
        _ORACLE[key] = oracle_lib.count_threaded(bases.tobytes(), k, w_prefix, mode, threads=16)
    return _ORACLE[key]


def _count_and_check(ops, oracle_lib, torch_cuda, key, bases, k, mode, want_n=None):
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
    whi, wlo, wcn, wni = _oracle(oracle_lib, key, bases, k, cfg.w_prefix, mode)
    if want_n is not None:
        assert wni == want_n
    assert info.n_instances == wni and info.n_distinct == len(wlo)
    assert np.array_equal(klo, wlo) and np.array_equal(khi, whi) and np.array_equal(counts, wcn)
    assert prof.pass_launches[1] > 0                                # two digits really
    assert prof.pass_bytes[0] < 14 * prof.pass_keys[0]              # ... and narrowed: 5 or 8 B in, 4 B out
    return prof


# one below, at and one above a multiple of 16384, 24576 and 20480 keys: a full last tile, a one-key last tile, a tile short by one
@pytest.mark.parametrize("n", [196607, 196608, 196609, 204799, 204800, 204801])
def test_tile_edges_exact_key_count(ops, oracle_lib, torch_cuda, monkeypatch, n):
    # (n >> 16) <= 3 < (n >> 15): sixteen top bits, two eight-bit digits -- the plan of the judged files
    monkeypatch.setenv("MGC_FINISH_TARGET", "3")
    bases = _one_file_input(n, n)
    assert bases.size >= 1 << 22                                    # (the high-digit-first path)
    prof = _count_and_check(ops, oracle_lib, torch_cuda, ("edge", n), bases, 21, FORWARD, want_n=n)
    assert prof.pass_keys[0] == n and prof.narrow_digit_widths == 1 << 8


@pytest.mark.parametrize("name,n,target,prefixes,width", [
    ("one_run_ff", 196608, 3, ("GGGG",), 8),                        # digit 0xFF in every key: the whole tile one run
    ("two_runs_00_ff", 196608, 3, ("AAAA", "GGGG"), 8),            # digits 0 and 255, alternating
    # (n >> 18) <= 1 < (n >> 17): eighteen top bits, two nine-bit digits.  A = 0, C = 1, T = 2, G = 3: the digit of `TAAAA` is 256,
    # of `GAAAA` 384, of `GGGGG` 511 -- the ninth bit set with all, some and none of the others
    ("ninth_bit", 270_000, 1, ("TAAAA", "GGGGG", "GAAAA"), 9),
])
def test_digit_extremes(ops, oracle_lib, torch_cuda, monkeypatch, name, n, target, prefixes, width):
    monkeypatch.setenv("MGC_FINISH_TARGET", str(target))
    bases = _one_file_input(n, 7, prefixes)
    prof = _count_and_check(ops, oracle_lib, torch_cuda, ("extreme", name), bases, 21, FORWARD, want_n=n)
    assert prof.narrow_digit_widths == 1 << width


# both input layouts, both fetch forms, the staggered start and the low-digit-first order on one edge size: the forms that fetch
# inside the look-back run on 16384-key tiles (196609 = 12 tiles + one key), the pipelined ones on 24576-key tiles (8 tiles + one key).
# MGC_GROUP_DBG=1 (one size only): the instrumented instantiations of both passes -- the pipelined 5-byte first pass, the 5-byte one
# that fetches inside the look-back, the whole-key one -- which report on stderr; a count instruments its first two files, whatever
# ran before in the process.
_FORMS = [{}, {"MGC_SOA5": "0"}, {"MGC_GROUP_PIPE": "0"}, {"MGC_PASS_STAGGER": "8"}, {"MGC_FINE_HIST": "0"}, {"MGC_SOA5": "0", "MGC_GROUP_PIPE": "0"}]
_DBG_FORMS = [{"MGC_GROUP_DBG": "1"}, {"MGC_GROUP_DBG": "1", "MGC_GROUP_PIPE": "0"}, {"MGC_GROUP_DBG": "1", "MGC_SOA5": "0"}]


def _form_cases():
    cases = [(n, target, env) for n, target in ((196609, 3), (270_001, 1)) for env in _FORMS] + [(196609, 3, env) for env in _DBG_FORMS]
    return [pytest.param(n, target, env, id="%d-%d-%s" % (n, target, ",".join("%s=%s" % kv for kv in env.items()) or "default"))
            for n, target, env in cases]


@pytest.mark.parametrize("n,target,env", _form_cases())
def test_layouts_and_fetch_forms(ops, oracle_lib, torch_cuda, monkeypatch, capfd, n, target, env):
    monkeypatch.setenv("MGC_FINISH_TARGET", str(target))
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    bases = _one_file_input(n, n)
    _count_and_check(ops, oracle_lib, torch_cuda, ("edge", n), bases, 21, FORWARD, want_n=n)
    err = capfd.readouterr().err
    if "MGC_GROUP_DBG" in env:                                      # the one file of the input, both passes
        first = "first (u64 -> u32)" if "MGC_SOA5" in env else ("first (5 B -> u32)" if "MGC_GROUP_PIPE" in env else "first (5 B -> u32, fetch a tile ahead)")
        assert "[groupdbg] %s pass, %d keys" % (first, n) in err and "[groupdbg] second (u32 -> u32) pass, %d keys" % n in err
    else:
        assert "[groupdbg]" not in err


# canonical k-mers of ordinary reads.  k = 23: 40 bits below the file, the widest 5-byte key -- 32-bit words with no spare bit.
# ~81 K k-mers per file: target 1 gives sixteen top bits (eight-bit first digits); MGC_FINISH_MIN_TOP=18 the large-input plan
# (two nine-bit digits) on the same input.
@pytest.mark.parametrize("min_top,width", [(None, 8), (18, 9)])
@pytest.mark.parametrize("k", [21, 23])
def test_canonical_reads_both_digit_widths(ops, oracle_lib, torch_cuda, monkeypatch, k, min_top, width):
    monkeypatch.setenv("MGC_FINISH_TARGET", "1")
    if min_top is not None:
        monkeypatch.setenv("MGC_FINISH_MIN_TOP", str(min_top))
    bases = oracle_lib.synth_reads(500 + k, 300_000, 0, 40_000)
    prof = _count_and_check(ops, oracle_lib, torch_cuda, ("reads", k), bases, k, 0)
    assert prof.pass_launches[0] > 50 and prof.narrow_digit_widths & (1 << width)
