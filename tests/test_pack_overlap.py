"""Early packing: a file is packed on a third stream while the files after it are still being counted (mgc_count.cpp,
Count::pack_plan / pack_step / pack_finish; the decision and the capacity: mgc_pack_plan.hpp; the gate and the per-file scan:
mgc_finish.hip, pack_gate_scan_kernel).  Run with -m gpu on an MI355X.

Every case counts the same input with MGC_PACK_OVERLAP=1 and =0 and compares keys, counts, block starts and totals for equality,
compares with the oracle, and asserts from the profile what the packing chain did: early_pack_files (files packed by the chain, not
deferred -- that the chain's path was taken; when its launches ran against the count kernels only a kernel trace shows) and
early_pack_deferred (files the device's gate left to the serial path).

The result needs room before the total is known.  A count with a probe file sizes it from the probe's distinct / instances ratio;
the small narrowed inputs here have no probe file (the distinct-sized count is forced with MGC_HASH_STREAM=1, as in
test_count_stream_insert.py), so their first count in a session finds an empty arena and takes the serial path, and every later
count of the session packs early into what the arena holds by then.  The cases therefore count twice (or more) in one session.
MGC_PACK_RATIO stands in for the probe's ratio in some cases: there the first count of a session packs early, and MGC_PACK_MARGIN
makes the estimate fall short by construction.  A narrowed k = 21 count needs files of 75 M k-mers for a probe file; a `compress`
count at k = 31 with small buckets has one at 15 Mbases (as in test_gpu_parity.py), and one case runs that: the probe file's own
ratio sizes the result and the first count of the session packs early."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CANONICAL, FORWARD = 0, 1
K, MIN_TOP = 21, 16


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
_INPUT = {}


def _reads30(oracle_lib):
    """30x reads of a 300 kb genome: 9 Mbases, ~140 K k-mers per file"""
    if "r30" not in _INPUT:
        _INPUT["r30"] = oracle_lib.synth_reads(521, 300_000, 0, 60_000)
    return _INPUT["r30"]


def _oracle(oracle_lib, key, bases, k, w_prefix, mode):
    """the threaded port's result of an input, computed once per module run and left unchanged"""
    if key not in _ORACLE:
        _ORACLE[key] = oracle_lib.count_threaded(bases.tobytes(), k, w_prefix, mode, threads=16)
    return _ORACLE[key]


def _stream_env(monkeypatch):
    """tiny inputs on the narrowed, streamed plan: two eight-bit digits, 20-bit suffixes, hash_count_stream_kernel on every file"""
    monkeypatch.setenv("MGC_FINISH_MIN_TOP", str(MIN_TOP))
    monkeypatch.setenv("MGC_HASH_STREAM", "1")


def _session_counts(ops, torch_cuda, monkeypatch, overlap, inputs, k, mode, env=()):
    """one session, one count per entry of `inputs` (numpy byte arrays of ONE length: the device buffer is rewritten in place
    between the counts); returns per count (keys_lo, keys_hi, counts, block starts, (n_distinct, n_instances), profile)"""
    from meryl_amd import capi
    out = []
    with monkeypatch.context() as m:
        m.setenv("MGC_PACK_OVERLAP", "1" if overlap else "0")
        for n, v in env:
            m.setenv(n, v)
        cfg = capi.configure(k, inputs[0].size, 1 << 30, mode)
        cfg.use_simple = 0
        d = torch_cuda.from_numpy(inputs[0].copy()).cuda()
        with ops.Session(cfg) as s:
            s.set_profiling(True)
            s.push_bases_device(d)
            for b in inputs:
                assert b.size == inputs[0].size
                d.copy_(torch_cuda.from_numpy(b.copy()))
                torch_cuda.cuda.synchronize()
                s.count()
                klo, khi, counts, bstart = s.result_wide()
                info = s.info()
                out.append((klo, khi, counts, bstart, (info.n_distinct, info.n_instances), s.profile(), cfg))
    return out


def _same(a, b):
    for x, y in zip(a[:4], b[:4]):
        assert x.dtype == y.dtype and np.array_equal(x, y)
    assert a[4] == b[4]


def _check_oracle(oracle_lib, key, bases, k, mode, got):
    whi, wlo, wcn, wni = _oracle(oracle_lib, key, bases, k, got[6].w_prefix, mode)
    assert got[4] == (len(wlo), wni)
    assert np.array_equal(got[0], wlo) and np.array_equal(got[1], whi) and np.array_equal(got[2], wcn)


def _files(prof):
    return prof.early_pack_files, prof.early_pack_deferred


def _nfiles(whi, wlo, k):
    """files (top six bits of the k-mer) that hold k-mers"""
    top = (wlo >> np.uint64(2 * k - 6)) if k <= 32 else (whi >> np.uint64(2 * k - 6 - 64))
    return int(np.unique(top).size)


def _ab(ops, oracle_lib, torch_cuda, monkeypatch, key, inputs, k, mode, env=()):
    """the counts of `inputs` in one session with early packing on and off: equal to each other and to the oracle; returns the
    profiles of the session with it on (files_with_kmers added: the files that hold k-mers)"""
    on = _session_counts(ops, torch_cuda, monkeypatch, True, inputs, k, mode, env)
    off = _session_counts(ops, torch_cuda, monkeypatch, False, inputs, k, mode, env)
    for i, (a, b) in enumerate(zip(on, off)):
        _same(a, b)
        _check_oracle(oracle_lib, key + (i,), inputs[i], k, mode, a)
        a[5].files_with_kmers = _nfiles(a[1], a[0], k)
        a[5].n_distinct_seen = a[4][0]
        assert _files(b[5]) == (0, 0)                                  # MGC_PACK_OVERLAP=0: the serial path for every file
        assert a[5].stage_launches[3] == b[5].stage_launches[3]
    return [a[5] for a in on]


def _no_file(bases, first3):
    """the reads without forward k-mers of one file: an N in place of the third base of every occurrence of its three bases"""
    return np.frombuffer(bases.tobytes().replace(first3, first3[:2] + b"N"), dtype=np.uint8).copy()


def test_all_files_early_with_an_empty_file_between(ops, oracle_lib, torch_cuda, monkeypatch):
    """30x reads, forward k-mers, no k-mer in file AAG (index 3): the first count of the session sizes the arena on the serial
    path, the second packs every file that holds k-mers early -- the chain steps over the empty file"""
    _stream_env(monkeypatch)
    bases = _no_file(_reads30(oracle_lib), b"AAG")
    profs = _ab(ops, oracle_lib, torch_cuda, monkeypatch, ("r30-aag", FORWARD), [bases, bases], K, FORWARD)
    print("first count %s, second count %s, stream files %d, retries %d" % (_files(profs[0]), _files(profs[1]), profs[1].stream_files, profs[1].stream_retries))
    assert _files(profs[0]) == (0, 0)                                  # nothing to pack into before the total was known
    assert profs[1].stream_files == 63 and profs[1].stream_retries == 0
    assert _files(profs[1]) == (63, 0)


def _planted(prefix11, n, seed):
    """n reads of one 21-mer each: the eleven bases that fix file and sub-bucket, then n DISTINCT ten-base tails -- more distinct
    suffixes than hash_count_stream_kernel's table holds (1280): the sub-bucket goes on its file's retry list"""
    rng = np.random.default_rng(seed)
    tails = rng.choice(4 ** 10, size=n, replace=False)
    a = np.full((n, 22), ord("."), dtype=np.uint8)
    a[:, :11] = np.frombuffer(prefix11, dtype=np.uint8)
    for j in range(10):
        a[:, 11 + j] = np.frombuffer(b"ACGT", dtype=np.uint8)[(tails >> (2 * (9 - j))) & 3]
    return a.reshape(-1)


@pytest.mark.parametrize("prefix,first_deferred", [(b"CATCATCATCA", 18), (b"AAACATCATCA", 0)])
def test_retry_list_defers_from_its_file_on(ops, oracle_lib, torch_cuda, monkeypatch, prefix, first_deferred):
    """a sub-bucket of 3000 distinct k-mers in file CAT (index 18) / in file AAA (index 0): its count kernel leaves a retry list, the
    gate defers that file and every later one, the files before it stay packed (all but the last of them, whose packing launch
    waits for the scan of the deferred file: q - 1 files), the serial path counts the retry list and packs the rest"""
    _stream_env(monkeypatch)
    bases = np.concatenate([_planted(prefix, 3000, 5), _reads30(oracle_lib)])
    profs = _ab(ops, oracle_lib, torch_cuda, monkeypatch, ("r30-plant", prefix), [bases, bases], K, FORWARD)
    print("first deferred %d: second count %s, retries %d" % (first_deferred, _files(profs[1]), profs[1].stream_retries))
    assert profs[1].stream_retries >= 1
    assert _files(profs[1]) == (max(first_deferred - 1, 0), 64 - first_deferred)


@pytest.mark.parametrize("ratio", [None, "200"])
def test_second_count_larger_than_the_first(ops, oracle_lib, torch_cuda, monkeypatch, ratio):
    """the arena holds the first count's result -- half the reads -- when the second, of all reads, is queued.
    With an estimate (MGC_PACK_RATIO 200/1000 where 0.176 of the instances are distinct): the arena, which holds less, grows to it
    BEFORE anything is queued, and the second count packs every file early with nothing deferred.
    Without one (no probe file): nothing grows beforehand; the gate defers from the first file that does not fit, the result grows
    afterwards and, having moved, is packed again from its first file.  The third count (the same reads) fits either way"""
    _stream_env(monkeypatch)
    full = _reads30(oracle_lib)
    half = full.copy()
    half[half.size // 2:] = ord(".")
    env = (("MGC_PACK_RATIO", ratio),) if ratio else ()
    profs = _ab(ops, oracle_lib, torch_cuda, monkeypatch, ("r30-grow", FORWARD), [half, full, full], K, FORWARD, env)
    print("ratio %s: half %s, all %s, all again %s" % ((ratio,) + tuple(_files(p) for p in profs)))
    assert profs[1].files_with_kmers == 64 and profs[0].n_distinct_seen < profs[1].n_distinct_seen      # the second really is larger
    if ratio:                                                                         # (half the reads are half the coverage: 0.26 distinct, their own estimate is short)
        assert _files(profs[1]) == (64, 0)                                            # grown before the chain was queued
    else:
        assert _files(profs[0]) == (0, 0)
        assert profs[1].early_pack_deferred > 0 and profs[1].early_pack_files == 0      # (moved: none of the chain's launches counts)
    assert _files(profs[2]) == (64, 0)


def test_probe_file_sizes_the_result_of_the_first_count(ops, oracle_lib, torch_cuda, monkeypatch):
    """`compress`, k = 31, buckets of 200 K bases, MGC_HASH_STREAM unset: the count picks a probe file on its own (not file 0: the
    smallest bucket that is a fair sample), counts it first, and its distinct / instances ratio -- no stand-in -- sizes the result
    before the chain is queued: the FIRST count of the session packs early, nothing deferred.  The probe file's count launch ended
    long before its turn in the chain.  Equal to MGC_PACK_OVERLAP=0 and to the oracle's compress + brute-force count"""
    from meryl_amd import capi
    k, reads, read_len = 31, 3000, 5000
    monkeypatch.setenv("MGC_BUCKET_BASES", "200000")
    monkeypatch.setenv("MGC_FINISH_TARGET", "100")
    bases = oracle_lib.synth_reads(290 + k, reads * read_len // 8, 0, reads, read_len, 3000, 300)
    stretched = bases.tobytes().decode().replace("AC", "AAAC").replace("GT", "GTTT")
    whi, wlo, wcn, wni = oracle_lib.count_brute(oracle_lib.compress_stream(stretched), k, CANONICAL)
    got = {}
    for overlap in (True, False):
        with monkeypatch.context() as m:
            m.setenv("MGC_PACK_OVERLAP", "1" if overlap else "0")
            cfg = capi.configure(k, len(stretched), 2 << 30, CANONICAL, homopoly_compress=1)
            d = torch_cuda.from_numpy(np.frombuffer(stretched.encode(), dtype=np.uint8).copy()).cuda()
            with ops.Session(cfg) as s:
                s.set_profiling(True)
                s.push_bases_device(d)
                s.count()
                klo, khi, counts, bstart = s.result_wide()
                got[overlap] = (klo, khi, counts, bstart, (s.info().n_distinct, s.info().n_instances), s.profile())
        assert got[overlap][4] == (len(wlo), wni)
        assert np.array_equal(got[overlap][0], wlo) and np.array_equal(got[overlap][1], whi) and np.array_equal(got[overlap][2], wcn)
    _same(got[True], got[False])
    on, off = got[True][5], got[False][5]
    print("probe file %d, ratio %.4f, stream files %d: first count %s" % (on.probe_file, on.probe_ratio, on.stream_files, _files(on)))
    assert on.probe_file > 0 and on.probe_ratio > 0                     # a probe ran, and it was not file 0
    assert (off.probe_file, off.probe_ratio) == (on.probe_file, on.probe_ratio) and _files(off) == (0, 0)
    assert on.early_pack_files > 0 and on.early_pack_deferred == 0


@pytest.mark.parametrize("k,mode", [(31, CANONICAL), (51, CANONICAL)])
def test_whole_key_files(ops, oracle_lib, torch_cuda, monkeypatch, k, mode):
    """whole 8-byte keys (k = 31) and K96 records / 16-byte keys (k = 51): the same chain, their own packing kernels"""
    monkeypatch.setenv("MGC_FINISH_TARGET", "1")
    bases = _reads30(oracle_lib)
    profs = _ab(ops, oracle_lib, torch_cuda, monkeypatch, ("r30", k, mode), [bases, bases], k, mode)
    print("k = %d: second count %s" % (k, _files(profs[1])))
    assert _files(profs[1]) == (profs[1].files_with_kmers, 0)


@pytest.mark.parametrize("stream_max,early", [(None, True), ("5000", False)])
def test_oversized_subbuckets(ops, oracle_lib, torch_cuda, monkeypatch, stream_max, early):
    """a poly-A run and a repeated 21-mer: two sub-buckets above the count kernels' capacity, 8980 and 6000 keys.  Their files'
    oversized lists are streamed on the second stream: the packing chain waits for that launch as well and every file is packed
    early.  With MGC_STREAM_MAX below them the host asks a probe launch about the file first -- the count is not eligible, every
    file is packed behind the last count kernel"""
    _stream_env(monkeypatch)
    if stream_max:
        monkeypatch.setenv("MGC_STREAM_MAX", stream_max)
    rep = np.frombuffer((b"ACGTTGCAACGTTGCAACGTT." * 6000) + (b"A" * 9000) + b".", dtype=np.uint8)
    bases = np.concatenate([rep, _reads30(oracle_lib)])
    profs = _ab(ops, oracle_lib, torch_cuda, monkeypatch, ("r30-rep", FORWARD), [bases, bases], K, FORWARD)
    print("stream_max %s: %s, %s" % (stream_max, _files(profs[0]), _files(profs[1])))
    assert _files(profs[0]) == (0, 0)
    assert _files(profs[1]) == ((64, 0) if early else (0, 0))


@pytest.mark.parametrize("ratio,margin,short", [("1000", None, False), ("100", "-600", True)])
def test_result_sized_before_anything_is_queued(ops, oracle_lib, torch_cuda, monkeypatch, ratio, margin, short):
    """the FIRST count of a session packs early when there is an estimate to size the result by.  These inputs are too small for a
    probe file, MGC_PACK_RATIO stands in for its distinct / instances ratio.  1000/1000: room for every instance, the arena grows
    before the chain is queued, every file is packed early.  100/1000 with the margin at -600/1000: room for 0.04 of the instances
    where 0.13 are distinct -- the gate defers from the first file that does not fit, the result grows afterwards and is packed
    again from its first file.  The second count of either session packs everything early"""
    _stream_env(monkeypatch)
    bases = _reads30(oracle_lib)
    env = (("MGC_PACK_RATIO", ratio),) + ((("MGC_PACK_MARGIN", margin),) if margin else ())
    profs = _ab(ops, oracle_lib, torch_cuda, monkeypatch, ("r30", K, FORWARD), [bases, bases], K, FORWARD, env)
    print("ratio %s margin %s: first count %s, second %s" % (ratio, margin, _files(profs[0]), _files(profs[1])))
    if short:
        assert profs[0].early_pack_deferred > 0 and profs[0].early_pack_files == 0
    else:
        assert _files(profs[0]) == (64, 0)
    assert _files(profs[1]) == (64, 0)


@pytest.mark.parametrize("room", ["exact", "ample", "short"])
def test_caller_buffers(ops, oracle_lib, torch_cuda, monkeypatch, room):
    """mgc_count_buckets_into: the chain packs straight into the caller's buffers, whose size is the capacity; too small a pair is
    met by the gate (deferral), and the result goes to the arena instead"""
    from meryl_amd import capi
    _stream_env(monkeypatch)
    bases = _reads30(oracle_lib)
    whi, wlo, wcn, _ = _oracle(oracle_lib, ("r30", K, CANONICAL, 0), bases, K, capi.configure(K, bases.size, 1 << 30).w_prefix, CANONICAL)
    nd, files = len(wlo), _nfiles(whi, wlo, K)
    cap = {"exact": nd, "ample": nd + 12345, "short": nd - 1}[room]
    got = {}
    for overlap in (True, False):
        with monkeypatch.context() as m:
            m.setenv("MGC_PACK_OVERLAP", "1" if overlap else "0")
            cfg = capi.configure(K, bases.size, 1 << 30)
            with ops.Session(cfg) as s:
                s.set_profiling(True)
                keys, counts = ops.dev_kmer_partition(torch_cuda.from_numpy(bases).cuda(), K, 0, 6)
                out_k = torch_cuda.zeros(cap, dtype=torch_cuda.int64, device="cuda")
                out_c = torch_cuda.zeros(cap, dtype=torch_cuda.int32, device="cuda")
                n, fitted = s.count_partitioned_into(keys, counts, out_k, out_c)
                assert n == nd and fitted == (room != "short")
                if fitted:
                    rk, rc = out_k[:n].cpu().numpy().view(np.uint64), out_c[:n].cpu().numpy().view(np.uint32)
                else:
                    uk, uc = s.result_device()
                    rk, rc = uk.cpu().numpy().view(np.uint64), uc.cpu().numpy().view(np.uint32)
                got[overlap] = (rk, rc, s.profile())
        assert np.array_equal(got[overlap][0], wlo) and np.array_equal(got[overlap][1], wcn)
    on, off = got[True][2], got[False][2]
    print("caller buffers, %s: %s" % (room, _files(on)))
    assert _files(off) == (0, 0)
    if room == "short":
        assert on.early_pack_deferred > 0 and on.early_pack_files == 0            # (the result moved to the arena: packed again)
    else:
        assert _files(on) == (files, 0)
