"""hash_count_stream_kernel's insert phase and table sweep at their edges (run with -m gpu on an MI355X).

The kernel cuts a sub-bucket of n keys into one to three chunks of whole 256-key rows, probes full rows without a lane predicate and
the partial last row with one, queues the keys whose first probe met another suffix per wave and probes them on densely, counts
every claim into one of 256 bins by the top eight suffix bits (D, and "more than DCAP distinct", are the bin total), and reads the
distinct entries off the table by a sweep that puts each at its bin's cursor.  The sub-buckets planted here sit on every one of
those edges; they are built the way
test_count_structured_keys.py builds its own -- the same ~4.5 Mbase filler reads (so that the judged plan is on), prefixes whose
sub-buckets the filler leaves empty, MGC_FINISH_MIN_TOP / MGC_FINISH_NOLIST / MGC_HASH_STREAM=1 -- several of them per run, and
every run is compared exactly with the oracle's brute-force count of the same text (k-mers and counts).  Every run asserts
profile().stream_files > 0: it cannot pass on another kernel."""
import numpy as np
import pytest

import plant_helpers as ph
import structured_helpers as sh

pytestmark = pytest.mark.gpu

K, MIN_TOP = 21, 16
LOW = 2 * K - 6 - MIN_TOP                       # 20 suffix bits: ten bases behind the eleven that fix file and sub-bucket
PLEN = 11
DCAP64 = 1024                                   # FIN_STREAM64_DCAP
QCAP = 128                                      # STREAM_QCAP: keys a wave's queue holds

# chunk and row edges: one row and its neighbours, the largest single chunk (1536) and two-chunk sub-bucket (3072) with theirs,
# 1280 = DCAP, the capacity
EDGES = (1, 2, 255, 256, 257, 1279, 1280, 1281, 1535, 1536, 1537, 3071, 3072, 3073, 4093, 4094)


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


def _env(monkeypatch, nolist="1", min_top=MIN_TOP):
    monkeypatch.setenv("MGC_FINISH_MIN_TOP", str(min_top))
    monkeypatch.setenv("MGC_FINISH_NOLIST", nolist)
    monkeypatch.setenv("MGC_HASH_STREAM", "1")


class Planter:
    """Sub-buckets planted into prefixes the filler leaves empty; check() finds each of them in the oracle's result."""

    def __init__(self, oracle_lib, k, min_top, seed, plen):
        self.oracle, self.k, self.min_top, self.plen = oracle_lib, k, min_top, plen
        self.low = 2 * k - 6 - min_top
        self.rng = np.random.default_rng(seed)
        self.occ = ph.occupied(oracle_lib, k, self.low, (1,))
        self.text, self.planted, self.used = "", [], set()

    def prefix(self, head="A"):
        for _ in range(1000):
            pre, _ = ph.pick_prefix(head, self.plen, self.min_top, self.occ, self.rng)
            if pre not in self.used:
                self.used.add(pre)
                return pre
        raise AssertionError("no free prefix")

    def plant(self, tails, n, pre=None):
        """n reads of one k-mer each over `tails` (each at least once) in a sub-bucket of their own"""
        pre = pre or self.prefix()
        assert all(len(t) == self.k - len(pre) for t in tails) and len(set(tails)) == len(tails)
        self.text += ph.plant(pre, list(tails), n, self.rng)
        self.planted.append((pre, n, len(tails)))
        return pre

    def run(self, ops):
        text = self.text + ph.filler(self.oracle, self.k)
        whi, wlo, wcn, prof = ph.count_and_compare(ops, self.oracle, text, self.k, 1)
        for pre, n, d in self.planted:            # the sub-buckets are what the case says: n keys, d distinct, nothing else in them
            assert ph.subbucket(whi, wlo, wcn, self.low, ph.id_range(pre[:PLEN], self.min_top)) == (n, d), (pre, n, d)
        assert prof.stream_files > 0, prof.stream_files
        return whi, wlo, wcn, prof


def _tails(n, length, seed):
    return sh.random_tails(n, length, seed)


@pytest.mark.parametrize("nolist", ["1", "0"])
def test_chunk_and_row_edges_seven_distinct(ops, oracle_lib, torch_cuda, monkeypatch, nolist):
    """every edge size with (up to) seven distinct suffixes: nearly all keys are duplicates of a claimed entry; once on the whole
    grid and once on the list of non-empty sub-buckets (the LIST instantiation)"""
    _env(monkeypatch, nolist)
    p = Planter(oracle_lib, K, MIN_TOP, 7000 + int(nolist), PLEN)
    for i, n in enumerate(EDGES):
        p.plant(_tails(min(7, n), K - PLEN, 100 + i), n)
    _, _, _, prof = p.run(ops)
    assert prof.stream_retries == 0, prof.stream_retries


def test_chunk_and_row_edges_all_distinct(ops, oracle_lib, torch_cuda, monkeypatch):
    """the edge sizes up to DCAP with every key another suffix: the sweep finds n entries, 1280 of them fill srt exactly"""
    _env(monkeypatch)
    p = Planter(oracle_lib, K, MIN_TOP, 7100, PLEN)
    for i, n in enumerate(e for e in EDGES if e <= sh.DCAP_STREAM):
        p.plant(_tails(n, K - PLEN, 200 + i), n)
    _, _, _, prof = p.run(ops)
    assert prof.stream_retries == 0, prof.stream_retries


@pytest.mark.parametrize("distinct,retries", [((1279, 1280), 0), ((1281,), 1)])
def test_capacity_edge(ops, oracle_lib, torch_cuda, monkeypatch, distinct, retries):
    """4094 keys with DCAP - 1 and DCAP distinct suffixes stay in the first launch; DCAP + 1 is decided by the bin total,
    nothing of it is written, and the retry launch counts it"""
    _env(monkeypatch)
    p = Planter(oracle_lib, K, MIN_TOP, 7200 + len(distinct), PLEN)
    for d in distinct:
        p.plant(_tails(d, K - PLEN, 300 + d), sh.CAP_STREAM)
    _, _, _, prof = p.run(ops)
    assert (prof.stream_retries == 0) if retries == 0 else (prof.stream_retries >= 1), prof.stream_retries


def test_count_maximum_and_crowded_bins(ops, oracle_lib, torch_cuda, monkeypatch):
    """one k-mer 4094 times (the count field's maximum), and 600 and 1280 distinct suffixes that share their top eight bits: one of
    the 256 bins takes them all, the rank inside that bin orders them"""
    _env(monkeypatch)
    p = Planter(oracle_lib, K, MIN_TOP, 7300, PLEN)
    pre = p.plant(["CTGACTGACT"], sh.CAP_STREAM)
    for d, n, top in ((600, 1500, "GTCA"), (1280, 3000, "TTTT")):
        p.plant([top + t for t in _tails(d, K - PLEN - 4, 400 + d)], n)
    whi, wlo, wcn, prof = p.run(ops)
    i = int(np.searchsorted(wlo, np.uint64(sh.encode(pre + "CTGACTGACT"))))
    assert int(wcn[i]) == sh.CAP_STREAM
    assert prof.stream_retries == 0, prof.stream_retries


def test_dense_pending_lanes_without_retry(ops, oracle_lib, torch_cuda, monkeypatch):
    """60 distinct suffixes on ONE home slot of the 2048-slot table, ~60 copies each (3600 keys): after the first probe nearly every
    lane holds a pending key -- a row queues up to 64 per wave, three rows overflow the queue's 128, which is drained in between --
    and every chain stays below PROBE_MAX steps: no retry"""
    _env(monkeypatch)
    p = Planter(oracle_lib, K, MIN_TOP, 7400, PLEN)
    pre = p.prefix()
    n, m = 3600, 60
    assert sh.slots_stream(n, 2048) == 2048
    tails, homes = sh.colliding_tails(K, MIN_TOP, pre, m, 777, 1, 2048, "fib32")
    assert set(homes.tolist()) == {777} and sh.linear_probe_max_steps(homes, 2048) == m - 1 < sh.PROBE_MAX
    assert 6 * 64 * (m - 1) // m > QCAP                     # pending keys a wave meets in one chunk: more than its queue holds
    p.plant(tails, n, pre)
    _, _, _, prof = p.run(ops)
    assert prof.stream_retries == 0, prof.stream_retries


def test_retry_instantiation_all_distinct(ops, oracle_lib, torch_cuda, monkeypatch):
    """3000 keys, all distinct: above DCAP, counted by the retry instantiation (8192 slots, a sweep of 32 entries per thread)"""
    _env(monkeypatch)
    p = Planter(oracle_lib, K, MIN_TOP, 7500, PLEN)
    p.plant(_tails(3000, K - PLEN, 500), 3000)
    _, _, _, prof = p.run(ops)
    assert prof.stream_retries >= 1, prof.stream_retries


def test_u64_instantiation_row_and_capacity_edges(ops, oracle_lib, torch_cuda, monkeypatch):
    """whole 8-byte k-mers (k = 31, 40-bit suffixes, 64-bit entries: two per 16-byte vector of the sweep): the row edges 256 / 257 /
    1537 and the capacity edge of its 1024-entry srt"""
    k, plen = 31, 11
    _env(monkeypatch)
    p = Planter(oracle_lib, k, MIN_TOP, 7600, plen)
    for i, n in enumerate((256, 257, 1537)):
        p.plant(_tails(7, k - plen, 600 + i), n)
    for d in (DCAP64 - 1, DCAP64, DCAP64 + 1):
        p.plant(_tails(d, k - plen, 700 + d), sh.CAP_STREAM)
    _, _, _, prof = p.run(ops)
    assert prof.stream_retries >= 1, prof.stream_retries


def _file_with_empty(occ, min_top, first):
    """a file (three bases) whose first (or last) two sub-buckets the filler leaves empty; returns the prefix of the outermost one"""
    for f in range(64):
        head = sh.decode(f, 3)
        a = head + ("A" if first else "G") * (PLEN - 3)
        b = a[:-1] + ("C" if first else "T")                 # A0 C1 T2 G3: the sub-bucket next to it
        if ph.strays(occ, ph.id_range(a, min_top)) == 0 and ph.strays(occ, ph.id_range(b, min_top)) == 0:
            return a
    raise AssertionError("no file whose %s two sub-buckets are free of filler k-mers" % ("first" if first else "last"))


def test_first_and_last_subbucket_of_a_file(ops, oracle_lib, torch_cuda, monkeypatch):
    """planted sub-buckets that are the first and the last of their file, the sub-bucket beside each empty: the chunk loads clamp to
    the sub-bucket's own last key and the bounds come from the file's first and last `starts`"""
    _env(monkeypatch)
    p = Planter(oracle_lib, K, MIN_TOP, 7700, PLEN)
    for first, n in ((True, 1537), (False, 257)):
        pre = _file_with_empty(p.occ, MIN_TOP, first)
        lo, hi = ph.id_range(pre, MIN_TOP)
        assert hi == lo + 1 and (lo if first else hi) % (1 << MIN_TOP) == 0
        p.plant(_tails(300 if first else 257, K - PLEN, 800 + n), n, pre)
    _, _, _, prof = p.run(ops)
    assert prof.stream_retries == 0, prof.stream_retries
