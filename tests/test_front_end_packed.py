"""The packed base stream of a count (meryl_amd/csrc/mgc_kmer.hip, PackedBases): the histogram kernel stores the 2-bit codes and
invalid-base masks of the input, the partition stages its tiles from them.  Every count here runs twice -- with the stream and
with MGC_PACKED_BASES=0 (the partition decodes the ASCII bases again) -- and both are compared with the oracle's brute-force
count: instances, distinct k-mers, counts, per-file totals.

The fine-histogram path needs 2^22 bases, so the inputs are 2^22 + r bases, r in {0, 1, 15, 17, 4095, 4097}: whole tiles, one
base into the next tile, one short of / one past a 16-base word, one short of / one past a tile.  At the first tile boundary an
input holds a non-ACGT byte at stream position 4095, 4096 or 4097, or the pair at 4096 +- (k - 1) -- one of the four, so that
the k-mers around it are decided by that byte alone; the same bytes all together around later boundaries.  Every input also
holds lower-case runs (one across a tile boundary), reads shorter than k, a word of bytes that are no text, and reads drawn
from a small genome so that counts go well above one.  Its end is one of: inside
a k-mer (a separator k - 2 bases before the end), on an invalid byte, or on a complete k-mer; the base pointer is 16-byte
aligned or 1 or 8 bytes past that.  Which boundary byte, which end and which alignment a case takes rotates with r and k, so
that every k meets all of them."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RS = (0, 1, 15, 17, 4095, 4097)
KS = (21, 22, 31, 51)                                     # constant-k 5-byte layout; generic; constant-k 8-byte; constant-k K96 records
OFFSETS = (0, 1, 8)
ENDS = ("inside", "invalid", "whole")
N0 = 1 << 22
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


@pytest.fixture(scope="module")
def torch_cuda(native_lib):
    import torch
    assert torch.cuda.is_available(), "the -m gpu tests need a GPU"
    torch.cuda.set_device(0)
    return torch


def make_input(n, k, end, seed, boundary=3):
    rng = np.random.default_rng(seed)
    genome = rng.choice(ACGT, size=60_000)
    read_len = 150
    n_reads = n // (read_len + 1) + 2
    starts = rng.integers(0, genome.size - read_len, size=n_reads)
    reads = genome[starts[:, None] + np.arange(read_len + 1)[None, :]]
    reads[:, read_len] = ord(".")
    b = reads.reshape(-1)[:n].copy()
    # the first tile boundary, one of the stream positions the cases rotate through: the last base of tile 0, the first and second of
    # tile 1, or the pair k - 1 before / after the boundary (the last window that ends in tile 1's first base is cut off, and the
    # first window that starts behind the boundary byte's reach is not)
    if boundary < 3:
        b[4095 + boundary] = (ord("N"), ord("R"), ord("."))[boundary]
    else:
        b[4096 - (k - 1)] = ord("n")
        b[4096 + (k - 1)] = ord("\n")
    for p in (4095, 4096, 4097):                                       # all three together, around a later boundary
        b[p + 3 * 4096] = ord("N")
    for kk in KS:                                                      # and every k's pair around a boundary of its own
        t = 4096 * (5 + 4 * KS.index(kk))
        b[t - (kk - 1)] = ord("n")
        b[t + (kk - 1)] = ord("\n")
    for lo, hi in ((100, 180), (8 * 4096 - 40, 8 * 4096 + 40), (n - 700, n - 600)):      # lower-case runs
        seg = b[lo:hi]
        up = (seg >= 65) & (seg <= 90)
        seg[up] += 32
    for p in range(20_000, 20_200, 7):                                 # reads shorter than every k
        b[p] = ord(".")
    b[50_000:50_016] = 0xFF                                            # one word of bytes that are no text at all
    b[n - 400:n] = rng.choice(ACGT, size=400)                          # the end: plain bases, then what the case asks for
    if end == "inside":
        b[n - (k - 1)] = ord(".")                                      # k - 2 bases follow: no k-mer, the stream ends inside one
    elif end == "invalid":
        b[n - 1] = ord("N")
    return b


def oracle_count(oracle_lib, bases, k):
    hi, lo, cn, ni = oracle_lib.count_brute(bases.tobytes(), k)
    files = (lo >> np.uint64(2 * k - 6)) if k <= 32 else (hi >> np.uint64(2 * k - 6 - 64))
    per_file = np.bincount(files.astype(np.int64), weights=cn.astype(np.float64), minlength=64).astype(np.int64)
    return {"lo": lo, "hi": hi, "counts": cn, "instances": int(ni), "per_file": per_file}


def device_count(torch, monkeypatch, dev_bases, k, packed, refill=None):
    """One session over the device buffer; refill: (tensor, bases) -- the buffer is overwritten and counted AGAIN in the same session"""
    from meryl_amd import capi, count
    if packed:
        monkeypatch.delenv("MGC_PACKED_BASES", raising=False)
    else:
        monkeypatch.setenv("MGC_PACKED_BASES", "0")
    cfg = capi.configure(k, dev_bases.numel(), 1 << 30)
    with count.Session(cfg, 0) as s:
        s.push_bases_device(dev_bases)
        s.count()
        if refill is not None:
            dev_bases.copy_(refill)
            torch.cuda.synchronize()                                   # (the session counts on a stream of its own)
            s.count()
        info = s.info()
        lo, hi, counts, _ = s.result_wide()
        prof = s.profile()
    # the profile reports the bytes really moved: the histogram stores the stream on top of reading the bases
    n = dev_bases.numel()
    if packed:
        assert prof.hist_bytes > n + 6 * (n // 16), "the packed path did not run"
    else:
        assert prof.hist_bytes == n
    return {"lo": lo, "hi": hi, "counts": counts, "instances": int(info.n_instances), "distinct": int(info.n_distinct),
            "per_file": np.asarray(list(info.file_instances), dtype=np.int64)}


def assert_same(got, want, what):
    assert got["instances"] == want["instances"], what
    assert got["lo"].size == want["lo"].size, what
    assert np.array_equal(got["lo"], want["lo"]) and np.array_equal(got["hi"], want["hi"]), what
    assert np.array_equal(got["counts"], want["counts"]), what
    assert np.array_equal(got["per_file"], want["per_file"]), what


def on_device(torch, bases, offset):
    """the bases at `offset` bytes past a 16-byte aligned address"""
    buf = torch.empty(bases.size + 32, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    d = buf[offset:offset + bases.size]
    d.copy_(torch.from_numpy(bases))
    assert d.data_ptr() % 16 == offset
    return d


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("r", RS)
def test_packed_stream_counts_match_oracle_and_ascii_path(torch_cuda, oracle_lib, monkeypatch, r, k):
    i = RS.index(r) + KS.index(k)
    offset, end = OFFSETS[i % 3], ENDS[(i // 3 + RS.index(r)) % 3]
    bases = make_input(N0 + r, k, end, seed=1000 * k + r, boundary=(RS.index(r) + 2 * KS.index(k)) % 4)
    want = oracle_count(oracle_lib, bases, k)
    assert want["counts"].max() > 20 and want["instances"] > N0 // 2
    d = on_device(torch_cuda, bases, offset)
    packed = device_count(torch_cuda, monkeypatch, d, k, True)
    ascii_ = device_count(torch_cuda, monkeypatch, d, k, False)
    assert packed["distinct"] == ascii_["distinct"] == want["lo"].size
    assert_same(packed, want, "packed stream against the oracle")
    assert_same(ascii_, want, "ASCII path against the oracle")
    assert_same(packed, ascii_, "packed stream against the ASCII path")


def test_second_input_in_one_session_reads_nothing_of_the_first(torch_cuda, oracle_lib, monkeypatch):
    """The session counts its device buffer again at every mgc_count: the buffer is overwritten with a different input between two
    counts of ONE session, whose packed stream still holds the first input's words when the second count starts.  Any word of it
    that the second count read would show as a k-mer of the first input (different genome, different invalid bytes)."""
    k, n = 21, N0 + 4097
    first = make_input(n, k, "whole", seed=7)
    second = make_input(n, k, "inside", seed=8)[::-1].copy()          # reversed: its separators and lower-case runs sit elsewhere too
    want = oracle_count(oracle_lib, second, k)
    d = on_device(torch_cuda, first, 8)
    got = device_count(torch_cuda, monkeypatch, d, k, True, refill=torch_cuda.from_numpy(second).cuda())
    assert_same(got, want, "second count of the session against the oracle")
    d.copy_(torch_cuda.from_numpy(first))
    ascii_ = device_count(torch_cuda, monkeypatch, d, k, False, refill=torch_cuda.from_numpy(second).cuda())
    assert_same(got, ascii_, "second count of the session against the ASCII path")


def test_packed_stream_below_the_fine_histogram(torch_cuda, oracle_lib, monkeypatch):
    """inputs under 2^22 bases take the plain histogram kernel, which stores the stream as well: three tiles and 17 bases"""
    for k in (21, 51):
        bases = make_input(N0, k, "inside", seed=k)[:3 * 4096 + 17].copy()
        want = oracle_count(oracle_lib, bases, k)
        d = on_device(torch_cuda, bases, 1)
        packed = device_count(torch_cuda, monkeypatch, d, k, True)
        ascii_ = device_count(torch_cuda, monkeypatch, d, k, False)
        assert_same(packed, want, "packed stream against the oracle")
        assert_same(packed, ascii_, "packed stream against the ASCII path")
