"""Hash-structured sub-buckets for the count stage's tests (pure numpy, no GPU).

The count kernels put a sub-bucket's suffixes into an LDS hash table with linear probing; the home slot is a multiplicative
(Fibonacci) hash of the suffix.  Random k-mers spread evenly over such a table, so random inputs never build a long probe chain.
This module SEARCHES the free tail bases of a k-mer for suffixes whose home slots fall into a small window of the table.

The guarantee.  Linear probing never places a key before its home slot.  m distinct keys whose homes lie in a window of w
consecutive slots end in m different slots at or after the window's first slot, so one of them sits at least m - 1 slots past the
window's start and its home is at most w - 1 slots past it: that key is at least m - w (we claim only m - w - 1) steps away
from its home -- in EVERY insertion order, the order of the GPU's atomics included.  Keys of other homes only lengthen the chain.

Every mirror below is a copy of one line of meryl_amd/csrc/mgc_finish.hip, named in its comment; a mirror takes the suffix as
(lo, hi) 64-bit halves (numpy uint64 arrays or Python ints) and the table size of the sub-bucket.
"""
from collections import namedtuple

import numpy as np

BASES = "ACTG"                                    # base codes A0 C1 T2 G3
CODE = {c: i for i, c in enumerate(BASES)}
M32 = 0xFFFFFFFF
M64 = 0xFFFFFFFFFFFFFFFF
FIB32 = 0x9E3779B1
FIB64 = 0x9E3779B97F4A7C15
MUR32 = 0x85EBCA6B
MIX64 = 0xD6E8FEB86659FD93

PROBE_MAX = 64                                    # hash_count_stream_kernel: probe steps of one key in the first launch
DCAP_STREAM = 1280                                # FIN_STREAM_DCAP
CAP_STREAM = 4094                                 # FIN_CAP_STREAM
CAP_HASH = 1536                                   # FIN_CAP_HASH


def encode(s):
    v = 0
    for ch in s:
        v = (v << 2) | CODE[ch]
    return v


def decode(v, n):
    return "".join(BASES[(int(v) >> (2 * (n - 1 - i))) & 3] for i in range(n))


def _u64(x):
    return np.asarray(x, dtype=np.uint64)


def _mul64(a, b):                                 # (a * b) mod 2^64 on uint64 arrays
    with np.errstate(over="ignore"):
        return _u64(a) * np.uint64(b)


def _log2(slots):
    assert slots > 0 and slots & (slots - 1) == 0
    return slots.bit_length() - 1


# ---- home slots ----

def home_fib32(lo, hi, slots, tag=0, low_bits=0):
    """hash_count_kernel:            hh[j] = (kk[j] * 0x9E3779B1u) >> sshift;
    hash_count_multi_kernel:      hh[j] = (comp[j] * 0x9E3779B1u) >> sshift;      comp = suffix | tag << low_bits (tag_keys)
    hash_count_stream_kernel<u32>: hh[j] = (comp[j] * 0x9E3779B1u) >> sshift;"""
    comp = (_u64(lo) | np.uint64(tag << low_bits)) & np.uint64(M32)
    return ((comp * np.uint64(FIB32)) & np.uint64(M32)) >> np.uint64(32 - _log2(slots))


def home_w64(lo, hi, slots):
    """hash_count_stream_kernel<u64> (W64):
    hh[j] = ((((u32)comp[j]) ^ ((u32)(comp[j] >> 32) * 0x85EBCA6Bu)) * 0x9E3779B1u) >> sshift;"""
    lo = _u64(lo)
    l32, h32 = lo & np.uint64(M32), lo >> np.uint64(32)
    x = (l32 ^ ((h32 * np.uint64(MUR32)) & np.uint64(M32))) & np.uint64(M32)
    return ((x * np.uint64(FIB32)) & np.uint64(M32)) >> np.uint64(32 - _log2(slots))


def home_countw(lo, hi, slots):
    """hash_countw_kernel:  mix = K16 ? (klo ^ (khi * 0xD6E8FEB86659FD93ull)) * 0x9E3779B97F4A7C15ull : klo * 0x9E3779B97F4A7C15ull;
    hh[j] = (u32)(mix >> 32) >> sshift;        (8-byte keys: hi == 0, where both forms agree)
    hash_count128_huge_body takes the same mix of (klo, khi)."""
    x = _u64(lo) ^ _mul64(hi, MIX64)
    return (_mul64(x, FIB64) >> np.uint64(32)) >> np.uint64(32 - _log2(slots))


def home_huge(lo, hi, slots):
    """hash_count_huge_body:  hh[j] = (u32)((sfx * 0x9E3779B97F4A7C15ull) >> 32) >> sshift;"""
    return (_mul64(lo, FIB64) >> np.uint64(32)) >> np.uint64(32 - _log2(slots))


def home_scalar(name, lo, hi, slots, tag=0, low_bits=0):
    """The same functions once more on Python integers (the host test compares the two statements)."""
    sh = 32 - _log2(slots)
    if name == "fib32":
        return ((((lo | (tag << low_bits)) & M32) * FIB32) & M32) >> sh
    if name == "w64":
        return ((((lo & M32) ^ (((lo >> 32) * MUR32) & M32)) * FIB32) & M32) >> sh
    if name == "countw":
        return ((((lo ^ ((hi * MIX64) & M64)) * FIB64) & M64) >> 32) >> sh
    if name == "huge":
        return (((lo * FIB64) & M64) >> 32) >> sh
    raise KeyError(name)


HASHES = {"fib32": home_fib32, "w64": home_w64, "countw": home_countw, "huge": home_huge}


# ---- table sizes ----

def slots_stream(n, table):
    """hash_count_stream_kernel slots_for: 256 up to 128 keys, else the power of two >= 2n, at most SLOTS (2048; the retry launch 8192)."""
    if 2 * n <= 256:
        return 256
    return min(1 << (2 * n - 1).bit_length(), table)


def slots_quarter(n, table=2048):
    """hash_count_kernel / hash_count_multi_kernel / hash_countw_kernel slots_for: the power of two >= n + n / 4, 256 .. SLOTS."""
    s = 256
    while s < n + n // 4 and s < table:
        s <<= 1
    return s


HUGE_SLOTS32, HUGE_SLOTS128 = 8192, 4096          # hash_count_huge_body (32-bit suffixes) / hash_count128_huge_body: fixed tables


# ---- the search ----

def prefix_len(min_top):
    """bases that fix the file (6 bits) and the sub-bucket (min_top bits) with one base to spare, as the neighbouring tests take it"""
    return (6 + min_top + 1) // 2 + 1


def split_suffix(kmers_lo, kmers_hi, low):
    """(lo, hi) halves of  kmer & ((1 << low) - 1)  for k-mers given as 64-bit halves"""
    lo, hi = _u64(kmers_lo), _u64(kmers_hi)
    if low >= 64:
        return lo, hi & np.uint64((1 << (low - 64)) - 1)
    return lo & np.uint64((1 << low) - 1), hi & np.uint64(0)


def colliding_tails(k, min_top, pre, m, home, width, slots, hash_name, seed=0, last=None, tag=0, enum_bases=10):
    """m distinct tails t (k - len(pre) bases each) such that the suffix of the k-mer pre + t -- kmer & ((1 << low) - 1) with
    low = 2k - 6 - min_top, the k-mer read in forward mode with A0 C1 T2 G3 -- has its home slot, under HASHES[hash_name] in a
    table of `slots` entries, inside the window home, home + 1, .. home + width - 1 (modulo slots).  pre holds at least the bases
    that fix file and sub-bucket (ceil((6 + min_top) / 2); prefix_len(min_top) by default in the cases below); last: the tail's
    last base (G keeps a k-mer whose first base is A canonical).  The last enum_bases bases are enumerated, the bases between
    pre and them drawn at random and drawn again until m tails are found.  Returns (tails, homes)."""
    low = 2 * k - 6 - min_top
    free = k - len(pre)
    assert 2 * len(pre) >= 6 + min_top and free >= 1 and 1 <= width < slots
    nf = min(free, enum_bases)
    rng = np.random.default_rng(seed)
    fn = HASHES[hash_name]
    tails, homes, seen = [], [], set()
    for _ in range(4096):
        mid = "".join(BASES[i] for i in rng.integers(0, 4, free - nf))
        base = encode(pre + mid) << (2 * nf)
        e = np.arange(1 << (2 * nf), dtype=np.uint64)
        if last is not None:
            e = e[(e & np.uint64(3)) == np.uint64(CODE[last])]
        # (the enumerated bases lie in the low 64 bits: nf <= 10)
        klo = np.uint64(base & M64) | e
        khi = np.uint64(base >> 64)
        slo, shi = split_suffix(klo, np.full(e.shape, khi, dtype=np.uint64), low)
        h = fn(slo, shi, slots, tag, low) if hash_name == "fib32" else fn(slo, shi, slots)
        hit = np.nonzero(((h - np.uint64(home)) & np.uint64(slots - 1)) < np.uint64(width))[0]
        for i in hit:
            t = mid + decode(e[i], nf)
            if t not in seen:
                seen.add(t)
                tails.append(t)
                homes.append(int(h[i]))
                if len(tails) == m:
                    return tails, np.array(homes, dtype=np.int64)
        if free == nf:
            break                                 # nothing left to draw again
    raise ValueError("only %d of %d tails with homes in [%d, %d) of %d slots" % (len(tails), m, home, home + width, slots))


def random_tails(n, length, seed, exclude=(), last=None):
    """n distinct random tails outside `exclude`"""
    rng = np.random.default_rng(seed)
    out, seen = [], set(exclude)
    while len(out) < n:
        t = "".join(BASES[i] for i in rng.integers(0, 4, length))
        if last is not None:
            t = t[:-1] + last
        if t not in seen:
            seen.add(t)
            out.append(t)
    return out


def suffix_homes(k, min_top, pre, tails, slots, hash_name, tag=0):
    """home slots of the k-mers pre + t, one Python integer at a time (home_scalar)"""
    low = 2 * k - 6 - min_top
    out = []
    for t in tails:
        s = encode(pre + t) & ((1 << low) - 1)
        out.append(home_scalar(hash_name, s & M64, s >> 64, slots, tag, low))
    return np.array(out, dtype=np.int64)


def window_of(homes, slots):
    """the narrowest window (start, width) of consecutive slots, modulo the table size, that holds every home"""
    hs = np.unique(np.asarray(homes, dtype=np.int64))
    if len(hs) == 1:
        return int(hs[0]), 1
    gaps = np.diff(np.concatenate([hs, [hs[0] + slots]]))
    i = int(np.argmax(gaps))                      # the window starts behind the widest gap
    start = int(hs[(i + 1) % len(hs)])
    return start, int(slots - gaps[i] + 1)


def pigeonhole_steps(m, width):
    """steps from its home that some key of m distinct ones needs at least, their homes in a window of `width` slots (see above)"""
    return m - width - 1


def linear_probe_max_steps(homes, slots):
    """Sequential linear probing of distinct keys with these home slots into an empty table: the largest number of steps
    ((hh + 1) & smask) any key takes beyond its home."""
    assert len(homes) < slots, "the table fills"
    nxt = list(range(slots))                      # nxt[p]: a slot at or after p (cyclically) that leads to the first free one
    worst = 0
    for h in homes:
        p = int(h)
        path = []
        while nxt[p] != p:                        # (p is free exactly when nxt[p] == p)
            path.append(p)
            p = nxt[p]
        for q in path:
            nxt[q] = p
        nxt[p] = (p + 1) & (slots - 1)
        worst = max(worst, (p - int(h)) & (slots - 1))
    return worst


# ---- the cases of tests/test_count_structured_keys.py (the host test checks every one of them) ----

# kernel: whose hash and slots_for; plen: bases of the prefix (None: prefix_len(min_top)); slots: the table the m colliding suffixes
# are built for; home < 0: counted from the table's end (-1: the last slot, so that the chain wraps to slot 0); last: see above;
# steps: the probe steps the case has to force (PROBE_MAX + 1 trips the stream kernel's bound)
Case = namedtuple("Case", "name kernel hash k min_top plen slots m home width last steps")

_S = PROBE_MAX + 1
CASES = [
    # hash_count_stream_kernel<u32>, k = 21 (MGC_HASH_STREAM=1).  c, d and e free the whole suffix (plen = the bases of file and
    # sub-bucket alone): sixteen free bits hold at most ~70 suffixes per eight slots of 8192, ten bits ~80 per twenty of 256.
    Case("stream_a", "stream", "fib32", 21, 16, None, 256, 100, 77, 1, "G", _S),
    Case("stream_b", "stream", "fib32", 21, 16, None, 256, 100, -1, 1, "G", _S),
    Case("stream_c", "stream", "fib32", 21, 18, 12, 8192, 110, 5000, 8, None, _S),
    Case("stream_d", "stream", "fib32", 21, 18, 12, 2048, 90, 1234, 1, None, _S),
    # twelve-bit suffixes: the plan gives the distinct-sized count at most 18 grouping bits, so twelve bits below them is k = 15
    Case("stream_e", "stream", "fib32", 15, 12, 9, 256, 100, 200, 20, None, _S),
    # hash_count_stream_kernel<u64>: 40- and 33-bit suffixes under the W64 hash
    Case("stream64_k31_a", "stream", "w64", 31, 16, None, 256, 100, 31, 1, "G", _S),
    Case("stream64_k31_b", "stream", "w64", 31, 16, None, 256, 100, -1, 1, "G", _S),
    Case("stream64_k28_a", "stream", "w64", 28, 17, None, 256, 100, 31, 1, "G", _S),
    Case("stream64_k28_b", "stream", "w64", 28, 17, None, 256, 100, -1, 1, "G", _S),
    # hash_count_multi_kernel: R = 1 counts a 120-key sub-bucket in 256 slots, R = 2 / 4 a range of two of them in 512
    Case("multi1_a", "quarter", "fib32", 21, 18, 12, 256, 100, 9, 1, "G", _S),
    Case("multi1_b", "quarter", "fib32", 21, 18, 12, 256, 100, -1, 1, "G", _S),
    Case("multi24_a", "quarter", "fib32", 21, 18, 12, 512, 100, 9, 1, "G", _S),
    Case("multi24_b", "quarter", "fib32", 21, 18, 12, 512, 100, -1, 1, "G", _S),
    # hash_count_kernel (one sub-bucket at a time), 20-bit suffixes
    Case("hash_a", "quarter", "fib32", 21, 16, None, 256, 100, 140, 1, "G", _S),
    Case("hash_b", "quarter", "fib32", 21, 16, None, 256, 100, -1, 1, "G", _S),
    Case("hash_600", "quarter", "fib32", 21, 16, 11, 1024, 300, 700, 1, None, 256),      # (a slot of 1024 holds 256 such suffixes ending in G)
    # hash_countw_kernel: 8-byte keys with 40-bit suffixes; K96 records with 84-bit ones (the high word is part of the mix)
    Case("countw_k31_a", "quarter", "countw", 31, 16, None, 256, 100, 3, 1, "G", _S),
    Case("countw_k31_b", "quarter", "countw", 31, 16, None, 256, 100, -1, 1, "G", _S),
    Case("countw_k31_600", "quarter", "countw", 31, 16, None, 1024, 300, -1, 1, "G", 256),
    Case("countw_k51_a", "quarter", "countw", 51, 12, None, 256, 100, 3, 1, "G", _S),
    Case("countw_k51_b", "quarter", "countw", 51, 12, None, 256, 100, -1, 1, "G", _S),
    Case("countw_k51_600", "quarter", "countw", 51, 12, None, 1024, 300, -1, 1, "G", 256),
    # the oversized path: 5000 distinct suffixes in 64 slots of the streaming kernels' fixed tables (a pass takes SLOTS / 2 distinct
    # suffixes -- HUGE_CAP32 / HUGE_CAP128 -- and leaves the rest of the suffix range to the next pass)
    Case("huge_k21", "huge", "huge", 21, 16, 11, HUGE_SLOTS32, 5000, HUGE_SLOTS32 - 32, 64, None, HUGE_SLOTS32 // 4),
    Case("huge_k40", "huge", "countw", 40, 12, None, HUGE_SLOTS128, 5000, HUGE_SLOTS128 - 32, 64, "G", HUGE_SLOTS128 // 4),
]
CASE = {c.name: c for c in CASES}


def case_plen(c):
    return c.plen if c.plen is not None else prefix_len(c.min_top)


def case_home(c):
    return c.home % c.slots


def case_tails(c, pre, seed=0):
    """the case's m colliding tails behind the prefix `pre` (case_plen(c) bases) and their home slots"""
    assert len(pre) == case_plen(c)
    return colliding_tails(c.k, c.min_top, pre, c.m, case_home(c), c.width, c.slots, c.hash, seed=seed, last=c.last)
