"""Inputs and cases of tests/test_group_wide_edges.py: the whole-key grouping passes (mgc_sort.hip, launch_group_wide) at their
tile, region and digit edges.  No GPU needed: tests/test_wide_edge_helpers_host.py checks that the edges really are in the inputs.

An input is n sequences of exactly k bases joined by `.`, counted forward: every sequence is one k-mer, and all of them lie in one
file.  The k-mers are built AS INTEGERS first (two 64-bit words, hi above lo; 2 bits per base, A = 0, C = 1, T = 2, G = 3) and the
text is written from them.  From the top of the 2k bits: the file (6 bits), the high digit (bA bits), the low digit (bB bits),
then random bits -- a plan of t grouping bits splits them into a low digit of ceil(t / 2) and a high one of floor(t / 2) bits
(make_sort_plan), and the high-digit-first passes take the high one first.  One k-mer in four draws what lies below the digits
from two values only, so that counts above one are plenty.

`compress` inputs repeat no base (compression leaves them as they are) and are built from dense ranks: a base that may not repeat
the one before it is one of three, d = c - (c > previous), and five of them make a digit 0..242 (mgc_common.hpp, hpc_digit)."""
from typing import NamedTuple, Optional

import numpy as np

FORWARD = 1
FILE = 0b100111                                                     # `TCG`: the one file of every input (it repeats no base)
FILE_BITS = 6
LETTERS = np.frombuffer(b"ACTG", dtype=np.uint8)
M64 = np.uint64(0xFFFFFFFFFFFFFFFF)

# keys per tile of the whole-key instantiations (tests/test_group_route_host.py pins them against mgc_group_route.hpp), and keys
# per 16-byte load of a lane's fetch
TILE = {"u64": 16384, "k96": 12288, "k128": 8192}
VEC = {"u64": 2, "k96": 4, "k128": 1}
# 196608 = 12 * 16384 = 16 * 12288 = 24 * 8192: a tile short by one key, a full last tile, a last tile of one key -- for all three
N_EDGES = (196607, 196608, 196609)
N_ODD = 196609


class Kind(NamedTuple):
    name: str
    k: int
    layout: str                                                     # u64 (k = 24..32), k96 (12-byte records, k = 33..51), k128
    env: dict


KINDS = {x.name: x for x in (
    Kind("u64", 31, "u64", {}),
    Kind("u64_k26", 26, "u64", {}),
    Kind("k96", 51, "k96", {}),                                     # 96 bits below the file: the record's every bit
    Kind("k96_k40", 40, "k96", {}),                                 # 74 bits: the top word of the record mostly empty
    Kind("k128", 64, "k128", {}),
    Kind("k128_k51", 51, "k128", {"MGC_K96": "0"}),
)}


class Plan(NamedTuple):
    name: str
    hi_bits: int                                                    # the plan's pass_bits[1]: the high digit (a `compress` rank: its ten-bit field)
    lo_bits: int                                                    # pass_bits[0]
    env: dict

    @property
    def t(self):
        return self.hi_bits + self.lo_bits

    @property
    def widths(self):                                               # mgc_profile.wide_digit_widths of one file on this plan
        return (1 << self.hi_bits) | (1 << (16 + self.lo_bits))


# CountPlan::plan_top: the smallest t with (n >> t) <= MGC_FINISH_TARGET, at least MGC_FINISH_MIN_TOP.  For every n of 131072 ..
# 212991: target 12 -> 14, target 3 -> 16, target 1 -> 17.
# `compress` (dense-rank digits): 243 * target < n <= 59049 * target -> two ranks, twenty bits; MGC_HASH_STREAM=1 and 19683 * 3 <= n <=
# 19683 * 10 with target 10 -> the mixed plan: a rank above the plain eight bits of four bases (plan_hpc_kind).
PLANS = {x.name: x for x in (
    Plan("t14", 7, 7, {"MGC_FINISH_TARGET": "12"}),
    Plan("t16", 8, 8, {"MGC_FINISH_TARGET": "3"}),
    Plan("t17", 8, 9, {"MGC_FINISH_TARGET": "1"}),
    Plan("t18", 9, 9, {"MGC_FINISH_TARGET": "1", "MGC_FINISH_MIN_TOP": "18"}),
    Plan("hpc1", 10, 10, {"MGC_FINISH_TARGET": "4"}),
    Plan("mixed", 10, 8, {"MGC_FINISH_TARGET": "10", "MGC_HASH_STREAM": "1"}),
)}


class Input(NamedTuple):
    shape: str
    kind: str
    n: int
    hi_bits: int = 0                                                # where the shape puts its digits (0: nowhere, the digits are random)
    lo_bits: int = 0


class Case(NamedTuple):
    name: str
    group: str
    inp: Input
    plan: str
    env: dict                                                       # beyond the kind's and the plan's
    msd: bool = True                                                # False: MGC_WIDE_MSD=0, the low-digit-first fallback
    stream: bool = False                                            # the distinct-sized count takes the file
    compress: bool = False

    @property
    def kind(self):
        return KINDS[self.inp.kind]

    @property
    def k96(self):                                                  # (`compress` never lays a file as K96 records: CountPlan::k96_layout)
        return self.kind.layout == "k96" and self.msd and not self.compress

    def environ(self):
        e = dict(self.kind.env)
        e.update(PLANS[self.plan].env)
        if self.kind.k <= 32 and "MGC_HASH_STREAM" not in e:        # (the coarser distinct-sized plan could take a grouping bit away)
            e["MGC_HASH_STREAM"] = "2"
        e.update(self.env)
        if not self.msd:
            e["MGC_WIDE_MSD"] = "0"
        return e


# ---- integers <-> text --------------------------------------------------------------------------------------------------------

def field(hi, lo, shift, width):
    """bits [shift, shift + width) of the two-word integers (width <= 32)"""
    m = np.uint64((1 << width) - 1)
    if shift >= 64:
        return (hi >> np.uint64(shift - 64)) & m
    if shift + width <= 64 or shift == 0:
        return (lo >> np.uint64(shift)) & m
    return ((lo >> np.uint64(shift)) | (hi << np.uint64(64 - shift))) & m


def compose(k, top, top_bits, rng, few):
    """k-mers whose top `top_bits` bits are `top`; the bits below random -- where `few` is set, one of two values"""
    n = top.size
    s = 2 * k - top_bits
    top = top.astype(np.uint64)
    rest_lo = rng.integers(0, 1 << 63, size=n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=n, dtype=np.uint64)
    rest_hi = rng.integers(0, 1 << 63, size=n, dtype=np.uint64)
    rest_lo[few] = rng.integers(0, 2, size=int(few.sum()), dtype=np.uint64)
    rest_hi[few] = 0
    if s >= 64:
        rest_hi &= np.uint64((1 << (s - 64)) - 1)
        return (top << np.uint64(s - 64)) | rest_hi, rest_lo
    rest_lo &= np.uint64((1 << s) - 1)
    return top >> np.uint64(64 - s), ((top << np.uint64(s)) & M64) | rest_lo


def codes_of(k, hi, lo):
    """(n, k) 2-bit codes, first base first"""
    c = np.empty((hi.size, k), dtype=np.uint8)
    for i in range(k):
        c[:, i] = field(hi, lo, 2 * (k - 1 - i), 2)
    return c


def keys_of_codes(c):
    n, k = c.shape
    hi = np.zeros(n, dtype=np.uint64)
    lo = np.zeros(n, dtype=np.uint64)
    for i in range(k):
        hi = (hi << np.uint64(2)) | (lo >> np.uint64(62))
        lo = (lo << np.uint64(2)) | c[:, i].astype(np.uint64)
    return hi, lo


def text_of(k, hi, lo):
    a = np.full((hi.size, k + 1), ord("."), dtype=np.uint8)
    a[:, :k] = LETTERS[codes_of(k, hi, lo)]
    return a.reshape(-1)


def keys_of_text(k, text):
    """the inverse of text_of, stated on its own: every (k + 1)-th byte a `.`, the letters looked up one by one"""
    a = text.reshape(-1, k + 1)
    assert (a[:, k] == ord(".")).all()
    code = np.full(256, 255, dtype=np.uint8)
    for v, ch in enumerate("ACTG"):
        code[ord(ch)] = v
    c = code[a[:, :k]]
    assert (c < 4).all()
    return keys_of_codes(c)


def unique_ref(hi, lo):
    """sorted distinct k-mers and their counts: np.unique for two words"""
    order = np.lexsort((lo, hi))
    h, l = hi[order], lo[order]
    first = np.ones(h.size, dtype=bool)
    first[1:] = (h[1:] != h[:-1]) | (l[1:] != l[:-1])
    at = np.flatnonzero(first)
    return h[at], l[at], np.diff(np.append(at, h.size)).astype(np.uint32)


# ---- digits ---------------------------------------------------------------------------------------------------------------------

def planted_sizes(tile):
    """high-digit value -> keys, in the order the regions lie; every other value but 0 and the highest takes what the generator gives it"""
    return {1: tile + 1, 2: 0, 3: 1, 4: tile - 1, 5: tile, 6: 0, 7: 2 * tile + 3}


PLANTED_AHEAD = 1001                                                # keys of high digit 0: odd, and 1 mod 4 -- see planted_starts


def planted_starts(tile):
    """key index at which the region of each planted high-digit value starts.  With 1001 keys ahead: the TILE + 1 region starts at
    1001, the TILE - 1 region at 1001 + TILE + 2 -- odd both, 1 and 3 mod 4: off a 16-byte boundary as 8-byte and as 12-byte keys"""
    at, out = PLANTED_AHEAD, {}
    for v, c in planted_sizes(tile).items():
        out[v] = at
        at += c
    return out


def planted_high(n, top_value, tile, rng):
    """n high digits: the planted regions, 1001 keys of digit 0, five of the highest value, the rest spread over the values between"""
    parts = [np.full(c, v, dtype=np.uint64) for v, c in planted_sizes(tile).items()]
    parts.append(np.zeros(PLANTED_AHEAD, dtype=np.uint64))
    parts.append(np.full(5, top_value, dtype=np.uint64))
    left = n - sum(p.size for p in parts)
    assert left > 0
    parts.append(rng.integers(8, top_value + 1, size=left, dtype=np.uint64))
    a = np.concatenate(parts)
    rng.shuffle(a)
    return a


NINTH = (256, 384, 511)                                             # the ninth bit with none, some and all of the others


def plain_digits(inp, rng):
    """(A, B): the high and the low digit of every key"""
    n, ba, bb = inp.n, inp.hi_bits, inp.lo_bits
    if inp.shape == "random":
        return None, None
    a = rng.integers(0, 1 << ba, size=n, dtype=np.uint64)
    b = rng.integers(0, 1 << bb, size=n, dtype=np.uint64)
    i = np.arange(n)
    if inp.shape == "planted":
        a = planted_high(n, (1 << ba) - 1, TILE[KINDS[inp.kind].layout], rng)
    elif inp.shape == "ones_hi":                                    # one region of n keys; every first-pass tile one run
        a[:] = (1 << ba) - 1
    elif inp.shape == "one_lo":                                     # every second-pass tile one run; one counter of the low digit's histogram
        b[:] = 0x155 & ((1 << bb) - 1)
    elif inp.shape == "alt_hi":
        a = np.where(i % 2 == 0, 0, (1 << ba) - 1).astype(np.uint64)
    elif inp.shape == "ninth_hi":
        assert ba == 9
        a = np.array(NINTH, dtype=np.uint64)[i % 3]
    elif inp.shape == "ninth_lo":
        assert bb == 9
        b = np.array(NINTH, dtype=np.uint64)[i % 3]
    else:
        raise ValueError(inp.shape)
    return a, b


def hpc_digit(x):
    """mgc_common.hpp, hpc_digit, restated: x = 12 key bits, the top two the base before the five; d = c - (c > previous), base 3"""
    x = np.asarray(x, dtype=np.uint64)
    prev = (x >> np.uint64(10)) & np.uint64(3)
    d = np.zeros(x.shape, dtype=np.uint64)
    for i in range(5):
        c = (x >> np.uint64(8 - 2 * i)) & np.uint64(3)
        d = d * np.uint64(3) + (c - (c > prev).astype(np.uint64))
        prev = c
    return d


def hpc_keys(inp, rng):
    """k-mers of file `TCG` that repeat no base: a dense rank (five ternary choices) right below the file -- planted or random --
    and ternary choices below it"""
    kind = KINDS[inp.kind]
    n, k = inp.n, kind.k
    if inp.shape == "hpc_planted":
        rank = planted_high(n, 242, TILE[kind.layout], rng)
    else:
        assert inp.shape == "hpc_random"
        rank = rng.integers(0, 243, size=n, dtype=np.uint64)
    d = rng.integers(0, 3, size=(n, k), dtype=np.uint8)
    few = np.arange(n) % 4 == 0
    d[few, 13:] = 0                                                 # (below the two ranks: one of three values)
    d[few, k - 1] = rng.integers(0, 3, size=int(few.sum()), dtype=np.uint8)
    for j in range(5):
        d[:, 3 + j] = (rank // np.uint64(3 ** (4 - j))) % np.uint64(3)
    c = np.empty((n, k), dtype=np.uint8)
    for j in range(3):
        c[:, j] = (FILE >> (4 - 2 * j)) & 3
    for j in range(3, k):
        c[:, j] = d[:, j] + (d[:, j] >= c[:, j - 1])
    return keys_of_codes(c)


class Built(NamedTuple):
    k: int
    hi: np.ndarray
    lo: np.ndarray
    a: Optional[np.ndarray]                                         # the high digits the shape asked for (None: random)
    b: Optional[np.ndarray]


def _seed(inp):
    return [KINDS[inp.kind].k, inp.n, inp.hi_bits, inp.lo_bits] + [ord(ch) for ch in inp.shape]


def build(inp):
    kind = KINDS[inp.kind]
    k = kind.k
    rng = np.random.default_rng(_seed(inp))
    if inp.shape.startswith("hpc_"):
        hi, lo = hpc_keys(inp, rng)
        return Built(k, hi, lo, None, None)
    few = np.arange(inp.n) % 4 == 0
    a, b = plain_digits(inp, rng)
    if a is None:                                                   # eighteen random bits below the file: the digits of every plan
        top = (np.uint64(FILE) << np.uint64(18)) | rng.integers(0, 1 << 18, size=inp.n, dtype=np.uint64)
        hi, lo = compose(k, top, FILE_BITS + 18, rng, few)
    else:
        top = (((np.uint64(FILE) << np.uint64(inp.hi_bits)) | a) << np.uint64(inp.lo_bits)) | b
        hi, lo = compose(k, top, FILE_BITS + inp.hi_bits + inp.lo_bits, rng, few)
    return Built(k, hi, lo, a, b)


def digits_of(k, hi, lo, plan):
    """the two digits of every key as the plan's passes see them: bit fields, or dense ranks of the twelve bits at the field"""
    p = PLANS[plan]
    low = 2 * k - FILE_BITS - p.t
    if p.name == "hpc1":
        return hpc_digit(field(hi, lo, low + 10, 12)), hpc_digit(field(hi, lo, low, 12))
    if p.name == "mixed":
        return hpc_digit(field(hi, lo, low + 8, 12)), field(hi, lo, low, 8)
    return field(hi, lo, low + p.lo_bits, p.hi_bits), field(hi, lo, low, p.lo_bits)


# ---- the cases ------------------------------------------------------------------------------------------------------------------

def _plain(shape, kind, n, plan):
    p = PLANS[plan]
    return Input(shape, kind, n) if shape == "random" else Input(shape, kind, n, p.hi_bits, p.lo_bits)


def _cases():
    out = []

    def add(group, shape, kind, n, plan, env=None, **kw):
        compress = shape.startswith("hpc_")
        inp = Input(shape, kind, n) if compress else _plain(shape, kind, n, plan)
        env = env or {}
        name = "-".join([group, shape, kind, str(n), plan] + ["%s=%s" % kv for kv in env.items()] + ([] if kw.get("msd", True) else ["lsd"]))
        out.append(Case(name, group, inp, plan, env, compress=compress, **kw))

    # 1. first-pass tile edges, random digits (cases that share an input stand together: the module keeps one input at a time)
    for kind in ("u64", "k96", "k96_k40", "k128", "k128_k51"):
        for n in N_EDGES:
            for plan in ("t16", "t18"):
                add("edge", "random", kind, n, plan)
            if kind == "u64" and n == N_ODD:                        # the distinct-sized count on the same sixteen bits
                add("edge", "random", kind, n, "t16", {"MGC_HASH_STREAM": "1"}, stream=True)
    add("edge", "random", "u64_k26", N_ODD, "t14")                 # (sixteen top bits would leave 30 below them: a narrowed file)
    # 2. planted regions for the second pass; 5. the same input with the low digit first
    for kind in ("u64", "k96", "k96_k40", "k128", "k128_k51"):
        for plan in (("t16", "t17", "t18") if kind == "u64" else ("t16", "t18")):
            add("planted", "planted", kind, N_ODD, plan)
            if plan == "t16":
                add("fallback", "planted", kind, N_ODD, plan, msd=False)
    # 3. digit extremes
    for kind in ("u64", "k96", "k128"):
        for shape, plan in (("ones_hi", "t16"), ("alt_hi", "t16"), ("one_lo", "t18"), ("ninth_hi", "t18"), ("ninth_lo", "t18")):
            add("extreme", shape, kind, N_ODD, plan)
    add("extreme", "ones_hi", "u64", N_ODD, "t17")                  # 255 of an eight-bit digit among 512 counters
    add("extreme", "ninth_lo", "u64", N_ODD, "t17")
    # 4. `compress`: sequences that repeat no base
    for n in N_EDGES:
        add("compress", "hpc_random", "u64", n, "hpc1", {"MGC_HASH_STREAM": "2"})
        add("compress", "hpc_random", "u64", n, "mixed", stream=True)
        add("compress", "hpc_random", "k128", n, "hpc1")
    add("compress", "hpc_random", "k96", N_ODD, "hpc1")            # k = 51: 16-byte keys all the same
    add("compress", "hpc_planted", "u64", N_ODD, "hpc1", {"MGC_HASH_STREAM": "2"})
    add("compress", "hpc_planted", "u64", N_ODD, "mixed", stream=True)
    add("compress", "hpc_planted", "k128", N_ODD, "hpc1")
    return out


CASES = _cases()
INPUTS = sorted(set((c.inp, c.compress) for c in CASES))
