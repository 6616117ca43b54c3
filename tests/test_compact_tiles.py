"""Kept items on tile borders of the order-preserving compactions (count per tile, scan, emit at the tile's base): the value
filter of a lookup table and the run edges of -bed-runs (tiles of 2048 entries), the line starts, header lines and de-lined
copy of the FASTA filter (4096 bytes of text, 2048 lines) and homopolymer compression (4096 bytes).  Every case is exact
against the numpy / Python models the suite already has; the shapes are the smallest that put a kept item on the last slot
of one tile and the first of the next, leave a whole tile empty, or end one item before, on and after a border."""
import numpy as np
import pytest

from test_lookup_filter import cuda_bytes, restated_filter
from test_lookup_filter import windows as byte_windows
from test_lookup_report import process_sequence, restated_report, stream_of, windows

pytestmark = pytest.mark.gpu

TILE = 2048                                                                  # entries (value filter), positions (run edges), lines
TEXT_TILE = 4096                                                             # bytes of text (FASTA filter), of bases (compression)


# ---- value filter ------------------------------------------------------------------------------------------------------
def filter_patterns(n):
    """name -> which of n entries the value filter keeps"""
    i = np.arange(n)
    return {"none": np.zeros(n, dtype=bool), "all": np.ones(n, dtype=bool), "border": (i == TILE - 1) | (i == TILE),
            "empty_middle_tile": (i < TILE) | (i >= 2 * TILE), "alternating": i % 2 == 0}


@pytest.mark.parametrize("k", [21, 51])
def test_value_filter_on_tile_borders(native_lib, k):
    import torch
    from meryl_amd import lookup
    for n in (1, TILE - 1, TILE, TILE + 1, 3 * TILE + 5):
        i = np.arange(n, dtype=np.uint64)
        if k > 32:                                                           # {lo, hi}, ascending by (hi, lo)
            host = np.stack([(i & np.uint64(1)) * np.uint64(1 << 40) + i * np.uint64(7), i >> np.uint64(1)], axis=1)
        else:
            host = i * np.uint64(0x1F3D5B79) + np.uint64(3)                  # spread over the index's buckets, below 4^21
        keys = torch.from_numpy(host.view(np.int64).copy()).cuda()
        for name, keep in filter_patterns(n).items():
            vals = np.where(keep, 2 + np.arange(n) % 5, 1).astype(np.int32)  # min_value = 2 drops the ones
            with lookup.Lookup.from_device(keys, torch.from_numpy(vals).cuda(), k, min_value=2) as lk:
                got = lk.values(keys).cpu().numpy()
                assert np.array_equal(got, np.where(keep, vals, 0)), (k, n, name, np.nonzero(got != np.where(keep, vals, 0))[0][:10])
                assert (lk.info.n_kmers, lk.info.n_kmers_in_db) == (int(keep.sum()), n), (k, n, name)


# ---- run edges of -bed-runs --------------------------------------------------------------------------------------------
# per table: the runs [first hit, first position after the last hit) of its flags
RUNS = [[(TILE - 1, TILE + 12), (3000, 2 * TILE)],                           # begins on a tile's last position; ends on a border
        [(TILE, TILE + 1)],                                                  # begins at 2048, ends at 2049
        [(2000, TILE), (2 * TILE - 1, 2 * TILE + 1)],                        # ends at 2048; one edge on each side of a border
        [(TILE - 8, 2 * TILE + 4)]]                                          # spans the whole middle tile: no edge in it


def test_run_edges_on_tile_borders(native_lib):
    import torch
    from meryl_amd import lookup
    k = 21
    rng = np.random.default_rng(2048)
    seq = "".join(rng.choice(list("ACGT"), 2 * TILE + 700))                  # with its breaker: three tiles of positions
    canon = [min(f, r) for _, f, r in windows(seq, k)]
    assert len(set(canon)) == len(canon)                                     # a hit pattern is then exactly the chosen positions
    tables, lks = [], []
    for runs in RUNS:
        tab = {canon[p] for b, e in runs for p in range(b, e)}
        tables.append(tab)
        keys = torch.tensor(sorted(tab), dtype=torch.int64).cuda()
        lks.append(lookup.Lookup.from_device(keys, torch.ones(len(tab), dtype=torch.int32).cuda(), k))
    exist, _ = process_sequence(seq, k, tables, "presence", True)
    for t, runs in enumerate(RUNS):                                          # the model sees the edges where they were put
        flags = np.array(exist[t] + [False])
        edges = np.nonzero(flags[1:] != flags[:-1])[0] + 1
        assert edges.tolist() == [x for run in runs for x in run], t
    text, starts = stream_of([seq])
    bases = torch.from_numpy(np.frombuffer(text.encode(), dtype=np.uint8).copy()).cuda()
    labels = ["t%d" % t for t in range(len(RUNS))]
    got = lookup.report(lks, "bed-runs", ["s"], bases, starts, labels=labels)
    assert got == restated_report(["s"], [seq], k, tables, "bed-runs", labels)
    assert got.count(b"\n") == sum(map(len, RUNS))
    for t in range(len(RUNS)):                                               # one table, no labels: the "found in any table" flag
        assert lookup.report([lks[t]], "bed-runs", ["s"], bases, starts) == restated_report(["s"], [seq], k, [tables[t]], "bed-runs")
    for lk in lks:
        lk.close()


# ---- line starts, header lines and the de-lined copy of the FASTA filter ----------------------------------------------
def fasta_border_texts(rng):
    """name -> FASTA text; every second record is of the table's genome (see the test)"""
    rand = lambda n: bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), n))
    own = rand(6000)
    body = lambda j, n: own[(37 * j) % 5000:(37 * j) % 5000 + n] if j % 2 == 0 else rand(n)
    head = b">r0\n"
    texts = {
        # text[4095] and text[4096] are newlines: the last line start of one tile and the first of the next
        "newlines_4095_4096": head + body(0, TEXT_TILE - 1 - len(head)) + b"\n\n" + b">r1\n" + body(1, 50) + b"\n>r2\n" + body(2, 50) + b"\n",
        "len_4096": head + body(0, TEXT_TILE - 1 - len(head)) + b"\n",
        "len_4096_open": head + body(0, TEXT_TILE - len(head)),
        "len_4097": head + body(0, TEXT_TILE - len(head)) + b"\n",
        "len_4097_open": head + body(0, TEXT_TILE - 1 - len(head)) + b"\nA",
    }
    # more than 2048 lines; lines 2047 and 2048 are header lines (the first of them an empty record)
    lines = [b">first", body(0, 40), body(0, 33)]
    j = 1
    while len(lines) < TILE - 1:
        lines += [b">r%d" % j, body(j, 30 + j % 17)]
        j += 1
    assert len(lines) == TILE - 1
    lines += [b">empty", b">after", body(j, 45)]
    for j in range(j + 1, j + 6):
        lines += [b">r%d some words" % j, body(j, 41), body(j, 7)]
    texts["headers_2047_2048"] = b"\n".join(lines)                          # (unterminated last line)
    assert lines[TILE - 1][:1] == b">" and lines[TILE][:1] == b">" and len(lines) > TILE
    # a header line longer than two tiles of text: a tile whose de-lined copy is empty
    texts["long_header"] = (b">a\n" + body(0, 100) + b"\n>b " + b"x" * (2 * TEXT_TILE + 900) + b"\n" + body(2, 60) + b"\n" + body(2, 25) +
                            b"\n>c\n" + body(3, 70) + b"\n")
    return own, texts


def test_fasta_filter_on_tile_borders(native_lib):
    import torch
    from meryl_amd import lookup
    k = 21
    own, texts = fasta_border_texts(np.random.default_rng(4096))
    table = {min(f, r) for _, f, r in byte_windows(own, k)}
    keys = torch.tensor(sorted(table), dtype=torch.int64).cuda()
    assert texts["newlines_4095_4096"][TEXT_TILE - 1:TEXT_TILE + 1] == b"\n\n"
    assert [len(texts[x]) for x in ("len_4096", "len_4096_open", "len_4097", "len_4097_open")] == [4096, 4096, 4097, 4097]
    with lookup.Lookup.from_device(keys, torch.ones(len(table), dtype=torch.int32).cuda(), k) as lk:
        for name, text in texts.items():
            dev = [cuda_bytes(text)]
            kept_both = 0
            for mode in ("include", "exclude"):
                want, n, kept = restated_filter([text], k, table, ("compact", name), mode == "include", 0)
                got, res = lookup.filter_text(lk, mode, dev)
                assert (res.n_records, res.n_kept) == (n, kept), (name, mode)
                assert got[0] == want[0], (name, mode)
                assert res.consumed[0] == len(text) and res.out_bytes[0] == len(want[0])
                kept_both += kept
            assert kept_both == n                                            # the two outputs hold every record's bases once
        # the many-record text really has records on both sides
        _, n, kept = restated_filter([texts["headers_2047_2048"]], k, table, ("compact", "headers_2047_2048"), True, 0)
        assert n > 1024 and n / 4 < kept < 3 * n / 4


# ---- homopolymer compression --------------------------------------------------------------------------------------------
def test_homopoly_compress_on_tile_borders(native_lib, oracle_lib):
    import torch
    from meryl_amd import count
    for n in (TEXT_TILE - 1, TEXT_TILE, TEXT_TILE + 1, 3 * TEXT_TILE + 1):
        streams = {"one_base": b"A" * n,                                     # one byte kept, then tiles with none
                   "no_repeats": (b"ACGT" * (n // 4 + 1))[:n]}               # everything kept
        for name, s in streams.items():
            want = oracle_lib.compress_stream(s)
            assert len(want) == (1 if name == "one_base" else n)
            for off in range(4):                                             # the input pointer 0..3 bytes past a 16-byte boundary
                big = torch.from_numpy(np.frombuffer(b"." * off + s, dtype=np.uint8).copy()).cuda()
                got = count.dev_homopoly_compress(big[off:]).cpu().numpy().tobytes()
                assert got == want, (n, name, off)
