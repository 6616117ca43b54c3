"""BAM input decoded on the device: the decode kernel against a numpy model (mgc_dev_bam_decode), and the session route
(mgc_begin_bam / mgc_push_bam / mgc_end_bam, mgc_push_bam_file) against the same bases given to push_bases_device.

The BAM bytes are written here and by tests/test_seq_bam.py's writer, from the SAM specification (SAMv1 4.1 BGZF, 4.2 BAM)."""
import ctypes
import gzip
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
from test_seq_bam import NT16, bam_bytes, bgzf, bgzf_block, random_records  # noqa: E402

pytestmark = pytest.mark.gpu

TILE = 4096                                                  # output bytes per workgroup of the decode kernel
LDS_SEGS = 512                                               # segments of a tile it stages in LDS
DOT = 1 << 31
L_SEQS = (0, 1, 2, 3, 15, 16, 17, 31, 32, 33)
LETTERS = np.frombuffer(NT16.encode(), dtype=np.uint8)
SEG = np.dtype([("src_off", "<u4"), ("nbf", "<u4"), ("out_off", "<u8")])


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


# ---- the model ---------------------------------------------------------------------------------------------------------
def build_piece(specs, seed):
    """specs: [(n_bases, dot, pad)] -> (piece uint8[], table SEG[], out_total): `pad` bytes of noise, then the segment's packed
    bases (random codes; the low nibble of a last odd byte is noise too), one after the other"""
    rng = np.random.default_rng(seed)
    parts, table, at, out = [], np.zeros(len(specs), dtype=SEG), 0, 0
    for i, (nb, dot, pad) in enumerate(specs):
        parts.append(rng.integers(0, 256, pad, dtype=np.uint8))
        at += pad
        table[i] = (at, nb | (DOT if dot else 0), out)
        parts.append(rng.integers(0, 256, (nb + 1) // 2, dtype=np.uint8))
        at += (nb + 1) // 2
        out += nb + (1 if dot else 0)
    parts.append(rng.integers(0, 256, 3, dtype=np.uint8))
    return np.concatenate(parts), table, out


def expand(piece, table):
    """what the table says of the piece, in numpy: SAMv1 4.2, high nibble first, '.' after a flagged segment"""
    out = []
    for src, nbf, _ in table.tolist():
        nb = nbf & (DOT - 1)
        b = piece[src:src + (nb + 1) // 2]
        codes = np.empty(2 * b.size, dtype=np.uint8)
        codes[0::2] = b >> 4
        codes[1::2] = b & 15
        out.append(LETTERS[codes[:nb]])
        if nbf & DOT:
            out.append(np.frombuffer(b".", dtype=np.uint8))
    return np.concatenate(out) if out else np.zeros(0, np.uint8)


def decode_on_device(torch, piece, table, out_total, shift=0, guard=64):
    """mgc_dev_bam_decode into a buffer `shift` bytes past a 16-byte boundary -> (output, guards untouched)"""
    from meryl_amd import capi
    d_piece = torch.from_numpy(piece.copy()).cuda()
    d_tab = torch.from_numpy(np.frombuffer(table.tobytes(), dtype=np.uint8).copy()).cuda()
    buf = torch.full((guard + 16 + out_total + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0 and d_tab.data_ptr() % 16 == 0
    first = guard + shift
    torch.cuda.synchronize()
    capi.check(capi.lib().mgc_dev_bam_decode(ctypes.c_void_p(d_piece.data_ptr()), piece.size, ctypes.c_void_p(d_tab.data_ptr()), len(table),
                                             out_total, ctypes.c_void_p(buf.data_ptr() + first), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)),
               "mgc_dev_bam_decode")
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    untouched = bool((h[:first] == 0xA5).all() and (h[first + out_total:] == 0xA5).all())
    return h[first:first + out_total], untouched


def check_case(torch, specs, seed, shifts=(0,)):
    piece, table, out_total = build_piece(specs, seed)
    want = expand(piece, table)
    assert want.size == out_total
    for shift in shifts:
        got, untouched = decode_on_device(torch, piece, table, out_total, shift)
        assert np.array_equal(got, want), (specs[:4], shift, int(np.argmax(got != want)) if got.size else -1)
        assert untouched, (specs[:4], shift)


# ---- 1. the kernel against the model -----------------------------------------------------------------------------------
def test_kernel_one_segment_of_each_short_length(torch_cuda):
    for i, n in enumerate(L_SEQS):
        check_case(torch_cuda, [(n, True, 5)], 100 + i, shifts=(0, 7))
    check_case(torch_cuda, [(n, True, 1 + i) for i, n in enumerate(L_SEQS)], 120, shifts=(0, 13))


def test_kernel_more_empty_records_than_a_tile_holds_in_lds(torch_cuda):
    # 5000 '.'-only segments in a row: one tile's slice of the table is 4096 segments (> LDS_SEGS: read from global memory) and a
    # thread's sixteen bytes come from sixteen segments
    assert 5000 > TILE > LDS_SEGS
    specs = [(150, True, 36)] * 3 + [(0, True, 36)] * 5000 + [(151, True, 36)] * 3
    check_case(torch_cuda, specs, 130, shifts=(0, 9))


def test_kernel_segments_that_end_around_a_tile_border(torch_cuda):
    for end in (TILE - 1, TILE, TILE + 1):
        check_case(torch_cuda, [(end - 1, True, 3), (40, True, 36)], 140 + end)                        # the '.' of the first closes at `end`
        check_case(torch_cuda, [(end - 1, True, 3)], 150 + end, shifts=(0, 1))                         # ... and nothing follows
        check_case(torch_cuda, [(100, True, 2), (end - 101, True, 36), (7, True, 36)], 160 + end, shifts=(0, 15))
    check_case(torch_cuda, [(TILE, False, 3)], 169)                                                    # an unflagged (even) segment fills the tile


def test_kernel_a_segment_of_three_tiles_and_five_bases(torch_cuda):
    check_case(torch_cuda, [(3 * TILE + 5, True, 11)], 170, shifts=(0, 1, 8))
    check_case(torch_cuda, [(33, True, 36), (3 * TILE + 5, True, 37), (2, True, 36)], 171, shifts=(5,))


def test_kernel_unflagged_segments_of_a_straddling_seq(torch_cuda):
    # the first piece of a straddle ends with an unflagged, even segment; the next piece begins with the continuation at offset 0
    check_case(torch_cuda, [(150, True, 36), (64, False, 40)], 180, shifts=(0, 3))
    check_case(torch_cuda, [(87, True, 0), (150, True, 236)], 181, shifts=(0, 3))
    check_case(torch_cuda, [(2 * TILE, False, 0)], 182, shifts=(0, 6))


def test_kernel_source_at_every_byte_alignment(torch_cuda):
    specs, at = [], 0
    for r in range(16):
        pad = (r - at) % 16 + 16
        nb = 45 + 2 * r + (r % 2)
        specs.append((nb, True, pad))
        at += pad + (nb + 1) // 2
    piece, table, _ = build_piece(specs, 190)
    assert sorted(int(s) % 16 for s in table["src_off"]) == list(range(16))
    check_case(torch_cuda, specs, 190, shifts=(0, 4))


def test_kernel_output_at_every_byte_alignment_leaves_its_neighbours_alone(torch_cuda):
    specs = [(150, True, 36), (0, True, 36), (1, True, 36), (301, True, 36)] * 9 + [(TILE + 17, True, 36), (20, False, 36)]
    check_case(torch_cuda, specs, 200, shifts=tuple(range(16)))
    check_case(torch_cuda, [(1, True, 0)], 201, shifts=tuple(range(16)))                               # two bytes of output in all
    check_case(torch_cuda, [(0, True, 0)], 202, shifts=tuple(range(16)))


# ---- the session ------------------------------------------------------------------------------------------------------
def stream_of(records):
    return "".join(s + "." for _, _, s in records).encode()


def count_of_stream(ops, torch, cfg, stream):
    d = torch.from_numpy(np.frombuffer(stream, dtype=np.uint8).copy()).cuda()
    with ops.Session(cfg) as s:
        s.push_bases_device(d)
        s.count()
        return s.result_wide(), s.info().n_instances


def test_stream_is_the_concatenation_of_everything_pushed(ops, torch_cuda, tmp_path):
    from meryl_amd import capi
    recs = random_records(400, 31)
    raw = bam_bytes(recs)
    bam_stream = stream_of(recs)
    fq_reads = ["ACGTTGCAAGGCTTAACCGGTTAAC", "TTGACCA", "GGGGGCCCCCAAAAATTTTTACGTACGTAGCATCGATCAGCTAC"]
    fq = "".join("@q%d\n%s\n+\n%s\n" % (i, r, "I" * len(r)) for i, r in enumerate(fq_reads))
    files = []
    for block in (300, 0xff00):
        p = tmp_path / ("x%d.bam" % block)
        p.write_bytes(bgzf(raw, block))
        files.append(p)
    # (the text parser writes its '.' where a record STARTS, and mgc_end_text one more after the last: mgc_parse.hip)
    want = b"ACGTA" + bam_stream + ("".join("." + r for r in fq_reads) + ".").encode() + bam_stream + bam_stream
    cfg = capi.configure(21, len(want), 2 << 30)
    with ops.Session(cfg) as s:
        s.push_bases("ACGTA", end_of_sequence=False)                                   # the BAM begins at an odd stream offset
        L = capi.lib()
        capi.check(L.mgc_begin_bam(s._h), "mgc_begin_bam", s._h)
        for what in (lambda: L.mgc_push_bases(s._h, b"A", 1, 1), lambda: L.mgc_begin_text(s._h, 1), lambda: L.mgc_count(s._h),
                     lambda: L.mgc_push_text(s._h, b">a\n", 3), lambda: L.mgc_end_text(s._h),
                     lambda: L.mgc_staged_bases(s._h, ctypes.byref(ctypes.c_void_p()), ctypes.byref(ctypes.c_uint64()))):
            assert what() == capi.ESTATE                                               # one open file, and it is a BAM
        for i in range(0, 2000):
            capi.check(L.mgc_push_bam(s._h, raw[i:i + 1], 1), "mgc_push_bam", s._h)
        for i in range(2000, len(raw), 4099):
            piece = raw[i:i + 4099]
            capi.check(L.mgc_push_bam(s._h, piece, len(piece)), "mgc_push_bam", s._h)
        capi.check(L.mgc_end_bam(s._h), "mgc_end_bam", s._h)
        assert L.mgc_end_bam(s._h) == capi.ESTATE and L.mgc_push_bam(s._h, b"B", 1) == capi.ESTATE
        s.push_text(fq, "fastq")
        for p in files:
            s.push_bam_file(str(p), 3)
        got = s.staged_bases().cpu().numpy().tobytes()
        assert got == want
        s.count()
        res, n_inst = s.result_wide(), s.info().n_instances
    want_res, want_inst = count_of_stream(ops, torch_cuda, cfg, want)
    assert n_inst == want_inst and n_inst > 0
    for a, b in zip(res, want_res):
        assert np.array_equal(a, b)
    # the convenience wrapper, whole and in pieces
    for pieces in (None, 777):
        with ops.Session(cfg) as s:
            s.push_bam(raw, pieces)
            assert s.staged_bases().cpu().numpy().tobytes() == bam_stream


def bgzf_blocks_fast(data, block=0xff00, level=1):
    out = []
    for i in range(0, len(data), block):
        d = data[i:i + block]
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        cd = c.compress(d) + c.flush()
        bs = 12 + 6 + len(cd) + 8
        out.append(struct.pack("<BBBBIBBH", 0x1f, 0x8b, 8, 4, 0, 0, 0xff, 6) + b"BC" + struct.pack("<HH", 2, bs - 1) + cd +
                   struct.pack("<II", zlib.crc32(d) & 0xffffffff, len(d)))
    return out


def fixed_records(rows):
    """rows: uint8[reads, 150] of letters -> uint8[reads, 263]: BAM records of one shape (name "r", qualities 0xff, no aux)"""
    reads = rows.shape[0]
    lut = np.zeros(256, dtype=np.uint8)
    for i, ch in enumerate(NT16.encode()):
        lut[ch] = i
    codes = lut[rows]
    packed = (codes[:, 0::2] << 4) | codes[:, 1::2]
    fixed = struct.pack("<iiBBHHHiiii", -1, -1, 2, 0, 4680, 0, 4, 150, -1, -1, 0) + b"r\0"
    recb = np.empty((reads, 4 + len(fixed) + 75 + 150), dtype=np.uint8)
    recb[:, :4] = np.frombuffer(struct.pack("<i", len(fixed) + 75 + 150), dtype=np.uint8)
    recb[:, 4:4 + len(fixed)] = np.frombuffer(fixed, dtype=np.uint8)
    recb[:, 4 + len(fixed):4 + len(fixed) + 75] = packed
    recb[:, 4 + len(fixed) + 75:] = 0xff
    return recb


@pytest.fixture(scope="module")
def big(ops, torch_cuda, tmp_path_factory):
    """~270 000 records of 150 bases in fixed-shape numpy records: 71 MB of BAM, three upload chunks, the last partial.
    -> (path, the BGZF blocks, the base stream, its count at k = 21)"""
    from meryl_amd import capi
    reads = 270_000
    rng = np.random.default_rng(41)
    genome = rng.integers(0, 4, 400_000, dtype=np.uint8)
    starts = rng.integers(0, genome.size - 150, reads)
    rows = np.frombuffer(b"ACGT", dtype=np.uint8)[genome[starts[:, None] + np.arange(150)[None, :]]]
    rows[rng.random(rows.shape) < 0.0005] = ord("N")
    raw = b"BAM\x01" + struct.pack("<ii", 0, 0) + fixed_records(rows).tobytes()
    assert 2 * (32 << 20) < len(raw) < 3 * (32 << 20)
    blocks = bgzf_blocks_fast(raw)
    half = len(blocks) // 2
    blocks = blocks[:half] + [bgzf_block(b"")] * 3 + blocks[half:] + [bgzf_block(b"")]             # empty blocks in the middle, the EOF marker
    path = tmp_path_factory.mktemp("bam_big") / "big.bam"
    path.write_bytes(b"".join(blocks))
    stream = np.empty((reads, 151), dtype=np.uint8)
    stream[:, :150] = rows
    stream[:, 150] = ord(".")
    stream = stream.tobytes()
    cfg = capi.configure(21, len(stream), 8 << 30)
    return path, blocks, stream, cfg, count_of_stream(ops, torch_cuda, cfg, stream)


def test_ring_of_three_chunks(ops, torch_cuda, big):
    path, _, stream, cfg, (want, want_inst) = big
    with ops.Session(cfg) as s:
        s.push_bam_file(str(path), 5)
        assert s.staged_bases().cpu().numpy().tobytes() == stream
        s.count()
        got, n_inst = s.result_wide(), s.info().n_instances
    assert n_inst == want_inst
    for a, b in zip(got, want):
        assert np.array_equal(a, b)


def test_ring_chunks_that_hold_nothing_for_the_device(ops, torch_cuda, big, tmp_path):
    # A record with 104 MiB of aux after the big file's records, then more records: two upload chunks lie wholly inside the aux, give
    # no segment and are not uploaded.  The ring hands a slot back two chunks after its submit because every submit waits for the
    # chunk two before it; the chunks that queue nothing must not let a slot go while its upload still reads it.
    _, blocks, stream, cfg, _ = big
    CH = 32 << 20
    aux = 104 << 20
    seq = "ACGTACGTTGCATGCAAGTCAGTCA"
    packed = bytearray(13)
    for i, ch in enumerate(seq):
        packed[i // 2] |= NT16.index(ch) << (4 if i % 2 == 0 else 0)
    body = struct.pack("<iiBBHHHiiii", -1, -1, 2, 0, 4680, 0, 4, len(seq), -1, -1, 0) + b"x\0" + bytes(packed) + b"\xff" * len(seq)
    fat = struct.pack("<i", len(body) + aux) + body + bytes(aux)
    rng = np.random.default_rng(43)
    rows = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, (140_000, 150))]             # 37 MB of records: a whole chunk after the aux
    data_blocks = [b for b in blocks if struct.unpack_from("<I", b, len(b) - 4)[0]]
    before = sum(struct.unpack_from("<I", b, len(b) - 4)[0] for b in data_blocks)
    all_blocks = data_blocks + bgzf_blocks_fast(fat + fixed_records(rows).tobytes()) + [bgzf_block(b"")]
    # the reader's plan, restated: whole blocks, at most 32 MiB of them per chunk
    chunks, at, start = [], 0, 0
    for b in all_blocks:
        n = struct.unpack_from("<I", b, len(b) - 4)[0]
        if at - start + n > CH:
            chunks.append((start, at))
            start = at
        at += n
    chunks.append((start, at))
    aux_begin, aux_end = before + 4 + len(body), before + len(fat)
    empty = [i for i, (a, b) in enumerate(chunks) if aux_begin <= a and b <= aux_end]
    assert len(empty) >= 2 and 0 < empty[0] and empty[-1] + 2 < len(chunks), (chunks, aux_begin, aux_end)
    path = tmp_path / "fat_aux.bam"
    path.write_bytes(b"".join(all_blocks))
    want = stream + seq.encode() + b"." + np.concatenate([rows, np.full((rows.shape[0], 1), ord("."), dtype=np.uint8)], axis=1).tobytes()
    with ops.Session(cfg) as s:
        s.push_bam_file(str(path), 8)
        got = s.staged_bases().cpu().numpy().tobytes()
    assert len(got) == len(want) and got == want


def test_batches_cut_inside_the_file(ops, torch_cuda, big, tmp_path):
    from meryl_amd import db
    path, _, _, cfg, (want, want_inst) = big
    with ops.Session(cfg) as s:
        s.set_batch_bases(1 << 20)
        s.push_bam_file(str(path), 5)
        s.count()
        assert s.profile().n_batches >= 2                                              # a chunk holds more than a batch: a cut after each of the first two
        n_inst = s.info().n_instances
        if s.out_of_core():
            out = str(tmp_path / "batched.meryl")
            s.write_database(out)
            r = db.Reader(out)
            lo, hi, cn = r.read_all()
            r.close()
            got = (lo, hi, cn)
        else:
            got = s.result_wide()[:3]
    assert n_inst == want_inst
    for a, b in zip(got, want[:3]):
        assert np.array_equal(a, b)


def test_refused_files_leave_nothing_behind(ops, torch_cuda, big, tmp_path):
    from meryl_amd import capi
    recs = random_records(1500, 51, longest=200)
    raw = bam_bytes(recs)
    good = tmp_path / "good.bam"
    good.write_bytes(bgzf(raw, 3000))
    blocks = [bgzf_block(raw[i:i + 3000]) for i in range(0, len(raw), 3000)]
    assert len(blocks) > 45
    b39 = bytearray(blocks[39])
    b39[18 + (len(b39) - 26) // 2] ^= 0x40                                             # inside the 40th block's deflate data
    flipped = tmp_path / "flipped.bam"
    flipped.write_bytes(b"".join(blocks[:39]) + bytes(b39) + b"".join(blocks[40:]) + bgzf_block(b""))
    # cut inside a record, at a BGZF block border: every block inflates, only the walker can see it
    l_text, = struct.unpack_from("<i", raw, 4)
    at = 8 + l_text + 4
    for _ in range(2):
        at += 8 + struct.unpack_from("<i", raw, at)[0]
    borders = {at}
    while at < len(raw):
        at += 4 + struct.unpack_from("<i", raw, at)[0]
        borders.add(at)
    cut = next(c for c in range(30 * 3000, len(raw), 3000) if c not in borders)
    truncated = tmp_path / "truncated.bam"
    truncated.write_bytes(bgzf(raw[:cut], 3000))
    bs31 = tmp_path / "bs31.bam"
    bs31.write_bytes(bgzf(bam_bytes(recs[:1000]) + struct.pack("<i", 31) + bytes(40), 3000))
    plain = tmp_path / "plain_gzip.bam"
    plain.write_bytes(gzip.compress(raw))
    first = b"ACGTTGCATGCATGCAAGTCGATGCA."
    cfg = capi.configure(21, 1 << 20, 2 << 30)
    with ops.Session(cfg) as s:
        s.push_bases(first, end_of_sequence=False)
        s.push_bam_file(str(good), 2)
        before = s.staged_bases().cpu().numpy().tobytes()
        assert before == first + stream_of(recs)
        for p, words in ((flipped, "BGZF block 39 failed to inflate"), (truncated, "truncated BAM record"), (bs31, "block_size 31 < 32"),
                         (plain, "not a BGZF block")):
            with pytest.raises(capi.MgcError) as e:
                s.push_bam_file(str(p), 3)
            assert e.value.code == capi.EFORMAT, p.name
            msg = capi.last_error(s._h)
            assert p.name in msg and words in msg, msg
            assert s.staged_bases().cpu().numpy().tobytes() == before, p.name
        with pytest.raises(capi.MgcError) as e:
            s.push_bam_file(str(tmp_path / "missing.bam"))
        assert e.value.code == capi.EINVAL
        with pytest.raises(capi.MgcError) as e:                                       # the same through mgc_push_bam: refused where it is seen
            s.push_bam(bam_bytes(recs[:1000]) + struct.pack("<i", 31) + bytes(40), 5000)
        assert e.value.code == capi.EFORMAT and "block_size 31 < 32" in capi.last_error(s._h)
        assert s.staged_bases().cpu().numpy().tobytes() == before
        s.push_bam_file(str(good), 3)
        assert s.staged_bases().cpu().numpy().tobytes() == before + stream_of(recs)
        s.count()
        got, n_inst = s.result_wide(), s.info().n_instances
    want, want_inst = count_of_stream(ops, torch_cuda, cfg, before + stream_of(recs))
    assert n_inst == want_inst
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    # damage beyond the first cut cannot be taken back: MGC_EINVAL, as for text
    _, big_blocks, _, big_cfg, _ = big
    late = tmp_path / "late.bam"
    late.write_bytes(b"".join(big_blocks[:-6]) + bgzf_block(b""))                      # ends inside a record of the third chunk
    kept = sum(struct.unpack_from("<I", b, len(b) - 4)[0] for b in big_blocks[:-6])
    assert kept > 2 * (32 << 20) and (kept - 12) % 263 != 0
    with ops.Session(big_cfg) as s:
        s.set_batch_bases(1 << 20)
        with pytest.raises(capi.MgcError) as e:
            s.push_bam_file(str(late), 5)
        assert e.value.code == capi.EINVAL
        msg = capi.last_error(s._h)
        assert "late.bam" in msg and "truncated BAM record" in msg and "after part of the file was counted" in msg


# ---- the command line ----------------------------------------------------------------------------------------------------
def test_cli_default_route_equals_the_host_reader(native_lib, tmp_path):
    from meryl_amd import build, db
    meryl = build.build_cli()
    rng = np.random.default_rng(61)
    genome = rng.integers(0, 4, 40_000)
    reads = ["".join("ACGT"[c] for c in genome[a:a + 150]) for a in rng.integers(0, 40_000 - 150, 3000)]
    recs = [("r%d" % i, (0, 16, 256, 4)[i % 4], r) for i, r in enumerate(reads)]
    recs.insert(5, ("noseq", 4, ""))
    bam = tmp_path / "reads.bam"
    bam.write_bytes(bgzf(bam_bytes(recs), 5000))

    def run(out, extra_env, src=bam, check=True):
        env = dict(os.environ, MGC_IO_TRACE="1", **extra_env)
        p = subprocess.run([meryl, "-V", "-V", "k=21", "memory=2", "threads=4", "count", str(src), "output", str(out)], capture_output=True, text=True,
                           timeout=600, env=env)
        assert (p.returncode == 0) == check, p.stderr[-2000:]
        return p

    p_dev = run(tmp_path / "dev.meryl", {})
    p_host = run(tmp_path / "host.meryl", {"MERYL_HOST_PARSER": "1"})
    assert "[io] BAM file" in p_dev.stderr and "%d records" % len(recs) in p_dev.stderr
    assert "[io] BAM file" not in p_host.stderr
    res = []
    for name in ("dev.meryl", "host.meryl"):
        r = db.Reader(str(tmp_path / name))
        res.append(r.read_all() + (r.info.num_total,))
        r.close()
    assert res[0][3] == res[1][3] > 0
    for a, b in zip(res[0][:3], res[1][:3]):
        assert np.array_equal(a, b)
    cut = tmp_path / "cut.bam"
    whole = bam.read_bytes()
    cut.write_bytes(whole[:len(whole) // 2])
    p = run(tmp_path / "cut.meryl", {}, src=cut, check=False)
    assert "truncated" in p.stderr and "cut.bam" in p.stderr
