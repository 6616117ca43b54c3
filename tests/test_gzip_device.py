"""Plain gzip input: the device side of the parallel reader (mgc_dev_gzip_resolve, mgc_dev_crc32_pieces; mgc_gzip.hip) against
numpy and zlib, the session route (Session.push_text_gzip_file) against the same text through mgc_push_text, and the command
line against the uncompressed file and against the host reader.  The files are those of tests/test_gzip_host.py."""
import ctypes
import ctypes.util
import filecmp
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import gzip_cases as gc  # noqa: E402

pytestmark = pytest.mark.gpu

WIN = 32768
MARK = 0x8000


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


# ---- mgc_dev_gzip_resolve against numpy ----------------------------------------------------------------------------------
def model(text, sym, window, window_valid):
    """(resolved text, next window, error bits)"""
    out = text.copy()
    s = sym.astype(np.int64)
    n = s.size
    lit = s < 256
    junk = (~lit) & (s < MARK)
    early = (s >= MARK) & (s - MARK < WIN - window_valid)
    ok = (s >= MARK) & ~early
    head = np.zeros(n, dtype=np.uint8)
    head[lit] = s[lit]
    head[ok] = window[s[ok] - MARK]
    out[:n] = head
    nxt = np.concatenate([window, out])[-WIN:]
    return out, nxt, (1 if junk.any() else 0) | (2 if early.any() else 0)


def make_case(rng, text_bytes, prefix, window_valid, edge_markers=False):
    text = rng.integers(0, 256, text_bytes, dtype=np.uint8)
    window = rng.integers(0, 256, WIN, dtype=np.uint8)
    sym = text[:prefix].astype(np.uint16)                      # a literal's symbol is its byte ...
    if window_valid:
        marks = rng.random(prefix) < 0.5
        sym[marks] = MARK + rng.integers(WIN - window_valid, WIN, int(marks.sum()))
        if edge_markers and prefix >= 2:
            sym[0], sym[prefix - 1] = MARK + WIN - window_valid, MARK + WIN - 1
    text[:prefix][sym >= MARK] = 0xEE                          # ... and where a marker stands the text holds junk
    return text, sym, window


def on_device(torch, text, sym, window, window_valid, shift=0, guard=64, want_window=True):
    """-> (text after the call, window out, error word, guards untouched)"""
    from meryl_amd import capi
    n = text.size
    buf = torch.full((guard + 16 + n + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    first = guard + shift
    assert buf.data_ptr() % 16 == 0
    buf[first:first + n] = torch.from_numpy(text.copy()).cuda()
    d_sym = torch.from_numpy(sym.view(np.int16).copy()).cuda() if sym.size else None
    d_win = torch.from_numpy(window.copy()).cuda()
    d_out = torch.full((WIN,), 0x5A, dtype=torch.uint8, device="cuda")
    d_err = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    capi.check(capi.lib().mgc_dev_gzip_resolve(ctypes.c_void_p(buf.data_ptr() + first), n, ctypes.c_void_p(d_sym.data_ptr() if sym.size else 0), sym.size,
                                               ctypes.c_void_p(d_win.data_ptr()), window_valid, ctypes.c_void_p(d_out.data_ptr() if want_window else 0),
                                               ctypes.c_void_p(d_err.data_ptr()), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)),
               "mgc_dev_gzip_resolve")
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    untouched = bool((h[:first] == 0xA5).all() and (h[first + n:] == 0xA5).all())
    return h[first:first + n], d_out.cpu().numpy(), int(d_err.item()), untouched


def check(torch, text, sym, window, window_valid, shift=0):
    want, want_win, want_err = model(text, sym, window, window_valid)
    got, got_win, err, untouched = on_device(torch, text, sym, window, window_valid, shift)
    assert np.array_equal(got, want), (text.size, sym.size, window_valid, shift, int(np.argmax(got != want)))
    assert np.array_equal(got_win, want_win), (text.size, sym.size, window_valid, shift, int(np.argmax(got_win != want_win)))
    assert err == want_err and untouched, (text.size, sym.size, window_valid, shift, err)


def test_resolve_sizes_prefixes_and_windows(torch_cuda):
    rng = np.random.default_rng(71)
    for text_bytes in (1, 15, 16, 17, 4099):
        for prefix in sorted({0, 1, min(16, text_bytes), text_bytes}):
            for window_valid in (0, 5, WIN):
                text, sym, window = make_case(rng, text_bytes, prefix, window_valid, edge_markers=True)
                check(torch_cuda, text, sym, window, window_valid)


def test_resolve_markers_at_both_ends_of_the_window(torch_cuda):
    rng = np.random.default_rng(72)
    text, sym, window = make_case(rng, 4099, 4099, WIN)
    sym[:] = MARK
    sym[1::2] = MARK + WIN - 1
    got, _, err, _ = on_device(torch_cuda, text, sym, window, WIN)
    assert err == 0 and (got[0::2] == window[0]).all() and (got[1::2] == window[WIN - 1]).all()


def test_resolve_destination_at_every_shift_leaves_its_neighbours_alone(torch_cuda):
    rng = np.random.default_rng(73)
    for shift in range(16):
        for text_bytes, prefix in ((4099, 4099), (4099, 33), (17, 16)):
            text, sym, window = make_case(rng, text_bytes, prefix, WIN)
            check(torch_cuda, text, sym, window, WIN, shift)


def test_resolve_more_tiles_than_workgroups(torch_cuda):
    rng = np.random.default_rng(74)
    n = 1024 * 4096 + 4096 + 5                                         # the kernel's grid holds 1024 workgroups of one 4 KiB tile each
    text, sym, window = make_case(rng, n, n, WIN)
    check(torch_cuda, text, sym, window, WIN, 3)


def test_window_out_for_short_and_long_pieces(torch_cuda):
    rng = np.random.default_rng(75)
    for text_bytes in (1, WIN - 1, WIN, WIN + 1, 40_000):
        for prefix in (0, text_bytes):
            text, sym, window = make_case(rng, text_bytes, prefix, WIN)
            check(torch_cuda, text, sym, window, WIN, shift=text_bytes % 16)
    text, sym, window = make_case(rng, 100, 10, WIN)
    _, win_out, _, _ = on_device(torch_cuda, text, sym, window, WIN, want_window=False)
    assert (win_out == 0x5A).all()                                     # no window asked for: none written


def test_resolve_error_cases_set_the_error_word_and_write_zero(torch_cuda):
    rng = np.random.default_rng(76)
    text, sym, window = make_case(rng, 4099, 4099, 5)
    window[:] = 7
    sym[100], sym[4000] = 0x0100, 0x7fff                               # neither a byte nor a marker
    got, _, err, untouched = on_device(torch_cuda, text, sym, window, 5)
    assert err == 1 and got[100] == 0 and got[4000] == 0 and untouched
    sym[100], sym[4000] = text[100], text[4000]
    sym[200], sym[3000] = MARK + WIN - 6, MARK                         # before the start of the member
    want, _, _ = model(text, sym, window, 5)
    got, _, err, untouched = on_device(torch_cuda, text, sym, window, 5)
    assert err == 2 and got[200] == 0 and got[3000] == 0 and np.array_equal(got, want) and untouched
    from meryl_amd import capi
    L = capi.lib()
    assert L.mgc_dev_gzip_resolve(ctypes.c_void_p(64), 4, ctypes.c_void_p(64), 5, None, 0, None, ctypes.c_void_p(64), None) == capi.EINVAL
    assert L.mgc_dev_gzip_resolve(ctypes.c_void_p(64), 4, ctypes.c_void_p(64), 1, ctypes.c_void_p(64), WIN + 1, None, ctypes.c_void_p(64), None) == capi.EINVAL


# ---- mgc_dev_crc32_pieces against zlib -------------------------------------------------------------------------------------
def crc_pieces(torch, text, begins, lens):
    from meryl_amd import capi
    d_text = torch.from_numpy(text.copy()).cuda()
    d_begin = torch.from_numpy(np.asarray(begins, dtype=np.int64)).cuda()
    d_len = torch.from_numpy(np.asarray(lens, dtype=np.int32)).cuda()
    d_crc = torch.zeros(len(lens), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    capi.check(capi.lib().mgc_dev_crc32_pieces(ctypes.c_void_p(d_text.data_ptr()), ctypes.c_void_p(d_begin.data_ptr()), ctypes.c_void_p(d_len.data_ptr()),
                                               len(lens), ctypes.c_void_p(d_crc.data_ptr()), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)),
               "mgc_dev_crc32_pieces")
    torch.cuda.synchronize()
    return d_crc.cpu().numpy().view(np.uint32)


def test_crc32_of_pieces_of_every_length_at_unaligned_begins(torch_cuda):
    rng = np.random.default_rng(77)
    text = rng.integers(0, 256, 100_000, dtype=np.uint8)
    begins, lens = [], []
    for n in (0, 1, 2, 15, 16, 17, 31, 4095, 4096):
        for b in (0, 1, 7, 15, 16, 4097, 50_003):
            begins.append(b)
            lens.append(n)
    got = crc_pieces(torch_cuda, text, begins, lens)
    want = [zlib.crc32(text[b:b + n].tobytes()) & 0xffffffff for b, n in zip(begins, lens)]
    assert got.tolist() == want


def test_crc32_pieces_combine_to_the_crc_of_a_megabyte(torch_cuda):
    z = ctypes.CDLL(ctypes.util.find_library("z") or "libz.so.1")
    z.crc32_combine.restype = ctypes.c_ulong
    z.crc32_combine.argtypes = [ctypes.c_ulong, ctypes.c_ulong, ctypes.c_long]
    rng = np.random.default_rng(78)
    text = rng.integers(0, 256, 1_000_003, dtype=np.uint8)
    begins = list(range(0, text.size, 4096))
    lens = [min(4096, text.size - b) for b in begins]
    got = crc_pieces(torch_cuda, text, begins, lens)
    crc = 0
    for c, n in zip(got.tolist(), lens):
        crc = z.crc32_combine(crc, c, n)
    assert crc == zlib.crc32(text.tobytes()) & 0xffffffff


# ---- the session route -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("gzip_files")
    paths = {}
    for name, (data, _, _) in gc.good_files().items():
        paths[name] = d / (name + ".gz")
        paths[name].write_bytes(data)
    for name, data in gc.damaged_files().items():
        paths[name] = d / (name + ".gz")
        paths[name].write_bytes(data)
    return paths


@pytest.fixture(scope="module")
def cfg(ops):
    from meryl_amd import capi
    return capi.configure(21, 4 * len(gc.fastq_text()), 2 << 30)


_BASES = {}


def bases_of_text(ops, cfg, text, fmt="fastq"):
    """the base stream mgc_push_text makes of the text (computed once per text)"""
    key = (zlib.crc32(text), len(text), fmt)
    if key not in _BASES:
        with ops.Session(cfg) as s:
            s.push_text(text, fmt)
            _BASES[key] = s.staged_bases().cpu().numpy().tobytes()
    return _BASES[key]


def push_gz(s, path, monkeypatch, span=gc.SPAN, cap=gc.CAP, threads=4):
    monkeypatch.setenv("MGC_GZIP_SPAN", str(span))
    monkeypatch.setenv("MGC_GZIP_TEXT_CAP", str(cap))
    return s.push_text_gzip_file(str(path), threads)


@pytest.mark.parametrize("name", list(gc.good_files()))
def test_session_bases_equal_those_of_the_text(ops, cfg, files, monkeypatch, name):
    data, text, members = gc.good_files()[name]
    want = bases_of_text(ops, cfg, text)
    for cap in (gc.CAP, gc.SMALL_CAP):
        with ops.Session(cfg) as s:
            info = push_gz(s, files[name], monkeypatch, cap=cap)
            assert s.staged_bases().cpu().numpy().tobytes() == want, (name, cap)
        assert (info["members"], info["text_bytes"]) == (members, len(text)), info
        assert info["chunks"] == len(data) // gc.SPAN + info["cuts"] and info["symbol_bytes"] <= 2 * info["text_bytes"]
        if name in ("level1", "level6", "level9"):
            assert info["chunks"] >= 4 and info["confirmed"] == info["chunks"] - 1 - info["cuts"] and info["discarded"] == 0, info
        if name == "fixed":
            assert info["confirmed"] == 0, info
        if name == "near_chunk":
            assert info["confirmed"] == info["chunks"] - 1 - info["cuts"], info
        if name != "stored":                                           # (a span of stored blocks holds 256 KiB of text: under the small cap)
            assert (info["cuts"] >= 4) if cap == gc.SMALL_CAP else (info["cuts"] == 0), info


def test_session_spans_without_a_block_start_and_one_thread(ops, cfg, files, monkeypatch):
    want = bases_of_text(ops, cfg, gc.fastq_text())
    for span, threads in ((gc.SMALL_SPAN, 4), (gc.SPAN, 1), (1 << 30, 4)):
        with ops.Session(cfg) as s:
            info = push_gz(s, files["level6"], monkeypatch, span=span, threads=threads)
            assert s.staged_bases().cpu().numpy().tobytes() == want
        assert info["discarded"] + info["confirmed"] < info["chunks"]


def test_session_fasta_and_files_one_after_the_other(ops, cfg, files, monkeypatch, tmp_path):
    fa = gc.fasta_text()
    p = tmp_path / "seqs.fa.gz"
    p.write_bytes(gc.member(fa[:len(fa) // 2], 6) + gc.member(fa[len(fa) // 2:], 9))
    want = bases_of_text(ops, cfg, fa, "fasta")
    fq = bases_of_text(ops, cfg, gc.fastq_text())
    from meryl_amd import capi
    assert capi.lib().mgc_is_gzip_file(os.fsencode(str(p))) == 1
    with ops.Session(cfg) as s:
        s.push_bases("ACGTA", end_of_sequence=False)                   # the file begins at an odd stream offset
        info = push_gz(s, p, monkeypatch, span=gc.SMALL_SPAN, cap=gc.SMALL_CAP)
        assert info["members"] == 2 and info["text_bytes"] == len(fa)
        push_gz(s, files["level1"], monkeypatch)
        assert s.staged_bases().cpu().numpy().tobytes() == b"ACGTA" + want + fq


def count_of_stream(ops, torch, cfg, stream):
    d = torch.from_numpy(np.frombuffer(stream, dtype=np.uint8).copy()).cuda()
    with ops.Session(cfg) as s:
        s.push_bases_device(d)
        s.count()
        return s.result_wide(), s.info().n_instances


def test_refused_files_leave_nothing_behind(ops, torch_cuda, cfg, files, monkeypatch, tmp_path):
    from meryl_amd import capi
    text = gc.fastq_text()
    multi = tmp_path / "multiline.fq.gz"
    multi.write_bytes(gc.member(b"@a\nACGTACGTACGTACGTACGTACGTAC\nGTACGTTT\n+\nIIIIIIIIIIIIIIIIIIIIIIIIII\nIIIIIIII\n" + text[:300_000], 6))
    not_gz = tmp_path / "plain.fq"
    not_gz.write_bytes(text[:5000])
    neither = tmp_path / "neither.gz"
    neither.write_bytes(gc.member(b"#hello\n" + text[:5000], 6))
    want = bases_of_text(ops, cfg, text)
    with ops.Session(cfg) as s:
        s.push_bases("ACGTTGCATTGACCAGGATTACAGGAT")
        before = s.staged_bases().cpu().numpy().tobytes()
        for p, word in ((multi, "FASTQ"), (not_gz, "not a gzip file"), (neither, "neither FASTA nor FASTQ"), (files["flipped_bit"], "flipped_bit.gz"),
                        (files["cut_in_block"], "compressed offset"), (files["cut_in_trailer"], "compressed offset"), (files["wrong_isize"], "compressed offset")):
            with pytest.raises(capi.MgcError) as e:
                push_gz(s, p, monkeypatch, cap=gc.SMALL_CAP)
            assert e.value.code == capi.EFORMAT, (p.name, e.value)
            assert word in capi.last_error(s._h), (p.name, capi.last_error(s._h))
            assert s.staged_bases().cpu().numpy().tobytes() == before, p.name
            push_gz(s, files["level6"], monkeypatch, cap=gc.SMALL_CAP)  # after every refusal a good file still comes out right
            before += want
            assert s.staged_bases().cpu().numpy().tobytes() == before, p.name
        with pytest.raises(capi.MgcError) as e:
            push_gz(s, tmp_path / "missing.gz", monkeypatch)
        assert e.value.code == capi.EINVAL
        push_gz(s, files["level6"], monkeypatch)                       # the next file still counts right
        before += want
        assert s.staged_bases().cpu().numpy().tobytes() == before
        s.count()
        got, n_inst = s.result_wide(), s.info().n_instances
    want_res, want_inst = count_of_stream(ops, torch_cuda, cfg, before)
    assert n_inst == want_inst > 0
    for a, b in zip(got, want_res):
        assert np.array_equal(a, b)


def test_damage_after_a_batch_was_counted_cannot_be_taken_back(ops, cfg, files, monkeypatch, tmp_path):
    from meryl_amd import capi
    data = bytearray(gc.good_files()["level6"][0])
    data[len(data) * 9 // 10] ^= 0x10
    late = tmp_path / "late.gz"
    late.write_bytes(bytes(data))
    with ops.Session(cfg) as s:
        s.set_batch_bases(1 << 20)
        push_gz(s, files["level6"], monkeypatch)                       # 2 MB of bases: counted as a batch while it is read
        with pytest.raises(capi.MgcError) as e:
            push_gz(s, late, monkeypatch)
        assert e.value.code == capi.EINVAL
        msg = capi.last_error(s._h)
        assert "late.gz" in msg and "after part of the file was counted" in msg


# ---- the command line ----------------------------------------------------------------------------------------------------
def same_database(a, b):
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b)) and names
    _, mismatch, errors = filecmp.cmpfiles(a, b, names, shallow=False)
    return not mismatch and not errors


def test_cli_database_is_byte_identical(native_lib, files, tmp_path):
    from meryl_amd import build
    meryl = build.build_cli()
    plain = tmp_path / "reads.fq"
    plain.write_bytes(gc.fastq_text())
    gz = tmp_path / "reads.fq.gz"
    gz.write_bytes(gc.good_files()["level6"][0])

    def run(out, src, extra_env=None, check=True):
        env = dict(os.environ, MGC_IO_TRACE="1", MGC_GZIP_SPAN=str(gc.SPAN), **(extra_env or {}))
        p = subprocess.run([meryl, "k=21", "memory=2", "threads=4", "count", str(src), "output", str(out)], capture_output=True, text=True,
                           timeout=600, env=env)
        assert check is None or (p.returncode == 0) == check, p.stderr[-2000:]
        return p

    p_new = run(tmp_path / "new.meryl", gz)
    p_old = run(tmp_path / "old.meryl", gz, {"MERYL_GZIP_GENERIC": "1"})
    run(tmp_path / "plain.meryl", plain)
    assert "[io] gzip file" in p_new.stderr and "[io] gzip file" not in p_old.stderr
    assert same_database(tmp_path / "new.meryl", tmp_path / "plain.meryl")
    assert same_database(tmp_path / "new.meryl", tmp_path / "old.meryl")
    # bytes after the last member: the verdict of the host reader, whatever it is
    p_new = run(tmp_path / "tail_new.meryl", files["trailing_bytes"], check=None)
    p_old = run(tmp_path / "tail_old.meryl", files["trailing_bytes"], {"MERYL_GZIP_GENERIC": "1"}, check=None)
    assert p_new.returncode == p_old.returncode
    if p_new.returncode == 0:
        assert "[io] gzip file" in p_new.stderr
        assert same_database(tmp_path / "tail_new.meryl", tmp_path / "tail_old.meryl")
    # a damaged file: refused by the device route, read again by the host reader, which says what is wrong
    p = run(tmp_path / "cut.meryl", files["cut_in_block"], check=False)
    assert "cut_in_block.gz" in p.stderr
