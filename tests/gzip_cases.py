"""The gzip files of tests/test_gzip_host.py and tests/test_gzip_device.py: about 4 MB of FASTQ-shaped text, compressed by
Python's zlib in every way the parallel reader (meryl_amd/csrc/mgc_gzip_par.hpp) has to cope with, and damaged in the ways it
has to refuse.  SPAN is 256 KiB: zlib at its default memLevel closes a block after at most 16384 symbols of at most 48 bits, so
a block is under 100 KiB compressed and every span of a level 1 / 6 / 9 file holds a block start."""
import functools
import struct
import zlib

import numpy as np

SPAN = 262144
SMALL_SPAN = 32768
CAP = 8 << 20                       # no cut: a span of these files holds well under 8 MiB of text
SMALL_CAP = 300_000                 # forces cuts: a span holds about 0.5 MB of text


@functools.lru_cache(maxsize=None)
def fastq_text(n_reads=16000, seed=5):
    """strict four-line FASTQ, reads of 100 .. 150 bases, a few N, random qualities: about 4 MB"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(100, 151, size=n_reads)
    bases = rng.choice(np.frombuffer(b"ACGTACGTACGTACGTN", dtype=np.uint8), size=int(lens.sum()))
    quals = rng.integers(35, 74, size=int(lens.sum()), dtype=np.uint8)
    out, at = [], 0
    for i, n in enumerate(lens):
        n = int(n)
        out.append(b"@run7.%d %d:N:0 length=%d\n" % (i + 1, i % 97, n))
        out.append(bases[at:at + n].tobytes() + b"\n+\n" + quals[at:at + n].tobytes() + b"\n")
        at += n
    return b"".join(out)


def fasta_text(n_seqs=40, seed=6):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n_seqs):
        n = int(rng.integers(1, 30000))
        s = rng.choice(np.frombuffer(b"ACGTacgtN", dtype=np.uint8), size=n).tobytes()
        out.append(b">seq%d some words\n" % i + b"\n".join(s[j:j + 70] for j in range(0, n, 70)) + b"\n")
    return b"".join(out)


def member(text, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_every=0, flush_mode=zlib.Z_FULL_FLUSH, first_flush=0,
           fname=None, extra=None, hcrc=False):
    """one gzip member; flush_every: a flush point after every so many bytes of text; first_flush: one after that many"""
    flg = (8 if fname is not None else 0) | (4 if extra is not None else 0) | (2 if hcrc else 0)
    head = b"\x1f\x8b\x08" + bytes([flg]) + b"\0\0\0\0\0\x03"
    if extra is not None:
        head += struct.pack("<H", len(extra)) + extra
    if fname is not None:
        head += fname + b"\0"
    if hcrc:
        head += struct.pack("<H", zlib.crc32(head) & 0xffff)
    z = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    body, at = [], 0
    if first_flush:
        body += [z.compress(text[:first_flush]), z.flush(zlib.Z_SYNC_FLUSH)]
        at = first_flush
    if flush_every:
        while at < len(text):
            body += [z.compress(text[at:at + flush_every]), z.flush(flush_mode)]
            at += flush_every
    else:
        body.append(z.compress(text[at:]))
    body.append(z.flush())
    return head + b"".join(body) + struct.pack("<II", zlib.crc32(text) & 0xffffffff, len(text) & 0xffffffff)


@functools.lru_cache(maxsize=None)
def near_chunk_file():
    """two members: the first ends 0.5 .. 2.5 KB before the start of span 1, the second has a flush point -- a block start,
    inside span 1 -- after 8000 bytes of its text: a piece that starts there has 8000 bytes of window, not 32 KiB"""
    text = fastq_text()
    n = len(text) // 4
    for _ in range(40):
        m1 = member(text[:n])
        if SPAN - 2500 <= len(m1) <= SPAN - 500:
            break
        n = max(1000, int(n * (SPAN - 1500) / len(m1)))
    else:
        raise AssertionError("no first member of the wanted size")
    data = m1 + member(text[n:], first_flush=8000)
    return data, text


@functools.lru_cache(maxsize=None)
def good_files():
    """name -> (file bytes, text, members)"""
    t = fastq_text()
    a, b = len(t) // 3, 2 * len(t) // 3
    near, near_text = near_chunk_file()
    return {
        "level1": (member(t, 1), t, 1),
        "level6": (member(t, 6), t, 1),
        "level9": (member(t, 9), t, 1),
        "fixed": (member(t, 6, zlib.Z_FIXED), t, 1),
        "stored": (member(t, 0), t, 1),
        "full_flush": (member(t, 6, flush_every=150_000), t, 1),
        "sync_flush": (member(t, 6, flush_every=150_000, flush_mode=zlib.Z_SYNC_FLUSH), t, 1),
        "three_members": (member(t[:a], 6) + member(b"", 6) + member(t[a:], 6), t, 3),
        "near_chunk": (near, near_text, 2),
        "header_flags": (member(t, 6, fname=b"reads.fastq", extra=b"XY\x03\0abc", hcrc=True), t, 1),
        "trailing_bytes": (member(t[:b], 6) + b"\0\0\0\0 not gzip", t[:b], 1),
    }


@functools.lru_cache(maxsize=None)
def damaged_files():
    """name -> file bytes; every one of them is refused (zlib's gzread refuses them too)"""
    data = good_files()["level6"][0]
    flipped = bytearray(data)
    flipped[len(data) // 2] ^= 0x10
    return {
        "flipped_bit": bytes(flipped),
        "cut_in_block": data[:len(data) // 2 + 77],
        "cut_in_trailer": data[:-5],
        "wrong_isize": data[:-4] + struct.pack("<I", (len(fastq_text()) + 1) & 0xffffffff),
    }
