"""ctypes/torch plumbing of the exact k-mer lookup table (include/meryl_lookup.h)."""
import ctypes

import numpy as np

from . import capi

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

U64_MAX = (1 << 64) - 1


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else ctypes.c_void_p(0)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class Lookup:
    """merylExactLookup on the device: load(db, min, max) / value(kmers) / per-window stream lookups / -existence."""

    def __init__(self, handle):
        if not handle:
            raise capi.MgcError(-1, "mgc_lookup", capi.lib().mgc_lookup_error().decode("utf-8", "replace"))
        self._h = handle
        self.info = capi.LookupInfo()
        capi.check(capi.lib().mgc_lookup_get_info(self._h, ctypes.byref(self.info)), "mgc_lookup_get_info")

    @classmethod
    def load(cls, db_path, min_value=0, max_value=U64_MAX, device=-1, host_threads=16):
        return cls(capi.lib().mgc_lookup_load(db_path.encode(), min_value, max_value, device, host_threads))

    @classmethod
    def from_device(cls, keys, counts, k, min_value=0, max_value=U64_MAX):
        torch.cuda.current_stream(keys.device).synchronize()
        return cls(capi.lib().mgc_lookup_from_device(_ptr(keys), _ptr(counts), keys.shape[0], k, min_value, max_value, -1))

    def close(self):
        if self._h:
            capi.lib().mgc_lookup_free(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def values(self, kmers):
        """kmers: int64[n] (or int64[n, 2] {lo, hi}) cuda tensor -> int32[n] values (0 = absent)"""
        out = torch.empty(kmers.shape[0], dtype=torch.int32, device=kmers.device)
        capi.check(capi.lib().mgc_lookup_values(self._h, _ptr(kmers), kmers.shape[0], _ptr(out), _stream()), "mgc_lookup_values")
        return out

    def stream(self, bases):
        """uint8 cuda tensor of bases -> int32[n_bases]: value of the k-mer starting at every base (0: absent / broken)"""
        out = torch.empty(bases.numel(), dtype=torch.int32, device=bases.device)
        capi.check(capi.lib().mgc_lookup_stream(self._h, _ptr(bases), bases.numel(), _ptr(out), _stream()), "mgc_lookup_stream")
        return out

    def existence(self, bases, seq_start):
        """seq_start: int64[n_seq + 1] offsets into `bases` -> (total k-mers, k-mers found) per sequence as numpy uint64"""
        ss = torch.as_tensor(np.asarray(seq_start, dtype=np.int64)).to(bases.device)
        n = ss.numel() - 1
        tot = torch.empty(max(n, 1), dtype=torch.int64, device=bases.device)
        fnd = torch.empty(max(n, 1), dtype=torch.int64, device=bases.device)
        capi.check(capi.lib().mgc_lookup_existence(self._h, _ptr(bases), bases.numel(), _ptr(ss), n, _ptr(tot), _ptr(fnd), _stream()),
                   "mgc_lookup_existence")
        return tot[:n].cpu().numpy().view(np.uint64), fnd[:n].cpu().numpy().view(np.uint64)


WHAT = {"presence": 0, "count": 1, "depth": 2}
MODES = {"bed": 0, "bed-runs": 1, "wig-count": 2, "wig-depth": 3}


def _tables(tables):
    hs = [t._h for t in tables]
    return (ctypes.c_void_p * max(len(hs), 1))(*hs), len(hs)


def positions(tables, what, bases):
    """mgc_lookup_positions (src/meryl-lookup/dump.C:89-245) over the Lookups `tables`: what = "presence" (bit t: table t holds
    the window's fmer or rmer), "count" (sum of value(f) + value(r) over the tables, uint32) or "depth" (windows of table 0
    covering each base).  bases: uint8 cuda tensor -> int32[n_bases] (read as uint32)."""
    arr, n = _tables(tables)
    out = torch.empty(bases.numel(), dtype=torch.int32, device=bases.device)
    _check(capi.lib().mgc_lookup_positions(arr, n, WHAT.get(what, what), _ptr(bases), bases.numel(), _ptr(out), _stream()),
           "mgc_lookup_positions")
    return out


def _check(rc, what):
    if rc != capi.MGC_OK:
        raise capi.MgcError(rc, what, capi.lib().mgc_lookup_error().decode("utf-8", "replace"))


def report(tables, mode, names, bases, seq_start, labels=None, chunk_bytes=64 << 20, pieces=None):
    """mgc_lookup_report: the text of meryl-lookup -bed / -bed-runs / -wig-count / -wig-depth (mode: one of MODES) as bytes.
    bases: uint8 cuda tensor holding the sequences one after the other, each non-empty one ending with a non-ACGT byte;
    seq_start: n_seq + 1 offsets from 0 to bases.numel(); names: the n_seq identifiers; labels: one per table (-labels).
    pieces: a list that receives the callback's pieces as they come (at most chunk_bytes each)."""
    arr, n = _tables(tables)
    ss = np.ascontiguousarray(np.asarray(seq_start, dtype=np.uint64))
    names_b = [s.encode() if isinstance(s, str) else bytes(s) for s in names]
    labels_b = [s.encode() if isinstance(s, str) else bytes(s) for s in (labels or [])]
    c_names = (ctypes.c_char_p * max(len(names_b), 1))(*names_b)
    c_labels = (ctypes.c_char_p * max(len(labels_b), 1))(*labels_b)
    if pieces is None:
        pieces = []

    def _write(data, nbytes, _user):
        pieces.append(ctypes.string_at(data, nbytes))
        return 0

    cb = capi.LOOKUP_WRITE_CB(_write)
    torch.cuda.current_stream(bases.device).synchronize()
    _check(capi.lib().mgc_lookup_report(arr, n, MODES.get(mode, mode), c_labels, len(labels_b), _ptr(bases), bases.numel(),
                                        ss.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), c_names, len(names_b), chunk_bytes,
                                        cb, None), "mgc_lookup_report")
    return b"".join(pieces)


FILTER_MODES = {"include": 0, "exclude": 1}


def filter_text(table, mode, texts, skip_first=0, final=True, outs=None):
    """mgc_lookup_filter_text: one step of meryl-lookup -include / -exclude (src/meryl-lookup/include-exclude.C) over raw
    FASTA/FASTQ text.  texts: one or two uint8 cuda tensors, each beginning at a record start; mode: "include" / "exclude";
    skip_first: 23 for -10x.  Returns (list of the kept text per input as bytes, capi.FilterResult).  outs: the output
    tensors to use as they are; without them they are sized here and grown once when the library asks for more.  A failed
    call raises capi.MgcError with the result (the sizes needed, when an output was too small) as its `result`."""
    n = len(texts)
    res = capi.FilterResult()
    c_text = (ctypes.c_void_p * 2)(*[_ptr(t).value for t in texts])
    c_n = (ctypes.c_uint64 * 2)(*[t.numel() for t in texts])
    dev = texts[0].device
    given = outs is not None
    if not given:
        outs = [torch.empty(t.numel() + t.numel() // 4 + 4096, dtype=torch.uint8, device=dev) for t in texts]
    for attempt in range(2):
        c_out = (ctypes.c_void_p * 2)(*[_ptr(o).value for o in outs])
        c_cap = (ctypes.c_uint64 * 2)(*[o.numel() for o in outs])
        rc = capi.lib().mgc_lookup_filter_text(table._h, FILTER_MODES.get(mode, mode), skip_first, n, c_text, c_n, 1 if final else 0,
                                               c_out, c_cap, ctypes.byref(res), _stream())
        short = rc == capi.MGC_EINVAL and any(res.out_bytes[i] > outs[i].numel() for i in range(n))
        if rc == capi.MGC_OK or given or not short or attempt:
            break
        outs = [torch.empty(max(int(res.out_bytes[i]), 1), dtype=torch.uint8, device=dev) for i in range(n)]
    if rc != capi.MGC_OK:
        err = capi.MgcError(rc, "mgc_lookup_filter_text", capi.lib().mgc_lookup_error().decode("utf-8", "replace"))
        err.result = res
        raise err
    torch.cuda.current_stream(dev).synchronize()
    return [bytes(outs[i][:int(res.out_bytes[i])].cpu().numpy().tobytes()) for i in range(n)], res


def filter_files(table, mode, paths, outputs, skip_first=0, batch_bytes=0, pieces=None):
    """mgc_lookup_filter_files: the same over whole files (plain, gzip, BGZF), one or two of them.  outputs: per input a
    path or a binary file object that receives the kept text.  pieces: a list that receives (input, bytes) as the callbacks
    are called.  Returns capi.FilterResult with the totals."""
    files = [open(o, "wb") if isinstance(o, (str, bytes)) or hasattr(o, "__fspath__") else o for o in outputs]
    res = capi.FilterResult()

    def _writer(i):
        def _write(data, nbytes, _user):
            b = ctypes.string_at(data, nbytes)
            if pieces is not None:
                pieces.append((i, b))
            files[i].write(b)
            return 0
        return capi.LOOKUP_WRITE_CB(_write)

    cbs = [_writer(i) for i in range(len(paths))]
    null_cb = ctypes.cast(None, capi.LOOKUP_WRITE_CB)
    try:
        rc = capi.lib().mgc_lookup_filter_files(table._h, FILTER_MODES.get(mode, mode), skip_first, str(paths[0]).encode(),
                                                str(paths[1]).encode() if len(paths) > 1 else None, batch_bytes, cbs[0], None,
                                                cbs[1] if len(paths) > 1 else null_cb, None, ctypes.byref(res))
    finally:
        for f, o in zip(files, outputs):
            if f is not o:
                f.close()
    if rc != capi.MGC_OK:
        err = capi.MgcError(rc, "mgc_lookup_filter_files", capi.lib().mgc_lookup_error().decode("utf-8", "replace"))
        err.result = res
        raise err
    return res
