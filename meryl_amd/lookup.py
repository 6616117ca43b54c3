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
