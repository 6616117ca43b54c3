"""ctypes/torch plumbing of the k-mer position index and of query painting (include/meryl_positions.h): what the reference's
position-lookup does (src/meryl-lookup/position-lookup.C), over torch CUDA tensors."""
import ctypes

import numpy as np

from . import capi

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

NONE = 0xFFFFFFFF                       # MGC_POS_NONE; -1 in the int32 tensors
HITS, MERS, QUERIES = 1, 2, 4           # MGC_PAINT_*
_WHAT = {"hits": HITS, "mers": MERS, "queries": QUERIES}


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else ctypes.c_void_p(0)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _check(rc, what):
    if rc != capi.MGC_OK:
        raise capi.MgcError(rc, what, capi.lib().mgc_lookup_error().decode("utf-8", "replace"))


def _what_mask(what):
    if isinstance(what, int):
        return what
    if isinstance(what, str):
        what = [what]
    return sum({_WHAT[w] for w in what})


_hip = None


def _copy_from_device(ptr, count, dtype, device):
    """a torch tensor holding `count` items copied from a device pointer the library lends"""
    global _hip
    out = torch.empty(count, dtype=dtype, device=device)
    if count:
        if _hip is None:
            _hip = ctypes.CDLL(capi._load_hip_runtime(), mode=ctypes.RTLD_GLOBAL)
            _hip.hipMemcpy.restype = ctypes.c_int
            _hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        torch.cuda.synchronize(device)
        rc = _hip.hipMemcpy(out.data_ptr(), ptr, count * out.element_size(), 3)       # hipMemcpyDeviceToDevice
        if rc != 0:
            raise capi.MgcError(capi.MGC_EHIP, "hipMemcpy", "error %d" % rc)
    return out


class PositionIndex:
    """merylExactLookup::loadPositions on the device: for every k-mer of `lookup` (a meryl_amd.lookup.Lookup, which must stay
    open) the ascending begin offsets, in the base stream `ref_bases` (uint8 cuda tensor, '.' after each sequence), of the
    reference windows whose canonical k-mer it is."""

    def __init__(self, lookup, ref_bases):
        self.lookup = lookup
        self.device = ref_bases.device
        self._h = capi.lib().mgc_posidx_build(lookup._h, _ptr(ref_bases), ref_bases.numel(), _stream())
        if not self._h:
            raise capi.MgcError(capi.MGC_EINVAL, "mgc_posidx_build", capi.lib().mgc_lookup_error().decode("utf-8", "replace"))
        self.info = capi.PosIndexInfo()
        _check(capi.lib().mgc_posidx_get_info(self._h, ctypes.byref(self.info)), "mgc_posidx_get_info")

    def close(self):
        if self._h:
            capi.lib().mgc_posidx_free(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def arrays(self):
        """copies of (ref_slot int32[n_ref_bases], -1 = none; pos_start int64[n_kmers + 1]; pos_data int32[n_placed])"""
        a, b, c = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        _check(capi.lib().mgc_posidx_arrays(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)), "mgc_posidx_arrays")
        i = self.info
        return (_copy_from_device(a, i.n_ref_bases, torch.int32, self.device), _copy_from_device(b, i.n_kmers + 1, torch.int64, self.device),
                _copy_from_device(c, i.n_placed, torch.int32, self.device))

    def find(self, kmers):
        """kmers: int64[n] (or int64[n, 2] {lo, hi} for k > 32) cuda tensor, looked up as given -> (begin int64[n], count
        int32[n]): the k-mer's list is pos_data[begin : begin + count]; an absent k-mer gives 0, 0"""
        n = kmers.shape[0]
        begin = torch.empty(n, dtype=torch.int64, device=kmers.device)
        count = torch.empty(n, dtype=torch.int32, device=kmers.device)
        _check(capi.lib().mgc_posidx_find(self._h, _ptr(kmers), n, _ptr(begin), _ptr(count), _stream()), "mgc_posidx_find")
        return begin, count


class Painter:
    """Accumulates query sequences against a PositionIndex (which must stay open).  what: a mask of HITS | MERS | QUERIES, or
    names among "hits", "mers", "queries"."""

    def __init__(self, index, what=HITS | MERS | QUERIES):
        self.index = index
        self.what = _what_mask(what)
        self._h = capi.lib().mgc_paint_open(index._h, self.what)
        if not self._h:
            raise capi.MgcError(capi.MGC_EINVAL, "mgc_paint_open", capi.lib().mgc_lookup_error().decode("utf-8", "replace"))

    def close(self):
        if self._h:
            capi.lib().mgc_paint_close(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def add(self, bases, seq_start):
        """One batch of whole sequences: bases uint8 cuda tensor, seq_start the n_seq + 1 offsets from 0 to bases.numel().
        Returns (n_per, t_cov) as numpy uint32[n_seq] -- position-lookup's -hpq columns -- or (None, None) without HITS."""
        ss = torch.as_tensor(np.asarray(seq_start, dtype=np.int64)).to(bases.device)
        n = max(ss.numel() - 1, 0)
        hits = bool(self.what & HITS)
        per = torch.empty(max(n, 1), dtype=torch.int32, device=bases.device) if hits else None
        cov = torch.empty(max(n, 1), dtype=torch.int32, device=bases.device) if hits else None
        _check(capi.lib().mgc_paint_add(self._h, _ptr(bases), bases.numel(), _ptr(ss), n, _ptr(per), _ptr(cov), _stream()), "mgc_paint_add")
        if not hits:
            return None, None
        return per[:n].cpu().numpy().view(np.uint32), cov[:n].cpu().numpy().view(np.uint32)

    def _get(self, which):
        out = torch.empty(self.index.info.n_ref_bases, dtype=torch.int32, device=self.index.device)
        _check(capi.lib().mgc_paint_get(self._h, which, _ptr(out), _stream()), "mgc_paint_get")
        return out

    def mers(self):
        """int32[n_ref_bases] (read as uint32): the query windows that hit the k-mer beginning at each reference base"""
        return self._get(MERS)

    def queries(self):
        """int32[n_ref_bases]: the distinct query sequences that hit the k-mer beginning at each reference base"""
        return self._get(QUERIES)
