"""ctypes/torch plumbing of `meryl-analyze` (include/meryl_analyze.h): GC / GA / GT composition histograms on the device.

Keys are int64 tensors holding the uint64 bit patterns: shape [n] for k <= 32, [n, 2] ({lo, hi}) above; values are int32
tensors holding uint32 bit patterns.  There is no CPU path: everything here launches the library's HIP kernels."""
import ctypes

import numpy as np

from . import capi

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

GC, GA, GT = 0, 1, 2
FORWARD, REVERSE, COMBINED = 0, 1, 2
MAX_K = 64
DENSE_VALUES = 96            # MGC_ANALYZE_DENSE_VALUES: values below it take the dense tier, the others the overflow list
TYPES = {"gc": GC, "ga": GA, "gt": GT}
# the report files of a type in the order they are written: (name in <prefix>.<name>.hist, which histogram)
FILES = {GC: (("GC", FORWARD), ("AT", REVERSE)),
         GA: (("GA_TC", COMBINED), ("GA", FORWARD), ("TC", REVERSE)),
         GT: (("GT_AC", COMBINED), ("GT", FORWARD), ("AC", REVERSE))}


def _error():
    s = capi.lib().mgc_analyze_error()
    return s.decode("utf-8", "replace") if s else ""


def _check(rc, what):
    if rc != capi.MGC_OK:
        raise capi.MgcError(rc, what, _error())


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else ctypes.c_void_p(0)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _type(t):
    return TYPES[t] if isinstance(t, str) else int(t)


def scores(keys, k, type):
    """mgc_dev_analyze_scores -> (fscore, rscore) uint8 cuda tensors, one entry per k-mer of `keys`"""
    n = int(keys.shape[0])
    f = torch.empty(n, dtype=torch.uint8, device=keys.device)
    r = torch.empty(n, dtype=torch.uint8, device=keys.device)
    _check(capi.lib().mgc_dev_analyze_scores(_ptr(keys), n, k, _type(type), _ptr(f), _ptr(r), _stream()), "mgc_dev_analyze_scores")
    torch.cuda.current_stream().synchronize()
    return f, r


class Analyzer:
    """One report (type "gc" / "ga" / "gt") over k-mers of size k, accumulated on one device."""

    def __init__(self, k, type, device=-1):
        self.k, self.type = k, _type(type)
        h = ctypes.c_void_p()
        _check(capi.lib().mgc_analyze_open(k, self.type, device, ctypes.byref(h)), "mgc_analyze_open")
        self._h = h

    def close(self):
        if self._h:
            capi.lib().mgc_analyze_close(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def add_device(self, keys, values):
        """every (k-mer, value) of the two cuda tensors is one insertion; returns once they are counted"""
        n = int(keys.shape[0])
        assert int(values.numel()) == n and keys.is_contiguous() and values.is_contiguous()
        assert (keys.dim() == 2 and keys.shape[1] == 2) == (self.k > 32)
        _check(capi.lib().mgc_analyze_add_device(self._h, _ptr(keys), _ptr(values), n, _stream()), "mgc_analyze_add_device")

    def add_database(self, path, host_threads=0):
        """all 64 files of the database directory `path`, decoded on the device"""
        _check(capi.lib().mgc_analyze_add_database(self._h, str(path).encode(), host_threads), "mgc_analyze_add_database")

    def result(self, which):
        """histogram `which` -> (scores uint32, values uint32, occurrences uint64) numpy arrays, rows ascending by (score, value)"""
        n = ctypes.c_uint64(0)
        _check(capi.lib().mgc_analyze_result_rows(self._h, which, ctypes.byref(n)), "mgc_analyze_result_rows")
        s = np.zeros(n.value, dtype=np.uint32)
        v = np.zeros(n.value, dtype=np.uint32)
        o = np.zeros(n.value, dtype=np.uint64)
        if n.value:
            _check(capi.lib().mgc_analyze_result(self._h, which, s.ctypes.data, v.ctypes.data, o.ctypes.data), "mgc_analyze_result")
        return s, v, o

    def write(self, prefix):
        """the report's <prefix>.<NAME>.hist files; returns their paths"""
        _check(capi.lib().mgc_analyze_write(self._h, str(prefix).encode()), "mgc_analyze_write")
        return ["%s.%s.hist" % (prefix, name) for name, _ in FILES[self.type]]

    def info(self):
        i = capi.AnalyzeInfo()
        _check(capi.lib().mgc_analyze_get_info(self._h, ctypes.byref(i)), "mgc_analyze_get_info")
        return i.as_dict()
