"""ctypes/torch plumbing of `meryl-import` (include/meryl_import.h): `kmer value` text -> database, and its device steps.

Keys are int64 tensors holding the uint64 bit patterns: shape [n] for k <= 32, [n, 2] ({lo, hi}) above; values are int32
tensors holding uint32 bit patterns.  There is no CPU path: everything here launches the library's HIP kernels."""
import ctypes

from . import capi

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

BAD_NAMES = {0: None, 1: "base", 2: "short", 3: "value", 4: "hash"}
MIN_K, MAX_K, W_PREFIX = 6, 64, 10


class ImportRefused(capi.MgcError):
    """The text holds a line meryl-import refuses: .line (1-based) and .kind ("base", "short", "value", "hash")."""

    def __init__(self, rc, info, detail):
        super().__init__(rc, "meryl-import", detail)
        self.line = int(info.bad_line)
        self.kind = BAD_NAMES.get(int(info.bad_kind))


def _error():
    s = capi.lib().mgc_import_error()
    return s.decode("utf-8", "replace") if s else ""


def _finish(rc, info):
    if rc == capi.EFORMAT and info.bad_kind:
        raise ImportRefused(rc, info, _error())
    if rc != capi.MGC_OK:
        raise capi.MgcError(rc, "meryl-import", _error())
    return info.as_dict()


def import_file(path, k, output, mode=capi.MODE_CANONICAL, device=-1, host_threads=0):
    """mgc_import_file: the text file at `path` ("-": standard input; plain or gzip) -> database directory `output`."""
    info = capi.ImportInfo()
    rc = capi.lib().mgc_import_file(str(path).encode(), k, mode, str(output).encode(), device, host_threads, ctypes.byref(info))
    return _finish(rc, info)


def import_text(text, k, output, mode=capi.MODE_CANONICAL, device=-1, host_threads=0):
    """mgc_import_text: `text` (bytes / str / a uint8 numpy array) -> database directory `output`."""
    if isinstance(text, str):
        text = text.encode("ascii")
    info = capi.ImportInfo()
    if isinstance(text, (bytes, bytearray)):
        buf, n = bytes(text), len(text)
        rc = capi.lib().mgc_import_text(buf, n, k, mode, str(output).encode(), device, host_threads, ctypes.byref(info))
    else:                                                   # numpy uint8, contiguous
        n = int(text.size)
        rc = capi.lib().mgc_import_text(ctypes.cast(ctypes.c_void_p(text.ctypes.data), ctypes.c_char_p), n, k, mode,
                                        str(output).encode(), device, host_threads, ctypes.byref(info))
    return _finish(rc, info)


# ---- the device steps on their own, over torch tensors ---------------------------------------------------------------
def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else ctypes.c_void_p(0)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _key_words(keys):
    return 2 if keys.dim() == 2 else 1


class Parser:
    """The line parser with its state on the device: feed chunks of whole lines (uint8 cuda tensors) in order."""

    def __init__(self, k, mode=capi.MODE_CANONICAL, device="cuda"):
        self.k, self.mode = k, mode
        L = capi.lib()
        self.state = torch.zeros(L.mgc_dev_import_parse_state_bytes(), dtype=torch.uint8, device=device)
        capi.check(L.mgc_dev_import_parse_begin(_ptr(self.state), _stream()), "mgc_dev_import_parse_begin")

    def parse(self, text):
        """-> (keys, values, ImportParseResult); keys / values are None when the chunk is refused (result.bad_kind != 0)"""
        L = capi.lib()
        n = int(text.numel())
        ws = torch.empty(L.mgc_dev_import_parse_workspace_bytes(n), dtype=torch.uint8, device=text.device)
        res = capi.ImportParseResult()
        rc = L.mgc_dev_import_parse_count(_ptr(text), n, self.k, _ptr(self.state), _ptr(ws), ws.numel(), ctypes.byref(res), _stream())
        if rc != capi.MGC_OK:
            raise capi.MgcError(rc, "mgc_dev_import_parse_count", _error())
        if res.bad_kind:
            return None, None, res
        nr = int(res.n_records)
        keys = torch.empty((nr, 2) if self.k > 32 else (nr,), dtype=torch.int64, device=text.device)
        vals = torch.empty(nr, dtype=torch.int32, device=text.device)
        rc = L.mgc_dev_import_parse(_ptr(text), n, self.k, self.mode, _ptr(self.state), _ptr(ws), ws.numel(), _ptr(keys), _ptr(vals), _stream())
        if rc != capi.MGC_OK:
            raise capi.MgcError(rc, "mgc_dev_import_parse", _error())
        torch.cuda.current_stream().synchronize()
        return keys, vals, res


def sort_pairs(keys, values, begin_bit, end_bit):
    """mgc_dev_sort_pairs -> (sorted keys, their values); the inputs are used as one of the two ping-pong buffer pairs"""
    L = capi.lib()
    n = int(keys.shape[0])
    ak, av = torch.empty_like(keys), torch.empty_like(values)
    ws = torch.empty(L.mgc_dev_sort_pairs_workspace_bytes(n), dtype=torch.uint8, device=keys.device)
    in_alt = ctypes.c_int(0)
    rc = L.mgc_dev_sort_pairs(_ptr(keys), _ptr(values), _ptr(ak), _ptr(av), n, _key_words(keys), begin_bit, end_bit, _ptr(ws), ws.numel(),
                              ctypes.byref(in_alt), _stream())
    if rc != capi.MGC_OK:
        raise capi.MgcError(rc, "mgc_dev_sort_pairs", _error())
    torch.cuda.current_stream().synchronize()
    return (ak, av) if in_alt.value else (keys, values)


def reduce_pairs(keys, values):
    """mgc_dev_reduce_pairs_count + _emit over pairs sorted by key -> (distinct keys, wrapped uint32 sums)"""
    L = capi.lib()
    n = int(keys.shape[0])
    kw = _key_words(keys)
    ws = torch.empty(L.mgc_dev_reduce_pairs_workspace_bytes(n), dtype=torch.uint8, device=keys.device)
    nd = ctypes.c_uint64(0)
    rc = L.mgc_dev_reduce_pairs_count(_ptr(keys), _ptr(values), n, kw, _ptr(ws), ws.numel(), ctypes.byref(nd), _stream())
    if rc != capi.MGC_OK:
        raise capi.MgcError(rc, "mgc_dev_reduce_pairs_count", _error())
    ok = torch.empty((nd.value, 2) if kw == 2 else (nd.value,), dtype=torch.int64, device=keys.device)
    ov = torch.empty(nd.value, dtype=torch.int32, device=keys.device)
    rc = L.mgc_dev_reduce_pairs_emit(_ptr(keys), _ptr(values), n, kw, _ptr(ws), ws.numel(), _ptr(ok), _ptr(ov), _stream())
    if rc != capi.MGC_OK:
        raise capi.MgcError(rc, "mgc_dev_reduce_pairs_emit", _error())
    torch.cuda.current_stream().synchronize()
    return ok, ov
