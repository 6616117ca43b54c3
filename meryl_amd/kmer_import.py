"""ctypes/torch plumbing of `meryl-import` (include/meryl_import.h): `kmer value` text -> database, and its device steps.
With label_width 1..64 (include/meryl_import_labelled.h): the meryl 2 dialect, `kmer value label` text -> labelled database.

Keys are int64 tensors holding the uint64 bit patterns: shape [n] for k <= 32, [n, 2] ({lo, hi}) above; values are int32
tensors holding uint32 bit patterns; labels are int64 tensors holding uint64 bit patterns.  There is no CPU path: everything here launches the library's HIP kernels."""
import ctypes

from . import capi

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

BAD_NAMES = {0: None, 1: "base", 2: "short", 3: "value", 4: "hash", 5: "label", 6: "assign"}
MIN_K, MAX_K, W_PREFIX = 6, 64, 10
W_PREFIX_LABELLED = 6


class ImportRefused(capi.MgcError):
    """The text holds a line meryl-import refuses: .line (1-based) and .kind ("base", "short", "value", "hash";
    with a label width also "label", "assign")."""

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


def import_file(path, k, output, mode=capi.MODE_CANONICAL, device=-1, host_threads=0, label_width=0):
    """mgc_import_file: the text file at `path` ("-": standard input; plain or gzip) -> database directory `output`.
    label_width 1..64: mgc_import_labelled_file, the meryl 2 dialect."""
    info = capi.ImportInfo()
    if label_width:
        rc = capi.lib().mgc_import_labelled_file(str(path).encode(), k, mode, label_width, str(output).encode(), device, host_threads,
                                                 ctypes.byref(info))
        return _finish(rc, info)
    rc = capi.lib().mgc_import_file(str(path).encode(), k, mode, str(output).encode(), device, host_threads, ctypes.byref(info))
    return _finish(rc, info)


def import_text(text, k, output, mode=capi.MODE_CANONICAL, device=-1, host_threads=0, label_width=0):
    """mgc_import_text: `text` (bytes / str / a uint8 numpy array) -> database directory `output`.
    label_width 1..64: mgc_import_labelled_text, the meryl 2 dialect."""
    if isinstance(text, str):
        text = text.encode("ascii")
    info = capi.ImportInfo()
    if isinstance(text, (bytes, bytearray)):
        buf, n = bytes(text), len(text)
    else:                                                   # numpy uint8, contiguous
        buf, n = ctypes.cast(ctypes.c_void_p(text.ctypes.data), ctypes.c_char_p), int(text.size)
    if label_width:
        rc = capi.lib().mgc_import_labelled_text(buf, n, k, mode, label_width, str(output).encode(), device, host_threads, ctypes.byref(info))
    else:
        rc = capi.lib().mgc_import_text(buf, n, k, mode, str(output).encode(), device, host_threads, ctypes.byref(info))
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

    def __init__(self, k, mode=capi.MODE_CANONICAL, label_width=0, device="cuda"):
        self.k, self.mode, self.label_width = k, mode, label_width
        L = capi.lib()
        if label_width:                                     # the meryl 2 dialect: both persistent words live in the state
            self.persistent_label = 0
            self.state = torch.zeros(L.mgc_dev_import2_parse_state_bytes(), dtype=torch.uint8, device=device)
            capi.check(L.mgc_dev_import2_parse_begin(_ptr(self.state), _stream()), "mgc_dev_import2_parse_begin")
            return
        self.state = torch.zeros(L.mgc_dev_import_parse_state_bytes(), dtype=torch.uint8, device=device)
        capi.check(L.mgc_dev_import_parse_begin(_ptr(self.state), _stream()), "mgc_dev_import_parse_begin")

    def parse(self, text):
        """-> (keys, values, ImportParseResult); keys / values are None when the chunk is refused (result.bad_kind != 0).
        With a label width: (keys, values, labels, result), and .persistent_label is the label that holds after the chunk."""
        if self.label_width:
            return self._parse_labelled(text)
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

    def _parse_labelled(self, text):
        L = capi.lib()
        n = int(text.numel())
        ws = torch.empty(L.mgc_dev_import2_parse_workspace_bytes(n), dtype=torch.uint8, device=text.device)
        res = capi.ImportParseResult()
        plab = ctypes.c_uint64(0)
        rc = L.mgc_dev_import2_parse_count(_ptr(text), n, self.k, self.label_width, _ptr(self.state), _ptr(ws), ws.numel(), ctypes.byref(res),
                                           ctypes.byref(plab), _stream())
        if rc != capi.MGC_OK:
            raise capi.MgcError(rc, "mgc_dev_import2_parse_count", _error())
        if res.bad_kind:
            return None, None, None, res
        self.persistent_label = int(plab.value)
        nr = int(res.n_records)
        keys = torch.empty((nr, 2) if self.k > 32 else (nr,), dtype=torch.int64, device=text.device)
        vals = torch.empty(nr, dtype=torch.int32, device=text.device)
        labs = torch.empty(nr, dtype=torch.int64, device=text.device)
        rc = L.mgc_dev_import2_parse(_ptr(text), n, self.k, self.mode, self.label_width, _ptr(self.state), _ptr(ws), ws.numel(), _ptr(keys),
                                     _ptr(vals), _ptr(labs), _stream())
        if rc != capi.MGC_OK:
            raise capi.MgcError(rc, "mgc_dev_import2_parse", _error())
        torch.cuda.current_stream().synchronize()
        return keys, vals, labs, res


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


def sort_triples(keys, values, labels, begin_bit, end_bit):
    """mgc_dev_sort_triples -> (sorted keys, their values, their labels); equal keys keep their input order"""
    L = capi.lib()
    n = int(keys.shape[0])
    ak, av, al = torch.empty_like(keys), torch.empty_like(values), torch.empty_like(labels)
    ws = torch.empty(L.mgc_dev_sort_triples_workspace_bytes(n), dtype=torch.uint8, device=keys.device)
    in_alt = ctypes.c_int(0)
    rc = L.mgc_dev_sort_triples(_ptr(keys), _ptr(values), _ptr(labels), _ptr(ak), _ptr(av), _ptr(al), n, _key_words(keys), begin_bit, end_bit,
                                _ptr(ws), ws.numel(), ctypes.byref(in_alt), _stream())
    if rc != capi.MGC_OK:
        raise capi.MgcError(rc, "mgc_dev_sort_triples", _error())
    torch.cuda.current_stream().synchronize()
    return (ak, av, al) if in_alt.value else (keys, values, labels)


def reduce_triples(keys, values, labels, label_width):
    """mgc_dev_reduce_triples_count + _emit over triples sorted by key -> (distinct keys, wrapped uint32 value sums, label sums
    modulo 2^label_width)"""
    L = capi.lib()
    n = int(keys.shape[0])
    kw = _key_words(keys)
    ws = torch.empty(L.mgc_dev_reduce_triples_workspace_bytes(n), dtype=torch.uint8, device=keys.device)
    nd = ctypes.c_uint64(0)
    rc = L.mgc_dev_reduce_triples_count(_ptr(keys), _ptr(values), _ptr(labels), n, kw, _ptr(ws), ws.numel(), ctypes.byref(nd), _stream())
    if rc != capi.MGC_OK:
        raise capi.MgcError(rc, "mgc_dev_reduce_triples_count", _error())
    ok = torch.empty((nd.value, 2) if kw == 2 else (nd.value,), dtype=torch.int64, device=keys.device)
    ov = torch.empty(nd.value, dtype=torch.int32, device=keys.device)
    ol = torch.empty(nd.value, dtype=torch.int64, device=keys.device)
    rc = L.mgc_dev_reduce_triples_emit(_ptr(keys), _ptr(values), _ptr(labels), n, kw, label_width, _ptr(ws), ws.numel(), _ptr(ok), _ptr(ov),
                                       _ptr(ol), _stream())
    if rc != capi.MGC_OK:
        raise capi.MgcError(rc, "mgc_dev_reduce_triples_emit", _error())
    torch.cuda.current_stream().synchronize()
    return ok, ov, ol
