"""ctypes plumbing for the database writer/reader (include/meryl_db.h)."""
import ctypes

import numpy as np

from . import capi


class DbError(RuntimeError):
    pass


def _err(what):
    s = capi.lib().mdb_last_error()
    return DbError("%s: %s" % (what, s.decode("utf-8", "replace") if s else ""))


class Writer:
    """merylFileWriter + merylBlockWriter for the count path."""

    def __init__(self, path, k, w_prefix, label_size=0, part=0, n_parts=1):
        """part / n_parts: one writer of a sharded database (finish with merge_parts once all are closed)."""
        self._h = capi.lib().mdb_writer_open_ex(path.encode(), k, w_prefix, label_size, part, n_parts)
        if not self._h:
            raise _err("mdb_writer_open")

    def add_block(self, prefix, suffix_lo, counts, suffix_hi=None, label=0, labels=None):
        """labels: one label per k-mer (their low label_size bits are stored); None: the constant `label` for all of them"""
        slo = np.ascontiguousarray(suffix_lo, dtype=np.uint64)
        cnt = np.ascontiguousarray(counts, dtype=np.uint32)
        shi = None if suffix_hi is None else np.ascontiguousarray(suffix_hi, dtype=np.uint64)
        lab = None if labels is None else np.ascontiguousarray(labels, dtype=np.uint64)
        if lab is not None and lab.size != slo.size:
            raise ValueError("labels: %d entries for %d k-mers" % (lab.size, slo.size))
        rc = capi.lib().mdb_writer_add_block_labelled(self._h, int(prefix), slo.size, slo.ctypes.data if slo.size else None,
                                                      shi.ctypes.data if shi is not None and shi.size else None,
                                                      cnt.ctypes.data if cnt.size else None,
                                                      lab.ctypes.data if lab is not None and lab.size else None, int(label))
        if rc != 0:
            raise _err("mdb_writer_add_block")

    def close(self):
        if self._h:
            rc = capi.lib().mdb_writer_close(self._h)
            self._h = None
            if rc != 0:
                raise _err("mdb_writer_close")


def merge_parts(path, n_parts):
    """Stitches the part files of a sharded database into the final 64+64+1 files (one caller, after every part closed)."""
    rc = capi.lib().mdb_merge_parts(path.encode(), int(n_parts))
    if rc != 0:
        raise _err("mdb_merge_parts")


def write_database(session, path, host_threads=8):
    """Count result of a meryl_amd.count.Session -> database directory."""
    rc = capi.lib().mgc_write_database(session._h, path.encode(), host_threads)
    if rc != 0:
        raise _err("mgc_write_database (%s)" % capi.last_error(session._h))


class Reader:
    def __init__(self, path):
        self._h = capi.lib().mdb_reader_open(path.encode())
        if not self._h:
            raise _err("mdb_reader_open")
        self.info = capi.DbInfo()
        capi.lib().mdb_reader_info(self._h, ctypes.byref(self.info))

    def histogram(self):
        n = self.info.hist_len
        v = np.zeros(n, dtype=np.uint64)
        o = np.zeros(n, dtype=np.uint64)
        if n:
            capi.lib().mdb_reader_histogram(self._h, v.ctypes.data, o.ctypes.data)
        return v, o

    def read_file(self, ff, labels=False):
        lo = ctypes.c_void_p()
        hi = ctypes.c_void_p()
        cn = ctypes.c_void_p()
        lb = ctypes.c_void_p()
        n = ctypes.c_uint64(0)
        rc = capi.lib().mdb_reader_read_file_ex(self._h, ff, ctypes.byref(lo), ctypes.byref(hi), ctypes.byref(cn),
                                                ctypes.byref(lb), ctypes.byref(n))
        if rc != 0:
            raise _err("mdb_reader_read_file")
        m = n.value

        def take(p, dtype):
            if m == 0:
                out = np.zeros(0, dtype=dtype)
            else:
                out = np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(np.ctypeslib.as_ctypes_type(dtype))),
                                            shape=(m,)).copy()
            capi.lib().mdb_free(p)
            return out

        out = (take(lo, np.uint64), take(hi, np.uint64), take(cn, np.uint32), take(lb, np.uint64))
        return out if labels else out[:3]

    def read_all(self, labels=False):
        cols = [[] for _ in range(4 if labels else 3)]
        for ff in range(64):
            for c, a in zip(cols, self.read_file(ff, labels)):
                c.append(a)
        return tuple(np.concatenate(c) for c in cols)

    def file_index(self, ff):
        """(prefix, position, n_kmers) rows of file ff's index"""
        n = 1 << self.info.num_blocks_bits
        arr = (capi.IndexEntry * n)()
        if capi.lib().mdb_reader_file_index(self._h, ff, arr) != 0:
            raise _err("mdb_reader_file_index")
        return [(e.prefix, e.position, e.n_kmers) for e in arr]

    def block_header(self, ff, position):
        h = capi.BlockHeader()
        if capi.lib().mdb_reader_block_header(self._h, ff, position, ctypes.byref(h)) != 0:
            raise _err("mdb_reader_block_header")
        return h

    def close(self):
        if self._h:
            capi.lib().mdb_reader_close(self._h)
            self._h = None


MERGE_WORDS = {"union-sum": 0, "union-min": 1, "union-max": 2, "intersect-sum": 3, "intersect-min": 4, "intersect-max": 5,
               "intersect": 6, "subtract": 7, "difference": 8, "symmetric-difference": 9, "union": 10}
VALUE_WORDS = {"less-than": 0, "greater-than": 1, "at-least": 2, "at-most": 3, "equal-to": 4, "not-equal-to": 5,
               "increase": 6, "decrease": 7, "multiply": 8, "divide": 9, "divide-round": 10, "modulo": 11}


def _label_option(label):
    """the "label" option of a node -> (MGC_LABEL_* code, constant): "or", ("and", 0x0F), or a number for the word"""
    if label is None:
        return capi.LABEL_OPS["default"], 0
    word, const = (label, None) if isinstance(label, (str, int)) else tuple(label)
    if isinstance(word, str) and word not in capi.LABEL_OPS:
        raise ValueError("unknown label operation '%s'" % word)
    code = capi.LABEL_OPS[word] if isinstance(word, str) else int(word)
    if const is None:
        const = int(capi.lib().mgc_label_default_constant(code))
    return code, int(const) & 0xFFFFFFFFFFFFFFFF


def parse_selector(words, n_inputs):
    """selector words ("input:2-all", "not", "value:@2>@1", "or", ...) of a node of n_inputs inputs -> list of capi.SelectTerm,
    through mgc_select_parse -- the one parser, which the command line uses too"""
    words = [w.encode() if isinstance(w, str) else bytes(w) for w in words]
    arr = (ctypes.c_char_p * max(len(words), 1))(*words)
    terms = (capi.SelectTerm * capi.SELECT_MAX_TERMS)()
    n = ctypes.c_uint32(0)
    rc = capi.lib().mgc_select_parse(arr, len(words), int(n_inputs), terms, capi.SELECT_MAX_TERMS, ctypes.byref(n))
    if rc != 0:
        msg = capi.lib().mgc_last_error(None)
        raise capi.MgcError(rc, "mgc_select_parse", msg.decode("utf-8", "replace") if msg else "")
    return [terms[i] for i in range(n.value)]


def parse_value_assign(text):
    """what follows value= on the command line ("sub", "max#5", "#1") -> (MGC_ASSIGN_* code, constant), through
    mgc_value_assign_parse -- the one parser, which the command line uses too"""
    code, const = ctypes.c_int32(0), ctypes.c_uint64(0)
    rc = capi.lib().mgc_value_assign_parse(text.encode() if isinstance(text, str) else bytes(text), ctypes.byref(code), ctypes.byref(const))
    if rc != 0:
        msg = capi.lib().mgc_last_error(None)
        raise capi.MgcError(rc, "mgc_value_assign_parse", msg.decode("utf-8", "replace") if msg else "")
    return code.value, const.value


def value_assign_option(value):
    """the "value" option of a node -> (MGC_ASSIGN_* code, constant): the command-line text ("sub#3"), (word, constant) with a word of
    capi.ASSIGN_OPS or a number for the word (a constant of None: the word's default), or None (no assignment)"""
    if value is None:
        return capi.ASSIGN_OPS["none"], 0
    if isinstance(value, (str, bytes)):
        return parse_value_assign(value)
    word, const = (value, None) if isinstance(value, int) else tuple(value)
    if isinstance(word, str) and word not in capi.ASSIGN_OPS:
        raise ValueError("unknown value assignment '%s'" % word)
    code = capi.ASSIGN_OPS[word] if isinstance(word, str) else int(word)
    if const is None:
        const = int(capi.lib().mgc_value_default_constant(code))
    return code, int(const) & 0xFFFFFFFFFFFFFFFF


def _walk(tree, allowed):
    """The one tree walk: `tree` is a database path, or (word, *children) for the merge operations, or (word, constant, child) for
    the value operations; a dict as the last element holds the node's options, of which only `allowed` are taken.
    -> ([node record], [children], root index); a record is a dict of kind, op, constant, path, first, n and the raw options
    label, select, value (None where not given), histogram and list (bools); children come before their parent.  A database is
    flagged for a histogram or a list as ({"database": path, "histogram": True, "list": True})."""
    nodes, kids = [], []

    def add(t):
        if isinstance(t, dict):                                     # a database with options: {"database": path, "histogram": True}
            flags = {"histogram", "list"} & set(allowed)             # what this entry point lets a database carry
            if set(t) - {"database"} - flags or "database" not in t or not flags:
                raise ValueError("a database with options is {'database': path, 'histogram': bool%s}: %r" % (", 'list': bool" if "list" in flags else "", t))
            i = add(t["database"])
            nodes[i]["histogram"] = bool(t.get("histogram"))
            nodes[i]["list"] = bool(t.get("list"))
            return i
        if isinstance(t, (str, bytes)):
            nodes.append(dict(kind=capi.NODE_DATABASE, op=0, constant=0, path=t if isinstance(t, bytes) else t.encode(), first=0, n=0,
                              label=None, select=None, value=None, histogram=False, list=False))
            return len(nodes) - 1
        t = tuple(t)
        opts = {}
        if t and isinstance(t[-1], dict):
            opts = dict(t[-1])
            t = t[:-1]
        unknown = sorted(set(opts) - set(allowed))
        if unknown:
            raise ValueError("unknown options %r" % unknown)
        if not t or not isinstance(t[0], str):
            raise ValueError("an operation is (word, ...): %r" % (t,))
        word = t[0]
        if word in VALUE_WORDS:
            if len(t) != 3:
                raise ValueError("'%s' takes a constant and one input" % word)
            kind, op, constant, args = capi.NODE_VALUE, VALUE_WORDS[word], int(t[1]), t[2:]
        elif word in MERGE_WORDS:
            kind, op, constant, args = capi.NODE_MERGE, MERGE_WORDS[word], 0, t[1:]
        else:
            raise ValueError("unknown operation '%s'" % word)
        ch = [add(a) for a in args]
        out, words = opts.get("output"), opts.get("select")
        nodes.append(dict(kind=kind, op=op, constant=constant, path=None if out is None else (out if isinstance(out, bytes) else out.encode()),
                          first=len(kids), n=len(ch), label=opts.get("label"), value=opts.get("value"), histogram=bool(opts.get("histogram")), list=bool(opts.get("list")),
                          select=None if words is None else ([words] if isinstance(words, str) else list(words))))
        kids.extend(ch)
        return len(nodes) - 1

    root = add(tree)
    return nodes, kids, root


def _fill(struct, tree, allowed):
    """_walk -> an array of `struct` with the fields of the options in `allowed` set: label -> label_op / label_constant, select ->
    first_term / n_terms (parsed for the node's input count), value -> value_assign / value_constant.
    -> (array, children array, number of children, root index, SelectTerm array, number of terms, the node records of _walk)"""
    nodes, kids, root = _walk(tree, allowed)
    arr = (struct * len(nodes))()
    for e, r in zip(arr, nodes):
        e.kind, e.op, e.constant, e.path, e.first_child, e.n_children = r["kind"], r["op"], r["constant"], r["path"], r["first"], r["n"]
    inner = [(e, r) for e, r in zip(arr, nodes) if r["kind"] != capi.NODE_DATABASE]
    if "label" in allowed:
        for e, r in inner:
            e.label_op, e.label_constant = _label_option(r["label"])
    terms = []
    if "select" in allowed:
        for e, r in zip(arr, nodes):
            e.first_term, e.n_terms = len(terms), 0
            if r["select"]:
                got = parse_selector(r["select"], r["n"])
                e.n_terms = len(got)
                terms.extend(got)
    if "value" in allowed:
        for e, r in inner:
            e.value_assign, e.value_constant = value_assign_option(r["value"])
    return arr, (ctypes.c_uint32 * max(len(kids), 1))(*kids), len(kids), root, (capi.SelectTerm * max(len(terms), 1))(*terms), len(terms), nodes


def build_tree(tree):
    """A tree of operations -> (EvalNode array, children array, number of children, root index) for mgc_db_eval.  `tree` is a
    database path, or (word, *children) for the merge operations, or (word, constant, child) for the value operations; a dict
    {"output": path} as the last element names the database the node writes."""
    return _fill(capi.EvalNode, tree, ("output",))[:4]


def build_tree_labelled(tree):
    """build_tree for mgc_db_eval_labelled: the same trees, and the options dict of a node also takes "label": a word of
    capi.LABEL_OPS ("or"), or (word, constant) (("and", 0x0F)); without it the node's label operation is the default of its
    operation.  -> (EvalNodeLabelled array, children array, number of children, root index)"""
    return _fill(capi.EvalNodeLabelled, tree, ("output", "label"))[:4]


def build_tree_selected(tree):
    """build_tree_labelled for mgc_db_eval_selected: the options dict of a node also takes "select": [words...], the selector
    words of the command line, parsed for the node's input count.
    -> (EvalNodeSelected array, children array, number of children, root index, SelectTerm array, number of terms)"""
    return _fill(capi.EvalNodeSelected, tree, ("output", "label", "select"))[:6]


def build_tree_assigned(tree):
    """build_tree_selected for mgc_db_eval_assigned: the options dict of a node also takes "value": what follows value= on the
    command line ("sub#3") or (word, constant) (value_assign_option).
    -> (EvalNodeAssigned array, children array, number of children, root index, SelectTerm array, number of terms)"""
    return _fill(capi.EvalNodeAssigned, tree, ("output", "label", "select", "value"))[:6]


def _evaluate(name, call, on_slice, labelled=True):
    """One evaluation through entry point `name`: call(cb) makes the native call with the slice callback; on_slice receives numpy
    copies (file, lo, hi_or_None, values[, labels]); an exception it raises is relayed once the native call has returned."""
    failure = []

    def trampoline(ctx, ff, lo, hi, vals, *rest):
        n = rest[-1]
        try:
            def take(p, dtype):
                return np.ctypeslib.as_array(p, shape=(n,)).astype(dtype, copy=True) if n else np.zeros(0, dtype=dtype)
            on_slice(ff, take(lo, np.uint64), take(hi, np.uint64) if hi else None, take(vals, np.uint32), *[take(p, np.uint64) for p in rest[:-1]])
        except BaseException as e:                               # not through the C frames
            failure.append(e)

    cb_type = capi.EVAL_SLICE_LABELLED_CB if labelled else capi.EVAL_SLICE_CB
    rc = call(cb_type(trampoline) if on_slice is not None else ctypes.cast(None, cb_type))
    if failure:
        raise failure[0]
    if rc != 0:
        msg = capi.lib().mgc_db_stream_error(None)
        raise capi.MgcError(rc, name, msg.decode("utf-8", "replace") if msg else "")


def evaluate(tree, on_slice=None, device=-1, host_threads=8):
    """A whole tree of merge / value operations over databases in ONE pass over the 64 file slices, intermediate results
    kept in HBM (mgc_db_eval).  Nodes given {"output": path} write a database; on_slice(file, lo, hi_or_None, values)
    receives the root's slices (numpy copies), files ascending."""
    arr, kids, n_kids, root = build_tree(tree)
    _evaluate("mgc_db_eval", lambda cb: capi.lib().mgc_db_eval(arr, len(arr), kids, n_kids, root, cb, None, device, host_threads), on_slice,
              labelled=False)


def evaluate_labelled(tree, on_slice=None, label_size=0, device=-1, host_threads=8):
    """evaluate() over databases that may store labels (mgc_db_eval_labelled): every node combines the labels of the inputs
    that hold a k-mer with its "label" option (build_tree_labelled), outputs store label_size bits per k-mer (0: the largest
    label size among the leaves), and on_slice(file, lo, hi_or_None, values, labels) also receives the root's labels as
    full 64-bit values."""
    arr, kids, n_kids, root = build_tree_labelled(tree)
    _evaluate("mgc_db_eval_labelled",
              lambda cb: capi.lib().mgc_db_eval_labelled(arr, len(arr), kids, n_kids, root, int(label_size), cb, None, device, host_threads), on_slice)


def evaluate_selected(tree, on_slice=None, with_labels=False, label_size=0, device=-1, host_threads=8):
    """evaluate_labelled() for trees whose nodes may carry selectors (mgc_db_eval_selected).  Labels travel when with_labels
    or label_size is set or a label: selector asks for them; otherwise the tree is evaluated as evaluate() does, and
    on_slice(file, lo, hi_or_None, values, labels) receives zeros for labels."""
    arr, kids, n_kids, root, terms, n_terms = build_tree_selected(tree)
    _evaluate("mgc_db_eval_selected",
              lambda cb: capi.lib().mgc_db_eval_selected(arr, len(arr), kids, n_kids, root, terms, n_terms, int(bool(with_labels)), int(label_size), cb,
                                                         None, device, host_threads), on_slice)


def evaluate_assigned(tree, on_slice=None, with_labels=False, label_size=0, device=-1, host_threads=8):
    """evaluate_selected() for trees whose nodes may carry value assignments (mgc_db_eval_assigned): a node with {"value": ...}
    keeps the presence rule of its operation and computes the value of a written k-mer by the assignment; k-mers whose assigned
    value is 0 are not written, and the node's selector and a value filter see the assigned value."""
    arr, kids, n_kids, root, terms, n_terms = build_tree_assigned(tree)
    _evaluate("mgc_db_eval_assigned",
              lambda cb: capi.lib().mgc_db_eval_assigned(arr, len(arr), kids, n_kids, root, terms, n_terms, int(bool(with_labels)), int(label_size), cb,
                                                         None, device, host_threads), on_slice)


def build_tree_reported(tree):
    """build_tree_assigned for mgc_db_eval_reported: the options dict of a node also takes "histogram": True -- the value histogram
    of that node's result is collected; a database is flagged as {"database": path, "histogram": True}.
    -> (EvalNodeAssigned array, children array, number of children, root index, SelectTerm array, number of terms, want array)"""
    allowed = ("output", "label", "select", "value", "histogram")
    filled = _fill(capi.EvalNodeAssigned, tree, allowed)
    return filled[:6] + ((ctypes.c_uint8 * len(filled[6]))(*[1 if r["histogram"] else 0 for r in filled[6]]),)


class ValueHistogram:
    """The value-histogram accumulator (mgc_value_hist_*, include/meryl_db.h) over torch device tensors of uint32 values (any 4-byte
    integer dtype: the bits are taken as uint32): add() any number of tensors, then get() / totals()."""

    def __init__(self, device=-1, handle=None):
        self._h = handle if handle is not None else capi.lib().mgc_value_hist_open(int(device))
        if not self._h:
            raise DbError("mgc_value_hist_open failed")

    @staticmethod
    def geometry():
        """(dense limit D: values below it are counted in LDS bins; values one workgroup takes per iteration)"""
        d, w = ctypes.c_uint32(0), ctypes.c_uint32(0)
        capi.lib().mgc_value_hist_geometry(ctypes.byref(d), ctypes.byref(w))
        return d.value, w.value

    def _check(self, rc, what):
        if rc != 0:
            msg = capi.lib().mgc_db_stream_error(None)
            raise capi.MgcError(rc, what, msg.decode("utf-8", "replace") if msg else "")

    def add(self, values):
        """values: a contiguous torch tensor on the device, 4 bytes per element"""
        import torch
        if not values.is_cuda or not values.is_contiguous() or values.element_size() != 4:
            raise ValueError("ValueHistogram.add takes a contiguous device tensor of 4-byte values")
        n = values.numel()
        stream = torch.cuda.current_stream(values.device).cuda_stream
        self._check(capi.lib().mgc_value_hist_add(self._h, values.data_ptr() if n else None, n, stream), "mgc_value_hist_add")

    def get(self):
        """(values, occurrences) as uint64 numpy arrays, ascending by value"""
        n = ctypes.c_uint64(0)
        self._check(capi.lib().mgc_value_hist_len(self._h, ctypes.byref(n)), "mgc_value_hist_len")
        v = np.zeros(n.value, dtype=np.uint64)
        o = np.zeros(n.value, dtype=np.uint64)
        self._check(capi.lib().mgc_value_hist_get(self._h, v.ctypes.data if n.value else None, o.ctypes.data if n.value else None), "mgc_value_hist_get")
        return v, o

    def totals(self):
        """(unique, distinct, total): occurrences of value 1, sum of occurrences, sum(value * occurrences) in uint64"""
        u, d, t = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
        self._check(capi.lib().mgc_value_hist_totals(self._h, ctypes.byref(u), ctypes.byref(d), ctypes.byref(t)), "mgc_value_hist_totals")
        return u.value, d.value, t.value

    def close(self):
        if self._h:
            capi.lib().mgc_value_hist_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def format_statistics(k, values, occurrences, unique, distinct, total):
    """the text of `meryl statistics` for a histogram (mdb_format_statistics)"""
    v = np.ascontiguousarray(values, dtype=np.uint64)
    o = np.ascontiguousarray(occurrences, dtype=np.uint64)
    args = (int(k), v.ctypes.data if v.size else None, o.ctypes.data if o.size else None, v.size, int(unique), int(distinct), int(total))
    n = capi.lib().mdb_format_statistics(*args, None, 0)
    buf = ctypes.create_string_buffer(n + 1)
    capi.lib().mdb_format_statistics(*args, buf, n + 1)
    return buf.value.decode()


def evaluate_reported(tree, on_slice=None, with_labels=False, label_size=0, device=-1, host_threads=8):
    """evaluate_assigned() that also collects value histograms (mgc_db_eval_reported): every node given {"histogram": True} (a
    database: {"database": path, "histogram": True}) has the values of its result counted on the device, slice by slice.
    -> [(values, occurrences)] as uint64 numpy arrays ascending by value, for the flagged nodes in pre-order (a node before its
    inputs, inputs left to right)."""
    arr, kids, n_kids, root, terms, n_terms, want = build_tree_reported(tree)
    hists = (ctypes.c_void_p * len(arr))()
    _evaluate("mgc_db_eval_reported",
              lambda cb: capi.lib().mgc_db_eval_reported(arr, len(arr), kids, n_kids, root, terms, n_terms, int(bool(with_labels)), int(label_size), cb,
                                                         None, device, host_threads, want, hists), on_slice)
    return _read_hists(arr, kids, root, want, hists)


def _read_hists(arr, kids, root, want, hists):
    """the accumulators an evaluation returned -> [(values, occurrences)] for the flagged nodes in pre-order; closes them"""
    order = []

    def pre(v):
        order.append(v)
        for i in range(arr[v].n_children):
            pre(kids[arr[v].first_child + i])
    pre(root)
    out = []
    for v in order:
        if want[v]:
            h = ValueHistogram(handle=hists[v])
            out.append(h.get())
            h.close()
    return out


def build_tree_listed(tree):
    """build_tree_reported for mgc_db_eval_listed: the options dict of a node also takes "list": True -- the text of that node's
    result is handed over; a database is flagged as {"database": path, "list": True}.
    -> (..., want-histogram array, want-list array)"""
    allowed = ("output", "label", "select", "value", "histogram", "list")
    filled = _fill(capi.EvalNodeAssigned, tree, allowed)
    flags = lambda key: (ctypes.c_uint8 * len(filled[6]))(*[1 if r[key] else 0 for r in filled[6]])      # noqa: E731
    return filled[:6] + (flags("histogram"), flags("list"))


def list_geometry(k, label_size=0):
    """(the longest line in bytes, the k-mers of one tile of the list kernels) for (k, label_size)"""
    return capi.lib().mgc_list_max_line(int(k), int(label_size)), capi.lib().mgc_list_tile_kmers(int(k), int(label_size))


def list_slice_name(name, file):
    """the list file of slice `file` for a name with '#' (mgc_list_slice_name); None for a name without"""
    raw = name.encode() if isinstance(name, str) else bytes(name)
    buf = ctypes.create_string_buffer(len(raw) + 80)
    n = capi.lib().mgc_list_slice_name(raw, int(file), buf, len(buf))
    return buf.raw[:n].decode() if n else None


LIST_CHUNK = 16 << 20


def format_kmers_device(keys, values, labels=None, *, k, label_size=0):
    """format_kmers that leaves the text on the device: -> a uint8 CUDA tensor (mgc_dev_list_lengths + mgc_dev_list_format)"""
    import torch
    L, n = capi.lib(), values.numel()
    stream = torch.cuda.current_stream(values.device).cuda_stream
    ws = torch.empty(max(L.mgc_dev_list_workspace_bytes(n, int(k), int(label_size)), 8), dtype=torch.uint8, device=values.device)
    total = ctypes.c_uint64(0)
    rc = L.mgc_dev_list_lengths(values.data_ptr() if n else None, n, int(k), int(label_size), ws.data_ptr(), ws.numel(), ctypes.byref(total), stream)
    text = torch.empty(total.value, dtype=torch.uint8, device=values.device)
    if rc == 0 and n:
        rc = L.mgc_dev_list_format(keys.data_ptr(), values.data_ptr(), labels.data_ptr() if labels is not None else None, n, int(k), int(label_size),
                                   ws.data_ptr(), ws.numel(), text.data_ptr(), stream)
    if rc != 0:
        msg = L.mgc_db_stream_error(None)
        raise capi.MgcError(rc, "mgc_dev_list_format", msg.decode("utf-8", "replace") if msg else "")
    return text


def format_kmers(keys, values, labels=None, *, k, label_size=0, chunk_bytes=LIST_CHUNK, on_piece=None):
    """The text of device-resident k-mers (mgc_list_kmers): keys a contiguous CUDA tensor of 8-byte integers, one per k-mer for
    k <= 32 and (lo, hi) pairs for k > 32; values 4-byte integers; labels 8-byte integers or None (zeros).  -> bytes: the lines
    `k-mer <TAB> value [<TAB> label] <NL>`.  on_piece(bytes) sees every piece as it leaves the device (at most chunk_bytes each,
    whole lines); a true return stops the listing (MgcError, MGC_ESTATE)."""
    import torch
    n = values.numel()
    tensors = [("keys", keys, 8, n * (2 if k > 32 else 1)), ("values", values, 4, n)] + ([("labels", labels, 8, n)] if labels is not None else [])
    for name, t, size, count in tensors:
        if not t.is_cuda or not t.is_contiguous() or t.element_size() != size or t.numel() != count:
            raise ValueError("format_kmers: %s must be a contiguous device tensor of %d %d-byte integers" % (name, count, size))
    pieces, failure = [], []

    def trampoline(text, nbytes, user):
        try:
            piece = ctypes.string_at(text, nbytes)
            pieces.append(piece)
            return 1 if on_piece is not None and on_piece(piece) else 0
        except BaseException as e:                               # not through the C frames
            failure.append(e)
            return 1

    stream = torch.cuda.current_stream(values.device).cuda_stream
    with torch.cuda.device(values.device):
        rc = capi.lib().mgc_list_kmers(keys.data_ptr() if n else None, values.data_ptr() if n else None,
                                       labels.data_ptr() if labels is not None and n else None, n, int(k), int(label_size), int(chunk_bytes),
                                       capi.LIST_WRITE_CB(trampoline), None, stream)
    if failure:
        raise failure[0]
    if rc != 0:
        msg = capi.lib().mgc_db_stream_error(None)
        raise capi.MgcError(rc, "mgc_list_kmers", msg.decode("utf-8", "replace") if msg else "")
    return b"".join(pieces)


def evaluate_listed(tree, on_text, on_slice=None, with_labels=False, label_size=0, device=-1, host_threads=8):
    """evaluate_reported() that also lists results as text (mgc_db_eval_listed): every node given {"list": True} (a database:
    {"database": path, "list": True}) has the k-mers of its result formatted on the device, slice by slice, and
    on_text(node_index, file, bytes) receives the text in pieces of whole lines -- node_index in the order of build_tree_listed
    (children before their parent), files ascending.  -> the histograms of the flagged nodes, as evaluate_reported."""
    arr, kids, n_kids, root, terms, n_terms, want, want_list = build_tree_listed(tree)
    hists = (ctypes.c_void_p * len(arr))()
    failure = []

    def text_trampoline(user, node, ff, text, nbytes):
        try:
            on_text(node, ff, ctypes.string_at(text, nbytes))
            return 0
        except BaseException as e:                               # not through the C frames
            failure.append(e)
            return 1

    list_cb = capi.EVAL_LIST_CB(text_trampoline) if on_text is not None else ctypes.cast(None, capi.EVAL_LIST_CB)
    try:
        _evaluate("mgc_db_eval_listed",
                  lambda cb: capi.lib().mgc_db_eval_listed(arr, len(arr), kids, n_kids, root, terms, n_terms, int(bool(with_labels)), int(label_size), cb,
                                                           None, device, host_threads, want, hists, want_list, list_cb, None), on_slice)
    except capi.MgcError:
        if failure:
            raise failure[0]
        raise
    return _read_hists(arr, kids, root, want, hists)
