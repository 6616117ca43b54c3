// mgc_eval.cpp -- operations over whole databases (include/meryl_db.h): mgc_db_merge, mgc_db_filter, and the operation trees of
// mgc_db_eval, mgc_db_eval_labelled, mgc_db_eval_selected, mgc_db_eval_assigned, mgc_db_eval_reported and mgc_db_eval_listed.  Inputs are decoded on the device, every
// operation is a count / emit pass pair over slices in HBM, and outputs go through the database stream (mgc_stream.cpp).  mgc_db_eval_listed
// also hands the flagged nodes' results to the text lister (mgc_list.hip).
#include "../../include/meryl_db.h"
#include "mdb_layout.h"
#include "mgc_dbfile.hpp"
#include "mgc_list.hpp"
#include "mgc_session.hpp"
#include "mgc_route.hpp"
#include "mgc_selector.hpp"
#include "mgc_value.hpp"

#include <algorithm>
#include <map>
#include <memory>
#include <thread>
#include <type_traits>

using mgc::DBuf;
using mgc::decode_on_host;
using mgc::set_err;

// ================================================================================================
//  union-sum & friends over whole databases
// ================================================================================================
// The reference streams the 64 file slices of its inputs through merylOperation::nextMer -- smallest k-mer over the
// inputs, values of the inputs that hold it combined (src/meryl/merylOp-nextMer.C:418-683; one slice per thread,
// src/meryl/meryl.C:250-263).  Here a slice is decoded by host threads (one per input), merged two inputs at a time on the
// device (mgc_merge.hip), encoded on the device and written by the database stream -- the same merge that folds the
// batches of an out-of-core count.
namespace {
// The slice (file ff) of every input in HBM: in_k[i] / in_c[i] / hn[i].  One host thread per input reads the data file (mgc_dbfile.hpp:
// raw, or host-decoded where only the host decoder follows the framing or under MGC_DECODE_HOST=1, which every entry point reads once);
// then the files are uploaded and decoded one after the other.
// in_l (the labelled evaluation; null otherwise): the labels of the inputs that store some, beside the values; an input without
// labels gets no buffer (its labels are zeros)
int load_slices(std::vector<mdb_reader *> &rd, uint32_t ff, uint32_t kw, std::vector<DBuf> &in_k, std::vector<DBuf> &in_c,
                std::vector<uint64_t> &hn, hipStream_t st, std::string *msg, bool host_decode, std::vector<DBuf> *in_l = nullptr) {
  const uint32_t n_inputs = (uint32_t)rd.size();
  std::vector<mgc::DbFile> file(n_inputs);
  {
    std::vector<std::thread> th;
    for (uint32_t i = 0; i < n_inputs; i++)
      th.emplace_back([&, i]() { mgc::dbfile_read(rd[i], ff, kw, host_decode, in_l != nullptr, &file[i]); });
    for (auto &t : th) t.join();
  }
  hn.assign(n_inputs, 0);
  for (uint32_t i = 0; i < n_inputs; i++) {
    hn[i] = file[i].n;
    if (file[i].rc != MGC_OK) { *msg = file[i].msg; return file[i].rc; }
  }
  int rc = MGC_OK;
  hipError_t e = hipSuccess;
  mgc::DbFileScratch scratch;
  for (uint32_t i = 0; i < n_inputs && rc == MGC_OK && e == hipSuccess; i++) {
    mdb_info inf;
    mdb_reader_info(rd[i], &inf);
    const bool with_l = in_l && inf.label_size;
    e = in_k[i].ensure(8 * (size_t)kw * hn[i]);
    if (e == hipSuccess) e = in_c[i].ensure(4 * hn[i]);
    if (e == hipSuccess && with_l) e = (*in_l)[i].ensure(8 * hn[i]);
    if (e != hipSuccess || !hn[i]) continue;
    uint32_t h_err = 0;
    e = mgc::dbfile_upload(file[i], inf, kw, scratch, in_k[i].p, in_c[i].as<uint32_t>(), with_l ? (*in_l)[i].as<uint64_t>() : nullptr, &h_err, st);
    if (e == hipSuccess && file[i].raw) e = hipStreamSynchronize(st);        // the scratch is reused by the next input
    if (e == hipSuccess) rc = mgc::dbfile_decode_rc(h_err, msg);
  }
  if (e == hipSuccess && rc == MGC_OK) e = hipStreamSynchronize(st);         // the host-decoded arrays go with `file`
  if (e != hipSuccess) { rc = (e == hipErrorOutOfMemory) ? MGC_ENOMEM : MGC_EHIP; *msg = std::string("uploading a slice: ") + hipGetErrorString(e); }
  return rc;
}

// inputs of one k, no labels, no multisets -> readers + the first one's info; false: message in the thread error
// (max_label_size given -- the labelled evaluation: labels are allowed, and the largest label_size among the inputs is returned)
bool open_merge_inputs(const char *const *inputs, uint32_t n_inputs, std::vector<mdb_reader *> &rd, mdb_info *first, const char *who,
                       uint32_t *max_label_size = nullptr) {
  rd.assign(n_inputs, nullptr);
  auto close_all = [&]() { for (mdb_reader *r : rd) if (r) mdb_reader_close(r); };
  memset(first, 0, sizeof(*first));
  for (uint32_t i = 0; i < n_inputs; i++) {
    rd[i] = inputs[i] ? mdb_reader_open(inputs[i]) : nullptr;
    if (!rd[i]) { set_err(nullptr, "%s: %s", who, mdb_last_error()); close_all(); return false; }
    mdb_info inf;
    mdb_reader_info(rd[i], &inf);
    // the merge combines VALUES only: labels would be dropped and a multiset's repeated k-mers folded -- refuse rather than
    // write something that silently differs
    if ((inf.label_size != 0 && !max_label_size) || (inf.flags & 1u)) {
      set_err(nullptr, "%s: '%s' %s: not supported here", who, inputs[i], (inf.label_size && !max_label_size) ? "stores labels" : "is a multiset");
      close_all();
      return false;
    }
    if (max_label_size) *max_label_size = std::max(*max_label_size, inf.label_size);
    if (i == 0) *first = inf;
    else if (inf.k != first->k) {
      set_err(nullptr, "%s: '%s' holds %u-mers, '%s' %u-mers", who, inputs[i], inf.k, inputs[0], first->k);   // merylOp.C: kmer size mismatch
      close_all();
      return false;
    }
  }
  return true;
}

// one (k-mer, value) stream in HBM
struct SliceRef { const void *k = nullptr; const uint32_t *c = nullptr; uint64_t n = 0; const uint64_t *l = nullptr; /*labelled evaluation; null: zeros*/ };

// buffers of the left fold (grow-only, reused from slice to slice)
struct FoldBufs {
  DBuf acc_k[2], acc_c[2], mem_k[2], mem_c[2], ones, ws;
};

// One count / emit pass pair, whatever the kernels: workspace -> count -> read the output length -> size the outputs -> emit ->
// synchronise.  launch(emit, out_keys, out_vals, out_labs) starts one pass; out_l null: no labels are written.
template <typename Launch>
hipError_t pass_pair(DBuf &ws, size_t ws_bytes, uint32_t kw, DBuf &out_k, DBuf &out_c, DBuf *out_l, hipStream_t st, uint64_t *n_new, Launch launch) {
  hipError_t e = ws.ensure(ws_bytes);
  if (e == hipSuccess) e = launch(false, nullptr, nullptr, nullptr);
  if (e == hipSuccess) e = mgc::merge_read_total(ws.p, n_new, st);
  if (e == hipSuccess) e = out_k.ensure(8 * (size_t)kw * *n_new);
  if (e == hipSuccess) e = out_c.ensure(4 * *n_new);
  if (e == hipSuccess && out_l) e = out_l->ensure(8 * *n_new);
  if (e == hipSuccess) e = launch(true, out_k.p, out_c.as<uint32_t>(), out_l ? out_l->as<uint64_t>() : nullptr);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  return e;
}

// a value transform of one stream without a program or labels (flags: fop 12, keep where flags[i] == 1)
hipError_t select_pair(const SliceRef &in, const uint32_t *flags, uint32_t kw, int fop, uint64_t constant, DBuf &ws, DBuf &out_k, DBuf &out_c,
                       hipStream_t st, uint64_t *n_new) {
  const mgc::SelectInput si{in.k, in.c, flags, nullptr, in.n, kw};
  return pass_pair(ws, mgc::select_workspace_bytes(in.n), kw, out_k, out_c, nullptr, st, n_new, [&](bool emit, void *ok, uint32_t *oc, uint64_t *) {
    return mgc::launch_select(emit, si, fop, constant, mgc::PassRule(), ws.p, ok, oc, st);
  });
}

// The inputs of one slice folded from the left with the two-input merge (mgc_merge.hip) -- mgc_db_merge, and the merge nodes
// of mgc_db_eval that do not go through merge_many.
//   union (value = how many inputs hold the k-mer, :559-561) = union-sum over values of one;
//   symmetric-difference over more than two inputs (in exactly ONE input, :609-612) = the union-sum of the values
//   filtered by "union-sum of ones == 1" (written to sel_k / sel_c, which must not hold the value fold's result);
//   everything else folds from the left with its own two-input step.
// *out: the result (an input's or one of the buffers' memory), valid once this returns (the stream is synchronised).
hipError_t fold_slices(const std::vector<SliceRef> &in, int op, uint32_t kw, FoldBufs &fb, DBuf &sel_k, DBuf &sel_c, hipStream_t st,
                       SliceRef *out, const char **what) {
  const uint32_t n_inputs = (uint32_t)in.size();
  const bool by_membership = (op == MGC_MERGE_SYMMETRIC_DIFFERENCE && n_inputs > 2);
  const int fold_op = (op == MGC_MERGE_UNION || by_membership) ? MGC_MERGE_UNION_SUM : op;
  // fold: values (and, for the membership forms, ones) through the same sequence of two-input steps
  auto fold = [&](bool use_ones, DBuf (&ak)[2], DBuf (&ac)[2], SliceRef *res) -> hipError_t {
    uint64_t most = 0;
    for (uint32_t i = 0; i < n_inputs; i++) most = std::max(most, in[i].n);
    if (use_ones) {
      hipError_t e = fb.ones.ensure(4 * most);
      if (e == hipSuccess) e = mgc::launch_fill_u32(fb.ones.as<uint32_t>(), most, 1u, st);
      if (e != hipSuccess) { *what = "ones"; return e; }
    }
    auto cof = [&](uint32_t i) -> const uint32_t * { return use_ones ? fb.ones.as<uint32_t>() : in[i].c; };
    SliceRef cur{in[0].k, cof(0), in[0].n};
    for (uint32_t i = 1; i < n_inputs; i++) {
      const int t = (int)(i & 1u);
      uint64_t n_new = 0;
      const hipError_t e = pass_pair(fb.ws, mgc::merge_workspace_bytes(cur.n, in[i].n), kw, ak[t], ac[t], nullptr, st, &n_new,
                                     [&](bool emit, void *ok, uint32_t *oc, uint64_t *) {
        return emit ? mgc::launch_merge_emit(cur.k, cur.c, cur.n, in[i].k, cof(i), in[i].n, kw, fold_op, fb.ws.p, ok, oc, st)
                    : mgc::launch_merge_count(cur.k, cur.n, in[i].k, in[i].n, kw, fold_op, fb.ws.p, st, cur.c, cof(i));
      });
      if (e != hipSuccess) { *what = "merging a slice"; return e; }
      cur = SliceRef{ak[t].p, ac[t].as<uint32_t>(), n_new};
    }
    *res = cur;
    return hipSuccess;
  };
  SliceRef res;
  hipError_t e = fold(op == MGC_MERGE_UNION, fb.acc_k, fb.acc_c, &res);
  if (e != hipSuccess) return e;
  if (by_membership) {
    SliceRef mem;                                            // same k-mers as the value fold, values = inputs holding each
    e = fold(true, fb.mem_k, fb.mem_c, &mem);
    if (e != hipSuccess) return e;
    uint64_t n_new = 0;
    *what = "selecting the k-mers of exactly one input";
    if (res.k == sel_k.p) { *what = "symmetric-difference buffers"; return hipErrorInvalidValue; }
    e = select_pair(res, mem.c, kw, 12, 0, fb.ws, sel_k, sel_c, st, &n_new);
    if (e != hipSuccess) return e;
    res = SliceRef{sel_k.p, sel_c.as<uint32_t>(), n_new};
  }
  *out = res;
  return hipSuccess;
}
}  // namespace

extern "C" int mgc_db_merge(const char *const *inputs, uint32_t n_inputs, int op, const char *output, int device, int host_threads) {
  if (!inputs || n_inputs == 0 || !output || op < MGC_MERGE_UNION_SUM || op > MGC_MERGE_UNION) {
    set_err(nullptr, "mgc_db_merge: bad arguments");
    return MGC_EINVAL;
  }
  std::vector<mdb_reader *> rd;
  mdb_info first;
  if (!open_merge_inputs(inputs, n_inputs, rd, &first, "mgc_db_merge")) return MGC_EINVAL;
  auto close_all = [&]() { for (mdb_reader *r : rd) if (r) mdb_reader_close(r); };
  const uint32_t k = first.k, w_prefix = first.prefix_size, kw = k > 32 ? 2u : 1u;
  if (device < 0) (void)hipGetDevice(&device);
  mgc_db_stream *d = mgc_db_stream_open(output, k, w_prefix, 0, 0, 0, 1, host_threads, device);
  if (!d) { close_all(); return MGC_EINVAL; }
  int rc = MGC_OK;
  std::string msg;
  auto hip_fail = [&](hipError_t e, const char *what) {
    rc = (e == hipErrorOutOfMemory) ? MGC_ENOMEM : MGC_EHIP;
    msg = std::string("mgc_db_merge: ") + what + ": " + hipGetErrorString(e);
  };
  {
    hipStream_t st = nullptr;
    std::vector<DBuf> in_k(n_inputs), in_c(n_inputs);
    FoldBufs fb;
    std::vector<uint64_t> hn;
    std::vector<SliceRef> in(n_inputs);
    const uint64_t blocks_per_file = 1ull << (w_prefix - MGC_NUM_FILES_BITS);
    const bool host_decode = decode_on_host();
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) hip_fail(e, "hipSetDevice(device)");
    else if ((e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking)) != hipSuccess) hip_fail(e, "hipStreamCreateWithFlags(&st, hipStreamNonBlocking)");
    for (uint32_t ff = 0; ff < MGC_NUM_FILES && rc == MGC_OK; ff++) {
      rc = load_slices(rd, ff, kw, in_k, in_c, hn, st, &msg, host_decode);
      if (rc != MGC_OK) { msg = "mgc_db_merge: " + msg; break; }
      for (uint32_t i = 0; i < n_inputs; i++) in[i] = SliceRef{in_k[i].p, in_c[i].as<uint32_t>(), hn[i]};
      SliceRef res;
      const char *what = "";
      const hipError_t fe = fold_slices(in, op, kw, fb, in_k[0], in_c[0] /*the first input's buffers are free by then*/, st, &res, &what);
      if (fe != hipSuccess) { hip_fail(fe, what); break; }
      rc = mgc_db_stream_write(d, res.k, res.c, res.n, (uint64_t)ff * blocks_per_file, ((uint64_t)ff + 1) * blocks_per_file);
      if (rc == MGC_OK) rc = mgc_db_stream_sync(d);         // the buffers are reused for the next slice
      if (rc != MGC_OK) msg = std::string("mgc_db_merge: ") + mgc_db_stream_error(d);
    }
    if (st) (void)hipStreamDestroy(st);
  }
  close_all();
  const int rc2 = mgc_db_stream_close(d, nullptr);
  if (rc == MGC_OK && rc2 != MGC_OK) { rc = rc2; msg = mgc_db_stream_error(nullptr); }
  if (rc != MGC_OK) set_err(nullptr, "%s", msg.c_str());
  return rc;
}

// The single-input operations over a whole database: less-than ... not-equal-to, increase ... modulo (MGC_VALUE_*).
extern "C" int mgc_db_filter(const char *input, int value_op, uint64_t constant, const char *output, int device, int host_threads) {
  if (!input || !output || value_op < MGC_VALUE_LESS_THAN || value_op > MGC_VALUE_MODULO) { set_err(nullptr, "mgc_db_filter: bad arguments"); return MGC_EINVAL; }
  std::vector<mdb_reader *> rd;
  mdb_info first;
  const char *ins[1] = {input};
  if (!open_merge_inputs(ins, 1, rd, &first, "mgc_db_filter")) return MGC_EINVAL;
  const uint32_t k = first.k, w_prefix = first.prefix_size, kw = k > 32 ? 2u : 1u;
  if (device < 0) (void)hipGetDevice(&device);
  mgc_db_stream *d = mgc_db_stream_open(output, k, w_prefix, 0, 0, 0, 1, host_threads, device);
  if (!d) { mdb_reader_close(rd[0]); return MGC_EINVAL; }
  int rc = MGC_OK;
  std::string msg;
  hipStream_t st = nullptr;
  std::vector<DBuf> in_k(1), in_c(1);
  DBuf out_k, out_c, ws;
  std::vector<uint64_t> hn;
  const uint64_t blocks_per_file = 1ull << (w_prefix - MGC_NUM_FILES_BITS);
  hipError_t e = hipSetDevice(device);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
  const bool host_decode = decode_on_host();
  for (uint32_t ff = 0; ff < MGC_NUM_FILES && rc == MGC_OK && e == hipSuccess; ff++) {
    rc = load_slices(rd, ff, kw, in_k, in_c, hn, st, &msg, host_decode);
    if (rc != MGC_OK) { msg = "mgc_db_filter: " + msg; break; }
    uint64_t n_new = 0;
    e = select_pair(SliceRef{in_k[0].p, in_c[0].as<uint32_t>(), hn[0]}, nullptr, kw, value_op, constant, ws, out_k, out_c, st, &n_new);
    if (e != hipSuccess) break;
    rc = mgc_db_stream_write(d, out_k.p, out_c.as<uint32_t>(), n_new, (uint64_t)ff * blocks_per_file, ((uint64_t)ff + 1) * blocks_per_file);
    if (rc == MGC_OK) rc = mgc_db_stream_sync(d);
    if (rc != MGC_OK) msg = std::string("mgc_db_filter: ") + mgc_db_stream_error(d);
  }
  if (e != hipSuccess && rc == MGC_OK) { rc = (e == hipErrorOutOfMemory) ? MGC_ENOMEM : MGC_EHIP; msg = std::string("mgc_db_filter: ") + hipGetErrorString(e); }
  if (st) (void)hipStreamDestroy(st);
  mdb_reader_close(rd[0]);
  const int rc2 = mgc_db_stream_close(d, nullptr);
  if (rc == MGC_OK && rc2 != MGC_OK) { rc = rc2; msg = mgc_db_stream_error(nullptr); }
  if (rc != MGC_OK) set_err(nullptr, "%s", msg.c_str());
  return rc;
}

// ================================================================================================
//  a tree of merge and value operations per file slice (include/meryl_db.h, mgc_db_eval)
// ================================================================================================
// The reference nests operations on the command line and streams k-mers through the whole tree, writing only where
// `output` is given (src/meryl/merylOp-nextMer.C:418-683, :227).  Here the slices of all leaves are loaded once per file,
// every inner node's result stays in HBM in the node's own buffers, and only outputs and the root's callback leave it.
namespace {
bool merge_many_enabled() { const char *e = getenv("MGC_MERGE_MANY"); return !(e && e[0] == '0'); }

struct EvalNode {
  DBuf k, c, l;                    // an inner node's result (l: labelled evaluation)
  std::unique_ptr<FoldBufs> fold;  // merge nodes that fold
  SliceRef res;
  mgc_db_stream *out = nullptr;
  mgc_value_hist *hist = nullptr;  // flagged nodes (mgc_db_eval_reported): the histogram of the result's values over all slices
  uint32_t leaf = 0;               // leaf: its reader; inner node: its leftmost leaf's
};

std::string plain_path(const char *p) {
  std::string s(p);
  while (s.size() > 1 && s.back() == '/') s.pop_back();
  return s;
}

// everything a node of any of the public structs can carry; what a narrower struct does not name keeps its default
struct Node {
  int32_t     kind = 0, op = 0;
  uint64_t    constant = 0;
  const char *path = nullptr;
  uint32_t    first_child = 0, n_children = 0;
  int32_t     label_op = MGC_LABEL_DEFAULT;          // read only where labels travel
  uint64_t    label_constant = 0;
  uint32_t    first_term = 0, n_terms = 0;           // the node's program in Eval::terms
  int32_t     value_assign = MGC_ASSIGN_NONE;
  uint64_t    value_constant = 0;
  bool        want_hist = false;                      // mgc_db_eval_reported: the value histogram of the node's result
  bool        want_list = false;                      // mgc_db_eval_listed: the text of the node's result
};

// one evaluation, as any of the six entry points states it
struct Eval {
  const char *who;                                   // the entry point, for messages
  std::vector<Node> nodes;
  const uint32_t *children; uint32_t n_children, root;
  const mgc_select_term *terms = nullptr; uint32_t n_terms = 0;
  bool     labels = false;                           // labels travel with the k-mers
  uint32_t label_size = 0;                           // of the outputs; 0: the largest among the leaves
  mgc_eval_slice_cb cb = nullptr;                    // mgc_db_eval's callback form, or
  mgc_eval_slice_labelled_cb lcb = nullptr;          //   the one that also takes labels (zeros when they do not travel)
  void    *ctx = nullptr;
  mgc_value_hist **hists = nullptr;                  // [n_nodes], out: the accumulators of the nodes with want_hist
  mgc_eval_list_cb list_cb = nullptr;                // receives the text of the nodes with want_list
  void    *list_user = nullptr;
};

template <typename T>
std::vector<Node> to_nodes(const T *src, uint32_t n) {
  constexpr bool plain = std::is_same<T, mgc_eval_node>::value, assigned = std::is_same<T, mgc_eval_node_assigned>::value;
  constexpr bool selected = assigned || std::is_same<T, mgc_eval_node_selected>::value;
  std::vector<Node> out(src ? n : 0);
  for (size_t i = 0; i < out.size(); i++) {
    Node &d = out[i];
    const T &s = src[i];
    d.kind = s.kind; d.op = s.op; d.constant = s.constant; d.path = s.path; d.first_child = s.first_child; d.n_children = s.n_children;
    if constexpr (!plain) { d.label_op = s.label_op; d.label_constant = s.label_constant; }
    if constexpr (selected) { d.first_term = s.first_term; d.n_terms = s.n_terms; }
    if constexpr (assigned) { d.value_assign = s.value_assign; d.value_constant = s.value_constant; }
  }
  return out;
}

// the six entry points: one walk, one validation, one slice loop
int eval_impl(const Eval &E, int device, int host_threads) {
  const char *who = E.who;
  const std::vector<Node> &nodes = E.nodes;
  const uint32_t n_nodes = (uint32_t)nodes.size(), n_children = E.n_children, root = E.root, *children = E.children;
  const bool labels = E.labels;
  auto bad = [&](const std::string &m) { set_err(nullptr, "%s: %s", who, m.c_str()); return MGC_EINVAL; };
  if (n_nodes == 0 || (E.n_terms && !E.terms)) return bad("bad arguments");
  if (E.label_size > 64) return bad("a label has at most 64 bits");
  if (root >= n_nodes || (n_children && !children)) return bad("bad arguments");
  for (uint32_t v = 0; v < n_nodes; v++)
    if (nodes[v].want_hist && !E.hists) return bad("node " + std::to_string(v) + ": a histogram is wanted but there is nowhere to return it");
  for (uint32_t v = 0; v < n_nodes; v++)
    if (nodes[v].want_list && !E.list_cb) return bad("node " + std::to_string(v) + ": a list is wanted but there is no callback to receive it");
  // ---- the tree: every node reached at most once, from the root (post-order = evaluation order)
  std::vector<uint32_t> order, leaves;
  {
    std::vector<uint8_t> seen(n_nodes, 0);
    struct Frame { uint32_t node, next; };
    std::vector<Frame> stack;
    seen[root] = 1;
    stack.push_back({root, 0});
    while (!stack.empty()) {
      Frame &f = stack.back();
      const Node &nd = nodes[f.node];
      if (f.next == 0) {
        const std::string id = "node " + std::to_string(f.node);
        if (nd.kind < MGC_NODE_DATABASE || nd.kind > MGC_NODE_VALUE) return bad(id + ": unknown kind");
        if ((uint64_t)nd.first_child + nd.n_children > n_children) return bad(id + ": its children are out of range");
        if (nd.kind == MGC_NODE_DATABASE && nd.n_children != 0) return bad(id + ": a database has no inputs");
        if (nd.kind == MGC_NODE_DATABASE && !nd.path) return bad(id + ": a database needs a path");
        if (nd.kind == MGC_NODE_VALUE && nd.n_children != 1) return bad(id + ": a value operation has exactly one input");
        if (nd.kind == MGC_NODE_VALUE && (nd.op < MGC_VALUE_LESS_THAN || nd.op > MGC_VALUE_MODULO)) return bad(id + ": unknown value operation");
        if (nd.kind == MGC_NODE_MERGE && nd.n_children == 0) return bad(id + ": a merge operation needs an input");
        if (nd.kind == MGC_NODE_MERGE && (nd.op < MGC_MERGE_UNION_SUM || nd.op > MGC_MERGE_UNION)) return bad(id + ": unknown merge operation");
        if (labels && nd.kind != MGC_NODE_DATABASE) {
          const int lop = nd.label_op;
          if (mgc::label_kernel_op(nd.kind == MGC_NODE_MERGE, nd.op, lop) < 0) return bad(id + ": unknown label operation " + std::to_string(lop));
          if (lop == MGC_LABEL_INVERT && nd.n_children > 1) return bad(id + ": label=invert takes one input, the node has " + std::to_string(nd.n_children));
          // the left fold combines two streams at a time: DIFFERENCE, MIN or LIGHTEST over all inputs at once cannot be folded
          if (nd.kind == MGC_NODE_MERGE && nd.n_children > MGC_MERGE_MANY_MAX)
            return bad(id + ": a merge of " + std::to_string(nd.n_children) + " inputs; with labels at most " + std::to_string(MGC_MERGE_MANY_MAX));
        }
        if (nd.n_terms) {
          if (nd.kind == MGC_NODE_DATABASE) return bad(id + ": a database takes no selector");
          if ((uint64_t)nd.first_term + nd.n_terms > E.n_terms) return bad(id + ": its selector terms are out of range");
          if (nd.n_children > MGC_MERGE_MANY_MAX)
            return bad(id + ": a merge of " + std::to_string(nd.n_children) + " inputs; with a selector at most " + std::to_string(MGC_MERGE_MANY_MAX));
          const std::string m = mgc::select_check(E.terms + nd.first_term, nd.n_terms, nd.n_children);
          if (!m.empty()) return bad(id + ": selector: " + m);
        }
        if (nd.value_assign != MGC_ASSIGN_NONE) {
          const int a = nd.value_assign;
          if (mgc::value_kernel_op(a) < 0) return bad(id + ": unknown value assignment " + std::to_string(a));
          if (nd.kind == MGC_NODE_DATABASE) return bad(id + ": a database takes no value assignment");
          if (nd.kind == MGC_NODE_VALUE && nd.op > MGC_VALUE_NOT_EQUAL_TO)
            return bad(id + ": an arithmetic value operation takes no value assignment (the operation is one)");
          if (nd.n_children > MGC_MERGE_MANY_MAX)
            return bad(id + ": a merge of " + std::to_string(nd.n_children) + " inputs; with a value assignment at most " + std::to_string(MGC_MERGE_MANY_MAX));
        }
      }
      if (f.next < nd.n_children) {
        const uint32_t ch = children[nd.first_child + f.next++];
        if (ch >= n_nodes) return bad("node " + std::to_string(f.node) + ": input " + std::to_string(ch) + " is out of range");
        if (seen[ch]) return bad("node " + std::to_string(ch) + " is reached twice (an input of two operations, or a cycle)");
        seen[ch] = 1;
        stack.push_back({ch, 0});                            // (f is dead from here)
        continue;
      }
      if (nd.kind == MGC_NODE_DATABASE) leaves.push_back(f.node);
      order.push_back(f.node);
      stack.pop_back();
    }
    for (uint32_t v = 0; v < n_nodes; v++)
      if (nodes[v].want_hist && !seen[v]) return bad("node " + std::to_string(v) + ": a histogram is wanted of a node the root does not reach");
    for (uint32_t v = 0; v < n_nodes; v++)
      if (nodes[v].want_list && !seen[v]) return bad("node " + std::to_string(v) + ": a list is wanted of a node the root does not reach");
  }
  // ---- outputs: named once, and not an input
  {
    std::map<std::string, uint32_t> names;
    for (uint32_t v : leaves) names.emplace(plain_path(nodes[v].path), v);
    for (uint32_t v : order) {
      if (nodes[v].kind == MGC_NODE_DATABASE || !nodes[v].path) continue;
      const auto ins = names.emplace(plain_path(nodes[v].path), v);
      if (!ins.second)
        return bad(std::string("output '") + nodes[v].path + "' of node " + std::to_string(v) +
                   (nodes[ins.first->second].kind == MGC_NODE_DATABASE ? " is also an input" : " is also the output of node " + std::to_string(ins.first->second)));
    }
  }
  // ---- leaves: open, one k, no labels, no multisets (leaves[] is in left-to-right order)
  std::vector<mdb_reader *> rd;
  mdb_info first;
  uint32_t leaf_label_size = 0;
  {
    std::vector<const char *> paths;
    for (uint32_t v : leaves) paths.push_back(nodes[v].path);
    if (!open_merge_inputs(paths.data(), (uint32_t)paths.size(), rd, &first, who, labels ? &leaf_label_size : nullptr)) return MGC_EINVAL;
  }
  const uint32_t label_size = labels ? (E.label_size ? E.label_size : leaf_label_size) : 0;
  if (label_size > 64) { for (mdb_reader *r : rd) if (r) mdb_reader_close(r); return bad("a label has at most 64 bits"); }
  auto close_readers = [&]() { for (mdb_reader *r : rd) if (r) mdb_reader_close(r); };
  const uint32_t k = first.k, kw = k > 32 ? 2u : 1u, n_leaves = (uint32_t)leaves.size();
  std::vector<EvalNode> ev(n_nodes);
  for (uint32_t i = 0; i < n_leaves; i++) ev[leaves[i]].leaf = i;
  for (uint32_t v : order)
    if (nodes[v].kind != MGC_NODE_DATABASE) ev[v].leaf = ev[children[nodes[v].first_child]].leaf;
  auto w_prefix_of = [&](uint32_t v) { mdb_info inf; mdb_reader_info(rd[ev[v].leaf], &inf); return inf.prefix_size; };

  // ---- device work from here
  const bool use_many = merge_many_enabled();
  const bool host_decode = decode_on_host();
  if (device < 0) (void)hipGetDevice(&device);
  int rc = MGC_OK;
  std::string msg;
  const std::string who_colon = std::string(who) + ": ";
  auto hip_fail = [&](hipError_t e, const char *what) {
    if (e == hipSuccess) return false;
    rc = (e == hipErrorOutOfMemory) ? MGC_ENOMEM : MGC_EHIP;
    msg = who_colon + what + ": " + hipGetErrorString(e);
    return true;
  };
  for (uint32_t v : order) {
    if (nodes[v].kind == MGC_NODE_DATABASE || !nodes[v].path) continue;
    ev[v].out = mgc_db_stream_open(nodes[v].path, k, w_prefix_of(v), label_size, 0, 0, 1, host_threads, device);
    if (!ev[v].out) { rc = MGC_EINVAL; msg = mgc_db_stream_error(nullptr); break; }
  }
  for (uint32_t v : order)
    if (nodes[v].want_hist && rc == MGC_OK) ev[v].hist = mgc_value_hist_open(device);
  // the lists: one pair of staging buffers for all flagged nodes; pieces of MGC_LIST_CHUNK bytes (tests), at least one line
  struct ListTo { mgc_eval_list_cb cb; void *user; uint32_t node, file; };
  std::unique_ptr<mgc::ListStage, void (*)(mgc::ListStage *)> list_stage(nullptr, mgc::list_stage_close);
  uint64_t list_chunk = 16ull << 20;
  if (const char *e = getenv("MGC_LIST_CHUNK")) { if (*e) list_chunk = strtoull(e, nullptr, 10); }
  list_chunk = std::max<uint64_t>(list_chunk, mgc_list_max_line(k, label_size));
  hipStream_t st = nullptr;
  std::vector<DBuf> in_k(n_leaves), in_c(n_leaves), in_l(labels ? n_leaves : 0);
  DBuf ws;
  std::vector<uint64_t> hn, h_keys, h_lo, h_hi, h_labs;
  std::vector<uint32_t> h_vals;
  if (rc == MGC_OK && !hip_fail(hipSetDevice(device), "hipSetDevice")) (void)hip_fail(hipStreamCreateWithFlags(&st, hipStreamNonBlocking), "hipStreamCreate");

  // one inner node of one slice: its inputs' results -> its own
  auto eval_node = [&](uint32_t v) -> bool {
    const Node &nd = nodes[v];
    EvalNode &me = ev[v];
    std::vector<SliceRef> in(nd.n_children);
    for (uint32_t i = 0; i < nd.n_children; i++) in[i] = ev[children[nd.first_child + i]].res;
    const bool is_merge = nd.kind == MGC_NODE_MERGE;
    const mgc::Route route = mgc::eval_route(!is_merge, nd.n_children, labels, nd.n_terms != 0, nd.value_assign != MGC_ASSIGN_NONE, use_many);
    if (route == mgc::ROUTE_FOLD) {
      if (!me.fold) me.fold.reset(new FoldBufs);
      const char *what = "";
      return !hip_fail(fold_slices(in, nd.op, kw, *me.fold, me.k, me.c, st, &me.res, &what), what);
    }
    // the rule both passes take: the label operation wherever labels are looked at or written, the program and the assignment
    // where the node has one
    mgc::PassRule rule;
    rule.lop = mgc::label_kernel_op_assigned(is_merge, nd.op, labels ? nd.label_op : MGC_LABEL_DEFAULT, nd.value_assign);
    rule.lc = labels ? nd.label_constant : 0;
    int op = nd.op;
    if (route == mgc::ROUTE_SELECT_SELECTED || route == mgc::ROUTE_MANY_SELECTED || route == mgc::ROUTE_MANY_ASSIGNED) {
      rule.select = true; rule.terms = nd.n_terms ? E.terms + nd.first_term : nullptr; rule.n_terms = nd.n_terms; rule.k = k;
    }
    if (route == mgc::ROUTE_MANY_ASSIGNED) {
      rule.vop = mgc::value_kernel_op(nd.value_assign); rule.vc = nd.value_constant;
      // a value filter node: its one input under the presence rule of a union, the filter on the assigned value
      if (!is_merge) { op = MGC_MERGE_UNION; rule.fop = nd.op; rule.fc = nd.constant; }
    }
    uint64_t n_new = 0;
    hipError_t e;
    if (mgc::route_merges_many(route)) {
      const void *kp[MGC_MERGE_MANY_MAX];
      const uint32_t *cp[MGC_MERGE_MANY_MAX];
      const uint64_t *lp[MGC_MERGE_MANY_MAX];
      uint64_t nn[MGC_MERGE_MANY_MAX];
      for (uint32_t i = 0; i < nd.n_children; i++) { kp[i] = in[i].k; cp[i] = in[i].c; lp[i] = in[i].l; nn[i] = in[i].n; }
      const mgc::MergeManyInputs mi{kp, cp, lp, nn, nd.n_children, kw};
      e = pass_pair(ws, mgc::merge_many_workspace_bytes(nn, nd.n_children, kw), kw, me.k, me.c, labels ? &me.l : nullptr, st, &n_new,
                    [&](bool emit, void *ok, uint32_t *oc, uint64_t *ol) {
        rule.out_labs = ol;
        return mgc::launch_merge_many(emit, mi, op, rule, ws.p, ok, oc, st);
      });
    } else {
      const mgc::SelectInput si{in[0].k, in[0].c, nullptr, in[0].l, in[0].n, kw};
      e = pass_pair(ws, mgc::select_workspace_bytes(in[0].n), kw, me.k, me.c, labels ? &me.l : nullptr, st, &n_new,
                    [&](bool emit, void *ok, uint32_t *oc, uint64_t *ol) {
        rule.out_labs = ol;
        return mgc::launch_select(emit, si, op, nd.constant, rule, ws.p, ok, oc, st);
      });
    }
    if (hip_fail(e, mgc::route_context(route))) return false;
    me.res = SliceRef{me.k.p, me.c.as<uint32_t>(), n_new, labels ? me.l.as<uint64_t>() : nullptr};
    return true;
  };

  for (uint32_t ff = 0; ff < MGC_NUM_FILES && rc == MGC_OK; ff++) {
    rc = load_slices(rd, ff, kw, in_k, in_c, hn, st, &msg, host_decode, labels ? &in_l : nullptr);
    if (rc != MGC_OK) { msg = who_colon + msg; break; }
    for (uint32_t v : order) {
      EvalNode &me = ev[v];
      if (nodes[v].kind == MGC_NODE_DATABASE)
        me.res = SliceRef{in_k[me.leaf].p, in_c[me.leaf].as<uint32_t>(), hn[me.leaf], (labels && in_l[me.leaf].p) ? in_l[me.leaf].as<uint64_t>() : nullptr};
      else if (!eval_node(v)) break;
      if (me.out) {
        const uint64_t blocks_per_file = 1ull << (w_prefix_of(v) - MGC_NUM_FILES_BITS);
        rc = mgc_db_stream_write_labelled(me.out, me.res.k, me.res.c, label_size ? me.res.l : nullptr, me.res.n, (uint64_t)ff * blocks_per_file,
                                          ((uint64_t)ff + 1) * blocks_per_file);
        if (rc != MGC_OK) { msg = who_colon + mgc_db_stream_error(me.out); break; }
      }
      if (me.hist) {                                         // the result's values, counted where they lie
        rc = mgc_value_hist_add(me.hist, me.res.c, me.res.n, st);
        if (rc != MGC_OK) { msg = who_colon + mgc_db_stream_error(nullptr); break; }
      }
      if (nodes[v].want_list) {                              // the result's text, formatted where it lies
        if (!list_stage) list_stage.reset(mgc::list_stage_open());
        ListTo to{E.list_cb, E.list_user, v, ff};
        rc = mgc::list_kmers(list_stage.get(), me.res.k, me.res.c, label_size ? me.res.l : nullptr, me.res.n, k, label_size, list_chunk,
                             [](const void *text, uint64_t n, void *u) {
                               const ListTo *t = static_cast<const ListTo *>(u);
                               return t->cb(t->user, t->node, t->file, text, n);
                             }, &to, st, who);
        if (rc != MGC_OK) { msg = mgc_db_stream_error(nullptr); break; }
      }
    }
    if (rc != MGC_OK) break;
    if (E.cb || E.lcb) {
      const SliceRef &r = ev[root].res;
      h_keys.resize((size_t)kw * r.n);
      h_vals.resize(r.n);
      if (E.lcb) h_labs.assign(r.n, 0);
      hipError_t e = hipSuccess;
      if (r.n) {
        e = hipMemcpyAsync(h_keys.data(), r.k, 8 * (size_t)kw * r.n, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(h_vals.data(), r.c, 4 * r.n, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && E.lcb && r.l) e = hipMemcpyAsync(h_labs.data(), r.l, 8 * r.n, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
      }
      if (hip_fail(e, "copying the root's slice")) break;
      const uint64_t *lo = h_keys.data(), *hi = nullptr;
      if (kw == 2) {
        h_lo.resize(r.n); h_hi.resize(r.n);
        for (uint64_t j = 0; j < r.n; j++) { h_lo[j] = h_keys[2 * j]; h_hi[j] = h_keys[2 * j + 1]; }
        lo = h_lo.data(); hi = h_hi.data();
      }
      if (E.lcb) E.lcb(E.ctx, ff, lo, hi, h_vals.data(), h_labs.data(), r.n);
      else E.cb(E.ctx, ff, lo, hi, h_vals.data(), r.n);
    }
    for (uint32_t v : order) {                               // the buffers are reused for the next slice
      if (!ev[v].out) continue;
      const int rs = mgc_db_stream_sync(ev[v].out);
      if (rs != MGC_OK && rc == MGC_OK) { rc = rs; msg = who_colon + mgc_db_stream_error(ev[v].out); }
    }
  }
  // an output whose node failed mid-slice may still be encoding from buffers about to go
  if (rc != MGC_OK) for (uint32_t v : order) if (ev[v].out) (void)mgc_db_stream_sync(ev[v].out);
  list_stage.reset();
  if (st) (void)hipStreamDestroy(st);
  close_readers();
  for (uint32_t v : order) {
    if (!ev[v].out) continue;
    const int rc2 = mgc_db_stream_close(ev[v].out, nullptr);
    if (rc == MGC_OK && rc2 != MGC_OK) { rc = rc2; msg = mgc_db_stream_error(nullptr); }
  }
  for (uint32_t v : order) {                                 // the accumulators go to the caller, or nowhere
    if (!ev[v].hist) continue;
    if (rc == MGC_OK) E.hists[v] = ev[v].hist;
    else mgc_value_hist_close(ev[v].hist);
  }
  if (rc != MGC_OK) set_err(nullptr, "%s", msg.c_str());
  return rc;
}

// labels travel when the caller says so, when the outputs are to store some, or when a program anywhere looks at them
bool labels_asked(const Eval &E, int with_labels) {
  bool labels = with_labels != 0 || E.label_size != 0;
  if (E.terms)
    for (const Node &nd : E.nodes)
      if ((uint64_t)nd.first_term + nd.n_terms <= E.n_terms)
        for (uint32_t j = 0; j < nd.n_terms; j++) labels = labels || E.terms[nd.first_term + j].quantity == MGC_SEL_LABEL;
  return labels;
}

// mgc_db_eval_selected and mgc_db_eval_assigned: the same arguments, the wider node struct
template <typename T>
int eval_with_programs(const char *who, const T *nodes, uint32_t n_nodes, const uint32_t *children, uint32_t n_children, uint32_t root,
                       const mgc_select_term *terms, uint32_t n_terms, int with_labels, uint32_t label_size, mgc_eval_slice_labelled_cb cb, void *ctx,
                       int device, int host_threads) {
  Eval E{who, to_nodes(nodes, n_nodes), children, n_children, root};
  E.terms = terms; E.n_terms = n_terms; E.label_size = label_size; E.lcb = cb; E.ctx = ctx;
  E.labels = labels_asked(E, with_labels);
  return eval_impl(E, device, host_threads);
}
}  // namespace

extern "C" int mgc_db_eval(const mgc_eval_node *nodes, uint32_t n_nodes, const uint32_t *children, uint32_t n_children, uint32_t root,
                           mgc_eval_slice_cb cb, void *ctx, int device, int host_threads) {
  Eval E{"mgc_db_eval", to_nodes(nodes, n_nodes), children, n_children, root};
  E.cb = cb; E.ctx = ctx;
  return eval_impl(E, device, host_threads);
}

// the same tree with labels (include/meryl_db.h): the label operation of every node is merylOpCompute::findOutputLabel
// (src/meryl2/merylOpCompute.C:286-395) over the inputs that hold the k-mer
extern "C" int mgc_db_eval_labelled(const mgc_eval_node_labelled *nodes, uint32_t n_nodes, const uint32_t *children, uint32_t n_children,
                                    uint32_t root, uint32_t label_size, mgc_eval_slice_labelled_cb cb, void *ctx, int device, int host_threads) {
  Eval E{"mgc_db_eval_labelled", to_nodes(nodes, n_nodes), children, n_children, root};
  E.labels = true; E.label_size = label_size; E.lcb = cb; E.ctx = ctx;
  return eval_impl(E, device, host_threads);
}

// the same tree with selector programs (include/meryl_db.h): nodes without one take the route they take in mgc_db_eval (labels do
// not travel) or mgc_db_eval_labelled (they do: with_labels, or a LABEL term anywhere in the tree)
extern "C" int mgc_db_eval_selected(const mgc_eval_node_selected *nodes, uint32_t n_nodes, const uint32_t *children, uint32_t n_children,
                                    uint32_t root, const mgc_select_term *terms, uint32_t n_terms, int with_labels, uint32_t label_size,
                                    mgc_eval_slice_labelled_cb cb, void *ctx, int device, int host_threads) {
  return eval_with_programs("mgc_db_eval_selected", nodes, n_nodes, children, n_children, root, terms, n_terms, with_labels, label_size, cb, ctx,
                            device, host_threads);
}

// the same tree with value assignments (include/meryl_db.h): a node without one takes the route it takes in mgc_db_eval_selected
extern "C" int mgc_db_eval_assigned(const mgc_eval_node_assigned *nodes, uint32_t n_nodes, const uint32_t *children, uint32_t n_children,
                                    uint32_t root, const mgc_select_term *terms, uint32_t n_terms, int with_labels, uint32_t label_size,
                                    mgc_eval_slice_labelled_cb cb, void *ctx, int device, int host_threads) {
  return eval_with_programs("mgc_db_eval_assigned", nodes, n_nodes, children, n_children, root, terms, n_terms, with_labels, label_size, cb, ctx,
                            device, host_threads);
}

// the same tree with reports (include/meryl_db.h): the flagged nodes' values of every slice go through their value-histogram
// accumulators (mgc_value_hist.hip); nothing else differs from mgc_db_eval_assigned
extern "C" int mgc_db_eval_reported(const mgc_eval_node_assigned *nodes, uint32_t n_nodes, const uint32_t *children, uint32_t n_children,
                                    uint32_t root, const mgc_select_term *terms, uint32_t n_terms, int with_labels, uint32_t label_size,
                                    mgc_eval_slice_labelled_cb cb, void *ctx, int device, int host_threads, const uint8_t *want_hist,
                                    mgc_value_hist **hists) {
  Eval E{"mgc_db_eval_reported", to_nodes(nodes, n_nodes), children, n_children, root};
  E.terms = terms; E.n_terms = n_terms; E.label_size = label_size; E.lcb = cb; E.ctx = ctx;
  E.labels = labels_asked(E, with_labels);
  E.hists = hists;
  if (hists) for (size_t v = 0; v < E.nodes.size(); v++) hists[v] = nullptr;       // on failure no handle is returned
  if (want_hist) for (size_t v = 0; v < E.nodes.size(); v++) E.nodes[v].want_hist = want_hist[v] != 0;
  return eval_impl(E, device, host_threads);
}

// the same tree with lists (include/meryl_db.h, include/meryl_list.h): the flagged nodes' results of every slice go through the text
// lister (mgc_list.hip) to the callback; nothing else differs from mgc_db_eval_reported
extern "C" int mgc_db_eval_listed(const mgc_eval_node_assigned *nodes, uint32_t n_nodes, const uint32_t *children, uint32_t n_children,
                                  uint32_t root, const mgc_select_term *terms, uint32_t n_terms, int with_labels, uint32_t label_size,
                                  mgc_eval_slice_labelled_cb cb, void *ctx, int device, int host_threads, const uint8_t *want_hist,
                                  mgc_value_hist **hists, const uint8_t *want_list, mgc_eval_list_cb list_cb, void *list_user) {
  Eval E{"mgc_db_eval_listed", to_nodes(nodes, n_nodes), children, n_children, root};
  E.terms = terms; E.n_terms = n_terms; E.label_size = label_size; E.lcb = cb; E.ctx = ctx;
  E.labels = labels_asked(E, with_labels);
  E.hists = hists; E.list_cb = list_cb; E.list_user = list_user;
  if (hists) for (size_t v = 0; v < E.nodes.size(); v++) hists[v] = nullptr;       // on failure no handle is returned
  if (want_hist) for (size_t v = 0; v < E.nodes.size(); v++) E.nodes[v].want_hist = want_hist[v] != 0;
  if (want_list) for (size_t v = 0; v < E.nodes.size(); v++) E.nodes[v].want_list = want_list[v] != 0;
  return eval_impl(E, device, host_threads);
}
