// mgc_positions.cpp -- C-ABI layer of include/meryl_positions.h: the position index of a reference over a lookup table and the
// painter that accumulates query batches against it.
//
// Reference side: posLookGlobal::initialize / lookupBatch / writeBatch of src/meryl-lookup/position-lookup.C:133-336.  The
// index is built once (slots of the reference's windows -> (slot, offset) pairs in stream order -> stable sort by slot ->
// list boundaries); a batch is one pass over its windows, the same pair compaction and sort with the query's number as the
// payload, and one pass over the sorted pairs that adds every slot's hits and distinct queries (mgc_positions.hip).
#include "../../include/meryl_gpu_count.h"
#include "../../include/meryl_positions.h"
#include "mgc_devbuf.hpp"
#include "mgc_import_dev.hpp"
#include "mgc_positions_dev.hpp"

#include <string>
#include <utility>

namespace {
using mgc::DBuf;

int pos_fail(const char *who, const char *what) {
  mgc::lk_set_error(std::string(who) + ": " + what);
  return MGC_EINVAL;
}
int pos_rc(hipError_t e, const char *what) {
  if (e == hipSuccess) return MGC_OK;
  mgc::lk_set_error(std::string(what) + ": " + hipGetErrorString(e));
  return e == hipErrorOutOfMemory ? MGC_ENOMEM : MGC_EHIP;
}
uint32_t slot_bits(uint64_t n_table) {                     // ceil(log2 n_table), at least 1
  uint32_t b = 1;
  while (b < 32 && (1ull << b) < n_table) b++;
  return b;
}

// what the index build and a painted batch share: the slots' (slot, payload) pairs of a stream, compacted in order and sorted
// by slot.  After sorted(): keys()/vals() hold the n pairs, other_keys() is free (n + 1 entries).
struct PairSort {
  DBuf k[2], v[2], sort_ws, pair_ws;
  uint64_t n = 0;
  int in_alt = 0;
  uint64_t *keys() const { return k[in_alt].as<uint64_t>(); }
  uint32_t *vals() const { return v[in_alt].as<uint32_t>(); }
  uint64_t *other_keys() const { return k[in_alt ^ 1].as<uint64_t>(); }

  hipError_t run(const uint32_t *d_slot, uint64_t n_bases, const uint64_t *d_seq_start, uint64_t n_seq, uint64_t n_table, hipStream_t st) {
    n = 0; in_alt = 0;
    hipError_t e = pair_ws.ensure(mgc::pos_pairs_workspace_bytes(n_bases));
    if (e == hipSuccess) e = mgc::launch_pos_pairs_count(d_slot, n_bases, pair_ws.p, st);
    if (e == hipSuccess) e = hipMemcpyAsync(&n, pair_ws.p, sizeof(uint64_t), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess || n == 0) return e;
    for (int i = 0; i < 2 && e == hipSuccess; i++) {
      e = k[i].ensure(sizeof(uint64_t) * (n + 1));
      if (e == hipSuccess) e = v[i].ensure(sizeof(uint32_t) * n);
    }
    if (e == hipSuccess) e = sort_ws.ensure(mgc::sort_pairs_workspace_bytes(n));
    if (e == hipSuccess) e = mgc::launch_pos_pairs_emit(d_slot, n_bases, d_seq_start, n_seq, pair_ws.p, k[0].as<uint64_t>(), v[0].as<uint32_t>(), st);
    if (e == hipSuccess)
      e = mgc::launch_sort_pairs(k[0].p, v[0].as<uint32_t>(), k[1].p, v[1].as<uint32_t>(), n, 1, 0, slot_bits(n_table), sort_ws.p, &in_alt, st);
    return e;
  }
};
}  // namespace

struct mgc_posidx {
  mgc::PosTable t;
  uint64_t n_bases = 0, n_placed = 0, n_used = 0, longest = 0;
  DBuf d_ref_slot, d_pos_start, d_pos_data;                  // uint32[n_bases], uint64[n + 1], uint32[n_placed]
};

struct mgc_paint {
  const mgc_posidx *idx = nullptr;
  uint32_t what = 0;
  DBuf d_hits, d_queries;                                   // per slot: H and Q (uint32 each; unallocated when not opened)
  DBuf slot, scratch;
  PairSort pairs;
};

extern "C" void mgc_posidx_free(mgc_posidx *idx) {
  if (!idx) return;
  (void)hipSetDevice(idx->t.device);
  delete idx;
}

extern "C" mgc_posidx *mgc_posidx_build(const mgc_lookup *table, const uint8_t *d_ref_bases, uint64_t n_bases, void *stream) {
  const char *who = "mgc_posidx_build";
  if (!table) { pos_fail(who, "no lookup table"); return nullptr; }
  if (n_bases && !d_ref_bases) { pos_fail(who, "no reference bases"); return nullptr; }
  if (n_bases >> 32) { pos_fail(who, "the reference holds 2^32 bases or more: positions are 32-bit"); return nullptr; }
  const mgc::PosTable t = mgc::pos_table_of(table);
  if (t.n > 0xFFFFFFFEull) { pos_fail(who, "the table holds more than 2^32 - 2 k-mers: slots are 32-bit"); return nullptr; }
  hipStream_t st = (hipStream_t)stream;
  mgc_posidx *idx = new mgc_posidx();
  idx->t = t; idx->n_bases = n_bases;
  PairSort ps;
  DBuf scratch, stats;
  uint64_t h_stats[2] = {0, 0};
  hipError_t e = hipSetDevice(t.device);
  uint32_t *d_ref_slot = nullptr;
  uint64_t *d_pos_start = nullptr;
  if (e == hipSuccess) e = idx->d_ref_slot.ensure(sizeof(uint32_t) * n_bases);
  if (e == hipSuccess) e = idx->d_pos_start.ensure(sizeof(uint64_t) * (t.n + 1));
  if (e == hipSuccess) { d_ref_slot = idx->d_ref_slot.as<uint32_t>(); d_pos_start = idx->d_pos_start.as<uint64_t>(); }
  if (e == hipSuccess) e = mgc::launch_pos_slots(t, d_ref_bases, n_bases, d_ref_slot, nullptr, 0, nullptr, nullptr, nullptr, st);
  if (e == hipSuccess) e = ps.run(d_ref_slot, n_bases, nullptr, 0, t.n, st);
  if (e == hipSuccess) e = scratch.ensure(sizeof(uint64_t) * mgc::pos_starts_scratch_elems(t.n));
  if (e == hipSuccess) e = stats.ensure(sizeof(h_stats));
  if (e == hipSuccess) e = hipMemsetAsync(stats.p, 0, sizeof(h_stats), st);
  if (e == hipSuccess) e = mgc::launch_pos_starts(ps.keys(), ps.n, t.n, d_pos_start, scratch.as<uint64_t>(), st);
  if (e == hipSuccess) e = mgc::launch_pos_list_stats(d_pos_start, t.n, stats.as<uint64_t>(), st);
  if (e == hipSuccess) e = hipMemcpyAsync(h_stats, stats.p, sizeof(h_stats), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) { pos_rc(e, who); mgc_posidx_free(idx); return nullptr; }
  idx->n_placed = ps.n; idx->n_used = h_stats[0]; idx->longest = h_stats[1];
  if (ps.n) idx->d_pos_data = std::move(ps.v[ps.in_alt]);   // the sorted payloads ARE the lists
  return idx;
}

extern "C" int mgc_posidx_get_info(const mgc_posidx *idx, mgc_posidx_info *info) {
  if (!idx || !info) return pos_fail("mgc_posidx_get_info", "no index or no info");
  info->k = idx->t.k; info->reserved = 0;
  info->n_kmers = idx->t.n; info->n_ref_bases = idx->n_bases; info->n_placed = idx->n_placed;
  info->n_slots_used = idx->n_used; info->longest_list = idx->longest;
  info->device_bytes = sizeof(uint32_t) * idx->n_bases + sizeof(uint64_t) * (idx->t.n + 1) + sizeof(uint32_t) * idx->n_placed;
  return MGC_OK;
}

extern "C" int mgc_posidx_arrays(const mgc_posidx *idx, const uint32_t **d_ref_slot, const uint64_t **d_pos_start, const uint32_t **d_pos_data) {
  if (!idx) return pos_fail("mgc_posidx_arrays", "no index");
  if (d_ref_slot) *d_ref_slot = idx->d_ref_slot.as<uint32_t>();
  if (d_pos_start) *d_pos_start = idx->d_pos_start.as<uint64_t>();
  if (d_pos_data) *d_pos_data = idx->d_pos_data.as<uint32_t>();
  return MGC_OK;
}

extern "C" int mgc_posidx_find(const mgc_posidx *idx, const void *d_kmers, uint64_t n, uint64_t *d_begin, uint32_t *d_count, void *stream) {
  if (!idx) return pos_fail("mgc_posidx_find", "no index");
  if (n && (!d_kmers || !d_begin || !d_count)) return pos_fail("mgc_posidx_find", "no k-mers or no outputs");
  return pos_rc(mgc::launch_pos_find(idx->t, d_kmers, n, idx->d_pos_start.as<uint64_t>(), d_begin, d_count, (hipStream_t)stream), "mgc_posidx_find");
}

extern "C" void mgc_paint_close(mgc_paint *p) {
  if (!p) return;
  (void)hipSetDevice(p->idx->t.device);
  delete p;
}

extern "C" mgc_paint *mgc_paint_open(const mgc_posidx *idx, uint32_t what) {
  const char *who = "mgc_paint_open";
  if (!idx) { pos_fail(who, "no index"); return nullptr; }
  if (what == 0 || (what & ~(MGC_PAINT_HITS | MGC_PAINT_MERS | MGC_PAINT_QUERIES))) {
    pos_fail(who, "'what' must be a mask of MGC_PAINT_HITS, MGC_PAINT_MERS and MGC_PAINT_QUERIES");
    return nullptr;
  }
  mgc_paint *p = new mgc_paint();
  p->idx = idx; p->what = what;
  const size_t bytes = sizeof(uint32_t) * (idx->t.n ? idx->t.n : 1);
  hipError_t e = hipSetDevice(idx->t.device);
  for (DBuf *a : {&p->d_hits, &p->d_queries}) {
    if (!(what & (a == &p->d_hits ? MGC_PAINT_MERS : MGC_PAINT_QUERIES))) continue;
    if (e == hipSuccess) e = a->ensure(bytes);
    if (e == hipSuccess) e = hipMemset(a->p, 0, bytes);
  }
  if (e != hipSuccess) { pos_rc(e, who); mgc_paint_close(p); return nullptr; }
  return p;
}

extern "C" int mgc_paint_add(mgc_paint *p, const uint8_t *d_bases, uint64_t n_bases, const uint64_t *d_seq_start, uint64_t n_seq,
                             uint32_t *d_n_per, uint32_t *d_t_cov, void *stream) {
  const char *who = "mgc_paint_add";
  if (!p) return pos_fail(who, "no painter");
  if ((n_bases && !d_bases) || (n_seq && !d_seq_start)) return pos_fail(who, "no bases or no seq_start");
  if (n_bases >> 32) return pos_fail(who, "a batch holds fewer than 2^32 bases");
  const bool hits = (p->what & MGC_PAINT_HITS) != 0;
  if (hits && n_seq && (!d_n_per || !d_t_cov)) return pos_fail(who, "MGC_PAINT_HITS needs n_per and t_cov");
  if (n_seq == 0) return n_bases ? pos_fail(who, "seq_start does not end at n_bases") : MGC_OK;
  hipStream_t st = (hipStream_t)stream;
  const mgc_posidx *idx = p->idx;
  uint64_t end = 0;
  hipError_t e = hipSetDevice(idx->t.device);
  if (e == hipSuccess) e = hipMemcpyAsync(&end, d_seq_start + n_seq, sizeof(uint64_t), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return pos_rc(e, who);
  if (end != n_bases) return pos_fail(who, "seq_start does not end at n_bases");
  if (hits) {
    e = hipMemsetAsync(d_n_per, 0, sizeof(uint32_t) * n_seq, st);
    if (e == hipSuccess) e = hipMemsetAsync(d_t_cov, 0, sizeof(uint32_t) * n_seq, st);
    if (e != hipSuccess) return pos_rc(e, who);
  }
  if (n_bases == 0) return MGC_OK;
  const bool paint = (p->what & (MGC_PAINT_MERS | MGC_PAINT_QUERIES)) != 0;
  if (paint) e = p->slot.ensure(sizeof(uint32_t) * n_bases);
  if (e == hipSuccess)
    e = mgc::launch_pos_slots(idx->t, d_bases, n_bases, paint ? p->slot.as<uint32_t>() : nullptr, d_seq_start, n_seq, idx->d_pos_start.as<uint64_t>(),
                              hits ? d_t_cov : nullptr, hits ? d_n_per : nullptr, st);
  if (e == hipSuccess && paint) {
    PairSort &ps = p->pairs;
    e = ps.run(p->slot.as<uint32_t>(), n_bases, d_seq_start, n_seq, idx->t.n, st);
    if (e == hipSuccess && ps.n) e = p->scratch.ensure(sizeof(uint64_t) * mgc::pos_sums_scratch_elems(ps.n));
    if (e == hipSuccess && ps.n)
      e = mgc::launch_pos_slot_sums(ps.keys(), ps.vals(), ps.n, p->d_hits.as<uint32_t>(), p->d_queries.as<uint32_t>(), ps.other_keys(), p->scratch.as<uint64_t>(), st);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(st);          // the batch's buffers are the next batch's
  return pos_rc(e, who);
}

extern "C" int mgc_paint_get(const mgc_paint *p, uint32_t which, uint32_t *d_out, void *stream) {
  const char *who = "mgc_paint_get";
  if (!p) return pos_fail(who, "no painter");
  if (which != MGC_PAINT_MERS && which != MGC_PAINT_QUERIES) return pos_fail(who, "'which' is MGC_PAINT_MERS or MGC_PAINT_QUERIES");
  if (!(p->what & which)) return pos_fail(who, "this output was not opened");
  if (p->idx->n_bases && !d_out) return pos_fail(who, "no output");
  return pos_rc(mgc::launch_pos_gather(p->idx->d_ref_slot.as<uint32_t>(), p->idx->n_bases, (which == MGC_PAINT_MERS ? p->d_hits : p->d_queries).as<uint32_t>(), d_out,
                                       (hipStream_t)stream), who);
}
