// mgc_list.hpp -- the k-mer text lister (mgc_list.hip) as the evaluator uses it: one set of staging buffers that serves any number
// of listings, one after the other.  The public form is include/meryl_list.h.  Internal.
#pragma once

#include "../../include/meryl_list.h"

#include <hip/hip_runtime.h>

namespace mgc {
struct ListStage;                                    // two device + two pinned staging buffers (grow-only), the copy stream, events
ListStage *list_stage_open();
void       list_stage_close(ListStage *s);           // s may be null
// mgc_list_kmers with the caller's staging buffers; `who` leads the failure text (the thread's last error)
int list_kmers(ListStage *s, const void *d_keys, const uint32_t *d_values, const uint64_t *d_labels_or_null, uint64_t n, uint32_t k,
               uint32_t label_size, uint64_t chunk_bytes, mgc_list_write_cb cb, void *user, hipStream_t st, const char *who);
}  // namespace mgc
