// thfhe_pack.h -- what the single-key engine (thfhe_sk.hip: thfhe_tree_lut_bootstrap, thfhe_dag_run_tree_batch) needs from the packing context of
// thfhe_threshold.hip: host functions only, hidden from the library's dynamic symbol table.  thfhe_poly_ctx itself stays private to
// thfhe_threshold.hip (it holds a KsKey, whose type lives in each translation unit's anonymous namespace).
#ifndef THFHE_PACK_H
#define THFHE_PACK_H

#include <hip/hip_runtime.h>

#include <mutex>

#include "../../include/thfhe_hip.h"

#pragma GCC visibility push(hidden)

namespace thfhe {

int pack_ctx_device(thfhe_poly_ctx *c);
hipStream_t pack_ctx_stream(thfhe_poly_ctx *c);
std::mutex &pack_ctx_mutex(thfhe_poly_ctx *c);
// the packing key's LWE dimension, 0 without a key; the caller holds pack_ctx_mutex
int pack_key_n(thfhe_poly_ctx *c);
// thfhe_pack_boxes on device-resident records, enqueued on `stream`: d_lwe int32[count][n+1] (n = pack_key_n, count a multiple of p, p a
// power of two in 2 .. N/2) -> d_a, d_b int32[count / p][N].  The caller holds pack_ctx_mutex, has made the context's device current and has
// checked the arguments; the context's padded-input and T_i scratch (8 KiB per record) grow as needed.
int pack_boxes_enqueue(thfhe_poly_ctx *c, const int32_t *d_lwe, size_t count, int p, int32_t *d_a, int32_t *d_b, hipStream_t stream);
// grow that scratch for `count` records now, so that no later pack_boxes_enqueue of up to `count` records allocates (the gate-DAG executor sizes
// its workspaces once, when a run starts); the caller holds pack_ctx_mutex, a key is set
int pack_boxes_reserve(thfhe_poly_ctx *c, size_t count);

}  // namespace thfhe

#pragma GCC visibility pop

#endif  // THFHE_PACK_H
