#pragma once
// Internal launcher of the full-neighbourhood aggregate (agg_full.hip), shared
// with the layer-wise driver (infer_full.hip).  Throws gs::Error.
#include "../host/full_plan.hpp"
#include "kcommon.hpp"

namespace gs {

// Bytes of fp32 partials the window [row0, row0 + n_rows) needs at width F.
int64_t agg_full_ws_need(const FullPlan& p, int64_t F, int64_t row0, int64_t n_rows);
// gs_agg_full (its argument checks included; every check before the first launch).
void agg_full_launch(const FullPlan& p, const gs_full_plan_dev& d, gs_agg op, gs_dtype dt, const void* X, int64_t ldx,
                     int64_t F, const int64_t* row_ptr, const int32_t* col, int64_t row0, int64_t n_rows, void* out,
                     int64_t ldo, void* ws, int64_t ws_bytes, hipStream_t st);

}  // namespace gs
