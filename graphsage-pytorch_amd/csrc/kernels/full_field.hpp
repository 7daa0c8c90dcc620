#pragma once
// The receptive field of a mini-batch on the device (full_field.hip): the
// buffer layout, and what one layer of a built field hands to the row-mapped
// aggregates (agg_full.hip, agg_full_bwd.hip) and the restricted step
// (train_full.hip).  Throws gs::Error.
#include "../host/full_plan.hpp"
#include "kcommon.hpp"

namespace gs {

struct FieldLayout {
    int64_t counts = 0, flags = 0, scan = 0;
    int64_t rows[GS_MAX_HOPS + 1], pos[GS_MAX_HOPS + 1];                                  // level 0..L
    int64_t items[GS_MAX_HOPS + 1], split[GS_MAX_HOPS + 1], t_items[GS_MAX_HOPS + 1], t_split[GS_MAX_HOPS + 1];
    int64_t scan_ints = 0, total = 0;
};
FieldLayout field_layout(const FullPlan& p, const FullPlan& tp, int n_layers);

// Layer l of a built field whose counts are on the host.
struct FieldLayer {
    const int* rows;       // R_l, ascending
    const int* pos;        // id -> index in rows, -1 outside
    const int* rows_prev;  // R_{l-1}
    const int* pos_prev;
    const int* items;      // forward items / split rows of R_l
    const int* split;
    const int* t_items;    // transposed items / split rows of R_{l-1}
    const int* t_split;
    int64_t n, n_prev, n_items, n_split, n_t_items, n_t_split;
};
// Checks f against the plans (sizes, alignment, counts inside their arrays) and 1 <= layer <= f.n_layers.
FieldLayer field_layer(const FullPlan& p, const FullPlan& tp, const gs_full_field& f, int layer);

}  // namespace gs
