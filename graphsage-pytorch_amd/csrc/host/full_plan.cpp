// The work plan of the full-neighbourhood aggregate (kernels/agg_full.hip):
// built once per graph, gcn flag and seg_len from the host CSR, uploaded by
// the caller, and read back through the C ABI for checks on the CPU.
//
// Destination row v with deg(v) entries becomes max(1, ceil(deg / seg_len))
// items (v, s): item s covers entries [row_ptr[v] + s·seg_len,
// min(row_ptr[v] + (s + 1)·seg_len, row_ptr[v + 1])), so the items of a row
// cover its entries exactly once, in order (a row without entries keeps one
// empty item: it still has an output row).  Rows of more than seg_len entries
// are "split": each of their items owns one fp32 partial slot, numbered in
// item order, and the row appears in split_rows for the combine pass.
//
// What a lane group that sees one segment cannot know is recorded per row:
// whether the row holds its own id (self loop), and the effective neighbour
// count (the divisor of MEAN): deg minus the self entries without gcn, deg
// plus one when gcn has to add the missing self.
#include "full_plan.hpp"

#include <algorithm>
#include <limits>

namespace gs {

FullPlan* full_plan_build(const int64_t* row_ptr, const int32_t* col, int64_t n, int gcn, int64_t seg_len) {
    GS_REQUIRE(n >= 0 && n < (int64_t(1) << 31), GS_EINVAL, "bad node count");
    GS_REQUIRE(row_ptr && (col || n == 0 || row_ptr[n] == 0), GS_EINVAL, "NULL CSR");
    if (seg_len <= 0) seg_len = std::numeric_limits<int64_t>::max();  // no split
    auto p = std::make_unique<FullPlan>();
    p->n = n;
    p->gcn = gcn != 0;
    p->seg_len = seg_len;
    p->n_entries = n ? row_ptr[n] : 0;
    GS_REQUIRE(n == 0 || row_ptr[0] == 0, GS_EINVAL, "row_ptr[0] must be 0");
    p->item_ptr.assign(n + 1, 0);
    p->slot_ptr.assign(n + 1, 0);
    p->split_ptr.assign(n + 1, 0);
    p->cnt.assign(n, 0);
    p->self_loop.assign(n, 0);
    for (int64_t v = 0; v < n; ++v) {
        const int64_t b = row_ptr[v], e = row_ptr[v + 1];
        GS_REQUIRE(e >= b, GS_EINVAL, "row_ptr must not decrease");
        const int64_t deg = e - b;
        GS_REQUIRE(deg < (int64_t(1) << 31) - 1, GS_EINVAL, "row longer than 2^31 entries");
        int64_t n_self = 0;
        for (int64_t t = b; t < e; ++t) {
            GS_REQUIRE(col[t] >= 0 && col[t] < n, GS_ERANGE, "column id out of range");
            n_self += col[t] == v;
        }
        p->self_loop[v] = n_self != 0;
        const int64_t c = p->gcn ? deg + (n_self == 0) : deg - n_self;
        p->cnt[v] = static_cast<int32_t>(c);
        if (c == 0) p->empty_rows.push_back(static_cast<int32_t>(v));
        const int64_t segs = deg == 0 ? 1 : (deg - 1) / seg_len + 1;
        const bool split = deg > seg_len;
        p->item_ptr[v + 1] = p->item_ptr[v] + segs;
        p->slot_ptr[v + 1] = p->slot_ptr[v] + (split ? segs : 0);
        p->split_ptr[v + 1] = p->split_ptr[v] + split;
        if (split) p->split_rows.push_back(static_cast<int32_t>(v));
    }
    const int64_t n_items = n ? p->item_ptr[n] : 0;
    GS_REQUIRE(n_items < (int64_t(1) << 31), GS_EINVAL, "more than 2^31 work items: raise seg_len");
    p->items.resize(2 * n_items);
    for (int64_t v = 0; v < n; ++v)
        for (int64_t it = p->item_ptr[v]; it < p->item_ptr[v + 1]; ++it) {
            p->items[2 * it] = static_cast<int32_t>(v);
            p->items[2 * it + 1] = static_cast<int32_t>(it - p->item_ptr[v]);
        }
    return p.release();
}

int64_t full_plan_empty_in(const FullPlan& p, int64_t row0, int64_t n_rows) {
    const auto lo = std::lower_bound(p.empty_rows.begin(), p.empty_rows.end(), row0);
    const auto hi = std::lower_bound(p.empty_rows.begin(), p.empty_rows.end(), row0 + n_rows);
    return hi - lo;
}

}  // namespace gs

extern "C" {

int gs_full_plan_create(const int64_t* row_ptr, const int32_t* col, int64_t n_nodes, int32_t gcn, int64_t seg_len,
                        gs_full_plan** out) {
    GS_API_BEGIN
    GS_REQUIRE(out, GS_EINVAL, "NULL out");
    *out = reinterpret_cast<gs_full_plan*>(gs::full_plan_build(row_ptr, col, n_nodes, gcn, seg_len));
    GS_API_END
}

void gs_full_plan_destroy(gs_full_plan* plan) { delete reinterpret_cast<gs::FullPlan*>(plan); }

int gs_full_plan_dims(const gs_full_plan* plan, int64_t* dims) {
    GS_API_BEGIN
    GS_REQUIRE(plan && dims, GS_EINVAL, "NULL argument");
    const gs::FullPlan& p = *reinterpret_cast<const gs::FullPlan*>(plan);
    dims[GS_FP_N_NODES] = p.n;
    dims[GS_FP_N_ITEMS] = static_cast<int64_t>(p.items.size() / 2);
    dims[GS_FP_N_SLOTS] = p.n ? p.slot_ptr[p.n] : 0;
    dims[GS_FP_N_SPLIT] = static_cast<int64_t>(p.split_rows.size());
    dims[GS_FP_N_EMPTY] = static_cast<int64_t>(p.empty_rows.size());
    dims[GS_FP_SEG_LEN] = p.seg_len;
    dims[GS_FP_GCN] = p.gcn;
    dims[GS_FP_N_ENTRIES] = p.n_entries;
    GS_API_END
}

const void* gs_full_plan_array(const gs_full_plan* plan, int32_t which) {
    if (!plan) return nullptr;
    const gs::FullPlan& p = *reinterpret_cast<const gs::FullPlan*>(plan);
    switch (which) {
        case GS_FP_ITEMS: return p.items.data();
        case GS_FP_ITEM_PTR: return p.item_ptr.data();
        case GS_FP_SLOT_PTR: return p.slot_ptr.data();
        case GS_FP_SPLIT_PTR: return p.split_ptr.data();
        case GS_FP_SPLIT_ROWS: return p.split_rows.data();
        case GS_FP_COUNT: return p.cnt.data();
        case GS_FP_SELF_LOOP: return p.self_loop.data();
        case GS_FP_EMPTY_ROWS: return p.empty_rows.data();
        default: return nullptr;
    }
}

}  // extern "C"
