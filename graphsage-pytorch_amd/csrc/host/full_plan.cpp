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
//
// The backward of "destination v reads its sources" is "source u reads every
// destination v whose effective neighbourhood holds u": full_plan_transpose
// builds that CSR with a stable counting sort over the forward rows (so each
// transposed row lists its destinations in ascending id order, an entry the
// forward row repeats repeated here), under the forward's rules -- a row's own
// id is dropped, and under gcn v is a destination of itself exactly once --
// and plans it like a forward CSR, at a seg_len of its own.  Symmetry of the
// input is never assumed.  The same pass records t_src: the forward entry
// each transposed entry came from (-1 for the self entry gcn adds to a row
// without a self loop), so per-edge weights in forward order can be permuted
// into transposed order, and replaced, without another plan.
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

FullPlan* full_plan_transpose(const FullPlan& fwd, const int64_t* row_ptr, const int32_t* col, int64_t seg_len) {
    GS_REQUIRE(!fwd.transposed, GS_EINVAL, "the plan is already a transposed one");
    const int64_t n = fwd.n;
    GS_REQUIRE(row_ptr && (col || fwd.n_entries == 0), GS_EINVAL, "NULL CSR");
    GS_REQUIRE((n ? row_ptr[n] : 0) == fwd.n_entries, GS_EINVAL, "the CSR is not the plan's");
    std::vector<int64_t> trp(n + 1, 0);
    for (int64_t v = 0; v < n; ++v) {
        for (int64_t t = row_ptr[v]; t < row_ptr[v + 1]; ++t) {
            GS_REQUIRE(col[t] >= 0 && col[t] < n, GS_ERANGE, "column id out of range");
            if (col[t] != v) ++trp[col[t] + 1];
        }
        if (fwd.gcn) ++trp[v + 1];
    }
    for (int64_t u = 0; u < n; ++u) trp[u + 1] += trp[u];
    std::vector<int32_t> tcol(static_cast<size_t>(n ? trp[n] : 0));
    std::vector<int64_t> tsrc(tcol.size());
    std::vector<int64_t> fill(trp.begin(), trp.end() - 1);
    for (int64_t v = 0; v < n; ++v) {  // ascending v: every transposed row ends up ascending
        int64_t self_t = -1;  // the row's (first) self entry
        for (int64_t t = row_ptr[v]; t < row_ptr[v + 1]; ++t) {
            const int32_t u = col[t];
            if (u != v) {
                tsrc[fill[u]] = t;
                tcol[fill[u]++] = static_cast<int32_t>(v);
            } else if (self_t < 0) {
                self_t = t;
            }
        }
        // v's own entry: every smaller destination of v is already in place and every larger one comes later
        if (fwd.gcn) {
            tsrc[fill[v]] = self_t;
            tcol[fill[v]++] = static_cast<int32_t>(v);
        }
    }
    std::unique_ptr<FullPlan> p(full_plan_build(trp.data(), tcol.data(), n, 0, seg_len));
    p->gcn = fwd.gcn;
    p->transposed = true;
    p->cnt = fwd.cnt;
    std::fill(p->self_loop.begin(), p->self_loop.end(), uint8_t(0));
    p->empty_rows.clear();
    p->t_row_ptr = std::move(trp);
    p->t_col = std::move(tcol);
    p->t_src = std::move(tsrc);
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

int gs_full_plan_transpose(const gs_full_plan* plan, const int64_t* row_ptr, const int32_t* col, int64_t seg_len,
                           gs_full_plan** out) {
    GS_API_BEGIN
    GS_REQUIRE(plan && out, GS_EINVAL, "NULL argument");
    *out = reinterpret_cast<gs_full_plan*>(
        gs::full_plan_transpose(*reinterpret_cast<const gs::FullPlan*>(plan), row_ptr, col, seg_len));
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
        case GS_FP_T_ROW_PTR: return p.transposed ? p.t_row_ptr.data() : nullptr;
        case GS_FP_T_COL: return p.transposed ? p.t_col.data() : nullptr;
        case GS_FP_T_SRC: return p.transposed ? p.t_src.data() : nullptr;
        default: return nullptr;
    }
}

int gs_full_plan_edge_denom(const gs_full_plan* plan, const int64_t* row_ptr, const int32_t* col, const float* w,
                            const float* self_weight, float* den) {
    GS_API_BEGIN
    GS_REQUIRE(plan && row_ptr && den, GS_EINVAL, "NULL argument");
    const gs::FullPlan& p = *reinterpret_cast<const gs::FullPlan*>(plan);
    GS_REQUIRE(!p.transposed, GS_EINVAL, "a forward plan expected");
    GS_REQUIRE((p.n ? row_ptr[p.n] : 0) == p.n_entries && (p.n_entries == 0 || (col && w)), GS_EINVAL,
               "the CSR is not the plan's");
    for (int64_t v = 0; v < p.n; ++v) {
        double s = 0.0;  // entry order, one rounding at the end: float(COUNT) for unit weights
        for (int64_t t = row_ptr[v]; t < row_ptr[v + 1]; ++t)
            if (p.gcn || col[t] != v) s += static_cast<double>(w[t]);
        if (p.gcn && !p.self_loop[v]) s += self_weight ? static_cast<double>(self_weight[v]) : 1.0;
        den[v] = static_cast<float>(s);
    }
    GS_API_END
}

}  // extern "C"
