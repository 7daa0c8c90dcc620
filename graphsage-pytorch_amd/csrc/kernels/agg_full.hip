// The full-neighbourhood aggregate over the device CSR (GraphSage.aggregate
// with num_sample=None, models.py:280-330): every destination reads its whole
// CSR row, 64-bit entry offsets, no sampled positions and no pack.
//
// Work items come from the host plan (host/full_plan.cpp): one lane group of
// G lanes per (row, segment), as agg_fwd_kernel owns a destination: kRows
// neighbour rows in flight, every load unconditional (slots past the segment
// re-read a row already in flight) and masked at the accumulate.  A row of at
// most seg_len entries is one item and writes its output row; a longer row's
// items each write an fp32 partial (the segment's sum, or max) into the
// caller's workspace, and agg_full_combine_kernel folds a row's partials in
// segment order, adds gcn's self row last (where the unsplit form adds it) and
// divides by the plan's count.  No atomics: the result is a pure function of
// the inputs and seg_len.  What a segment cannot see on its own -- whether the
// row holds a self loop, and MEAN's divisor -- is read from the plan.
//
// MAP (a template parameter of both kernels): the rows of a receptive field
// (full_field.hip).  The items and split rows are the field's, and a row is
// written to row pos[v] of a compact output; the walk, the partial slots and
// the combine order are the same, so a row is bitwise the unmapped one.
//
// WT (a template parameter of both kernels, MEAN only): per-edge weights.  The
// lane that loads col[e] loads w[e] beside it (the same index: coalesced), the
// weight is shuffled to the group like the row id -- when its row is
// accumulated, after the loads, so that it holds no register across them --
// and the accumulate is acc = fmaf(w, x, acc) in the same visiting order; gcn's appended self row
// takes sw[v], and the row is divided by den[v] (the weights' sum, from the
// caller) or, with den NULL, left as the weighted sum.  fmaf(1, x, acc) is
// acc + x, so unit weights with den = float(cnt) give the WT = false bits.
// The WT = false instantiations hold none of this.
#include "agg_dev.hpp"
#include "agg_full.hpp"

#include <algorithm>

namespace gs {

template <int OP, typename T, int VEC, int G, bool MAP, bool WT>
__global__ __launch_bounds__(kBlock) void agg_full_kernel(const T* __restrict__ X, T* __restrict__ out, FullArgs a) {
    const int gl = threadIdx.x % G;
    const int li = blockIdx.x * (kBlock / G) + threadIdx.x / G;
    if (li >= a.n_items) return;  // whole lane groups leave together
    const int2 it = reinterpret_cast<const int2*>(a.items)[li];
    const int node = it.x, seg = it.y;
    const int64_t rb = a.row_ptr[node], re = a.row_ptr[node + 1];
    const bool split = re - rb > a.seg_len;
    const int64_t beg = rb + seg * a.seg_len;  // seg == 0 unless split
    const int64_t end = split ? min(beg + a.seg_len, re) : re;
    const int F = a.F, gcn = a.gcn;
    const int nf = (F + G * VEC - 1) / (G * VEC);
    for (int fi = 0; fi < nf; ++fi) {
        const int f0 = fi * G * VEC + gl * VEC;
        const bool act = f0 < F;
        const int f0c = act ? f0 : 0;
        float acc[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[v] = (OP == GS_AGG_MAX) ? -INFINITY : 0.f;
        for (int64_t base = beg; base < end; base += G) {
            const int m = static_cast<int>(min(static_cast<int64_t>(G), end - base));
            const bool mine = gl < m;
            const int nb = a.col[mine ? base + gl : base];
            const int my = (mine && (gcn || nb != node)) ? nb : -1;  // self is skipped unless gcn
            float wf = 0.f;
            if constexpr (WT) wf = a.w[mine ? base + gl : base];
            for (int j = 0; j < m; j += kRows) {
                int rows[kRows];
                bool ok[kRows];
#pragma unroll
                for (int u = 0; u < kRows; ++u) {
                    rows[u] = __shfl(my, j + u < m ? j + u : j, G);
                    ok[u] = (j + u < m) && rows[u] >= 0;
                }
                const int fallback = rows[0] >= 0 ? rows[0] : node;
                float x[kRows][VEC];
#pragma unroll
                for (int u = 0; u < kRows; ++u)
                    RowIO<T, VEC>::load(X + static_cast<int64_t>(ok[u] ? rows[u] : fallback) * a.ldx + f0c, x[u]);
#pragma unroll
                for (int u = 0; u < kRows; ++u) {
                    float wu = 0.f;  // the weight joins its row here, after the loads: it holds no register across them
                    if constexpr (WT) wu = __shfl(wf, j + u < m ? j + u : j, G);
#pragma unroll
                    for (int v = 0; v < VEC; ++v) {
                        if constexpr (WT) acc[v] = fmaf(wu, ok[u] ? x[u][v] : 0.f, acc[v]);
                        else if (OP == GS_AGG_MEAN) acc[v] += ok[u] ? x[u][v] : 0.f;
                        else acc[v] = (ok[u] && x[u][v] > acc[v]) ? x[u][v] : acc[v];
                    }
                }
            }
        }
        if (split) {  // the segment's partial; the combine pass finishes the row
            if (act) part_store<VEC>(a.part + (a.slot_ptr[node] - a.slot0 + seg) * F + f0, acc);
            continue;
        }
        if (gcn && !a.self_loop[node]) {  // gcn keeps self exactly once (set semantics)
            float x[VEC];
            RowIO<T, VEC>::load(X + static_cast<int64_t>(node) * a.ldx + f0c, x);
            float sw = 1.f;
            if constexpr (WT) sw = a.sw ? a.sw[node] : 1.f;
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                if constexpr (WT) acc[v] = fmaf(sw, x[v], acc[v]);
                else if (OP == GS_AGG_MEAN) acc[v] += x[v];
                else acc[v] = x[v] > acc[v] ? x[v] : acc[v];
            }
        }
        if (!act) continue;
        if constexpr (WT) {
            if (a.den) {  // the weighted mean: the same true division, by the weights' sum
                const float c = a.den[node];
#pragma unroll
                for (int v = 0; v < VEC; ++v) acc[v] /= c;
            }
        } else if (OP == GS_AGG_MEAN) {
            // a true division (one rounding, as the reference's sum / count), not a product with a rounded
            // reciprocal: a bf16 output flips to the neighbouring value less often; count 0 -> NaN row (0/0, :313)
            const float c = static_cast<float>(a.cnt[node]);
#pragma unroll
            for (int v = 0; v < VEC; ++v) acc[v] /= c;
        }
        RowIO<T, VEC>::store(out + static_cast<int64_t>(MAP ? a.pos[node] : node - a.row0) * a.ldo + f0, acc);
    }
}

// One lane group per split row: its partials in segment order, four loads in
// flight, then gcn's self row (WT: times its weight), the mean's division (WT:
// by den, if any) and the output row.
template <int OP, typename T, int VEC, int G, bool MAP, bool WT>
__global__ __launch_bounds__(kBlock) void agg_full_combine_kernel(const T* __restrict__ X, T* __restrict__ out,
                                                                  FullArgs a) {
    constexpr int NP = 4;
    const int gl = threadIdx.x % G;
    const int r = blockIdx.x * (kBlock / G) + threadIdx.x / G;
    if (r >= a.n_split) return;
    const int node = a.split_rows[r];
    const int64_t deg = a.row_ptr[node + 1] - a.row_ptr[node];
    const int nseg = static_cast<int>((deg - 1) / a.seg_len + 1);
    const int F = a.F;
    const float* prow = a.part + (a.slot_ptr[node] - a.slot0) * F;
    const int nf = (F + G * VEC - 1) / (G * VEC);
    for (int fi = 0; fi < nf; ++fi) {
        const int f0 = fi * G * VEC + gl * VEC;
        if (f0 >= F) continue;
        float acc[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[v] = (OP == GS_AGG_MAX) ? -INFINITY : 0.f;
        for (int s0 = 0; s0 < nseg; s0 += NP) {
            float x[NP][VEC];
#pragma unroll
            for (int u = 0; u < NP; ++u)
                part_load<VEC>(prow + static_cast<int64_t>(min(s0 + u, nseg - 1)) * F + f0, x[u]);
#pragma unroll
            for (int u = 0; u < NP; ++u) {
                const bool ok = s0 + u < nseg;
#pragma unroll
                for (int v = 0; v < VEC; ++v) {
                    if (OP == GS_AGG_MEAN) acc[v] += ok ? x[u][v] : 0.f;
                    else acc[v] = (ok && x[u][v] > acc[v]) ? x[u][v] : acc[v];
                }
            }
        }
        if (a.gcn && !a.self_loop[node]) {
            float x[VEC];
            RowIO<T, VEC>::load(X + static_cast<int64_t>(node) * a.ldx + f0, x);
            float sw = 1.f;
            if constexpr (WT) sw = a.sw ? a.sw[node] : 1.f;
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                if constexpr (WT) acc[v] = fmaf(sw, x[v], acc[v]);
                else if (OP == GS_AGG_MEAN) acc[v] += x[v];
                else acc[v] = x[v] > acc[v] ? x[v] : acc[v];
            }
        }
        if constexpr (WT) {
            if (a.den) {
                const float c = a.den[node];
#pragma unroll
                for (int v = 0; v < VEC; ++v) acc[v] /= c;
            }
        } else if (OP == GS_AGG_MEAN) {
            const float c = static_cast<float>(a.cnt[node]);
#pragma unroll
            for (int v = 0; v < VEC; ++v) acc[v] /= c;
        }
        RowIO<T, VEC>::store(out + static_cast<int64_t>(MAP ? a.pos[node] : node - a.row0) * a.ldo + f0, acc);
    }
}

template <int OP, typename T>
static void launch_full_t(bool vec, const T* X, T* out, const FullArgs& a, hipStream_t st) {
    with_group<sizeof(T) == 4 ? 4 : 8>(vec, a.F, [&](auto vc, auto gc) {
        constexpr int VEC = decltype(vc)::value, G = decltype(gc)::value;
        if constexpr (OP == GS_AGG_MEAN) {
            if (a.w) {
                launch_walk_combine<G>(a.pos != nullptr, a.n_items, a.n_split, st,
                                       agg_full_kernel<OP, T, VEC, G, true, true>,
                                       agg_full_combine_kernel<OP, T, VEC, G, true, true>,
                                       agg_full_kernel<OP, T, VEC, G, false, true>,
                                       agg_full_combine_kernel<OP, T, VEC, G, false, true>, X, out, a);
                return;
            }
        }
        launch_walk_combine<G>(a.pos != nullptr, a.n_items, a.n_split, st,
                               agg_full_kernel<OP, T, VEC, G, true, false>,
                               agg_full_combine_kernel<OP, T, VEC, G, true, false>,
                               agg_full_kernel<OP, T, VEC, G, false, false>,
                               agg_full_combine_kernel<OP, T, VEC, G, false, false>, X, out, a);
    });
}

static void check_window(const FullPlan& p, int64_t row0, int64_t n_rows) {
    GS_REQUIRE(row0 >= 0 && n_rows >= 0 && row0 <= p.n && n_rows <= p.n - row0, GS_EINVAL,
               "rows outside [0, n_nodes)");
}

int64_t agg_full_ws_need(const FullPlan& p, int64_t F, int64_t row0, int64_t n_rows) {
    check_window(p, row0, n_rows);
    GS_REQUIRE(F >= 1 && F < (1 << 30), GS_EINVAL, "bad F");
    return (p.slot_ptr[row0 + n_rows] - p.slot_ptr[row0]) * F * static_cast<int64_t>(sizeof(float));
}

FullArgs full_args(const FullPlan& p, const gs_full_plan_dev& d, const int64_t* row_ptr, const int32_t* col,
                   int64_t row0, int64_t n_rows, int64_t F, int64_t ldx, int64_t ldo, void* ws, const FieldLayer* fl) {
    GS_REQUIRE(!fl || (row0 == 0 && n_rows == p.n), GS_EINVAL, "a field covers the whole plan");
    check_window(p, row0, n_rows);
    GS_REQUIRE(row_ptr && col && d.items && d.slot_ptr && d.count && d.self_loop, GS_EINVAL, "NULL device pointer");
    FullArgs a;
    a.n_split = fl ? static_cast<int>(fl->n_split) : static_cast<int>(p.split_ptr[row0 + n_rows] - p.split_ptr[row0]);
    GS_REQUIRE(a.n_split == 0 || d.split_rows, GS_EINVAL, "NULL split_rows");
    a.ldx = ldx;
    a.ldo = ldo;
    a.row_ptr = row_ptr;
    a.col = col;
    a.items = fl ? fl->items : d.items + 2 * p.item_ptr[row0];
    a.slot_ptr = d.slot_ptr;
    a.split_rows = fl ? fl->split : a.n_split ? d.split_rows + p.split_ptr[row0] : nullptr;
    a.cnt = d.count;
    a.self_loop = d.self_loop;
    a.pos = fl ? fl->pos : nullptr;
    GS_REQUIRE(d.weight || (!d.denom && !d.self_weight), GS_EINVAL, "denom / self_weight without weight");
    a.w = d.weight;
    a.den = d.denom;
    a.sw = d.self_weight;
    a.part = static_cast<float*>(ws);
    a.slot0 = p.slot_ptr[row0];
    a.seg_len = std::min<int64_t>(p.seg_len, (int64_t(1) << 31) - 1);
    a.F = static_cast<int>(F);
    a.n_items = static_cast<int>(fl ? fl->n_items : p.item_ptr[row0 + n_rows] - p.item_ptr[row0]);
    a.row0 = static_cast<int>(row0);
    a.gcn = p.gcn;
    return a;
}

void agg_full_launch(const FullPlan& p, const gs_full_plan_dev& d, gs_agg op, gs_dtype dt, const void* X, int64_t ldx,
                     int64_t F, const int64_t* row_ptr, const int32_t* col, int64_t row0, int64_t n_rows, void* out,
                     int64_t ldo, void* ws, int64_t ws_bytes, hipStream_t st, const FieldLayer* fl) {
    GS_REQUIRE(op == GS_AGG_MEAN || op == GS_AGG_MAX, GS_EINVAL, "agg_func must be MEAN or MAX");
    GS_REQUIRE(dt == GS_F32 || dt == GS_BF16, GS_EINVAL, "dtype must be f32 or bf16");
    GS_REQUIRE(op != GS_AGG_MAX || !d.weight, GS_EINVAL, "edge weights go with MEAN, not MAX");
    GS_REQUIRE(!d.weight || !p.transposed, GS_EINVAL, "a forward plan expected");
    const int64_t need = agg_full_ws_need(p, F, row0, n_rows);
    GS_REQUIRE(ldx >= F && ldo >= F, GS_EINVAL, "leading dimension smaller than F");
    if (n_rows == 0) return;
    GS_REQUIRE(X && out, GS_EINVAL, "NULL device pointer");
    const FullArgs a = full_args(p, d, row_ptr, col, row0, n_rows, F, ldx, ldo, ws, fl);
    if (op == GS_AGG_MAX && full_plan_empty_in(p, row0, n_rows) > 0)
        fail(GS_EEMPTY, "gs_agg_full: MAX aggregation over an empty neighbourhood (reference: models.py:321-325)");
    GS_REQUIRE(need == 0 || (ws && ws_bytes >= need), GS_EINVAL, "workspace smaller than gs_agg_full_ws_bytes");
    const int V = dt == GS_F32 ? 4 : 8;
    const bool vec = F % V == 0 && ldx % V == 0 && ldo % V == 0 && aligned16(X) && aligned16(out) &&
                     (need == 0 || aligned16(ws));
    if (op == GS_AGG_MEAN) {
        if (dt == GS_F32) launch_full_t<GS_AGG_MEAN, float>(vec, static_cast<const float*>(X), static_cast<float*>(out), a, st);
        else launch_full_t<GS_AGG_MEAN, bf16_t>(vec, static_cast<const bf16_t*>(X), static_cast<bf16_t*>(out), a, st);
    } else {
        if (dt == GS_F32) launch_full_t<GS_AGG_MAX, float>(vec, static_cast<const float*>(X), static_cast<float*>(out), a, st);
        else launch_full_t<GS_AGG_MAX, bf16_t>(vec, static_cast<const bf16_t*>(X), static_cast<bf16_t*>(out), a, st);
    }
    check_launch("gs_agg_full");
}

}  // namespace gs

extern "C" {

int64_t gs_agg_full_ws_bytes(const gs_full_plan* plan, int64_t F, int64_t row0, int64_t n_rows) {
    GS_BYTES_BEGIN
    if (!plan) return -1;
    return gs::agg_full_ws_need(*reinterpret_cast<const gs::FullPlan*>(plan), F, row0, n_rows);
    GS_BYTES_END
}

int gs_agg_full(const gs_full_plan* plan, const gs_full_plan_dev* dev, gs_agg op, gs_dtype dt, const void* X,
                int64_t ldx, int64_t F, const int64_t* row_ptr, const int32_t* col, int64_t row0, int64_t n_rows,
                void* out, int64_t ldo, void* ws, int64_t ws_bytes, void* stream) {
    GS_API_BEGIN
    GS_REQUIRE(plan && dev, GS_EINVAL, "NULL plan");
    gs::agg_full_launch(*reinterpret_cast<const gs::FullPlan*>(plan), *dev, op, dt, X, ldx, F, row_ptr, col, row0,
                        n_rows, out, ldo, ws, ws_bytes, gs::as_stream(stream));
    GS_API_END
}

}  // extern "C"
