// What training over full neighbourhoods adds to agg_full.hip: the MAX
// forward that records its argmax, and the backward of the aggregate.
//
// agg_full_argmax_kernel is agg_full_kernel<MAX, float> with one id per
// accumulator: the global id of the first maximal source in the order the
// kernel visits them (a strict >, as agg_dev.hpp and torch.max: first wins
// ties).  A split row's partials carry their ids in a second block of the
// workspace, and the combine pass folds them in segment order with the same
// strict >, then gcn's missing self row, so the choice is the unsplit one.
//
// agg_full_bwd_kernel runs over the transposed plan (host/full_plan.cpp): one
// lane group of G lanes per (source row u, segment), the forward's in-flight
// row loads over the destinations v of the segment,
//   MEAN  acc += dA[v] / cnt[v]                 (cnt: the forward's divisor; a true
//                                                division per element, as autograd's)
//   MAX   acc += dA[v] where argmax[v] == u     (a destination the row repeats counts once)
// fp32 partials for split rows, a combine pass in segment order, and an
// epilogue that adds the self-row gradient dSelf[u] and zeroes the row where
// Hprev[u] <= 0 (the relu of the layer below), so dH_{l-1} leaves finished.
// No atomics: a pure function of the inputs and seg_len.
//
// MAP (a template parameter, as in agg_full.hip): layer l of a receptive
// field.  The forward writes row pos_l[v] of compact outputs; the backward
// runs over the transposed items of R_{l-1}, masks a destination v outside
// R_l like a slot past the segment, reads dA and argmax at row pos_l[v] (the
// divisor cnt[v] and the compared ids stay global), adds dSelf[pos_l[u]]
// only where u is in R_l, and writes row pos_{l-1}[u] of a compact dH.
//
// WM (a template parameter of the MEAN backward walk): per-edge weights in the
// transposed plan's entry order.  The lane that loads t_col[e] loads w_t[e]
// and, for the weighted mean (WM == 1), den[v] in place of cnt[v]; den is
// shuffled with the row id as cnt is, the weight when its row is accumulated
// (it then holds no register across the loads: the weighted walk keeps the
// unweighted one's occupancy), and acc = fmaf(w, dA[v] / den[v], acc).  WM == 2
// is the weighted sum: no divisor and no division.  WM == 0 is the unweighted
// kernel, unchanged; unit weights with den = float(cnt) give its bits.
#include "agg_dev.hpp"
#include "agg_full.hpp"

#include <algorithm>

// The backward MEAN's quotient dA / count.  GS_FULL_BWD_QUOT_MODE is a build switch for measurements
// (tools/build_alt.sh, profiles/full_train_bwd_div_ab.json); the library build leaves it at 0:
//   0  a division per element, autograd's grad / count
//   1  a product with the rounded reciprocal: another arithmetic, 1.4-1.7x faster, measurement only
//   2  the division's result from one reciprocal per loaded row: with r = RN(1 / c), q = RN(x r) and
//      e = x - c q (exact in an FMA), RN(q + e r) is the correctly rounded x / c for a divisor whose
//      significand is not all ones and a normal quotient (Markstein).  Bitwise the division on
//      test_mean_backward_quotient_is_the_division's 1.3 M quotients, but only 10-18 % faster (it
//      costs 9 more registers and a wave of occupancy): not worth a second arithmetic to reason about.
#ifndef GS_FULL_BWD_QUOT_MODE
#define GS_FULL_BWD_QUOT_MODE 0
#endif

namespace gs {

namespace {

// x / c for the row's divisor c and r = 1.0f / c (see GS_FULL_BWD_QUOT_MODE).
__device__ __forceinline__ float mean_quot(float x, float c, float r) {
#if GS_FULL_BWD_QUOT_MODE == 0
    return x / c;
#elif GS_FULL_BWD_QUOT_MODE == 1
    return x * r;
#else
    const float q = x * r;
    return fmaf(fmaf(-c, q, x), r, q);
#endif
}

template <int VEC>
__device__ __forceinline__ void get_ids(const int* p, int (&v)[VEC]) {
    if constexpr (VEC == 1) {
        v[0] = *p;
    } else {
#pragma unroll
        for (int q = 0; q < VEC / 4; ++q) {
            const int4 t = reinterpret_cast<const int4*>(p)[q];
            v[4 * q] = t.x; v[4 * q + 1] = t.y; v[4 * q + 2] = t.z; v[4 * q + 3] = t.w;
        }
    }
}

template <int VEC>
__device__ __forceinline__ void put_ids(int* p, const int (&v)[VEC]) {
    if constexpr (VEC == 1) {
        *p = v[0];
    } else {
#pragma unroll
        for (int q = 0; q < VEC / 4; ++q)
            reinterpret_cast<int4*>(p)[q] = make_int4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
    }
}

struct ArgmaxOut {
    int* am;        // [n_rows][F] ids, row stride lda
    int64_t lda;
    int* part_ids;  // the partials' ids, indexed as FullArgs::part
};

// gcn's missing self row (last, as the unsplit forward adds it) and the output rows.
template <int VEC, bool MAP>
__device__ __forceinline__ void argmax_finish(const float* __restrict__ X, float* __restrict__ out, const FullArgs& a,
                                              const ArgmaxOut& o, int node, int f0, float (&acc)[VEC], int (&arg)[VEC]) {
    if (a.gcn && !a.self_loop[node]) {
        float x[VEC];
        RowIO<float, VEC>::load(X + static_cast<int64_t>(node) * a.ldx + f0, x);
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            const bool take = x[v] > acc[v];
            acc[v] = take ? x[v] : acc[v];
            arg[v] = take ? node : arg[v];
        }
    }
    const int64_t orow = MAP ? a.pos[node] : node - a.row0;
    RowIO<float, VEC>::store(out + orow * a.ldo + f0, acc);
    put_ids<VEC>(o.am + orow * o.lda + f0, arg);
}

template <int VEC, int G, bool MAP>
__global__ __launch_bounds__(kBlock) void agg_full_argmax_kernel(const float* __restrict__ X, float* __restrict__ out,
                                                                 FullArgs a, ArgmaxOut o) {
    constexpr int NR = kRows / 2;  // an id beside every accumulator: half the rows in flight
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
        int arg[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            acc[v] = -INFINITY;
            arg[v] = -1;
        }
        for (int64_t base = beg; base < end; base += G) {
            const int m = static_cast<int>(min(static_cast<int64_t>(G), end - base));
            const bool mine = gl < m;
            const int nb = a.col[mine ? base + gl : base];
            const int my = (mine && (gcn || nb != node)) ? nb : -1;  // self is skipped unless gcn
            for (int j = 0; j < m; j += NR) {
                int rows[NR];
                bool ok[NR];
#pragma unroll
                for (int u = 0; u < NR; ++u) {
                    rows[u] = __shfl(my, j + u < m ? j + u : j, G);
                    ok[u] = (j + u < m) && rows[u] >= 0;
                }
                const int fallback = rows[0] >= 0 ? rows[0] : node;
                float x[NR][VEC];
#pragma unroll
                for (int u = 0; u < NR; ++u)
                    RowIO<float, VEC>::load(X + static_cast<int64_t>(ok[u] ? rows[u] : fallback) * a.ldx + f0c, x[u]);
#pragma unroll
                for (int u = 0; u < NR; ++u) {
#pragma unroll
                    for (int v = 0; v < VEC; ++v) {
                        const bool take = ok[u] && x[u][v] > acc[v];  // strict: the first maximal entry stays
                        acc[v] = take ? x[u][v] : acc[v];
                        arg[v] = take ? rows[u] : arg[v];
                    }
                }
            }
        }
        if (!act) continue;
        if (split) {  // the segment's partial and its ids; the combine pass finishes the row
            const int64_t po = (a.slot_ptr[node] - a.slot0 + seg) * F + f0;
            part_store<VEC>(a.part + po, acc);
            put_ids<VEC>(o.part_ids + po, arg);
            continue;
        }
        argmax_finish<VEC, MAP>(X, out, a, o, node, f0, acc, arg);
    }
}

template <int VEC, int G, bool MAP>
__global__ __launch_bounds__(kBlock) void agg_full_argmax_combine_kernel(const float* __restrict__ X,
                                                                         float* __restrict__ out, FullArgs a,
                                                                         ArgmaxOut o) {
    const int gl = threadIdx.x % G;
    const int r = blockIdx.x * (kBlock / G) + threadIdx.x / G;
    if (r >= a.n_split) return;
    const int node = a.split_rows[r];
    const int64_t deg = a.row_ptr[node + 1] - a.row_ptr[node];
    const int nseg = static_cast<int>((deg - 1) / a.seg_len + 1);
    const int F = a.F;
    const int64_t p0 = (a.slot_ptr[node] - a.slot0) * F;
    const int nf = (F + G * VEC - 1) / (G * VEC);
    for (int fi = 0; fi < nf; ++fi) {
        const int f0 = fi * G * VEC + gl * VEC;
        if (f0 >= F) continue;
        float acc[VEC];
        int arg[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            acc[v] = -INFINITY;
            arg[v] = -1;
        }
        for (int s = 0; s < nseg; ++s) {  // segment order, strict >: an earlier segment keeps a tie
            float x[VEC];
            int id[VEC];
            part_load<VEC>(a.part + p0 + static_cast<int64_t>(s) * F + f0, x);
            get_ids<VEC>(o.part_ids + p0 + static_cast<int64_t>(s) * F + f0, id);
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                const bool take = x[v] > acc[v];
                acc[v] = take ? x[v] : acc[v];
                arg[v] = take ? id[v] : arg[v];
            }
        }
        argmax_finish<VEC, MAP>(X, out, a, o, node, f0, acc, arg);
    }
}

// ------------------------------------------------------------------ backward
struct BwdArgs {
    const int64_t* row_ptr;  // the transposed CSR
    const int* col;
    const int* items;
    const int64_t* slot_ptr;
    const int* split_rows;
    const int* cnt;          // the forward's effective neighbour counts
    const float* w;          // WM != 0: a weight per transposed entry
    const float* den;        // WM == 1: the weighted mean's divisor per destination
    const float* dA;
    const float* dSelf;      // may be NULL
    int64_t ldd;
    const int* am;           // MAX: the forward's argmax, row stride lda
    int64_t lda;
    const float* Hprev;      // may be NULL
    float* dH;
    int64_t ldh;
    const int* pos;          // MAP: a destination's row of dA / dSelf / am (a field's pos_l), -1: not in R_l
    const int* opos;         // MAP: a source row's row of dH (pos_{l-1})
    int64_t ldo;             // MAP: dH's row stride (Hprev keeps ldh)
    float* part;
    int64_t seg_len;         // clamped to 2^31 - 1
    int F, n_items, n_split;
};

// dH[u] = (acc + dSelf[u]) zeroed where Hprev[u] <= 0.  MAP: dSelf only where u is in R_l, dH compact.
template <int VEC, bool MAP>
__device__ __forceinline__ void bwd_finish(const BwdArgs& a, int node, int f0, float (&acc)[VEC]) {
    const int64_t srow = MAP ? a.pos[node] : node;
    if (a.dSelf && (!MAP || srow >= 0)) {
        float s[VEC];
        RowIO<float, VEC>::load(a.dSelf + srow * a.ldd + f0, s);
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[v] += s[v];
    }
    if (a.Hprev) {
        float h[VEC];
        RowIO<float, VEC>::load(a.Hprev + static_cast<int64_t>(node) * a.ldh + f0, h);
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[v] = h[v] <= 0.f ? 0.f : acc[v];
    }
    if (MAP) RowIO<float, VEC>::store(a.dH + static_cast<int64_t>(a.opos[node]) * a.ldo + f0, acc);
    else RowIO<float, VEC>::store(a.dH + static_cast<int64_t>(node) * a.ldh + f0, acc);
}

template <int OP, int VEC, int G, bool MAP, int WM>
__global__ __launch_bounds__(kBlock) void agg_full_bwd_kernel(BwdArgs a) {
    constexpr int NR = OP == GS_AGG_MAX ? kRows / 2 : kRows;  // MAX loads an id row beside every gradient row
    const int gl = threadIdx.x % G;
    const int li = blockIdx.x * (kBlock / G) + threadIdx.x / G;
    if (li >= a.n_items) return;  // whole lane groups leave together
    const int2 it = reinterpret_cast<const int2*>(a.items)[li];
    const int node = it.x, seg = it.y;
    const int64_t rb = a.row_ptr[node], re = a.row_ptr[node + 1];
    const bool split = re - rb > a.seg_len;
    const int64_t beg = rb + seg * a.seg_len;  // seg == 0 unless split
    const int64_t end = split ? min(beg + a.seg_len, re) : re;
    const int F = a.F;
    const int nf = (F + G * VEC - 1) / (G * VEC);
    for (int fi = 0; fi < nf; ++fi) {
        const int f0 = fi * G * VEC + gl * VEC;
        const bool act = f0 < F;
        const int f0c = act ? f0 : 0;
        float acc[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[v] = 0.f;
        for (int64_t base = beg; base < end; base += G) {
            const int m = static_cast<int>(min(static_cast<int64_t>(G), end - base));
            const bool mine = gl < m;
            const int64_t e = mine ? base + gl : base;
            const int nb = a.col[e];
            int my = mine ? nb : -1;
            float cf = 1.f, wf = 0.f;
            if constexpr (WM != 0) wf = a.w[e];
            if constexpr (WM == 1) cf = a.den[nb];
            else if constexpr (WM == 2) cf = 1.f;
            else if (OP == GS_AGG_MEAN) cf = static_cast<float>(a.cnt[nb]);
            // MAX routes a destination's gradient once, however often its row names this source (the
            // transposed row is ascending: repeats are neighbours, across a segment boundary too)
            else if (e > rb && a.col[e - 1] == nb) my = -1;
            if (MAP && my >= 0) my = a.pos[nb];  // the destination's compact row; -1: outside R_l, skipped
            for (int j = 0; j < m; j += NR) {
                int rows[NR];
                float c[NR];
                bool ok[NR];
#pragma unroll
                for (int u = 0; u < NR; ++u) {
                    const int src = j + u < m ? j + u : j;
                    rows[u] = __shfl(my, src, G);
                    if constexpr (OP == GS_AGG_MEAN && WM == 0) c[u] = __shfl(cf, src, G);
                    ok[u] = (j + u < m) && rows[u] >= 0;
                }
                const int fallback = rows[0] >= 0 ? rows[0] : (MAP ? 0 : node);  // R_l is never empty
                float x[NR][VEC];
                int id[OP == GS_AGG_MAX ? NR : 1][VEC];
#pragma unroll
                for (int u = 0; u < NR; ++u) {
                    const int64_t r = ok[u] ? rows[u] : fallback;
                    RowIO<float, VEC>::load(a.dA + r * a.ldd + f0c, x[u]);
                    if constexpr (OP == GS_AGG_MAX) get_ids<VEC>(a.am + r * a.lda + f0c, id[u]);
                }
#pragma unroll
                for (int u = 0; u < NR; ++u) {
                    float wu = 0.f;  // the weight (and its divisor) join the row here, after the loads: they hold
                                     // no register across them
                    if constexpr (WM != 0) wu = __shfl(wf, j + u < m ? j + u : j, G);
                    if constexpr (WM == 1) c[u] = __shfl(cf, j + u < m ? j + u : j, G);
                    const float r = (OP == GS_AGG_MEAN && WM != 2 && GS_FULL_BWD_QUOT_MODE != 0) ? 1.0f / c[u] : 0.f;
#pragma unroll
                    for (int v = 0; v < VEC; ++v) {
                        if constexpr (WM == 1) acc[v] = fmaf(wu, ok[u] ? mean_quot(x[u][v], c[u], r) : 0.f, acc[v]);
                        else if constexpr (WM == 2) acc[v] = fmaf(wu, ok[u] ? x[u][v] : 0.f, acc[v]);
                        else if constexpr (OP == GS_AGG_MEAN) acc[v] += ok[u] ? mean_quot(x[u][v], c[u], r) : 0.f;
                        else acc[v] += (ok[u] && id[u][v] == node) ? x[u][v] : 0.f;
                    }
                }
            }
        }
        if (!act) continue;
        if (split) {  // the segment's partial sum; the combine pass finishes the row
            part_store<VEC>(a.part + (a.slot_ptr[node] + seg) * F + f0, acc);
            continue;
        }
        bwd_finish<VEC, MAP>(a, node, f0, acc);
    }
}

// One lane group per split source row: its partial sums in segment order, four loads in flight.
template <int VEC, int G, bool MAP>
__global__ __launch_bounds__(kBlock) void agg_full_bwd_combine_kernel(BwdArgs a) {
    constexpr int NP = 4;
    const int gl = threadIdx.x % G;
    const int r = blockIdx.x * (kBlock / G) + threadIdx.x / G;
    if (r >= a.n_split) return;
    const int node = a.split_rows[r];
    const int64_t deg = a.row_ptr[node + 1] - a.row_ptr[node];
    const int nseg = static_cast<int>((deg - 1) / a.seg_len + 1);
    const int F = a.F;
    const float* prow = a.part + a.slot_ptr[node] * F;
    const int nf = (F + G * VEC - 1) / (G * VEC);
    for (int fi = 0; fi < nf; ++fi) {
        const int f0 = fi * G * VEC + gl * VEC;
        if (f0 >= F) continue;
        float acc[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[v] = 0.f;
        for (int s0 = 0; s0 < nseg; s0 += NP) {
            float x[NP][VEC];
#pragma unroll
            for (int u = 0; u < NP; ++u)
                part_load<VEC>(prow + static_cast<int64_t>(min(s0 + u, nseg - 1)) * F + f0, x[u]);
#pragma unroll
            for (int u = 0; u < NP; ++u) {
                const bool ok = s0 + u < nseg;
#pragma unroll
                for (int v = 0; v < VEC; ++v) acc[v] += ok ? x[u][v] : 0.f;
            }
        }
        bwd_finish<VEC, MAP>(a, node, f0, acc);
    }
}

template <int OP>
void launch_bwd_t(bool vec, const BwdArgs& a, hipStream_t st) {
    with_group<4>(vec, a.F, [&](auto vc, auto gc) {
        constexpr int VEC = decltype(vc)::value, G = decltype(gc)::value;
        if constexpr (OP == GS_AGG_MEAN) {
            if (a.w && a.den) {
                launch_walk_combine<G>(a.pos != nullptr, a.n_items, a.n_split, st,
                                       agg_full_bwd_kernel<OP, VEC, G, true, 1>, agg_full_bwd_combine_kernel<VEC, G, true>,
                                       agg_full_bwd_kernel<OP, VEC, G, false, 1>,
                                       agg_full_bwd_combine_kernel<VEC, G, false>, a);
                return;
            }
            if (a.w) {
                launch_walk_combine<G>(a.pos != nullptr, a.n_items, a.n_split, st,
                                       agg_full_bwd_kernel<OP, VEC, G, true, 2>, agg_full_bwd_combine_kernel<VEC, G, true>,
                                       agg_full_bwd_kernel<OP, VEC, G, false, 2>,
                                       agg_full_bwd_combine_kernel<VEC, G, false>, a);
                return;
            }
        }
        launch_walk_combine<G>(a.pos != nullptr, a.n_items, a.n_split, st, agg_full_bwd_kernel<OP, VEC, G, true, 0>,
                               agg_full_bwd_combine_kernel<VEC, G, true>, agg_full_bwd_kernel<OP, VEC, G, false, 0>,
                               agg_full_bwd_combine_kernel<VEC, G, false>, a);
    });
}

}  // namespace

int64_t agg_full_argmax_ws_need(const FullPlan& p, int64_t F, int64_t row0, int64_t n_rows) {
    return 2 * agg_full_ws_need(p, F, row0, n_rows);
}

void agg_full_argmax_launch(const FullPlan& p, const gs_full_plan_dev& d, gs_dtype dt, const void* X, int64_t ldx,
                            int64_t F, const int64_t* row_ptr, const int32_t* col, int64_t row0, int64_t n_rows,
                            void* out, int64_t ldo, int32_t* argmax, int64_t lda, void* ws, int64_t ws_bytes,
                            hipStream_t st, const FieldLayer* fl) {
    GS_REQUIRE(dt == GS_F32, GS_EINVAL, "gs_agg_full_argmax: fp32 rows only (a bf16 table's aggregate has no backward)");
    GS_REQUIRE(!d.weight, GS_EINVAL, "gs_agg_full_argmax: edge weights go with MEAN, not MAX");
    GS_REQUIRE(!p.transposed, GS_EINVAL, "gs_agg_full_argmax: a forward plan expected");
    const int64_t need = agg_full_argmax_ws_need(p, F, row0, n_rows);
    GS_REQUIRE(ldx >= F && ldo >= F && lda >= F, GS_EINVAL, "leading dimension smaller than F");
    if (n_rows == 0) return;
    GS_REQUIRE(X && out && argmax, GS_EINVAL, "NULL device pointer");
    const FullArgs a = full_args(p, d, row_ptr, col, row0, n_rows, F, ldx, ldo, ws, fl);
    if (full_plan_empty_in(p, row0, n_rows) > 0)
        fail(GS_EEMPTY, "gs_agg_full_argmax: MAX aggregation over an empty neighbourhood (reference: models.py:321-325)");
    GS_REQUIRE(need == 0 || (ws && ws_bytes >= need), GS_EINVAL,
               "workspace smaller than gs_agg_full_argmax_ws_bytes");
    const bool vec = F % 4 == 0 && ldx % 4 == 0 && ldo % 4 == 0 && lda % 4 == 0 && aligned16(X) && aligned16(out) &&
                     aligned16(argmax) && (need == 0 || aligned16(ws));
    ArgmaxOut o;
    o.am = argmax;
    o.lda = lda;
    o.part_ids = reinterpret_cast<int*>(static_cast<char*>(ws) + need / 2);  // F % 4 == 0 keeps it 16-byte aligned
    const float* Xf = static_cast<const float*>(X);
    float* of = static_cast<float*>(out);
    with_group<4>(vec, a.F, [&](auto vc, auto gc) {
        constexpr int VEC = decltype(vc)::value, G = decltype(gc)::value;
        launch_walk_combine<G>(a.pos != nullptr, a.n_items, a.n_split, st, agg_full_argmax_kernel<VEC, G, true>,
                               agg_full_argmax_combine_kernel<VEC, G, true>, agg_full_argmax_kernel<VEC, G, false>,
                               agg_full_argmax_combine_kernel<VEC, G, false>, Xf, of, a, o);
    });
    check_launch("gs_agg_full_argmax");
}

int64_t agg_full_bwd_ws_need(const FullPlan& tp, int64_t F) {
    GS_REQUIRE(tp.transposed, GS_EINVAL, "gs_agg_full_bwd: a transposed plan expected (gs_full_plan_transpose)");
    GS_REQUIRE(F >= 1 && F < (1 << 30), GS_EINVAL, "bad F");
    return (tp.n ? tp.slot_ptr[tp.n] : 0) * F * static_cast<int64_t>(sizeof(float));
}

void agg_full_bwd_launch(const FullPlan& tp, const gs_full_plan_dev& td, gs_agg op, int64_t F,
                         const int64_t* t_row_ptr, const int32_t* t_col, const float* dA, const float* dSelf,
                         int64_t ldd, const int32_t* argmax, int64_t lda, const float* Hprev, float* dH, int64_t ldh,
                         void* ws, int64_t ws_bytes, hipStream_t st, const FieldLayer* fl, int64_t ldo) {
    GS_REQUIRE(op == GS_AGG_MEAN || op == GS_AGG_MAX, GS_EINVAL, "agg_func must be MEAN or MAX");
    GS_REQUIRE(op != GS_AGG_MAX || !td.weight, GS_EINVAL, "edge weights go with MEAN, not MAX");
    GS_REQUIRE(td.weight || !td.denom, GS_EINVAL, "denom without weight");
    const int64_t need = agg_full_bwd_ws_need(tp, F);
    GS_REQUIRE(!fl || ldo >= F, GS_EINVAL, "leading dimension smaller than F");
    GS_REQUIRE(ldd >= F && ldh >= F && (op != GS_AGG_MAX || lda >= F), GS_EINVAL, "leading dimension smaller than F");
    if (tp.n == 0) return;
    GS_REQUIRE(t_row_ptr && t_col && dA && dH && td.items && td.slot_ptr && td.count, GS_EINVAL, "NULL device pointer");
    GS_REQUIRE(op != GS_AGG_MAX || argmax, GS_EINVAL, "MAX needs the forward's argmax");
    GS_REQUIRE(need == 0 || (ws && ws_bytes >= need), GS_EINVAL, "workspace smaller than gs_agg_full_bwd_ws_bytes");
    BwdArgs a;
    a.n_split = static_cast<int>(tp.split_rows.size());
    GS_REQUIRE(a.n_split == 0 || td.split_rows, GS_EINVAL, "NULL split_rows");
    const bool vec = F % 4 == 0 && ldd % 4 == 0 && ldh % 4 == 0 && (!fl || ldo % 4 == 0) && aligned16(dA) && aligned16(dH) &&
                     (!dSelf || aligned16(dSelf)) && (!Hprev || aligned16(Hprev)) &&
                     (op != GS_AGG_MAX || (lda % 4 == 0 && aligned16(argmax))) && (need == 0 || aligned16(ws));
    a.row_ptr = t_row_ptr;
    a.col = t_col;
    a.items = td.items;
    a.slot_ptr = td.slot_ptr;
    a.split_rows = td.split_rows;
    a.cnt = td.count;
    a.w = td.weight;
    a.den = td.denom;
    a.dA = dA;
    a.dSelf = dSelf;
    a.ldd = ldd;
    a.am = argmax;
    a.lda = lda;
    a.Hprev = Hprev;
    a.dH = dH;
    a.ldh = ldh;
    a.part = static_cast<float*>(ws);
    a.seg_len = std::min<int64_t>(tp.seg_len, (int64_t(1) << 31) - 1);
    a.F = static_cast<int>(F);
    a.n_items = static_cast<int>(tp.items.size() / 2);
    a.pos = a.opos = nullptr;
    a.ldo = ldh;
    if (fl) {
        a.items = fl->t_items;
        a.n_items = static_cast<int>(fl->n_t_items);
        a.split_rows = fl->t_split;
        a.n_split = static_cast<int>(fl->n_t_split);
        a.pos = fl->pos;
        a.opos = fl->pos_prev;
        a.ldo = ldo;
    }
    if (op == GS_AGG_MEAN) launch_bwd_t<GS_AGG_MEAN>(vec, a, st);
    else launch_bwd_t<GS_AGG_MAX>(vec, a, st);
    check_launch("gs_agg_full_bwd");
}

}  // namespace gs

extern "C" {

int64_t gs_agg_full_argmax_ws_bytes(const gs_full_plan* plan, int64_t F, int64_t row0, int64_t n_rows) {
    GS_BYTES_BEGIN
    if (!plan) return -1;
    return gs::agg_full_argmax_ws_need(*reinterpret_cast<const gs::FullPlan*>(plan), F, row0, n_rows);
    GS_BYTES_END
}

int gs_agg_full_argmax(const gs_full_plan* plan, const gs_full_plan_dev* dev, gs_dtype dt, const void* X, int64_t ldx,
                       int64_t F, const int64_t* row_ptr, const int32_t* col, int64_t row0, int64_t n_rows, void* out,
                       int64_t ldo, int32_t* argmax, int64_t lda, void* ws, int64_t ws_bytes, void* stream) {
    GS_API_BEGIN
    GS_REQUIRE(plan && dev, GS_EINVAL, "NULL plan");
    gs::agg_full_argmax_launch(*reinterpret_cast<const gs::FullPlan*>(plan), *dev, dt, X, ldx, F, row_ptr, col, row0,
                               n_rows, out, ldo, argmax, lda, ws, ws_bytes, gs::as_stream(stream));
    GS_API_END
}

int64_t gs_agg_full_bwd_ws_bytes(const gs_full_plan* tplan, int64_t F) {
    GS_BYTES_BEGIN
    if (!tplan) return -1;
    return gs::agg_full_bwd_ws_need(*reinterpret_cast<const gs::FullPlan*>(tplan), F);
    GS_BYTES_END
}

int gs_agg_full_bwd(const gs_full_plan* tplan, const gs_full_plan_dev* tdev, gs_agg op, int64_t F,
                    const int64_t* t_row_ptr, const int32_t* t_col, const float* dA, const float* dSelf, int64_t ldd,
                    const int32_t* argmax, int64_t lda, const float* Hprev, float* dH, int64_t ldh, void* ws,
                    int64_t ws_bytes, void* stream) {
    GS_API_BEGIN
    GS_REQUIRE(tplan && tdev, GS_EINVAL, "NULL plan");
    gs::agg_full_bwd_launch(*reinterpret_cast<const gs::FullPlan*>(tplan), *tdev, op, F, t_row_ptr, t_col, dA, dSelf,
                            ldd, argmax, lda, Hprev, dH, ldh, ws, ws_bytes, gs::as_stream(stream));
    GS_API_END
}

int gs_agg_full_field(const gs_full_plan* plan, const gs_full_plan_dev* dev, const gs_full_plan* tplan,
                      const gs_full_field* f, int32_t layer, gs_agg op, gs_dtype dt, const void* X, int64_t ldx,
                      int64_t F, const int64_t* row_ptr, const int32_t* col, void* out, int64_t ldo, int32_t* argmax,
                      int64_t lda, void* ws, int64_t ws_bytes, void* stream) {
    GS_API_BEGIN
    GS_REQUIRE(plan && dev && tplan && f, GS_EINVAL, "NULL argument");
    const gs::FullPlan& p = *reinterpret_cast<const gs::FullPlan*>(plan);
    const gs::FieldLayer fl = gs::field_layer(p, *reinterpret_cast<const gs::FullPlan*>(tplan), *f, layer);
    if (argmax) {
        GS_REQUIRE(op == GS_AGG_MAX, GS_EINVAL, "argmax is recorded for MAX only");
        gs::agg_full_argmax_launch(p, *dev, dt, X, ldx, F, row_ptr, col, 0, p.n, out, ldo, argmax, lda, ws, ws_bytes,
                                   gs::as_stream(stream), &fl);
    } else {
        gs::agg_full_launch(p, *dev, op, dt, X, ldx, F, row_ptr, col, 0, p.n, out, ldo, ws, ws_bytes,
                            gs::as_stream(stream), &fl);
    }
    GS_API_END
}

int gs_agg_full_bwd_field(const gs_full_plan* plan, const gs_full_plan* tplan, const gs_full_plan_dev* tdev,
                          const gs_full_field* f, int32_t layer, gs_agg op, int64_t F, const int64_t* t_row_ptr,
                          const int32_t* t_col, const float* dA, const float* dSelf, int64_t ldd,
                          const int32_t* argmax, int64_t lda, const float* Hprev, int64_t ldh, float* dH, int64_t ldo,
                          void* ws, int64_t ws_bytes, void* stream) {
    GS_API_BEGIN
    GS_REQUIRE(plan && tplan && tdev && f, GS_EINVAL, "NULL argument");
    const gs::FullPlan& tp = *reinterpret_cast<const gs::FullPlan*>(tplan);
    const gs::FieldLayer fl = gs::field_layer(*reinterpret_cast<const gs::FullPlan*>(plan), tp, *f, layer);
    gs::agg_full_bwd_launch(tp, *tdev, op, F, t_row_ptr, t_col, dA, dSelf, ldd, argmax, lda, Hprev, dH,
                            Hprev ? ldh : std::max(ldh, F), ws, ws_bytes, gs::as_stream(stream), &fl, ldo);
    GS_API_END
}

}  // extern "C"
