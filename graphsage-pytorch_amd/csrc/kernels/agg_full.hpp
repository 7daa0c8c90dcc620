#pragma once
// Internal launcher of the full-neighbourhood aggregate (agg_full.hip), shared
// with the layer-wise driver (infer_full.hip).  Throws gs::Error.
#include "../host/full_plan.hpp"
#include "agg_dev.hpp"
#include "full_field.hpp"
#include "kcommon.hpp"

#include <type_traits>

namespace gs {

// Every offset into a layer-wise driver's workspace (infer_full.hip, train_full.hip) is a multiple of kAlign.
constexpr int64_t kAlign = 256;
inline int64_t round_up(int64_t b) { return (b + kAlign - 1) / kAlign * kAlign; }

// fp32 partial rows of a split row's segments, and the kernels' arguments (agg_full.hip, agg_full_bwd.hip)
template <int VEC>
__device__ __forceinline__ void part_store(float* p, const float (&v)[VEC]) {
    if constexpr (VEC == 1) {
        *p = v[0];
    } else {
#pragma unroll
        for (int q = 0; q < VEC / 4; ++q)
            reinterpret_cast<float4*>(p)[q] = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
    }
}

template <int VEC>
__device__ __forceinline__ void part_load(const float* p, float (&v)[VEC]) {
    if constexpr (VEC == 1) {
        v[0] = *p;
    } else {
#pragma unroll
        for (int q = 0; q < VEC / 4; ++q) {
            const float4 t = reinterpret_cast<const float4*>(p)[q];
            v[4 * q] = t.x; v[4 * q + 1] = t.y; v[4 * q + 2] = t.z; v[4 * q + 3] = t.w;
        }
    }
}

struct FullArgs {
    int64_t ldx, ldo;
    const int64_t* row_ptr;
    const int* col;
    const int* items;       // the window's first item
    const int64_t* slot_ptr;
    const int* split_rows;  // the window's first split row
    const int* cnt;
    const uint8_t* self_loop;
    const int* pos;         // MAP kernels: the output row of a node (a field's pos_l); NULL otherwise
    const float* w;         // WT kernels: a weight per CSR entry (NULL: the unweighted kernels run)
    const float* den;       // WT kernels: the weighted mean's divisor per row; NULL: the weighted sum
    const float* sw;        // WT kernels: the weight of gcn's appended self row; NULL: 1
    float* part;
    int64_t slot0;          // slot_ptr[row0]: the window's partials start at part[0]
    int64_t seg_len;        // clamped to 2^31 - 1
    int F, n_items, n_split, row0, gcn;
};

// The arguments of the window [row0, row0 + n_rows), n_rows > 0, or of a field's rows (`fl`, below), after the
// checks both forward launchers share: the window, the field, the plan's and the CSR's pointers, the split rows.
FullArgs full_args(const FullPlan& p, const gs_full_plan_dev& d, const int64_t* row_ptr, const int32_t* col,
                   int64_t row0, int64_t n_rows, int64_t F, int64_t ldx, int64_t ldo, void* ws, const FieldLayer* fl);

// fn(VEC, G) as integral constants: one element per lane and 64 lanes unless `vec`, else V elements per lane and
// pick_group's 16, 32 or 64 lanes for a row of F.
template <int V, typename Fn>
void with_group(bool vec, int F, Fn fn) {
    using std::integral_constant;
    if (!vec) return fn(integral_constant<int, 1>{}, integral_constant<int, 64>{});
    const int G = pick_group(F, V);
    if (G == 16) fn(integral_constant<int, V>{}, integral_constant<int, 16>{});
    else if (G == 32) fn(integral_constant<int, V>{}, integral_constant<int, 32>{});
    else fn(integral_constant<int, V>{}, integral_constant<int, 64>{});
}

// An aggregate's two launches: the walk, one lane group of G per item, then the combine, one per split row; either
// is skipped when it has nothing to do.  `map`: a field's rows -- the same walk and combine, the MAP pair.
template <int G, typename Walk, typename Combine, typename... Args>
void launch_walk_combine(bool map, int n_items, int n_split, hipStream_t st, Walk walk_map, Combine combine_map,
                         Walk walk, Combine combine, const Args&... args) {
    constexpr int per = kBlock / G;
    if (map) {
        walk = walk_map;
        combine = combine_map;
    }
    if (n_items > 0) walk<<<dim3((n_items + per - 1) / per), kBlock, 0, st>>>(args...);
    if (n_split > 0) combine<<<dim3((n_split + per - 1) / per), kBlock, 0, st>>>(args...);
}

// Bytes of fp32 partials the window [row0, row0 + n_rows) needs at width F.
int64_t agg_full_ws_need(const FullPlan& p, int64_t F, int64_t row0, int64_t n_rows);
// gs_agg_full (its argument checks included; every check before the first launch).
void agg_full_launch(const FullPlan& p, const gs_full_plan_dev& d, gs_agg op, gs_dtype dt, const void* X, int64_t ldx,
                     int64_t F, const int64_t* row_ptr, const int32_t* col, int64_t row0, int64_t n_rows, void* out,
                     int64_t ldo, void* ws, int64_t ws_bytes, hipStream_t st, const FieldLayer* fl = nullptr);
// `fl` (both forward launchers, row0 = 0 and n_rows = n): the field's items and split rows of R_l instead of
// the plan's, row v written to row fl->pos[v] of a compact out (and argmax).
// gs_agg_full_argmax / gs_agg_full_bwd (agg_full_bwd.hip; every check before the first launch)
int64_t agg_full_argmax_ws_need(const FullPlan& p, int64_t F, int64_t row0, int64_t n_rows);
void agg_full_argmax_launch(const FullPlan& p, const gs_full_plan_dev& d, gs_dtype dt, const void* X, int64_t ldx,
                            int64_t F, const int64_t* row_ptr, const int32_t* col, int64_t row0, int64_t n_rows,
                            void* out, int64_t ldo, int32_t* argmax, int64_t lda, void* ws, int64_t ws_bytes,
                            hipStream_t st, const FieldLayer* fl = nullptr);
int64_t agg_full_bwd_ws_need(const FullPlan& tp, int64_t F);
void agg_full_bwd_launch(const FullPlan& tp, const gs_full_plan_dev& td, gs_agg op, int64_t F,
                         const int64_t* t_row_ptr, const int32_t* t_col, const float* dA, const float* dSelf,
                         int64_t ldd, const int32_t* argmax, int64_t lda, const float* Hprev, float* dH, int64_t ldh,
                         void* ws, int64_t ws_bytes, hipStream_t st, const FieldLayer* fl = nullptr, int64_t ldo = 0);
// `fl` (the backward): the transposed items and split rows of R_{l-1}; destinations v outside R_l are skipped,
// dA / dSelf / argmax are compact in R_l order, Hprev is the N-row table (row stride ldh) and dH is compact in
// R_{l-1} order with row stride ldo.

}  // namespace gs
