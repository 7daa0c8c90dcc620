// One full-batch training step over full neighbourhoods: the layer-wise
// forward of infer_full.hip with every A_l and H_l kept (no ping-pong, no row
// chunks: the backward reads them all), the loss head on the rows `nodes`, and
// the backward -- dW_l from [H_{l-1} | A_l], [dSelf | dA] = dH_l W_l, and
// dH_{l-1} from the backward aggregate (agg_full_bwd.hip) with the self-row
// gradient and the relu mask of H_{l-1} folded into its epilogue.  Every
// launch goes to the caller's stream and nothing is allocated: all buffers
// live in the caller's workspace (layout_of).
//
// One driver, train_full_run, runs the step over all N rows and restricted to
// the receptive field of `nodes` (full_field.hip): the checks, the parameter
// offsets, the forward loop, the head and the backward loop are written once,
// and what the restricted step does differently is data (LayerRows) and two
// `if (f)` blocks, described in front of the driver.
//
// Row counts: the weight-gradient launcher cuts N rows into slabs of at most
// 2048 rows (dw_rows_per_split) summed in slab order, its and the
// input-gradient launcher's row offsets are 64-bit and their grids
// ceil(N / 16) x tiles, so both take all N < 2^31 rows in one call; the
// slab workspace is sized here by gs_sage_linear_bwd_weight_ws.
#include "agg_full.hpp"
#include "internal.hpp"

#include <algorithm>

namespace gs {

namespace {

struct TrainLayout {
    int64_t w1lp = -1;
    int64_t a[GS_MAX_HOPS], h[GS_MAX_HOPS], am[GS_MAX_HOPS];  // A_l, H_l, argmax_l at index l - 1
    int64_t dh[2] = {0, 0}, dself = -1, da = 0, e = 0, de = 0, cls = 0, slab = 0, part = 0;
    int64_t slab_bytes = 0, part_bytes = 0, cls_bytes = 0, total = 0;
};

int64_t in_width(const gs_train_full_config& c, int l) {  // one concat half of layer l's input
    return l == 1 ? c.feat_dim : c.hidden;
}

void check_config(const FullPlan& p, const FullPlan& tp, const gs_train_full_config& c) {
    GS_REQUIRE(c.n_layers >= 1 && c.n_layers <= GS_MAX_HOPS, GS_EINVAL, "1 to 8 layers");
    GS_REQUIRE(c.hidden >= 16 && c.hidden <= 256 && c.hidden % 16 == 0, GS_EINVAL,
               "hidden must be a multiple of 16 in [16, 256]");
    GS_REQUIRE(c.agg == GS_AGG_MEAN || c.agg == GS_AGG_MAX, GS_EINVAL, "agg_func must be MEAN or MAX");
    GS_REQUIRE(c.feat_dtype == GS_F32 || c.feat_dtype == GS_BF16, GS_EINVAL, "dtype must be f32 or bf16");
    GS_REQUIRE(c.feat_dim >= 1 && c.feat_dim < (1 << 28) && c.feat_ld >= c.feat_dim, GS_EINVAL, "bad feature shape");
    GS_REQUIRE(c.n_classes >= 1 && c.n_classes + c.hidden < 16384, GS_EINVAL, "bad class count");
    GS_REQUIRE(c.head == 0 || c.head == 1, GS_EINVAL, "head: 0 = NLL, 1 = multi-label");
    GS_REQUIRE(c.head == 0 || gs_cls_bce_supported(c.hidden, c.n_classes), GS_EINVAL,
               "hidden and n_classes too large for the multi-label head (gs_cls_bce_supported)");
    GS_REQUIRE(p.n >= 1, GS_EINVAL, "empty graph");
    GS_REQUIRE(!p.transposed && tp.transposed && tp.n == p.n && tp.gcn == p.gcn, GS_EINVAL,
               "tplan must be the forward plan's transpose");
    GS_REQUIRE(c.max_nodes >= 1 && c.max_nodes <= p.n, GS_EINVAL, "max_nodes outside [1, n_nodes]");
}

TrainLayout layout_of(const FullPlan& p, const FullPlan& tp, const gs_train_full_config& c) {
    check_config(p, tp, c);
    TrainLayout lo;
    const int64_t n = p.n, H = c.hidden, F = c.feat_dim, L = c.n_layers;
    const int64_t es = c.feat_dtype == GS_BF16 ? 2 : 4;
    const int64_t m = p.gcn ? 1 : 2;
    int64_t off = 0;
    auto take = [&](int64_t bytes) {
        const int64_t at = off;
        off += round_up(bytes);
        return at;
    };
    if (c.feat_dtype == GS_BF16) lo.w1lp = take(H * m * F * 2);
    for (int l = 1; l <= L; ++l) {
        lo.a[l - 1] = take(n * (l == 1 ? F * es : H * 4));
        lo.h[l - 1] = take(n * H * 4);
        lo.am[l - 1] = (c.agg == GS_AGG_MAX && l >= 2) ? take(n * H * 4) : -1;
    }
    lo.dh[0] = take(n * H * 4);
    if (L >= 2) {
        lo.dh[1] = take(n * H * 4);
        if (!p.gcn) lo.dself = take(n * H * 4);
        lo.da = take(n * H * 4);
    }
    lo.e = take(c.max_nodes * H * 4);
    lo.de = take(c.max_nodes * H * 4);
    lo.cls_bytes = gs_cls_nll_ws_floats(c.max_nodes, H, c.n_classes) * 4;
    if (c.head == 1) lo.cls_bytes = std::max(lo.cls_bytes, gs_cls_bce_ws_bytes(c.max_nodes, H, c.n_classes));
    lo.cls = take(lo.cls_bytes);
    for (int l = 1; l <= L; ++l)
        lo.slab_bytes = std::max(lo.slab_bytes, gs_sage_linear_bwd_weight_ws(n, m * in_width(c, l), H));
    lo.slab = take(lo.slab_bytes);
    const int64_t fslots = p.slot_ptr[n], tslots = tp.slot_ptr[n];
    lo.part_bytes = std::max(fslots * std::max(F, L >= 2 ? H : int64_t(0)) * 4 * (c.agg == GS_AGG_MAX ? 2 : 1),
                             L >= 2 ? tslots * H * 4 : int64_t(0));
    lo.part = take(lo.part_bytes);
    lo.total = off;
    return lo;
}

// E[i] = Hs[nodes[i]] (scatter: Hs[nodes[i]] = E[i]); H % 4 == 0, 16-byte aligned rows.
template <bool SCATTER>
__global__ __launch_bounds__(256) void rows_by_id_kernel(float* __restrict__ Hs, float* __restrict__ E,
                                                         const int* __restrict__ nodes, int64_t B, int q) {
    const int64_t t = blockIdx.x * int64_t(256) + threadIdx.x;
    if (t >= B * q) return;
    const int64_t i = t / q;
    const int c = static_cast<int>(t % q);
    float4* hs = reinterpret_cast<float4*>(Hs) + static_cast<int64_t>(nodes[i]) * q + c;
    float4* e = reinterpret_cast<float4*>(E) + t;
    if (SCATTER) *hs = *e;
    else *e = *hs;
}

// D[map[nodes[i]]] = E[i]: the loss head's rows into the compact dH_L (map: the field's pos_L).
__global__ __launch_bounds__(256) void rows_by_map_kernel(float* __restrict__ D, const float* __restrict__ E,
                                                          const int* __restrict__ nodes, const int* __restrict__ map,
                                                          int64_t B, int q) {
    const int64_t t = blockIdx.x * int64_t(256) + threadIdx.x;
    if (t >= B * q) return;
    const int64_t i = t / q;
    const int c = static_cast<int>(t % q);
    const int r = map[nodes[i]];
    if (r < 0) return;  // not a root of this field: refused on the host before any launch
    reinterpret_cast<float4*>(D)[static_cast<int64_t>(r) * q + c] = reinterpret_cast<const float4*>(E)[t];
}

// The unsupervised head's last launch: dZ_L[target(i)] = E[i] > 0 ? dSup[i] + dNet[i] : 0 with target(i) =
// nodes[i], or map[nodes[i]] (the field's pos_L, compact dH_L); dSup NULL: no supervised term.  Thread 0 also
// folds the loss parts: loss[1] (the NLL mean, 0 without dSup) + loss[2] (the pair loss) -> loss[0].
__global__ __launch_bounds__(256) void head_combine_kernel(float* __restrict__ D, const float* __restrict__ E,
                                                           const float* __restrict__ dSup,
                                                           const float* __restrict__ dNet,
                                                           const int* __restrict__ nodes, const int* __restrict__ map,
                                                           int64_t B, int q, float* __restrict__ loss) {
    const int64_t t = blockIdx.x * int64_t(256) + threadIdx.x;
    if (t == 0) {
        const float sup = dSup ? loss[1] : 0.f;
        loss[1] = sup;
        loss[0] = dSup ? sup + loss[2] : loss[2];
    }
    if (t >= B * q) return;
    const int64_t i = t / q;
    const int c = static_cast<int>(t % q);
    const int r = map ? map[nodes[i]] : nodes[i];
    if (r < 0) return;  // not a root of this field: refused on the host before any launch
    const float4 e = reinterpret_cast<const float4*>(E)[t];
    float4 g = reinterpret_cast<const float4*>(dNet)[t];
    if (dSup) {  // sup first, then net
        const float4 s = reinterpret_cast<const float4*>(dSup)[t];
        g = make_float4(s.x + g.x, s.y + g.y, s.z + g.z, s.w + g.w);
    }
    g = make_float4(e.x > 0.f ? g.x : 0.f, e.y > 0.f ? g.y : 0.f, e.z > 0.f ? g.z : 0.f, e.w > 0.f ? g.w : 0.f);
    reinterpret_cast<float4*>(D)[static_cast<int64_t>(r) * q + c] = g;
}

// The supervised head over the B gathered rows E (dense [B, H]): the NLL of one class per node, or under
// c.head == 1 the multi-label BCE over the packed targets; dE comes back masked by relu'(E).
void sup_head_launch(const gs_train_full_config& c, const TrainLayout& lo, int64_t B, const float* E,
                     int64_t wc_off, int64_t bc_off, const int32_t* nodes, float* loss, float* dE, char* base,
                     hipStream_t st) {
    const int64_t H = c.hidden, C = c.n_classes;
    if (c.head == 1)
        ok(gs_cls_bce_fwd_bwd(B, H, C, E, H, c.params + wc_off, c.params + bc_off, c.labels, nodes, c.pos_weight, 1,
                              loss, dE, c.grads + wc_off, c.grads + bc_off, base + lo.cls, lo.cls_bytes, st));
    else
        ok(gs_cls_nll_fwd_bwd(B, H, C, E, c.params + wc_off, c.params + bc_off, c.labels, nodes, 1, loss, dE,
                              c.grads + wc_off, c.grads + bc_off, reinterpret_cast<float*>(base + lo.cls), st));
}

// The caller's buffer of the unsupervised head: the loss kernels' per-pair state, dE of the pair loss and the
// constant 1.0 that gs_unsup_loss_bwd reads as dloss.
struct UnsupLayout {
    int64_t pairs = 0, de = 0, one = 0, total = 0;
};

UnsupLayout unsup_layout_of(int64_t H, int64_t U, int64_t M, int64_t P, int64_t N) {
    UnsupLayout lo;
    lo.pairs = 0;
    lo.de = round_up(gs_unsup_loss_ws_floats(M, P, N) * 4);
    lo.one = lo.de + round_up(U * H * 4);
    lo.total = lo.one + round_up(4);
    return lo;
}

bool unsup_dims_ok(int64_t H, int64_t U, int64_t M, int64_t P, int64_t N) {
    const int64_t cap = int64_t(1) << 30;
    return H >= 16 && H <= 256 && H % 16 == 0 && U >= 1 && U < cap && M >= 1 && M < cap && P >= M && P < cap &&
           N >= M && N < cap;
}

// The rows layer l computes: all N, or R_l of a field.
struct LayerRows {
    int64_t n = 0;                   // N, or n_l
    const int* sidx = nullptr;       // the GEMMs' self rows: NULL (row i is node i), or R_l
    const FieldLayer* fl = nullptr;  // what the aggregates take: NULL, or the field's layer
};

// The step over all N rows (f NULL), or restricted to the receptive field f of `nodes`.  Restricted, the H_l tables
// stay N-row and indexed by global id, so col and the gather loop are unchanged: layer l scatters its n_l output
// rows into H_l and reads H_{l-1} on R_{l-1}, which layer l - 1 wrote.  A_l, argmax_l, dSelf and dA are compact in
// R_l order, and so is dH_l (unlike H_l: the GEMMs read dZ_l as n_l consecutive rows, the workspace has no spare
// [n_l, H] buffer to gather them into when L == 1, and the backward aggregate can write row pos_{l-1}[u] as
// cheaply as row u).  The forward GEMM's compact output waits in dH's first buffer, which is free until the head.
// No restricted launch works on N x width: no memset of dH_L (the head's rows are R_L, each written in full), and
// the restricted backward writes every row of R_{l-1}.  Every refusal names the path the caller took.
//
// u (nullable) swaps the head: the pair loss over E (unsup.hip) in place of, or with u->with_sup added to, the NLL
// head, and head_combine_kernel in place of the scatter; `loss` then holds three floats.  The forward and the
// backward stages do not know of it.
void train_full_run(const FullPlan& p, const gs_full_plan_dev& d, const FullPlan& tp, const gs_full_plan_dev& td,
                    const gs_train_full_config& c, const gs_full_field* f, const int32_t* nodes, int64_t B,
                    const gs_train_full_unsup* u, void* uws, int64_t uws_bytes, int reuse_agg1, int stages,
                    float* loss, void* ws, int64_t ws_bytes, hipStream_t st) {
    const TrainLayout lo = layout_of(p, tp, c);
    const int64_t H = c.hidden, L = c.n_layers, C = c.n_classes, m = p.gcn ? 1 : 2;
    auto require = [&](bool cond, const char* msg) {
        const char* who = u ? "train_full_unsup_run: " : f ? "train_full_field_run: " : "train_full_run: ";
        if (!cond) fail(GS_EINVAL, std::string(who) + msg);
    };
    require(c.X && c.row_ptr && c.col && c.t_row_ptr && c.t_col && c.labels && c.params && c.grads && loss,
            "NULL pointer");
    require(nodes && B >= 1 && B <= c.max_nodes, "nodes: 1 to max_nodes ids");
    require(stages >= 1 && stages <= GS_TF_ALL, "bad stages");
    require(ws && ws_bytes >= lo.total && (reinterpret_cast<uintptr_t>(ws) & (kAlign - 1)) == 0,
            "workspace smaller than gs_train_full_ws_bytes or not 256-byte aligned");
    require(aligned16(c.params) && aligned16(c.grads), "params / grads must be 16-byte aligned");
    require(!f || f->n_layers == L, "the field was built for another number of layers");
    require(c.agg != GS_AGG_MAX || (!d.weight && !td.weight), "edge weights go with MEAN, not MAX");
    require(!d.weight == !td.weight && !d.denom == !td.denom,
            "the forward and the transposed plan must carry the same edge-weight set");
    if (!p.empty_rows.empty())
        fail(GS_EEMPTY, "gs_train_full: a node's effective neighbourhood is empty (reference: models.py:313, :321-325)");
    FieldLayer fl[GS_MAX_HOPS + 1];
    LayerRows rows[GS_MAX_HOPS + 1];
    for (int l = 1; l <= L; ++l) {
        if (f) fl[l] = field_layer(p, tp, *f, l);
        rows[l] = f ? LayerRows{fl[l].n, fl[l].rows, &fl[l]} : LayerRows{p.n, nullptr, nullptr};
    }
    require(!f || fl[L].n == B, "the field was built for another set of nodes");
    UnsupLayout ul;
    if (u) {
        require(u->kind == 0 || u->kind == 1, "kind: 0 = sage, 1 = margin");
        require(u->M >= 1 && u->P >= 1 && u->N >= 1, "M, P and N must be at least 1");
        require(unsup_dims_ok(H, B, u->M, u->P, u->N), "bad plan sizes (every scored node owns a pair of each sign)");
        require(u->plan != nullptr, "NULL plan");
        ul = unsup_layout_of(H, B, u->M, u->P, u->N);
        require(uws && uws_bytes >= ul.total && (reinterpret_cast<uintptr_t>(uws) & (kAlign - 1)) == 0,
                "unsup workspace smaller than gs_train_full_unsup_ws_bytes or not 256-byte aligned");
    }
    char* base = static_cast<char*>(ws);
    const gs_agg op = static_cast<gs_agg>(c.agg);
    auto fptr = [&](int64_t o) { return reinterpret_cast<float*>(base + o); };
    // the flat parameter layout: W_1 .. W_L, Wc, bc
    int64_t woff[GS_MAX_HOPS + 1];
    woff[0] = 0;
    for (int l = 1; l <= L; ++l) woff[l] = woff[l - 1] + H * m * in_width(c, l);
    const int64_t wc_off = woff[L], bc_off = wc_off + C * H;
    const int q = static_cast<int>(H / 4);

    if (stages & GS_TF_FORWARD) {
        if (lo.w1lp >= 0) ok(gs_cast_f32_bf16(c.params, base + lo.w1lp, H * m * c.feat_dim, st));
        for (int l = 1; l <= L; ++l) {
            const LayerRows& r = rows[l];
            const gs_dtype dt = l == 1 ? static_cast<gs_dtype>(c.feat_dtype) : GS_F32;
            const char* in = l == 1 ? static_cast<const char*>(c.X) : base + lo.h[l - 2];
            const int64_t ldin = l == 1 ? c.feat_ld : H, fin = in_width(c, l);
            if (lo.am[l - 1] >= 0)
                agg_full_argmax_launch(p, d, dt, in, ldin, fin, c.row_ptr, c.col, 0, p.n, base + lo.a[l - 1], fin,
                                       reinterpret_cast<int32_t*>(base + lo.am[l - 1]), fin, base + lo.part,
                                       lo.part_bytes, st, r.fl);
            else if (l > 1 || !reuse_agg1)
                agg_full_launch(p, d, op, dt, in, ldin, fin, c.row_ptr, c.col, 0, p.n, base + lo.a[l - 1], fin,
                                base + lo.part, lo.part_bytes, st, r.fl);
            const void* W = (l == 1 && lo.w1lp >= 0) ? static_cast<const void*>(base + lo.w1lp)
                                                     : static_cast<const void*>(c.params + woff[l - 1]);
            // straight into H_l, or the compact rows into dH's first buffer and from there to their rows of H_l
            float* hl = fptr(lo.h[l - 1]);
            float* out = f ? fptr(lo.dh[0]) : hl;
            linear_fwd_launch(dt, r.n, fin, H, p.gcn ? nullptr : in, ldin, r.sidx, base + lo.a[l - 1], fin, W, out, H,
                              1, st);
            if (f) {
                rows_by_id_kernel<true><<<dim3(static_cast<unsigned>((r.n * q + 255) / 256)), 256, 0, st>>>(
                    hl, out, r.sidx, r.n, q);
                check_launch("gs_train_full_field(scatter H)");
            }
        }
    }
    float* dh_top = fptr(lo.dh[(L - 1) % 2]);
    if ((stages & GS_TF_HEAD) && u) {
        const unsigned grid = static_cast<unsigned>((B * q + 255) / 256);
        char* ub = static_cast<char*>(uws);
        float* pairs = reinterpret_cast<float*>(ub + ul.pairs);
        float* de_net = reinterpret_cast<float*>(ub + ul.de);
        float* one = reinterpret_cast<float*>(ub + ul.one);
        rows_by_id_kernel<false><<<dim3(grid), 256, 0, st>>>(fptr(lo.h[L - 1]), fptr(lo.e), nodes, B, q);
        check_launch("gs_train_full_unsup(gather)");
        GS_REQUIRE(hipMemsetD32Async(one, 0x3f800000, 1, st) == hipSuccess, GS_EHIP, "memset failed");  // 1.0f
        ok(gs_unsup_loss_fwd(u->kind, u->M, u->P, u->N, B, H, fptr(lo.e), H, u->plan, u->q, u->margin, loss + 2,
                             pairs, st));
        ok(gs_unsup_loss_bwd(u->M, u->P, u->N, B, H, fptr(lo.e), H, u->plan, pairs, one, de_net, H, st));
        if (u->with_sup)  // loss_sup over the whole extended batch, dE masked by relu'(H_L)
            sup_head_launch(c, lo, B, fptr(lo.e), wc_off, bc_off, nodes, loss + 1, fptr(lo.de), base, st);
        else  // the classifier takes no part in this loss
            GS_REQUIRE(hipMemsetAsync(c.grads + wc_off, 0, (C * H + C) * 4, st) == hipSuccess, GS_EHIP,
                       "memset failed");
        if (!f) GS_REQUIRE(hipMemsetAsync(dh_top, 0, p.n * H * 4, st) == hipSuccess, GS_EHIP, "memset failed");
        head_combine_kernel<<<dim3(grid), 256, 0, st>>>(dh_top, fptr(lo.e), u->with_sup ? fptr(lo.de) : nullptr,
                                                        de_net, nodes, f ? fl[L].pos : nullptr, B, q, loss);
        check_launch("gs_train_full_unsup(head combine)");
    } else if (stages & GS_TF_HEAD) {
        const unsigned grid = static_cast<unsigned>((B * q + 255) / 256);
        rows_by_id_kernel<false><<<dim3(grid), 256, 0, st>>>(fptr(lo.h[L - 1]), fptr(lo.e), nodes, B, q);
        check_launch(f ? "gs_train_full_field(gather)" : "gs_train_full(gather)");
        // dE masked by relu'(H_L): the rows of dZ_L, every other row of it zero
        sup_head_launch(c, lo, B, fptr(lo.e), wc_off, bc_off, nodes, loss, fptr(lo.de), base, st);
        if (f) {  // dZ_L, compact: R_L is `nodes`, so every one of its n_L rows is written
            rows_by_map_kernel<<<dim3(grid), 256, 0, st>>>(dh_top, fptr(lo.de), nodes, fl[L].pos, B, q);
            check_launch("gs_train_full_field(scatter dE)");
        } else {
            GS_REQUIRE(hipMemsetAsync(dh_top, 0, p.n * H * 4, st) == hipSuccess, GS_EHIP, "memset failed");
            rows_by_id_kernel<true><<<dim3(grid), 256, 0, st>>>(dh_top, fptr(lo.de), nodes, B, q);
            check_launch("gs_train_full(scatter)");
        }
    }
    if (stages & GS_TF_BACKWARD) {
        for (int l = static_cast<int>(L); l >= 1; --l) {
            const LayerRows& r = rows[l];
            const gs_dtype dt = l == 1 ? static_cast<gs_dtype>(c.feat_dtype) : GS_F32;
            const char* in = l == 1 ? static_cast<const char*>(c.X) : base + lo.h[l - 2];
            const int64_t ldin = l == 1 ? c.feat_ld : H, fin = in_width(c, l);
            const float* dz = fptr(lo.dh[(l - 1) % 2]);  // dH_l on the layer's rows, already masked by relu'(H_l)
            float* dW = c.grads + woff[l - 1];
            // gs_sage_linear_bwd_weight's two launches: row slabs, then their sum in slab order
            const int S = linear_dw_slabs(dt, r.n, fin, H, p.gcn ? nullptr : in, ldin, r.sidx, base + lo.a[l - 1], fin,
                                          dz, nullptr, H, 0, dW, base + lo.slab, lo.slab_bytes, st, -1,
                                          r.n >= 512 ? kDw1Phases : 1);
            if (S > 1) sum_slabs_launch(fptr(lo.slab), S, H * m * fin, dW, nullptr, st);
            if (l == 1) break;  // the feature table has no gradient
            float* dself = p.gcn ? nullptr : fptr(lo.dself);
            ok(gs_sage_linear_bwd_input(r.n, H, H, dz, nullptr, H, 0, c.params + woff[l - 1], dself, fptr(lo.da), H,
                                        st));
            agg_full_bwd_launch(tp, td, op, H, c.t_row_ptr, c.t_col, fptr(lo.da), dself, H,
                                lo.am[l - 1] >= 0 ? reinterpret_cast<const int32_t*>(base + lo.am[l - 1]) : nullptr, H,
                                fptr(lo.h[l - 2]), fptr(lo.dh[(l - 2) % 2]), H, base + lo.part, lo.part_bytes, st,
                                r.fl, H);
        }
    }
}

}  // namespace

}  // namespace gs

extern "C" {

int gs_train_full_field_forward_backward(const gs_full_plan* plan, const gs_full_plan_dev* dev,
                                         const gs_full_plan* tplan, const gs_full_plan_dev* tdev,
                                         const gs_train_full_config* cfg, const gs_full_field* f,
                                         const int32_t* nodes, int64_t n_nodes, int32_t reuse_agg1, int32_t stages,
                                         float* loss, void* ws, int64_t ws_bytes, void* stream) {
    GS_API_BEGIN
    GS_REQUIRE(plan && dev && tplan && tdev && cfg && f, GS_EINVAL, "NULL argument");
    gs::train_full_run(*reinterpret_cast<const gs::FullPlan*>(plan), *dev,
                       *reinterpret_cast<const gs::FullPlan*>(tplan), *tdev, *cfg, f, nodes, n_nodes, nullptr, nullptr,
                       0, reuse_agg1, stages, loss, ws, ws_bytes, gs::as_stream(stream));
    GS_API_END
}

int64_t gs_train_full_ws_bytes(const gs_full_plan* plan, const gs_full_plan* tplan, const gs_train_full_config* cfg) {
    GS_BYTES_BEGIN
    if (!plan || !tplan || !cfg) return -1;
    return gs::layout_of(*reinterpret_cast<const gs::FullPlan*>(plan),
                         *reinterpret_cast<const gs::FullPlan*>(tplan), *cfg).total;
    GS_BYTES_END
}

int64_t gs_train_full_ws_offset(const gs_full_plan* plan, const gs_full_plan* tplan, const gs_train_full_config* cfg,
                                int32_t which, int32_t layer) {
    GS_BYTES_BEGIN
    if (!plan || !tplan || !cfg || layer < 1 || layer > cfg->n_layers || which < 0 || which > 2) return -1;
    const gs::TrainLayout lo = gs::layout_of(*reinterpret_cast<const gs::FullPlan*>(plan),
                                             *reinterpret_cast<const gs::FullPlan*>(tplan), *cfg);
    return which == 0 ? lo.h[layer - 1] : which == 1 ? lo.a[layer - 1] : lo.dh[(layer - 1) % 2];
    GS_BYTES_END
}

int gs_train_full_forward_backward(const gs_full_plan* plan, const gs_full_plan_dev* dev, const gs_full_plan* tplan,
                                   const gs_full_plan_dev* tdev, const gs_train_full_config* cfg, const int32_t* nodes,
                                   int64_t n_nodes, int32_t reuse_agg1, int32_t stages, float* loss, void* ws,
                                   int64_t ws_bytes, void* stream) {
    GS_API_BEGIN
    GS_REQUIRE(plan && dev && tplan && tdev && cfg, GS_EINVAL, "NULL argument");
    gs::train_full_run(*reinterpret_cast<const gs::FullPlan*>(plan), *dev,
                       *reinterpret_cast<const gs::FullPlan*>(tplan), *tdev, *cfg, nullptr, nodes, n_nodes, nullptr,
                       nullptr, 0, reuse_agg1, stages, loss, ws, ws_bytes, gs::as_stream(stream));
    GS_API_END
}

int64_t gs_train_full_unsup_ws_bytes(int32_t hidden, int64_t n_nodes, int64_t M, int64_t P, int64_t N) {
    GS_BYTES_BEGIN
    if (!gs::unsup_dims_ok(hidden, n_nodes, M, P, N)) return -1;
    return gs::unsup_layout_of(hidden, n_nodes, M, P, N).total;
    GS_BYTES_END
}

int gs_train_full_unsup_forward_backward(const gs_full_plan* plan, const gs_full_plan_dev* dev,
                                         const gs_full_plan* tplan, const gs_full_plan_dev* tdev,
                                         const gs_train_full_config* cfg, const gs_full_field* f,
                                         const int32_t* nodes, int64_t n_nodes, const gs_train_full_unsup* u,
                                         void* uws, int64_t uws_bytes, int32_t reuse_agg1, int32_t stages,
                                         float* loss, void* ws, int64_t ws_bytes, void* stream) {
    GS_API_BEGIN
    GS_REQUIRE(plan && dev && tplan && tdev && cfg && u, GS_EINVAL, "NULL argument");
    gs::train_full_run(*reinterpret_cast<const gs::FullPlan*>(plan), *dev,
                       *reinterpret_cast<const gs::FullPlan*>(tplan), *tdev, *cfg, f, nodes, n_nodes, u, uws,
                       uws_bytes, reuse_agg1, stages, loss, ws, ws_bytes, gs::as_stream(stream));
    GS_API_END
}

}  // extern "C"
