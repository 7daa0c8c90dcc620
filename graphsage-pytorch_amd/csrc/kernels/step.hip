// Native training-step runtime: the reference's per-batch loop body
// (utils.py:157-191 — GraphSage forward, Classification + NLL, backward,
// clip_grad_norm_ per model, SGD) issued as one stream of the kernels in this
// library, with every intermediate carved from one caller-owned workspace.
// The Python host makes two calls per step (forward_backward, update) and
// puts the RCCL gradient all-reduce between them.
#include <algorithm>
#include <memory>
#include <utility>

#include "trainer.hpp"

namespace gs {

// Field f of hop `hop` (1-based) in a packed sample.
static inline const int32_t* pack_field(const int32_t* pack, const int64_t* offsets, int hop, int f) {
    const int64_t o = offsets[(hop - 1) * GS_PK_NFIELDS + f];
    GS_REQUIRE(o >= 0, GS_EINVAL, "pack field missing");
    return pack + o;
}

// The layer-1 gather-aggregate of one packed sample (models.py:291-330 at
// layer 1) into `out`, bracketed by the timing events when armed.
static void gather1(gs_trainer& T, const int32_t* pack, const int64_t* hop_sizes, const int64_t* offsets,
                    void* out, hipStream_t st, int64_t ldo = 0) {
    const gs_trainer_config& c = T.cfg;
    const int L = c.n_layers;
    const int64_t F = c.feat_dim;
    auto fld = [&](int f) { return pack_field(pack, offsets, L, f); };
    LaunchTimer timed = timed_arm(T, 0);
    agg_fwd_launch(static_cast<gs_agg>(c.agg), static_cast<gs_dtype>(c.feat_dtype), c.X, c.feat_ld, F,
                   hop_sizes[4 * (L - 1)], fld(GS_PK_POS_PTR), fld(GS_PK_POS), nullptr, c.col, fld(GS_PK_DST_IDS),
                   c.gcn, out, static_cast<gs_dtype>(c.feat_dtype), ldo > 0 ? ldo : F, nullptr, st, &timed);
    timed_done(T, 0, timed);
}

// The same aggregate in two launches on `st`: resolve the sampled positions
// into padded neighbour ids, then gather rows through them (the timed launch;
// bitwise the expand-mode result).
static void gather1_ids(gs_trainer& T, const int32_t* pack, const int64_t* hop_sizes, const int64_t* offsets,
                        GatherSlot& g, hipStream_t st) {
    const gs_trainer_config& c = T.cfg;
    const int L = c.n_layers;
    auto fld = [&](int f) { return pack_field(pack, offsets, L, f); };
    const int64_t n_dst = hop_sizes[4 * (L - 1)];
    const int64_t n_top = hop_sizes[0];
    g.top_ready = T.top_k > 0 && L == 2 && !c.gcn && n_top <= T.top_rows && g.top &&
                  hop_sizes[3] <= n_top * T.top_k;  // every root's list fits tk slots
    const int64_t n_rec = hop_sizes[2];  // |L1|: hop 1's sources
    g.rec_ready = g.top_ready && g.rec && n_rec <= T.rec_rows;
    if (g.top_ready) {
        auto f1 = [&](int f) { return pack_field(pack, offsets, 1, f); };
        resolve_top_launch(n_dst, T.k_ids, fld(GS_PK_POS_PTR), fld(GS_PK_POS), c.col, fld(GS_PK_DST_IDS), c.gcn, g.ids,
                           n_top, T.top_k, f1(GS_PK_NBR_PTR), f1(GS_PK_NBR), f1(GS_PK_SELF), g.top, st,
                           g.rec_ready ? n_rec : 0, f1(GS_PK_TPTR), f1(GS_PK_TIDX), g.rec);
    } else {
        resolve_ids_launch(n_dst, T.k_ids, fld(GS_PK_POS_PTR), fld(GS_PK_POS), c.col, fld(GS_PK_DST_IDS), c.gcn, g.ids,
                           st);
    }
    LaunchTimer timed = timed_arm(T, 0);
    if (T.self_rows) {  // [self | agg] rows
        char* base = static_cast<char*>(g.a1);
        const int64_t xsz = c.feat_dtype == GS_BF16 ? 2 : 4;
        agg_ids_launch(static_cast<gs_agg>(c.agg), static_cast<gs_dtype>(c.feat_dtype), c.X, c.feat_ld, c.feat_dim,
                       n_dst, T.k_ids, g.ids, fld(GS_PK_DST_IDS), c.gcn, base + c.feat_dim * xsz, 2 * c.feat_dim, st,
                       base, 2 * c.feat_dim, &timed);
        g.self_in = true;
    } else {
        agg_ids_launch(static_cast<gs_agg>(c.agg), static_cast<gs_dtype>(c.feat_dtype), c.X, c.feat_ld, c.feat_dim,
                       n_dst, T.k_ids, g.ids, fld(GS_PK_DST_IDS), c.gcn, g.a1, c.feat_dim, st, nullptr, 0, &timed);
    }
    timed_done(T, 0, timed);
}

// One step's sizes and its carve of the workspace (layer l at index l - 1).
struct StepPlan {
    int64_t rows[GS_MAX_HOPS], in_dim[GS_MAX_HOPS];  // rows and input width per layer
    void* agg[GS_MAX_HOPS];
    float* h[GS_MAX_HOPS];
    int32_t* am[GS_MAX_HOPS];  // MAX routing of the layers >= 2
    float *demb, *cls_ws, *dIn, *dbuf[2];
    char *dw_ws, *dw2_ws;  // dW row slabs; the fused top path's dW_2 slabs, which outlive the layer-1 dW
    int64_t dw_need, dw2_need, used;  // (used: bytes carved)
};

// The only code that carves the workspace (with ws == nullptr it only sizes).
// With a gather slot the layer-1 aggregate is that slot's; with embed_out
// the last layer writes there.
static StepPlan plan_step(gs_trainer& T, const int64_t* hop_sizes, int64_t B, char* ws, int64_t ws_bytes,
                          const GatherSlot* slot, float* embed_out) {
    const gs_trainer_config& c = T.cfg;
    const int L = c.n_layers;
    const int64_t H = c.hidden, F = c.feat_dim;
    GS_REQUIRE(hop_sizes[0] == B, GS_EINVAL, "roots / hop-1 size mismatch");
    Carve cv{ws, ws_bytes};
    StepPlan p{};
    for (int l = 1; l <= L; ++l) {
        p.rows[l - 1] = hop_sizes[4 * (L - l)];  // hop L - l + 1's destinations
        p.in_dim[l - 1] = l == 1 ? F : H;
        if (l == 1) {
            if (slot) {
                GS_REQUIRE(p.rows[0] <= T.a1_rows && slot->a1, GS_EINVAL, "gather slot too small");
                p.agg[0] = slot->a1;
            } else {
                p.agg[0] = cv.take<char>(p.rows[0] * F * (c.feat_dtype == GS_BF16 ? 2 : 4));
            }
        }
        // layer 2 of a 2-layer step: [self | agg] rows of 2H (the top launch writes
        // them dense, so the layer-2 weight gradient reads no self index)
        else p.agg[l - 1] = cv.take<float>(p.rows[l - 1] * (L == 2 ? 2 * H : H));
        p.h[l - 1] = (embed_out && l == L) ? embed_out : cv.take<float>(p.rows[l - 1] * H);
        if (l >= 2 && c.agg == GS_AGG_MAX) p.am[l - 1] = cv.take<int32_t>(p.rows[l - 1] * H);
    }
    p.demb = cv.take<float>(B * H);
    p.cls_ws = cv.take<float>(gs_cls_nll_ws_floats(B, H, c.n_classes));
    int64_t dx_rows = 0, dprev_rows = 0;
    for (int l = 1; l <= L; ++l) {
        p.dw_need = std::max(p.dw_need, gs_sage_linear_bwd_weight_ws(p.rows[l - 1], T.w_cols[l - 1], H));
        if (l >= 2) {
            dx_rows = std::max(dx_rows, p.rows[l - 1]);
            dprev_rows = std::max(dprev_rows, p.rows[l - 2]);
        }
    }
    p.dw_ws = cv.take<char>(p.dw_need);
    p.dw2_need = L == 2 ? gs_sage_linear_bwd_weight_ws(p.rows[1], T.w_cols[1], H) : 0;
    p.dw2_ws = p.dw2_need > 0 ? cv.take<char>(p.dw2_need) : nullptr;
    p.dIn = cv.take<float>(dx_rows * (c.gcn ? H : 2 * H));
    p.dbuf[0] = cv.take<float>(dprev_rows * H);
    p.dbuf[1] = cv.take<float>(dprev_rows * H);
    p.used = cv.at;
    return p;
}

// The layer-1 GEMMs' operands: X[dst_L] | agg, or the gather slot's dense
// [self | agg] rows (GS_TOPT_SELF_ROWS).
struct Layer1In {
    const void* x1;
    int64_t ldx1;
    const int32_t* sidx1;
    const void* a1;
    int64_t lda1;
};

// One forward + backward over a plan, stage by stage (run_step below).
struct Step {
    gs_trainer& T;
    const int32_t* pack;
    const int64_t* offsets;
    const int32_t* roots;
    int64_t B;
    float* loss;
    hipStream_t st;
    const GatherSlot* slot;  // the gather slot that holds the layer-1 aggregate, or NULL (the step gathers itself)
    const StepPlan p;
    const gs_trainer_config& c = T.cfg;
    const int L = c.n_layers;
    const int64_t H = c.hidden, F = c.feat_dim, K1 = T.w_cols[0];
    float *const P = c.params, *const G = c.grads;
    const gs_dtype dt = static_cast<gs_dtype>(c.feat_dtype);
    Layer1In in{};
    const void* W1 = nullptr;  // as this step's layer-1 forward reads it
    FwdSpec sp;                // the previous step's clip + SGD, when that forward applies it (pend)
    bool pend = false;

    const int32_t* fld(int hop, int f) const { return pack_field(pack, offsets, hop, f); }  // hop 1-based

    void layer1_operands() {
        in = {c.gcn ? nullptr : c.X, c.feat_ld, fld(L, GS_PK_DST_IDS), p.agg[0], F};
        if (slot && T.self_rows) {
            in.a1 = static_cast<const char*>(p.agg[0]) + F * (dt == GS_BF16 ? 2 : 4);
            in.lda1 = 2 * F;
            if (slot->self_in && !c.gcn) {
                in.x1 = p.agg[0];
                in.ldx1 = 2 * F;
                in.sidx1 = nullptr;
            }
        }
    }

    // bf16 features: the forward's bf16 W1 made current (gs_trainer::w1_lp's rules).
    void cast_w1_lowp() {
        if (dt != GS_BF16) return;
        if (T.defer) {  // deferring: lp_buf(w1_cur) is cast once, then kept by the updates
            if (!T.lp_valid && !T.pending) {
                ok(gs_cast_f32_bf16(T.w1_buf(T.w1_cur), T.lp_buf(T.w1_cur), T.w_rows[0] * K1, st));
                T.lp_valid = true;
            }
        } else if (!(T.lp_keep && T.lp_valid)) {
            ok(gs_cast_f32_bf16(P + T.w_off[0], T.w1_lp, T.w_rows[0] * K1, st));
            T.lp_valid = T.lp_keep;
        }
    }

    // A pending update that cannot ride the forward is applied on its own.
    void apply_pending_alone() {
        trainer_defer_update(&T, false, st);
        trainer_defer_update(&T, true, st);
    }

    // W1, sp and pend for this forward.
    void w1_for_forward() {
        const bool lowp = dt == GS_BF16;
        auto buf = [&](int i) { return lowp ? static_cast<const void*>(T.lp_buf(i)) : T.w1_buf(i); };
        W1 = lowp ? static_cast<const void*>(T.w1_lp) : P + T.w_off[0];
        pend = T.defer && T.pending;
        // the forward folds at most 512 partials per group, and only the wide
        // (16-B load) forward applies a pending update
        if (pend && !(T.pend_np[0] >= 1 && T.pend_np[0] <= 512 && T.pend_np[1] >= 1 && T.pend_np[1] <= 512 &&
                      linear_fwd_wide_ok(dt, F, in.x1, in.ldx1, in.a1, in.lda1, buf(T.w1_cur ^ 1)))) {
            apply_pending_alone();
            pend = false;
        }
        if (!T.defer) return;
        W1 = buf(pend ? T.w1_cur ^ 1 : T.w1_cur);
        if (!pend) return;
        sp = pending_spec(T);
        sp.Wn = T.w1_buf(T.w1_cur ^ 1);
        if (lowp) sp.S_lp = sp.Wn_lp = T.lp_buf(T.w1_cur ^ 1);
    }

    void forward_layer1() {  // models.py:255-267 at layer 1
        LaunchTimer timed = timed_arm(T, 1);
        linear_fwd_launch(dt, p.rows[0], F, H, in.x1, in.ldx1, in.sidx1, in.a1, in.lda1, W1, p.h[0], H, 1, st, &sp,
                          &timed);
        timed_done(T, 1, timed);
        if (pend) {  // the launch applied the pending update: W1 is now the other buffer
            T.w1_cur ^= 1;
            T.pending = false;
        }
    }

    void forward_upper() {  // the layers >= 2, where the top launch does not run them
        for (int l = 2; l <= L; ++l) {
            const int j = L - l + 1;
            ok(gs_agg_fwd(static_cast<gs_agg>(c.agg), GS_F32, p.h[l - 2], H, H, p.rows[l - 1], fld(j, GS_PK_NBR_PTR),
                          fld(j, GS_PK_NBR), nullptr, nullptr, nullptr, 0, p.agg[l - 1], GS_F32, H, p.am[l - 1], st));
            ok(gs_sage_linear_fwd(GS_F32, p.rows[l - 1], H, H, c.gcn ? nullptr : p.h[l - 2], H, fld(j, GS_PK_SELF),
                                  p.agg[l - 1], H, P + T.w_off[l - 1], p.h[l - 1], H, 1, st));
        }
    }

    // The fused backward's per-layer arguments, top layer first (L - 1
    // entries); returns whether every layer can take the fused launches.
    bool layer_bwd_args(bool top, LayerBwd* lb) const {
        int flip_f = 0;
        bool fusable = true;
        for (int l = L; l >= 2; --l) {
            const int j = L - l + 1;
            LayerBwd& a = lb[L - l];
            a.n = p.rows[l - 1];
            a.fin = H;
            a.H = H;
            a.Xs = c.gcn ? nullptr : p.h[l - 2];
            a.ldxs = H;
            a.sidx = fld(j, GS_PK_SELF);
            a.A = static_cast<const float*>(p.agg[l - 1]);
            if (top && l == L) {  // the top launch's dense [self | agg] rows: no self index
                a.Xs = static_cast<const float*>(p.agg[l - 1]);
                a.ldxs = 2 * H;
                a.sidx = nullptr;
                a.A = static_cast<const float*>(p.agg[l - 1]) + H;
                a.lda = 2 * H;
            }
            a.dZ = l == L ? p.demb : p.dbuf[flip_f ^ 1];
            a.W = P + T.w_off[l - 1];
            a.dW = G + T.w_off[l - 1];
            a.slabs = reinterpret_cast<float*>(p.dw_ws);
            a.slab_bytes = p.dw_need;
            a.dIn = p.dIn;
            a.agg = c.agg;
            a.n_src = p.rows[l - 2];
            a.tptr = fld(j, GS_PK_TPTR);
            a.tidx = fld(j, GS_PK_TIDX);
            a.ptr = fld(j, GS_PK_NBR_PTR);
            a.argmax = p.am[l - 1];
            a.Hprev = p.h[l - 2];
            a.dH = p.dbuf[flip_f];
            if (top && l == L && slot && slot->rec_ready)  // the side stream's records of hop 1's lists
                a.trec = reinterpret_cast<const int4*>(slot->rec);
            flip_f ^= 1;
            fusable = fusable && layer_bwd_fusable(a);
        }
        return fusable;
    }

    ClsReduce cls_reduce_role(int cls_rows) const {
        return {B, H, c.n_classes, cls_rows, p.cls_ws, G + T.cls_w_off, G + T.cls_b_off, loss, T.norm_part + T.pstride};
    }

    // The layer-1 weight gradient's row slabs from dH (timer site 2); returns their count.
    int dw1_slabs(const float* dH) {
        LaunchTimer timed = timed_arm(T, 2);
        const int S1 = linear_dw_slabs(dt, p.rows[0], F, H, in.x1, in.ldx1, in.sidx1, in.a1, in.lda1, dH, p.h[0], H, 0,
                                       G + T.w_off[0], p.dw_ws, p.dw_need, st, -1, kDw1Phases, &timed);
        timed_done(T, 2, timed);
        return S1;
    }

    // The step's clip-norm partials: np of group 0, the classifier reduce's of group 1.
    void keep_norm_parts(int np, bool parts) {
        T.npart[0] = np;
        T.npart[1] = cls_reduce_grid(c.n_classes, H);
        T.norm_ready = parts && np <= T.pstride && T.npart[1] <= T.pstride;
    }

    // The fused backward (bwd.hip) after the loss head's rows: same kernels and
    // summation order as backward_unfused, two launches per layer >= 2 instead
    // of five, then the layer-1 dW (in chunks for the runner's all-reduce hook).
    void backward_fused(const LayerBwd* lb, int n_lb, const ClsReduce& cr) {
        const float* dws = reinterpret_cast<const float*>(p.dw_ws);
        int np = 0;
        bool parts = true;
        for (int i = 0; i < n_lb; ++i) {
            const int n = layer_bwd(lb[i], i == 0 ? &cr : nullptr, T.norm_part + np, st);
            parts = parts && n > 0;
            np += n;
        }
        if (T.upper_hook) T.upper_hook(st);
        const float* dH1 = lb[n_lb - 1].dH;
        if (T.w1_chunk_hook && T.w1_chunks > 1 && H % (64 * T.w1_chunks) == 0) {
            // dW1 in row chunks, each summed and handed to the hook (its
            // all-reduce then runs under the next chunk's GEMM); the clip
            // of the communicator path recomputes the norm from the
            // reduced gradient, so no norm partials are kept
            const int64_t Hc = H / T.w1_chunks;
            for (int q = 0; q < T.w1_chunks; ++q) {
                const int64_t h0 = q * Hc;
                float* dWq = G + T.w_off[0] + h0 * K1;
                const int Sq = linear_dw_slabs(dt, p.rows[0], F, Hc, in.x1, in.ldx1, in.sidx1, in.a1, in.lda1, dH1 + h0,
                                               p.h[0] + h0, H, 0, dWq, p.dw_ws, p.dw_need, st, H, kDw1Phases);
                if (Sq > 1) sum_slabs_launch(dws, Sq, Hc * K1, dWq, nullptr, st);
                T.w1_chunk_hook(st, T.w_off[0] + h0 * K1, Hc * K1);
            }
            T.npart[0] = 0;
            T.npart[1] = 0;
            T.norm_ready = false;
            return;
        }
        const int S1 = dw1_slabs(dH1);
        if (S1 > 1) np += sum_slabs_launch(dws, S1, H * K1, G + T.w_off[0], T.norm_part + np, st);
        else parts = false;
        keep_norm_parts(np, parts);
    }

    // A 2-layer training step's backward from the top launch (top.hip: layer 2,
    // the loss head and layer 2's dIn in one launch).  Without a bucketed
    // all-reduce hook: one backward launch for layer 2, and its slab sum rides
    // layer 1's (same sums, partials, order) in the pair launch that also
    // writes the deferred update's speculative W1; else backward_fused.
    void backward_top(LayerBwd& lb2) {
        LaunchTimer timed = timed_arm(T, 3);
        const bool tids = slot && slot->top_ready;
        const int cls_rows = top_fwd_bwd(c.agg, B, c.n_classes, p.h[0], fld(1, GS_PK_NBR_PTR), fld(1, GS_PK_NBR),
                                         fld(1, GS_PK_SELF), P + T.w_off[1], P + T.cls_w_off, P + T.cls_b_off, c.labels,
                                         roots, static_cast<float*>(p.agg[1]), p.am[1], p.h[1], p.demb, p.dIn, p.cls_ws,
                                         st, tids ? slot->top : nullptr, tids ? T.top_k : 0, &timed);
        timed_done(T, 3, timed);
        lb2.din_ready = true;
        const ClsReduce cr = cls_reduce_role(cls_rows);
        const bool late_sum2 = !T.upper_hook && p.dw2_ws && sum_slabs_pair_ok(H * K1, H * T.w_cols[1]);
        if (!late_sum2) return backward_fused(&lb2, 1, cr);
        lb2.slabs = reinterpret_cast<float*>(p.dw2_ws);
        lb2.slab_bytes = p.dw2_need;
        SlabSum d2{};
        int np = layer_bwd_top(lb2, cr, &d2, st);
        bool parts = np > 0;
        const int S1 = dw1_slabs(lb2.dH);
        const int n_cls = cls_reduce_grid(c.n_classes, H);
        if (S1 > 1) {
            d2.part = T.norm_part;
            // deferred update: this launch also writes W1's update for clip
            // coefficient 1 (and carries the done flag); the clip + SGD
            // itself is left to the next forward
            const bool spec = T.defer && !T.defer_comm && parts && np + sum_slabs_grid(H * K1) <= T.pstride &&
                              n_cls <= T.pstride;
            LaunchTimer timed4 = timed_arm(T, 4);
            const SlabSum s1{reinterpret_cast<const float*>(p.dw_ws), S1, H * K1, G + T.w_off[0], T.norm_part + np};
            np += sum_slabs_pair_launch(s1, d2, st, spec ? T.w1_buf(T.w1_cur) : nullptr,
                                        spec ? T.w1_buf(T.w1_cur ^ 1) : nullptr, c.lr,
                                        spec && dt == GS_BF16 ? T.lp_buf(T.w1_cur ^ 1) : nullptr,
                                        spec ? T.take_done() : DoneFlag{}, &timed4);
            timed_done(T, 4, timed4);
            T.pending = spec;
            if (spec) {
                T.pend_part = T.norm_part;
                T.pend_pstride = T.pstride;
                T.pend_np[0] = np;
                T.pend_np[1] = n_cls;
                T.pend_scale = 1.f;
            }
        } else {
            if (d2.S > 1) sum_slabs_launch(d2.slabs, d2.S, d2.len, d2.out, nullptr, st);
            parts = false;
        }
        keep_norm_parts(np, parts);
    }

    // The unfused sequence: the loss head (models.py:8-27, utils.py:159-164;
    // labels gathered through the roots, demb comes back already masked by
    // relu'(h_L), i.e. dZ_L), then the backward (utils.py:184) layer by layer.
    void backward_unfused() {
        ok(gs_cls_nll_fwd_bwd(B, H, c.n_classes, p.h[L - 1], P + T.cls_w_off, P + T.cls_b_off, c.labels, roots, 1, loss,
                              p.demb, G + T.cls_w_off, G + T.cls_b_off, p.cls_ws, st));
        const float* dH = p.demb;
        const int relu = 0;  // every dH below is pre-masked
        int flip = 0;
        for (int l = L; l >= 1; --l) {
            const int j = L - l + 1;
            const bool first = l == 1;
            const void* x_in = first ? in.x1 : (c.gcn ? nullptr : p.h[l - 2]);
            const int32_t* sidx = first ? in.sidx1 : fld(j, GS_PK_SELF);
            const int64_t fin = p.in_dim[l - 1], ldx = first ? in.ldx1 : H;
            if (first && L >= 2 && T.upper_hook) T.upper_hook(st);
            {  // the fused path's slabs: layer 1 in kDw1Phases row phases, layers >= 2 in one
                const int64_t Kl = x_in ? 2 * fin : fin;
                const int Sl = linear_dw_slabs(first ? dt : GS_F32, p.rows[l - 1], fin, H, x_in, ldx, sidx,
                                               first ? in.a1 : p.agg[l - 1], first ? in.lda1 : fin, dH, p.h[l - 1], H,
                                               relu, G + T.w_off[l - 1], p.dw_ws, p.dw_need, st, -1,
                                               first ? kDw1Phases : 1);
                if (Sl > 1) sum_slabs_launch(reinterpret_cast<const float*>(p.dw_ws), Sl, H * Kl, G + T.w_off[l - 1],
                                             nullptr, st);
            }
            if (first) break;
            const int64_t ldd = c.gcn ? H : 2 * H;
            float* dSelf = c.gcn ? nullptr : p.dIn;
            float* dA = c.gcn ? p.dIn : p.dIn + H;
            ok(gs_sage_linear_bwd_input(p.rows[l - 1], H, H, dH, p.h[l - 1], H, relu, P + T.w_off[l - 1], dSelf, dA,
                                        ldd, st));
            float* dprev = p.dbuf[flip];
            flip ^= 1;
            ok(gs_agg_bwd(static_cast<gs_agg>(c.agg), p.rows[l - 2], H, fld(j, GS_PK_TPTR), fld(j, GS_PK_TIDX),
                          fld(j, GS_PK_NBR_PTR), dA, dSelf, ldd, p.am[l - 1], p.h[l - 2], H, dprev, st));
            dH = dprev;  // agg_bwd masks by relu'(h_{l-1})
        }
    }
};

// Runs (or, with ws == nullptr, only sizes) one forward + backward.  With
// a1_slot >= 0 the layer-1 aggregate was produced by gs_trainer_gather.  With
// embed_out the step is the forward alone (models.py:241-269 as called by
// get_gnn_embeddings, utils.py:59-78): the last layer writes its [B, H]
// embeddings straight into embed_out and nothing after the forward runs.
static int64_t run_step(gs_trainer& T, const int32_t* pack, const int64_t* hop_sizes, const int64_t* offsets,
                        const int32_t* roots, int64_t B, char* ws, int64_t ws_bytes, float* loss, hipStream_t st,
                        int a1_slot = -1, float* embed_out = nullptr) {
    const GatherSlot* slot = a1_slot >= 0 ? &T.slot[a1_slot] : nullptr;
    Step s{T, pack, offsets, roots, B, loss, st, slot, plan_step(T, hop_sizes, B, ws, ws_bytes, slot, embed_out)};
    const StepPlan& p = s.p;
    const int L = s.L;
    T.last_emb = p.h[L - 1];
    if (!ws) return p.used + 256;
    GS_REQUIRE(p.used <= ws_bytes, GS_EINVAL, "workspace too small");
    s.cast_w1_lowp();
    s.layer1_operands();
    GS_REQUIRE(!T.defer || !embed_out, GS_EINVAL, "deferred update: unsupported step");
    s.w1_for_forward();
    if (!slot) gather1(T, pack, hop_sizes, offsets, p.agg[0], st);
    s.forward_layer1();
    // a 2-layer training step runs layer 2, the loss head and layer 2's dIn in
    // one launch (top.hip) inside backward_top
    const bool top = !embed_out && roots && T.fuse_bwd && T.use_top && L == 2 &&
                     top_supported(s.H, T.cfg.n_classes, T.cfg.gcn != 0);
    if (!top) s.forward_upper();
    if (embed_out) return p.used;  // inference: no loss head, no backward
    T.norm_ready = false;
    if (T.fuse_bwd && L >= 2) {
        LayerBwd lb[GS_MAX_HOPS] = {};
        const bool fusable = s.layer_bwd_args(top, lb);
        GS_REQUIRE(!top || fusable, GS_EINVAL, "top launch needs the fused backward");
        if (fusable) {
            if (top) {
                s.backward_top(lb[0]);
            } else {
                const int cls_rows = cls_rows_launch(B, s.H, T.cfg.n_classes, p.h[L - 1], s.P + T.cls_w_off,
                                                     s.P + T.cls_b_off, T.cfg.labels, roots, 1, p.demb, p.cls_ws, st);
                s.backward_fused(lb, L - 1, s.cls_reduce_role(cls_rows));
            }
            return p.used;
        }
    }
    s.backward_unfused();
    return p.used;
}

// The parity capture of one finished training step (gs_trainer_capture).
static void capture_step(gs_trainer& T, int64_t B, hipStream_t st) {
    auto& c = T.cap;
    if (c.n >= c.max_steps || (!c.emb && !c.grads)) return;
    if (c.emb) {
        GS_REQUIRE(B * T.cfg.hidden <= c.emb_stride, GS_EINVAL, "capture: batch larger than the embedding stride");
        GS_REQUIRE(hipMemcpyAsync(c.emb + c.n * c.emb_stride, T.last_emb, B * T.cfg.hidden * sizeof(float),
                                  hipMemcpyDeviceToDevice, st) == hipSuccess,
                   GS_EHIP, "hipMemcpyAsync(capture)");
    }
    if (c.grads)
        GS_REQUIRE(hipMemcpyAsync(c.grads + c.n * T.total, T.cfg.grads, T.total * sizeof(float),
                                  hipMemcpyDeviceToDevice, st) == hipSuccess,
                   GS_EHIP, "hipMemcpyAsync(capture)");
    ++c.n;
}

void trainer_set_upper_hook(gs_trainer* t, std::function<void(hipStream_t)> hook) { t->upper_hook = std::move(hook); }
void trainer_set_w1_chunk_hook(gs_trainer* t, int chunks, std::function<void(hipStream_t, int64_t, int64_t)> hook) {
    t->w1_chunks = hook ? std::max(1, chunks) : 1;
    t->w1_chunk_hook = std::move(hook);
}

// Every gather slot's buffer `buf` anew, `bytes` bytes each (at least 256), or
// none with bytes < 0.  The caller zeroes the counts that describe these
// buffers before the call and sets them after it, so a refused allocation
// leaves counts that promise nothing, and the next reserve starts over.
template <class P>
static void regrow_slots(gs_trainer* t, P GatherSlot::*buf, int64_t bytes) {
    for (GatherSlot& s : t->slot) {
        if (s.*buf) t->mem.release(std::exchange(s.*buf, nullptr));
        if (bytes >= 0) s.*buf =static_cast<P>(static_cast<void*>(t->mem.alloc<char>(std::max<int64_t>(bytes, 256))));
    }
}

void trainer_reserve_top(gs_trainer* t, int64_t B, int32_t tk) {
    if (t->cfg.n_layers != 2 || t->cfg.gcn || tk < 1 || tk > 31 || B < 1) return;
    if (B <= t->top_rows && tk == t->top_k) return;
    t->top_rows = t->rec_rows = 0;
    t->top_k = 0;
    for (GatherSlot& s : t->slot) s.top_ready = s.rec_ready = false;
    regrow_slots(t, &GatherSlot::top, B * (tk + 1) * 4);
    // the backward's records for up to a1_rows layer-1 rows (gs_trainer_gather_reserve first)
    regrow_slots(t, &GatherSlot::rec, t->a1_rows * 8 * 4);
    t->top_rows = B;
    t->top_k = tk;
    t->rec_rows = t->a1_rows;
}

int64_t trainer_w1_floats(const gs_trainer* t) { return t->w_rows[0] * t->w_cols[0]; }

void trainer_set_done(gs_trainer* t, int64_t* ptr, int64_t value) { t->done = {ptr, value}; }
bool trainer_done_taken(const gs_trainer* t) { return t->done.ptr == nullptr; }

}  // namespace gs

extern "C" {

int gs_trainer_create(const gs_trainer_config* cfg, gs_trainer** out) {
    GS_API_BEGIN
    GS_REQUIRE(cfg && out, GS_EINVAL, "NULL argument");
    GS_REQUIRE(cfg->n_layers >= 1 && cfg->n_layers <= GS_MAX_HOPS, GS_EINVAL, "n_layers out of range");
    GS_REQUIRE(cfg->hidden >= 16 && cfg->hidden <= 256 && cfg->hidden % 16 == 0, GS_EINVAL, "bad hidden size");
    GS_REQUIRE(cfg->n_classes >= 1 && cfg->feat_dim >= 1 && cfg->feat_ld >= cfg->feat_dim, GS_EINVAL, "bad dims");
    GS_REQUIRE(cfg->X && cfg->col && cfg->labels && cfg->params && cfg->grads, GS_EINVAL,
               "NULL device pointer");
    std::unique_ptr<gs_trainer> T(new gs_trainer());
    T->cfg = *cfg;
    int64_t at = 0;
    for (int l = 1; l <= cfg->n_layers; ++l) {
        const int64_t in = l == 1 ? cfg->feat_dim : cfg->hidden;
        T->w_off.push_back(at);
        T->w_rows.push_back(cfg->hidden);
        T->w_cols.push_back(cfg->gcn ? in : 2 * in);
        at += cfg->hidden * T->w_cols.back();
    }
    T->cls_w_off = at;
    at += static_cast<int64_t>(cfg->n_classes) * cfg->hidden;
    T->cls_b_off = at;
    at += cfg->n_classes;
    T->total = at;
    {
        int64_t np = 0;
        for (int l = 1; l <= cfg->n_layers; ++l) np += gs::sum_slabs_grid(cfg->hidden * T->w_cols[l - 1]);
        np = std::max<int64_t>({np, gs::cls_reduce_grid(cfg->n_classes, cfg->hidden), 64});
        T->pstride = static_cast<int>((np + 63) / 64 * 64);
        T->norm_part = T->mem.alloc<float>(2 * T->pstride);
        if (cfg->feat_dtype == GS_BF16) T->w1_lp = T->mem.alloc<uint16_t>(T->w_rows[0] * T->w_cols[0]);
    }
    *out = T.release();
    GS_API_END
}

void gs_trainer_destroy(gs_trainer* t) { delete t; }

int64_t gs_trainer_n_params(const gs_trainer* t) { return t ? t->total : -1; }

float* gs_trainer_grads(const gs_trainer* t) { return t ? t->cfg.grads : nullptr; }

int gs_trainer_set_option(gs_trainer* t, int32_t opt, int32_t value) {
    GS_API_BEGIN
    GS_REQUIRE(t, GS_EINVAL, "NULL argument");
    GS_REQUIRE(!t->defer && !t->pending, GS_EINVAL, "options cannot change inside a runner loop");
    const bool on = value != 0;
    switch (opt) {
        case GS_TOPT_FUSED_BWD: t->fuse_bwd = on; break;
        case GS_TOPT_TOP_LAUNCH: t->use_top = on; break;
        case GS_TOPT_SELF_ROWS: t->want_self_rows = on; break;
        case GS_TOPT_DEFER_UPDATE: t->opt_defer = on; break;
        default: GS_REQUIRE(false, GS_EINVAL, "unknown trainer option");
    }
    GS_API_END
}

int64_t gs_trainer_ws_bytes(gs_trainer* t, const int64_t* hop_sizes) {
    try {
        std::vector<int64_t> off(GS_MAX_HOPS * GS_PK_NFIELDS, 0);
        return gs::run_step(*t, nullptr, hop_sizes, off.data(), nullptr, hop_sizes[0], nullptr, 0, nullptr,
                            nullptr);
    } catch (const gs::Error& e) {
        gs::set_error(e.what());
        return -1;
    }
}

int gs_trainer_forward_backward(gs_trainer* t, const int32_t* pack, const int64_t* hop_sizes,
                                const int64_t* offsets, const int32_t* roots, int64_t n_roots, void* ws,
                                int64_t ws_bytes, float* loss, void* stream) {
    GS_API_BEGIN
    GS_REQUIRE(t && pack && hop_sizes && offsets && roots && ws && loss, GS_EINVAL, "NULL argument");
    gs::run_step(*t, pack, hop_sizes, offsets, roots, n_roots, static_cast<char*>(ws), ws_bytes, loss,
                 gs::as_stream(stream));
    gs::capture_step(*t, n_roots, gs::as_stream(stream));
    GS_API_END
}

int gs_trainer_capture(gs_trainer* t, float* emb, int64_t emb_stride, float* grads, int64_t max_steps) {
    GS_API_BEGIN
    GS_REQUIRE(t && max_steps >= 0 && (!emb || emb_stride >= t->cfg.hidden), GS_EINVAL, "bad arguments");
    t->cap = {};
    t->cap.emb = emb;
    t->cap.emb_stride = emb_stride;
    t->cap.grads = grads;
    t->cap.max_steps = max_steps;
    GS_API_END
}

int64_t gs_trainer_captured(const gs_trainer* t) { return t ? t->cap.n : -1; }

int gs_trainer_gather_reserve(gs_trainer* t, int64_t max_rows, int32_t max_fanout) {
    GS_API_BEGIN
    GS_REQUIRE(t && max_rows >= 0 && max_fanout >= 0, GS_EINVAL, "bad arguments");
    const bool self_rows = t->want_self_rows && !t->cfg.gcn && t->cfg.n_layers >= 1;
    if (max_rows <= t->a1_rows && max_fanout <= t->k_ids && self_rows == t->self_rows) return GS_OK;
    max_rows = std::max(max_rows, t->a1_rows);
    GS_REQUIRE(max_rows * max_fanout < (int64_t(1) << 31), GS_EINVAL, "gather slot too large for int32 ids");
    t->a1_rows = 0;
    t->k_ids = 0;
    t->self_rows = self_rows;
    for (gs::GatherSlot& s : t->slot) s.self_in = false;
    gs::regrow_slots(t, &gs::GatherSlot::a1,
                     max_rows * t->cfg.feat_dim * (self_rows ? 2 : 1) * (t->cfg.feat_dtype == GS_BF16 ? 2 : 4));
    gs::regrow_slots(t, &gs::GatherSlot::ids, max_fanout > 0 ? max_rows * max_fanout * 4 : -1);
    t->a1_rows = max_rows;
    t->k_ids = max_fanout;
    GS_API_END
}

int gs_trainer_gather(gs_trainer* t, const int32_t* pack, const int64_t* hop_sizes, const int64_t* offsets,
                      int32_t slot, void* stream) {
    GS_API_BEGIN
    GS_REQUIRE(t && pack && hop_sizes && offsets && slot >= 0 && slot < gs_trainer::kSlots, GS_EINVAL,
               "bad arguments");
    const int L = t->cfg.n_layers;
    gs::GatherSlot& g = t->slot[slot];
    GS_REQUIRE(hop_sizes[4 * (L - 1)] <= t->a1_rows && g.a1, GS_EINVAL,
               "gather slot too small (gs_trainer_gather_reserve)");
    const int64_t n_dst = hop_sizes[4 * (L - 1)], n_pos = hop_sizes[4 * (L - 1) + 1];
    if (t->k_ids > 0 && n_pos <= n_dst * t->k_ids) {  // every neighbourhood fits k_ids slots
        gs::gather1_ids(*t, pack, hop_sizes, offsets, g, gs::as_stream(stream));
    } else if (t->self_rows) {  // the agg half only: the GEMMs gather the self rows themselves
        const int64_t F = t->cfg.feat_dim, xsz = t->cfg.feat_dtype == GS_BF16 ? 2 : 4;
        gs::gather1(*t, pack, hop_sizes, offsets, static_cast<char*>(g.a1) + F * xsz, gs::as_stream(stream), 2 * F);
        g.self_in = false;
    } else {
        gs::gather1(*t, pack, hop_sizes, offsets, g.a1, gs::as_stream(stream));
    }
    GS_API_END
}

int gs_trainer_forward_backward_gathered(gs_trainer* t, const int32_t* pack, const int64_t* hop_sizes,
                                         const int64_t* offsets, const int32_t* roots, int64_t n_roots,
                                         int32_t slot, void* ws, int64_t ws_bytes, float* loss, void* stream) {
    GS_API_BEGIN
    GS_REQUIRE(t && pack && hop_sizes && offsets && roots && ws && loss && slot >= 0 && slot < gs_trainer::kSlots,
               GS_EINVAL, "bad arguments");
    gs::run_step(*t, pack, hop_sizes, offsets, roots, n_roots, static_cast<char*>(ws), ws_bytes, loss,
                 gs::as_stream(stream), slot);
    gs::capture_step(*t, n_roots, gs::as_stream(stream));
    GS_API_END
}

int gs_trainer_forward(gs_trainer* t, const int32_t* pack, const int64_t* hop_sizes, const int64_t* offsets,
                       void* ws, int64_t ws_bytes, float* out, void* stream) {
    GS_API_BEGIN
    GS_REQUIRE(t && pack && hop_sizes && offsets && ws && out, GS_EINVAL, "NULL argument");
    gs::run_step(*t, pack, hop_sizes, offsets, nullptr, hop_sizes[0], static_cast<char*>(ws), ws_bytes, nullptr,
                 gs::as_stream(stream), -1, out);
    GS_API_END
}

int gs_trainer_forward_gathered(gs_trainer* t, const int32_t* pack, const int64_t* hop_sizes,
                                const int64_t* offsets, int32_t slot, void* ws, int64_t ws_bytes, float* out,
                                void* stream) {
    GS_API_BEGIN
    GS_REQUIRE(t && pack && hop_sizes && offsets && ws && out && slot >= 0 && slot < gs_trainer::kSlots, GS_EINVAL,
               "bad arguments");
    gs::run_step(*t, pack, hop_sizes, offsets, nullptr, hop_sizes[0], static_cast<char*>(ws), ws_bytes, nullptr,
                 gs::as_stream(stream), slot, out);
    GS_API_END
}

}  // extern "C"
