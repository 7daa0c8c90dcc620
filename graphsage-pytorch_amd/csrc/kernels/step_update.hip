// The native trainer's updates: the deferred clip + SGD (its state is
// gs_trainer's defer / pending fields), the bf16 W1 kept beside the updates,
// and the optimiser entry points (clip + SGD, clip + Adam).
#include "trainer.hpp"

namespace gs {

FwdSpec pending_spec(gs_trainer& T) {
    const gs_trainer_config& c = T.cfg;
    FwdSpec sp;
    sp.on = 1;
    sp.S = T.w1_buf(T.w1_cur ^ 1);
    sp.P = T.w1_buf(T.w1_cur);
    sp.G1 = c.grads + T.w_off[0];
    sp.part0 = T.pend_part;
    sp.part1 = T.pend_part + T.pend_pstride;
    sp.np0 = T.pend_np[0];
    sp.np1 = T.pend_np[1];
    sp.lr = c.lr;
    sp.max_norm = c.max_norm;
    sp.scale = T.pend_scale;
    sp.p = c.params;
    sp.g = c.grads;
    sp.up_lo = T.w_off[0] + T.w_rows[0] * T.w_cols[0];
    sp.up_hi = T.total;
    sp.grp1_lo = T.cls_w_off;
    return sp;
}

// The bf16 W1 that an SGD launch writes beside the update (runner loops
// only: lp_keep), passed to that launch; empty otherwise.
static LowpShadow lowp_shadow(const gs_trainer* t) {
    if (!(t->lp_keep && t->w1_lp)) return {};
    return {t->w1_lp, t->w_off[0], t->w_off[0] + t->w_rows[0] * t->w_cols[0]};
}

void trainer_keep_lowp(gs_trainer* t, bool keep) {
    t->lp_keep = keep;
    t->lp_valid = false;
}

// W1 back in the flat params (a pending update stays pending: its S and P
// buffers are then the flat W1 and w1_alt, or it is finalised by the caller).
static void w1_home(gs_trainer* t, hipStream_t st) {
    if (t->w1_cur == 0) return;
    GS_REQUIRE(!t->pending, GS_EINVAL, "W1 moved with an update pending");
    const int64_t n = t->w_rows[0] * t->w_cols[0];
    GS_REQUIRE(hipMemcpyAsync(t->w1_buf(0), t->w1_alt, n * sizeof(float), hipMemcpyDeviceToDevice, st) == hipSuccess,
               GS_EHIP, "hipMemcpyAsync(W1)");
    t->w1_cur = 0;
}

// The trainer's clip + Adam update number opt.step + 1: one launch from the
// step's own norm partials (parts), else the norm launch into ws first.
static void adam_update(gs_trainer* t, bool parts, float grad_scale, float* ws, hipStream_t st, LowpShadow shadow) {
    const gs_trainer_config& c = t->cfg;
    const gs_optimizer_config& o = t->opt;
    const int64_t goff[3] = {0, t->cls_w_off, t->total};
    const AdamStep a{c.lr, o.beta1, o.beta2, o.eps, o.weight_decay, o.step + 1};
    if (parts)
        adam_with_parts(2, goff, t->npart, t->pstride, c.params, c.grads, o.m, o.v, t->norm_part, grad_scale,
                        c.max_norm, a, st, shadow, t->take_done());
    else
        clip_adam_launch(2, goff, c.params, c.grads, o.m, o.v, grad_scale, c.max_norm, a, ws, st, shadow,
                         t->take_done());
    ++t->opt.step;
}

bool trainer_defer_update(gs_trainer* t, bool on, hipStream_t st, bool comm) {
    if (!on) {
        if (t->pending) {  // the last step's clip + SGD: the flat params become what sgd4 would leave
            spec_finalize_launch(pending_spec(*t), t->w1_buf(0), t->w_rows[0] * t->w_cols[0], st);
            t->pending = false;
            t->w1_cur = 0;
        }
        w1_home(t, st);
        t->defer = false;
        t->defer_comm = false;
        t->norm_ready = false;
        t->lp_valid = false;  // the next bf16 forward casts the flat W1 again
        return false;
    }
    const gs_trainer_config& c = t->cfg;
    const int64_t n1 = t->w_rows[0] * t->w_cols[0];
    // the pending update is applied by the wide (16-B load) layer-1 forward:
    // its feature rows must take 16-B loads (w1_for_forward, step.hip, re-checks each step's
    // operands and applies the update on its own where they do not)
    const int64_t epv = c.feat_dtype == GS_F32 ? 4 : 8;
    // (and only SGD is speculated on: sgd_elem in the slab sum, FwdSpec, sumsq_spec, spec_finalize)
    const bool can = t->opt.kind == GS_OPT_SGD && t->opt_defer &&
                    (c.feat_dtype == GS_F32 || (c.feat_dtype == GS_BF16 && t->w1_lp)) &&
                    t->fuse_bwd && t->use_top && c.n_layers == 2 && !c.gcn &&
                    (comm || (!t->upper_hook && !t->w1_chunk_hook)) && n1 % 4 == 0 &&
                    c.feat_dim % epv == 0 && c.feat_ld % epv == 0 && aligned16(c.X) &&
                    t->cls_w_off % 4 == 0 && t->total % 4 == 0 && aligned16(c.params) && aligned16(c.grads);
    if (!can) return false;
    if (!t->w1_alt) t->w1_alt = t->mem.alloc<float>(n1);
    if (c.feat_dtype == GS_BF16 && !t->w1_lp_alt) t->w1_lp_alt = t->mem.alloc<uint16_t>(n1);
    t->lp_valid = false;  // the first forward casts W1 into lp_buf(0)
    t->defer = true;
    t->defer_comm = comm;
    t->pending = false;
    t->w1_cur = 0;
    return true;
}

}  // namespace gs

extern "C" {

int gs_trainer_set_optimizer(gs_trainer* t, const gs_optimizer_config* oc) {
    GS_API_BEGIN
    GS_REQUIRE(t && oc, GS_EINVAL, "NULL argument");
    GS_REQUIRE(oc->kind == GS_OPT_SGD || oc->kind == GS_OPT_ADAM, GS_EINVAL, "unknown optimizer kind");
    GS_REQUIRE(!t->defer && !t->pending && !t->lp_keep, GS_EINVAL,
               "the optimizer cannot change while deferring, with an update pending or inside a runner loop");
    if (oc->kind == GS_OPT_ADAM) {
        gs::adam_require(oc->beta1, oc->beta2, oc->eps, oc->weight_decay);
        GS_REQUIRE(oc->m && oc->v, GS_EINVAL, "NULL moment buffer");
        GS_REQUIRE(oc->step >= 0, GS_EINVAL, "negative step count");
    }
    t->opt = *oc;
    GS_API_END
}

int64_t gs_trainer_opt_step(const gs_trainer* t) { return t ? t->opt.step : -1; }

int gs_trainer_update_local(gs_trainer* t, void* stream) {
    GS_API_BEGIN
    GS_REQUIRE(t, GS_EINVAL, "NULL argument");
    if (t->pending) {  // deferred update: the next forward (or trainer_defer_update(false)) applies it
        t->norm_ready = false;
        return GS_OK;
    }
    gs::w1_home(t, gs::as_stream(stream));  // a deferred-update step that could not defer
    const int64_t goff[3] = {0, t->cls_w_off, t->total};
    t->lp_valid = false;
    const gs::LowpShadow shadow = gs::lowp_shadow(t);
    if (t->opt.kind == GS_OPT_ADAM) {
        gs::adam_update(t, t->norm_ready, 1.0f, t->norm_part, gs::as_stream(stream), shadow);
    } else if (t->norm_ready) {
        gs::sgd_with_parts(2, goff, t->npart, t->pstride, t->cfg.params, t->cfg.grads, t->norm_part, 1.0f,
                           t->cfg.max_norm, t->cfg.lr, gs::as_stream(stream), shadow, t->take_done());
    } else {
        gs::clip_sgd_launch(2, goff, t->cfg.params, t->cfg.grads, 1.0f, t->cfg.max_norm, t->cfg.lr, t->norm_part,
                            gs::as_stream(stream), shadow, t->take_done());
    }
    t->lp_valid = shadow.p != nullptr;
    t->norm_ready = false;
    GS_API_END
}

int gs_trainer_update(gs_trainer* t, float grad_scale, float* ws, void* stream) {
    GS_API_BEGIN
    GS_REQUIRE(t && ws, GS_EINVAL, "NULL argument");
    t->norm_ready = false;
    GS_REQUIRE(!t->pending, GS_EINVAL, "gs_trainer_update with an update already pending");
    if (t->defer && t->defer_comm) {
        // deferred after the all-reduce: the norm partials of the summed gradient
        // and W1's speculative update in one launch; the next forward (or
        // trainer_defer_update(false)) applies the clip + SGD
        const int64_t goff[3] = {0, t->cls_w_off, t->total};
        const int64_t n1 = t->w_rows[0] * t->w_cols[0];
        const bool lowp = t->cfg.feat_dtype == GS_BF16;
        const int np = gs::sumsq_spec_launch(2, goff, t->cfg.grads, ws, t->w1_buf(t->w1_cur), t->w1_buf(t->w1_cur ^ 1),
                                             lowp ? t->lp_buf(t->w1_cur ^ 1) : nullptr, n1, t->cfg.lr, grad_scale,
                                             gs::as_stream(stream), t->take_done());
        t->pending = true;
        t->pend_part = ws;
        t->pend_pstride = np;
        t->pend_np[0] = np;
        t->pend_np[1] = np;
        t->pend_scale = grad_scale;
        return GS_OK;
    }
    gs::w1_home(t, gs::as_stream(stream));
    const int64_t goff[3] = {0, t->cls_w_off, t->total};
    t->lp_valid = false;
    const gs::LowpShadow shadow = gs::lowp_shadow(t);
    if (t->opt.kind == GS_OPT_ADAM)
        gs::adam_update(t, false, grad_scale, ws, gs::as_stream(stream), shadow);
    else
        gs::clip_sgd_launch(2, goff, t->cfg.params, t->cfg.grads, grad_scale, t->cfg.max_norm, t->cfg.lr, ws,
                            gs::as_stream(stream), shadow, t->take_done());
    t->lp_valid = shadow.p != nullptr;
    GS_API_END
}

int gs_trainer_defer(gs_trainer* t, int32_t on, int32_t* active, void* stream) {
    GS_API_BEGIN
    GS_REQUIRE(t, GS_EINVAL, "NULL argument");
    hipStream_t st = gs::as_stream(stream);
    if (active) *active = 0;
    if (on) {
        GS_REQUIRE(!t->defer && !t->pending, GS_EINVAL, "gs_trainer_defer: already deferring");
        gs::trainer_keep_lowp(t, true);  // the bf16 W1 follows every update, as in a runner loop
        const bool deferring = gs::trainer_defer_update(t, true, st, true);
        if (!deferring) gs::trainer_keep_lowp(t, false);
        if (active) *active = deferring ? 1 : 0;
    } else {
        if (t->defer) gs::trainer_defer_update(t, false, st);
        gs::trainer_keep_lowp(t, false);
    }
    GS_API_END
}

}  // extern "C"
