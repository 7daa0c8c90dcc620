// Exact layer-wise inference over full neighbourhoods: H_l for every node
// from H_{l-1}, chunk by chunk -- the full-neighbourhood aggregate of a chunk
// (agg_full.hip) into a chunk buffer A, then the SageLayer GEMM of the chunk
// (linear_fwd_launch: the chunk's own rows of H_{l-1} as self rows, identity
// index) into the chunk's rows of H_l.  A chunk's A is written and read back
// while it is still cache-resident instead of making a round trip of
// N x F through HBM.  Nothing is allocated here: the intermediate H buffers
// (ping-pong), A, the bf16 copy of W1 and the aggregate's partials live in
// the caller's workspace.
#include "agg_full.hpp"
#include "internal.hpp"

#include <algorithm>

namespace gs {

namespace {

struct FullLayout {
    int64_t chunk = 0, w1lp = -1, h[2] = {-1, -1}, a = 0, part = 0, part_bytes = 0, total = 0;
};

void check_config(const FullPlan& p, const gs_infer_full_config& c) {
    GS_REQUIRE(c.n_layers >= 1 && c.n_layers <= GS_MAX_HOPS, GS_EINVAL, "1 to 8 layers");
    GS_REQUIRE(c.hidden >= 16 && c.hidden <= 256 && c.hidden % 16 == 0, GS_EINVAL,
               "hidden must be a multiple of 16 in [16, 256]");
    GS_REQUIRE(c.agg == GS_AGG_MEAN || c.agg == GS_AGG_MAX, GS_EINVAL, "agg_func must be MEAN or MAX");
    GS_REQUIRE(c.feat_dtype == GS_F32 || c.feat_dtype == GS_BF16, GS_EINVAL, "dtype must be f32 or bf16");
    GS_REQUIRE(c.feat_dim >= 1 && c.feat_dim < (1 << 28) && c.feat_ld >= c.feat_dim, GS_EINVAL, "bad feature shape");
    GS_REQUIRE(p.n >= 1, GS_EINVAL, "empty graph");
}

FullLayout layout_of(const FullPlan& p, const gs_infer_full_config& c) {
    check_config(p, c);
    FullLayout lo;
    const int64_t n = p.n, H = c.hidden, F = c.feat_dim, L = c.n_layers;
    lo.chunk = c.chunk_rows <= 0 ? n : std::min<int64_t>(c.chunk_rows, n);
    const int64_t es = c.feat_dtype == GS_BF16 ? 2 : 4;
    int64_t off = 0;
    if (c.feat_dtype == GS_BF16) {
        lo.w1lp = off;
        off += round_up(H * (p.gcn ? F : 2 * F) * 2);
    }
    for (int i = 0; i < 2 && i < L - 1; ++i) {
        lo.h[i] = off;
        off += round_up(n * H * 4);
    }
    lo.a = off;
    off += round_up(lo.chunk * std::max(F * es, L >= 2 ? H * 4 : int64_t(0)));
    int64_t slots = 0;
    for (int64_t r0 = 0; r0 < n; r0 += lo.chunk)
        slots = std::max(slots, p.slot_ptr[std::min(n, r0 + lo.chunk)] - p.slot_ptr[r0]);
    lo.part = off;
    lo.part_bytes = slots * std::max(F, L >= 2 ? H : int64_t(0)) * 4;
    off += round_up(lo.part_bytes);
    lo.total = off;
    return lo;
}

}  // namespace

void infer_full_run(const FullPlan& p, const gs_full_plan_dev& d, const gs_infer_full_config& c, float* out,
                    int64_t ldo, void* ws, int64_t ws_bytes, hipStream_t st) {
    const FullLayout lo = layout_of(p, c);
    const int64_t n = p.n, H = c.hidden, L = c.n_layers;
    GS_REQUIRE(out && ldo >= H && c.X && c.row_ptr && c.col, GS_EINVAL, "NULL pointer or ldo < hidden");
    for (int l = 0; l < L; ++l) GS_REQUIRE(c.W[l], GS_EINVAL, "NULL weight");
    GS_REQUIRE(ws && ws_bytes >= lo.total && (reinterpret_cast<uintptr_t>(ws) & (kAlign - 1)) == 0, GS_EINVAL,
               "workspace smaller than gs_infer_full_ws_bytes or not 256-byte aligned");
    GS_REQUIRE(c.agg != GS_AGG_MAX || !d.weight, GS_EINVAL, "edge weights go with MEAN, not MAX");
    if (c.agg == GS_AGG_MAX && !p.empty_rows.empty())
        fail(GS_EEMPTY, "gs_infer_full: MAX aggregation over an empty neighbourhood (reference: models.py:321-325)");
    char* base = static_cast<char*>(ws);
    const gs_agg op = static_cast<gs_agg>(c.agg);
    if (lo.w1lp >= 0) {  // the forward's bf16 W1, as the trainer casts it
        const int rc = gs_cast_f32_bf16(c.W[0], base + lo.w1lp, H * (p.gcn ? c.feat_dim : 2 * c.feat_dim), st);
        if (rc != GS_OK) fail(rc, gs_last_error());
    }
    for (int l = 1; l <= L; ++l) {
        const gs_dtype dt = l == 1 ? static_cast<gs_dtype>(c.feat_dtype) : GS_F32;
        const int64_t es = dt == GS_BF16 ? 2 : 4;
        const char* in = l == 1 ? static_cast<const char*>(c.X) : base + lo.h[(l - 2) % 2];
        const int64_t ldin = l == 1 ? c.feat_ld : H, fin = l == 1 ? c.feat_dim : H;
        float* hout = l == L ? out : reinterpret_cast<float*>(base + lo.h[(l - 1) % 2]);
        const int64_t ldh = l == L ? ldo : H;
        const void* W = (l == 1 && lo.w1lp >= 0) ? static_cast<const void*>(base + lo.w1lp) : c.W[l - 1];
        for (int64_t r0 = 0; r0 < n; r0 += lo.chunk) {
            const int64_t m = std::min(lo.chunk, n - r0);
            agg_full_launch(p, d, op, dt, in, ldin, fin, c.row_ptr, c.col, r0, m, base + lo.a, fin, base + lo.part,
                            lo.part_bytes, st);
            linear_fwd_launch(dt, m, fin, H, p.gcn ? nullptr : in + r0 * ldin * es, ldin, nullptr, base + lo.a, fin,
                              W, hout + r0 * ldh, ldh, 1, st);
        }
    }
}

}  // namespace gs

extern "C" {

int64_t gs_infer_full_ws_bytes(const gs_full_plan* plan, const gs_infer_full_config* cfg) {
    GS_BYTES_BEGIN
    if (!plan || !cfg) return -1;
    return gs::layout_of(*reinterpret_cast<const gs::FullPlan*>(plan), *cfg).total;
    GS_BYTES_END
}

int gs_infer_full(const gs_full_plan* plan, const gs_full_plan_dev* dev, const gs_infer_full_config* cfg, float* out,
                  int64_t ldo, void* ws, int64_t ws_bytes, void* stream) {
    GS_API_BEGIN
    GS_REQUIRE(plan && dev && cfg, GS_EINVAL, "NULL argument");
    gs::infer_full_run(*reinterpret_cast<const gs::FullPlan*>(plan), *dev, *cfg, out, ldo, ws, ws_bytes,
                       gs::as_stream(stream));
    GS_API_END
}

}  // extern "C"
