// The classifier on frozen embeddings (reference utils.py:80-111,
// train_classification) as whole-run launches: every batch-`batch` SGD step of
// every epoch inside one persistent single-workgroup kernel.
//
// One step (utils.py:94-108 on features[nodes_batch]), n rows of the batch:
//   logits = E[rows]·Wᵀ + b;  logp = log_softmax (max-shifted)
//   loss   = -Σ_i logp[i, y_i] / n
//   G      = (softmax - onehot) / n;  dW = Gᵀ·E[rows];  db = Σ_i G[i]
//   coef   = min(1, max_norm / (‖(dW, db)‖ + 1e-6))   (clip_mult, cls_dev.hpp)
//   p      = fma(-lr, g·coef, p)                        (sgd_elem, cls_dev.hpp)
//
// Launch shape: one workgroup of kProbeThreads.  LDS, in floats (LD the padded
// tile row, LG the padded G row):
//   params  P4 = round4(C·D + C)    W row-major then b, resident for the launch
//   grads   P4                      the step's dW, db (the norm needs all of them
//                                   before the first update)
//   tile    round4(batch · LD)      the batch's rows; LD = D + 4 on the float4
//                                   path (rows 16-B aligned, a wave's b128 reads
//                                   of 16 rows on 16 distinct slots), D | 1 on
//                                   the scalar path (odd stride)
//   G       round4(batch · LG)      logits, then (softmax - onehot)/n; LG = C | 1
//   rowloss round4(batch)           -logp[i, y_i]
//   y       round4(batch)           the batch's labels
//   ids     2 · round4(batch)       row ids of the next two steps
//   red     32                      wave partials of Σ g²
// gs_cls_probe_supported: the sum, with LD = D + 4 where D % 4 == 0 and D | 1
// otherwise, times 4 bytes is at most the 160 KiB one workgroup may declare,
// and batch <= kProbeThreads: thread i carries row i's id and label from one
// step to the next, one row per thread.
//
// The next batch's rows are fetched into registers while the current batch is
// computed (`order` is known in advance): each thread issues up to kProbePre
// 16-byte (scalar path: 4-byte) loads at the start of a step and stores them
// into the one tile after the step's last read of it.  Rows beyond
// kProbeThreads · kProbePre loads are fetched at that point instead, not
// overlapped.  The row ids come from LDS (loaded two steps ahead), so the
// fetch is one memory round, not two dependent ones.
//
// Every sum is in an order fixed by the shape alone (dot products over d in
// four interleaved chains, dW over the batch rows in row order, Σ g² per
// thread in item order, then the wave tree of wave_sum, then the waves in
// order); no atomics: two runs are bitwise equal, wherever the host cuts the
// run into launches (the state between launches is `params`, and the first
// step of a launch loads its tile the way the prefetch would have).
#include <algorithm>
#include <cmath>
#include <mutex>

#include "cls_dev.hpp"

namespace gs {

constexpr int kProbeThreads = 512;
constexpr int kProbeWaves = kProbeThreads / 64;
constexpr int kProbePre = 4;                         // loads in flight per thread
constexpr int64_t kProbeLdsBytes = 160 * 1024;       // one workgroup's LDS on gfx950
constexpr int64_t kProbeMaxSteps = 65536;            // steps per launch (shared machines: short launches)

struct ProbeLayout {
    int ld, lg;                                      // padded row of the tile / of G, floats
    int oG, oT, oGm, oLoss, oY, oIds, oRed, floats;  // float offsets (params at 0), and the total
};

inline int64_t round4(int64_t x) { return (x + 3) & ~int64_t(3); }

// The layout for tile rows of `ld` floats; floats < 0: does not fit.
inline ProbeLayout probe_layout(int64_t D, int64_t C, int64_t batch, int64_t ld) {
    ProbeLayout L{};
    const int64_t cap = kProbeLdsBytes / 4;
    L.floats = -1;
    if (batch > kProbeThreads) return L;  // one thread per row for the ids and labels
    if (D < 1 || C < 1 || batch < 1 || D > cap || C > cap || batch > cap || C * D + C > cap) return L;
    const int64_t lg = C | 1, P4 = round4(C * D + C), B4 = round4(batch);
    if (batch * ld > cap || batch * lg > cap) return L;
    const int64_t oG = P4, oT = 2 * P4, oGm = oT + round4(batch * ld), oLoss = oGm + round4(batch * lg);
    const int64_t oY = oLoss + B4, oIds = oY + B4, oRed = oIds + 2 * B4, total = oRed + 32;
    if (total > cap) return L;
    L.ld = static_cast<int>(ld);
    L.lg = static_cast<int>(lg);
    L.oG = static_cast<int>(oG);
    L.oT = static_cast<int>(oT);
    L.oGm = static_cast<int>(oGm);
    L.oLoss = static_cast<int>(oLoss);
    L.oY = static_cast<int>(oY);
    L.oIds = static_cast<int>(oIds);
    L.oRed = static_cast<int>(oRed);
    L.floats = static_cast<int>(total);
    return L;
}

inline int64_t probe_ld(int64_t D, bool vec) { return vec ? D + 4 : (D | 1); }

struct ProbeArgs {
    const float* E;
    int64_t lde;
    int D, C, batch, n_train, spe;  // spe: steps per epoch
    const int32_t* labels;
    const int32_t* order;
    int64_t g0, g1;                 // this launch's steps [g0, g1) of the run
    int e0, s0;                     // g0 = e0 · spe + s0
    float* params;
    float lr, max_norm;
    float* snapshots;
    float* losses;
    ProbeLayout L;
};

// One element of a row: 16 bytes on the float4 path, 4 on the scalar one.
template <bool VEC>
struct ProbeElem;
template <>
struct ProbeElem<true> {
    using T = float4;
    static constexpr int W = 4;
    static __device__ __forceinline__ T zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
};
template <>
struct ProbeElem<false> {
    using T = float;
    static constexpr int W = 1;
    static __device__ __forceinline__ T zero() { return 0.f; }
};

__device__ __forceinline__ void probe_fma(float4& a, float4 e, float4 w) {
    a.x = fmaf(e.x, w.x, a.x);
    a.y = fmaf(e.y, w.y, a.y);
    a.z = fmaf(e.z, w.z, a.z);
    a.w = fmaf(e.w, w.w, a.w);
}

template <bool VEC>
__global__ __launch_bounds__(kProbeThreads) void cls_probe_kernel(const ProbeArgs a) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    using EL = ProbeElem<VEC>;
    using T = typename EL::T;
    constexpr int W = EL::W;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int D = a.D, C = a.C, batch = a.batch;
    const int DW = D / W;        // elements per row
    const int LDW = a.L.ld / W;  // elements per tile row
    const int LG = a.L.lg;
    const int P = C * D + C;
    float* const prm = sm;
    float* const grd = sm + a.L.oG;
    T* const tile = reinterpret_cast<T*>(sm + a.L.oT);
    float* const Gm = sm + a.L.oGm;
    float* const rowloss = sm + a.L.oLoss;
    int* const ylab = reinterpret_cast<int*>(sm + a.L.oY);
    int* const ids = reinterpret_cast<int*>(sm + a.L.oIds);  // [2][B4]
    float* const red = sm + a.L.oRed;
    const int B4 = (batch + 3) & ~3;

    // step g = e · spe + s covers order[e · n_train + s · batch ...], n rows
    auto rows_of = [&](int s) { return min(batch, a.n_train - s * batch); };
    auto base_of = [&](int e, int s) { return static_cast<int64_t>(e) * a.n_train + static_cast<int64_t>(s) * batch; };
    auto advance = [&](int& e, int& s) {
        if (++s == a.spe) {
            s = 0;
            ++e;
        }
    };
    auto row_ptr = [&](int rid, int col) {
        return reinterpret_cast<const T*>(a.E + static_cast<int64_t>(rid) * a.lde) + col;
    };

    // this thread's prefetch items (row, column) of any step: fixed by the shape
    int pr[kProbePre], pc[kProbePre];
#pragma unroll
    for (int k = 0; k < kProbePre; ++k) {
        const int q = tid + k * kProbeThreads;
        pr[k] = q / DW;
        pc[k] = q - pr[k] * DW;
    }
    // rows past the prefetch's reach, fetched synchronously into the tile
    auto fetch_rest = [&](const int* idv, int n) {
        for (int q = tid + kProbePre * kProbeThreads; q < n * DW; q += kProbeThreads) {
            const int r = q / DW, c = q - r * DW;
            tile[r * LDW + c] = *row_ptr(idv[r], c);
        }
    };

    // ---- prologue: the parameters, the first step's ids, labels and tile, the second step's ids
    for (int t = tid; t < P; t += kProbeThreads) prm[t] = a.params[t];
    int e = a.e0, s = a.s0;
    int64_t g = a.g0;
    {
        int e1 = e, s1 = s;
        advance(e1, s1);
        const int n0 = rows_of(s);
        if (tid < n0) {
            const int rid = a.order[base_of(e, s) + tid];
            ids[(g & 1) * B4 + tid] = rid;
            ylab[tid] = a.labels[rid];
        }
        if (g + 1 < a.g1 && tid < rows_of(s1)) ids[((g + 1) & 1) * B4 + tid] = a.order[base_of(e1, s1) + tid];
        lds_barrier();
        const int* idv = ids + (g & 1) * B4;
#pragma unroll
        for (int k = 0; k < kProbePre; ++k)
            if (pr[k] < n0) tile[pr[k] * LDW + pc[k]] = *row_ptr(idv[pr[k]], pc[k]);
        fetch_rest(idv, n0);
        lds_barrier();
    }

    for (; g < a.g1; ++g) {
        const int n = rows_of(s);
        const bool last_of_epoch = s + 1 == a.spe;
        int e1 = e, s1 = s;
        advance(e1, s1);
        int e2 = e1, s2 = s1;
        advance(e2, s2);
        const int n1 = g + 1 < a.g1 ? rows_of(s1) : 0;  // the next step's rows (0: none in this launch)
        const int n2 = g + 2 < a.g1 ? rows_of(s2) : 0;
        const int* idn = ids + ((g + 1) & 1) * B4;

        // ---- the next step's rows and labels, the ids of the step after it: loads in flight
        // (clamped rows under one uniform branch, not a branch per load: every load issues
        // before the first wait)
        T pv[kProbePre];
#pragma unroll
        for (int k = 0; k < kProbePre; ++k) pv[k] = EL::zero();
        int y_next = 0, id_next2 = 0;
        if (n1 > 0) {
#pragma unroll
            for (int k = 0; k < kProbePre; ++k) pv[k] = *row_ptr(idn[min(pr[k], n1 - 1)], pc[k]);
            y_next = a.labels[idn[min(tid, n1 - 1)]];
        }
        if (n2 > 0) id_next2 = a.order[base_of(e2, s2) + min(tid, n2 - 1)];

        // ---- logits: item (c, i), lanes along i (W row c broadcast)
        for (int it = tid; it < n * C; it += kProbeThreads) {
            const int c = it / n, i = it - c * n;
            const T* er = tile + i * LDW;
            const T* wr = reinterpret_cast<const T*>(prm + c * D);
            float z;
            if constexpr (VEC) {
                float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 8
                for (int k = 0; k < DW; ++k) probe_fma(acc, er[k], wr[k]);
                z = (acc.x + acc.y) + (acc.z + acc.w);
            } else {
                float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
                int k = 0;
                for (; k + 4 <= DW; k += 4) {
                    a0 = fmaf(er[k], wr[k], a0);
                    a1 = fmaf(er[k + 1], wr[k + 1], a1);
                    a2 = fmaf(er[k + 2], wr[k + 2], a2);
                    a3 = fmaf(er[k + 3], wr[k + 3], a3);
                }
                for (; k < DW; ++k) a0 = fmaf(er[k], wr[k], a0);
                z = (a0 + a1) + (a2 + a3);
            }
            Gm[i * LG + c] = z + prm[C * D + c];
        }
        lds_barrier();

        // ---- softmax, G and the row's -logp[y]: thread i owns row i
        for (int i = tid; i < n; i += kProbeThreads) {
            float* zr = Gm + i * LG;
            float m = zr[0];
            for (int c = 1; c < C; ++c) m = fmaxf(m, zr[c]);
            const int y = ylab[i];
            const bool has = static_cast<unsigned>(y) < static_cast<unsigned>(C);  // outside [0, C): no class
            const float zy = has ? zr[y] : m;
            float sum = 0.f;
            for (int c = 0; c < C; ++c) {  // one exp per element: softmax = exp(z - m) / Σ
                const float ex = expf(zr[c] - m);
                zr[c] = ex;
                sum += ex;
            }
            rowloss[i] = has ? -((zy - m) - logf(sum)) : 0.f;
            const float inv = 1.0f / sum, inv_n = 1.0f / static_cast<float>(n);
            for (int c = 0; c < C; ++c) zr[c] = (zr[c] * inv - (has && c == y ? 1.f : 0.f)) * inv_n;
        }
        lds_barrier();

        // ---- loss = Σ_i rowloss[i] / n: wave 0, lane-strided then the wave tree
        if (wave == 0) {
            float t = 0.f;
            for (int i = lane; i < n; i += 64) t += rowloss[i];
            t = wave_sum(t);
            if (lane == 0 && a.losses) a.losses[g] = t / static_cast<float>(n);
        }

        // ---- dW = Gᵀ·tile and db = Σ_i G[i] into grd; Σ g² of this thread's items
        const int nW = C * DW;
        float sq = 0.f;
        for (int t = tid; t < nW + C; t += kProbeThreads) {
            if (t < nW) {
                const int c = t / DW, d = t - c * DW;
                const float* gc = Gm + c;
                const T* tc = tile + d;
                if constexpr (VEC) {
                    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 4
                    for (int i = 0; i < n; ++i) {
                        const float gv = gc[i * LG];
                        probe_fma(acc, make_float4(gv, gv, gv, gv), tc[i * LDW]);
                    }
                    reinterpret_cast<float4*>(grd)[t] = acc;
                    sq += (acc.x * acc.x + acc.y * acc.y) + (acc.z * acc.z + acc.w * acc.w);
                } else {
                    float acc = 0.f;
#pragma unroll 4
                    for (int i = 0; i < n; ++i) acc = fmaf(gc[i * LG], tc[i * LDW], acc);
                    grd[t] = acc;
                    sq += acc * acc;
                }
            } else {
                const int c = t - nW;
                float acc = 0.f;
                for (int i = 0; i < n; ++i) acc += Gm[i * LG + c];
                grd[C * D + c] = acc;
                sq += acc * acc;
            }
        }
        sq = wave_sum(sq);
        if (lane == 0) red[wave] = sq;
        lds_barrier();  // the tile, G and the labels are free from here

        // ---- one clip over W and b together, then SGD on this thread's own items
        float sumsq = 0.f;
#pragma unroll
        for (int w = 0; w < kProbeWaves; ++w) sumsq += red[w];
        const float mult = clip_mult(sumsq, 1.0f, a.max_norm);
        float* snap = last_of_epoch && a.snapshots ? a.snapshots + static_cast<int64_t>(e) * P : nullptr;
        for (int t = tid; t < nW + C; t += kProbeThreads) {
            const int lo = t < nW ? t * W : C * D + (t - nW);
            const int cnt = t < nW ? W : 1;
            float gi;
#pragma unroll
            for (int u = 0; u < W; ++u) {
                if (u < cnt) {
                    const float pn = sgd_elem(prm[lo + u], grd[lo + u], mult, a.lr, gi);
                    prm[lo + u] = pn;
                    if (snap) snap[lo + u] = pn;
                }
            }
        }

        // ---- the next step's tile, labels and the ids of the step after it
#pragma unroll
        for (int k = 0; k < kProbePre; ++k)
            if (pr[k] < n1) tile[pr[k] * LDW + pc[k]] = pv[k];
        fetch_rest(idn, n1);
        if (tid < n1) ylab[tid] = y_next;
        if (tid < n2) ids[(g & 1) * B4 + tid] = id_next2;
        lds_barrier();
        e = e1;
        s = s1;
    }

    for (int t = tid; t < P; t += kProbeThreads) a.params[t] = prm[t];
}

// The kernel's LDS request is above the default launch limit for the larger
// shapes: raise it once per device (the attribute is the device's), for both
// instantiations, to the whole 160 KiB.
static void probe_lds_ready() {
    static std::mutex mu;
    static uint64_t done_mask = 0;  // devices 0..63 already raised; others raise on every call
    int dev = 0;
    hip_ok(hipGetDevice(&dev), "gs_cls_probe_run: current device");
    std::lock_guard<std::mutex> lock(mu);
    const bool cached = dev >= 0 && dev < 64;
    if (cached && (done_mask >> dev & 1)) return;
    hip_ok(hipFuncSetAttribute(reinterpret_cast<const void*>(cls_probe_kernel<true>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(kProbeLdsBytes)),
           "gs_cls_probe_run: LDS limit");
    hip_ok(hipFuncSetAttribute(reinterpret_cast<const void*>(cls_probe_kernel<false>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(kProbeLdsBytes)),
           "gs_cls_probe_run: LDS limit");
    if (cached) done_mask |= uint64_t(1) << dev;
}

static bool probe_supported(int64_t D, int64_t C, int64_t batch) {
    if (D < 1 || C < 1 || batch < 1) return false;
    return probe_layout(D, C, batch, probe_ld(D, D % 4 == 0)).floats > 0;
}

}  // namespace gs

extern "C" {

int gs_cls_probe_supported(int64_t D, int64_t C, int64_t batch) { return gs::probe_supported(D, C, batch) ? 1 : 0; }

int gs_cls_probe_run_ex(const float* E, int64_t lde, int64_t n_rows, int64_t D, int64_t C, const int32_t* labels,
                        const int32_t* order, int64_t n_train, int64_t batch, int64_t n_epochs, float* params,
                        float lr, float max_norm, float* snapshots, float* losses, int64_t max_steps_per_launch,
                        void* stream) {
    GS_API_BEGIN
    using namespace gs;
    GS_REQUIRE(E && labels && order && params, GS_EINVAL, "NULL device pointer");
    GS_REQUIRE(D >= 1 && C >= 1 && batch >= 1 && n_train >= 1 && n_epochs >= 1 && n_rows >= 1, GS_EINVAL,
               "sizes must be >= 1");
    GS_REQUIRE(lde >= D, GS_EINVAL, "lde < D");
    GS_REQUIRE(std::isfinite(lr), GS_EINVAL, "lr must be finite");
    GS_REQUIRE(max_norm > 0.f, GS_EINVAL, "max_norm must be positive (INFINITY: no clip)");  // NaN fails too
    GS_REQUIRE(probe_supported(D, C, batch), GS_EINVAL, "shape unsupported (gs_cls_probe_supported)");
    GS_REQUIRE(n_rows < (int64_t(1) << 31) && n_train < (int64_t(1) << 31) && n_epochs < (int64_t(1) << 31),
               GS_EINVAL, "sizes must be below 2^31");
    const int64_t spe = (n_train + batch - 1) / batch, total = spe * n_epochs;
    const int64_t cut = max_steps_per_launch >= 1 ? std::min(max_steps_per_launch, kProbeMaxSteps) : kProbeMaxSteps;
    const bool vec = D % 4 == 0 && lde % 4 == 0 && aligned16(E);
    ProbeArgs a;
    a.E = E;
    a.lde = lde;
    a.D = static_cast<int>(D);
    a.C = static_cast<int>(C);
    a.batch = static_cast<int>(batch);
    a.n_train = static_cast<int>(n_train);
    a.spe = static_cast<int>(spe);
    a.labels = labels;
    a.order = order;
    a.params = params;
    a.lr = lr;
    a.max_norm = max_norm;
    a.snapshots = snapshots;
    a.losses = losses;
    a.L = probe_layout(D, C, batch, probe_ld(D, vec));
    GS_REQUIRE(a.L.floats > 0, GS_EINVAL, "shape unsupported (gs_cls_probe_supported)");
    probe_lds_ready();
    const uint32_t smem = static_cast<uint32_t>(a.L.floats) * 4u;
    hipStream_t st = as_stream(stream);
    for (int64_t g0 = 0; g0 < total; g0 += cut) {
        a.g0 = g0;
        a.g1 = std::min(total, g0 + cut);
        a.e0 = static_cast<int>(g0 / spe);
        a.s0 = static_cast<int>(g0 % spe);
        if (vec) cls_probe_kernel<true><<<dim3(1), kProbeThreads, smem, st>>>(a);
        else cls_probe_kernel<false><<<dim3(1), kProbeThreads, smem, st>>>(a);
        check_launch("gs_cls_probe_run");
    }
    GS_API_END
}

int gs_cls_probe_run(const float* E, int64_t lde, int64_t n_rows, int64_t D, int64_t C, const int32_t* labels,
                     const int32_t* order, int64_t n_train, int64_t batch, int64_t n_epochs, float* params,
                     float lr, float max_norm, float* snapshots, float* losses, void* stream) {
    return gs_cls_probe_run_ex(E, lde, n_rows, D, C, labels, order, n_train, batch, n_epochs, params, lr, max_norm,
                               snapshots, losses, 0, stream);
}

}  // extern "C"
