// The classifier head, forward only, for evaluation: over B rows of H gathered
// by id and n_sets parameter sets [Wc | bc],
//   z = H[r]·Wcᵀ + bc;  logp = z - max - log Σ exp(z - max)   (max-shifted, as torch)
//   pred = the lowest class index among the maxima of z (np.argmax: a NaN
//          counts as maximal, the first NaN wins)
//   nll  = -logp[y], y = labels[r]; a label outside [0, C) is counted in n_bad
//          and left out of the loss and of the confusion matrix
// into pred [n_sets][B], logp [n_sets][B][C] (both optional), loss [n_sets]
// (the mean NLL over the counted rows) and counts [n_sets][C·C + 2] int64 (the
// confusion matrix counts[y·C + pred], then n_counted and n_bad).  No backward
// output, no N-row buffer: it reads B·D floats per set and writes B class ids.
//
// Launch shape.  Rows are cut into chunks of kEvalChunk = 64 consecutive rows,
// a cut that depends on B alone.  A workgroup has kEvalWaves = 4 waves; wave w
// of workgroup b takes the chunks gw, gw + GW, ... (gw = 4 b + w, GW the
// waves of the grid), so the grid strides over the chunks and may have any
// size (at most kEvalMaxBlocks workgroups; blockIdx.y is the parameter set).
// A wave walks its chunks in groups of RW <= 4 rows: the group's rows sit in a
// wave-private LDS tile, and the next group's rows, labels and the ids of the
// group after it are loaded into registers while the current group is
// computed (the probe kernel's scheme), so each wave keeps RW rows in flight.
// The rows of a group are computed side by side: one read of a Wc element
// serves them all and their dependent chains (dot product, shuffles, exp, log)
// interleave; row after row the kernel was bound by that chain's latency.
// Per row, lane (cl, dq) = (lane & 15, lane >> 4) computes the dot product of
// class c0 + cl over one quarter of D, two xor-shuffles add the quarters, and
// the classes are walked in groups of 16 as the training head walks them
// (misc.hip).  float4 path: D % 4 == 0, ldh % 4 == 0 and H 16-byte aligned;
// otherwise every load is a scalar one.
//
// Determinism.  A row's values depend on (D, C) and its own operands alone.
// A wave adds its chunk's fp32 NLL terms in row order, in double, and stores
// one partial per (set, chunk) into the workspace; cls_eval_loss_kernel adds
// the partials of a set in an order fixed by their number (thread-strided,
// then the threads in order), divides by n_counted and rounds to fp32 once:
// the mean adds no error of its own to the terms'.  No floating-point
// atomics.  The counts are integers: a per-workgroup LDS histogram (C·C <=
// kEvalHistLds) stored once as a slab of the workspace, the slabs added by
// cls_eval_counts_kernel; beyond, 64-bit global atomics per row into counts
// zeroed by a launch in front.  Their result does not depend on the order.  Set s never reads
// anything of another set, so its outputs do not depend on n_sets.
//
// Budget (gfx950, kEvalThreads = 256).  LDS, in floats:
//   Wc    C·wp when C·(D + 4) <= kEvalWcLds (32 KiB): wp = D + 4 (float4 path: rows 16-byte aligned, a
//         wave's b128 reads of 16 classes on distinct slots for D % 8 == 0) or D | 1 (scalar path);
//         else Wc is read through the cache, row pitch D
//   bc    round4(C)
//   hist  C·C ints when C·C <= kEvalHistLds (16 KiB), + 2 counters
//   per wave: RW · (round4(D) + round4(C)): the tile and the group's logits
// at most 64 KiB in all (no raised launch limit); RW is the largest of 4, 2, 1
// that fits, a function of (D, C).  At D = 128: C = 16 takes 19 KiB and C = 47
// 45 KiB, so LDS allows three to eight workgroups per CU.  Registers allow
// three on the float4 path: the compiler's resource remark gives 129 VGPRs
// (four rows' accumulators and operands beside the prefetch; one over the
// 128 that would allow a fourth wave per SIMD) and 97 on the scalar path (four
// workgroups), no scratch.  So 3 waves per SIMD = 12 waves = three workgroups
// per CU, with 2 KiB of rows in flight per wave (24 KiB per CU).  Held to 128
// VGPRs by an attribute, an earlier form of the kernel spilled.
// The work is memory-bound (B·D·4 bytes per set); per row and class group the
// float4 path issues D/8 ds_read_b128 per lane (W and the broadcast row).
#include <algorithm>
#include <climits>
#include <cmath>

#include "kcommon.hpp"

namespace gs {

constexpr int kEvalThreads = 256;
constexpr int kEvalWaves = kEvalThreads / 64;
constexpr int kEvalChunk = 64;                 // rows per loss partial: the cut of the rows
constexpr int kEvalRowsMax = 4;                // rows per group (in flight per wave)
constexpr int kEvalPre = 4;                    // prefetched elements per lane
constexpr int kEvalMaxBlocks = 2048;          // workgroups per set (any value gives the same result)
constexpr int64_t kEvalWcLds = 8 * 1024;       // floats of LDS for Wc
constexpr int64_t kEvalHistLds = 4 * 1024;     // ints of LDS for the confusion matrix
constexpr int64_t kEvalLdsFloats = 16 * 1024;  // 64 KiB: the default launch limit
constexpr int kEvalRedThreads = 256;

inline int64_t eval_round4(int64_t x) { return (x + 3) & ~int64_t(3); }

struct EvalLayout {
    int rw;                              // rows per group; 0: does not fit
    int wc_lds, hist_lds;
    int wp;                              // row pitch of Wc where it is read
    int ld;                              // row pitch of the tile
    int oB, oHist, oCnt, oWave, wave_floats, floats;
};

// The layout with Wc in LDS (want_wc, and while it is within its budget) or read through the cache.
inline EvalLayout eval_layout_with(int64_t D, int64_t C, bool vec, bool want_wc) {
    EvalLayout L{};
    if (D < 1 || C < 1 || D > kEvalLdsFloats || C > kEvalLdsFloats) return L;
    L.wc_lds = want_wc && C * (D + 4) <= kEvalWcLds ? 1 : 0;
    L.hist_lds = C * C <= kEvalHistLds ? 1 : 0;
    L.wp = static_cast<int>(L.wc_lds ? (vec ? D + 4 : (D | 1)) : D);
    L.ld = static_cast<int>(eval_round4(D));
    const int64_t oB = L.wc_lds ? eval_round4(C * L.wp) : 0;
    const int64_t oHist = oB + eval_round4(C);
    const int64_t oCnt = oHist + (L.hist_lds ? eval_round4(C * C) : 0);
    const int64_t oWave = oCnt + 4;
    for (int rw = kEvalRowsMax; rw >= 1; rw >>= 1) {
        const int64_t wf = rw * (L.ld + eval_round4(C));
        if (oWave + kEvalWaves * wf <= kEvalLdsFloats) {
            L.rw = rw;
            L.oB = static_cast<int>(oB);
            L.oHist = static_cast<int>(oHist);
            L.oCnt = static_cast<int>(oCnt);
            L.oWave = static_cast<int>(oWave);
            L.wave_floats = static_cast<int>(wf);
            L.floats = static_cast<int>(oWave + kEvalWaves * wf);
            return L;
        }
    }
    return L;
}

// Wc in LDS where the wave tiles still fit beside it; else (a wide D with few
// classes) Wc through the cache; rw == 0 only when the tiles alone do not fit.
inline EvalLayout eval_layout(int64_t D, int64_t C, bool vec) {
    const EvalLayout L = eval_layout_with(D, C, vec, true);
    return L.rw >= 1 ? L : eval_layout_with(D, C, vec, false);
}

struct EvalArgs {
    const float* H;
    int64_t ldh;
    const int32_t* rows;    // NULL: row i
    const int32_t* labels;
    int labels_by_row;      // labels[rows[i]] (else labels[i])
    const float* params;    // set s at params + s · set_stride: Wc [C][D], then bc [C]
    int64_t set_stride;
    int64_t B;
    int D, C;
    int n_chunks;
    int32_t* pred;          // NULL or [n_sets][B]
    float* logp;            // NULL or [n_sets][B][C]
    unsigned long long* counts;  // [n_sets][C·C + 2]
    double* part;           // [n_sets][n_chunks]
    int* slab;              // [n_sets][workgroups][C·C + 2]: the workgroups' histograms (hist_lds)
    EvalLayout L;
};

template <bool VEC>
struct EvalElem;
template <>
struct EvalElem<true> {
    using T = float4;
    static constexpr int W = 4;
};
template <>
struct EvalElem<false> {
    using T = float;
    static constexpr int W = 1;
};

// (za, ca) before (zb, cb) in np.argmax's order: a NaN before any number, the
// larger value, then the lower index.
__device__ __forceinline__ bool eval_better(float za, int ca, float zb, int cb) {
    const bool na = za != za, nb = zb != zb;
    if (na != nb) return na;
    if (na) return ca < cb;
    return za > zb || (za == zb && ca < cb);
}

template <bool VEC>
__global__ __launch_bounds__(kEvalThreads) void cls_eval_rows_kernel(const EvalArgs a) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    using T = typename EvalElem<VEC>::T;
    constexpr int W = EvalElem<VEC>::W;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform: the group bookkeeping stays scalar
    const int cl = lane & 15, dq = lane >> 4;
    const int D = a.D, C = a.C, RW = a.L.rw;
    const int DW = D / W;         // elements per row
    const int LDW = a.L.ld / W;   // elements per tile row
    const int wp = a.L.wp;
    const int set = blockIdx.y;
    const int64_t B = a.B;
    const float* const Wg = a.params + static_cast<int64_t>(set) * a.set_stride;
    const float* const bg = Wg + static_cast<int64_t>(C) * D;
    float* const sW = sm;
    float* const sB = sm + a.L.oB;
    int* const hist = reinterpret_cast<int*>(sm + a.L.oHist);
    int* const cnt = reinterpret_cast<int*>(sm + a.L.oCnt);
    float* const tilef = sm + a.L.oWave + wave * a.L.wave_floats;
    T* const tile = reinterpret_cast<T*>(tilef);
    float* const zbuf = tilef + RW * a.L.ld;  // [RW][CP]: the group's logits
    const int CP = (C + 3) & ~3;
    unsigned long long* const counts = a.counts + static_cast<int64_t>(set) * (static_cast<int64_t>(C) * C + 2);

    // ---- the workgroup's image: Wc (when it fits), bc, an empty histogram
    if (a.L.wc_lds)
        for (int t = tid; t < C * D; t += kEvalThreads) {
            const int c = t / D;
            sW[c * wp + (t - c * D)] = Wg[t];
        }
    for (int t = tid; t < C; t += kEvalThreads) sB[t] = bg[t];
    if (a.L.hist_lds)
        for (int t = tid; t < C * C; t += kEvalThreads) hist[t] = 0;
    if (tid < 2) cnt[tid] = 0;
    __syncthreads();
    const float* const Wsrc = a.L.wc_lds ? sW : Wg;

    // ---- this wave's groups: group j is rows [row0, row0 + n) of chunk gw + (j / GPC) · GW
    const int GW = static_cast<int>(gridDim.x) * kEvalWaves, gw = static_cast<int>(blockIdx.x) * kEvalWaves + wave;
    const int GPC = kEvalChunk / RW;                       // groups per chunk, a power of two:
    const int gsh = RW == 4 ? 4 : (RW == 2 ? 5 : 6);       // j / GPC = j >> gsh, j % GPC = j & (GPC - 1)
    const int nch = gw < a.n_chunks ? (a.n_chunks - gw + GW - 1) / GW : 0;
    const int n_groups = nch * GPC;
    auto row0_of = [&](int j) {
        return (static_cast<int64_t>(gw) + static_cast<int64_t>(j >> gsh) * GW) * kEvalChunk + (j & (GPC - 1)) * RW;
    };
    auto rows_of = [&](int j) {  // 0 for a group past B (the last chunk's tail) and past the wave's last group
        if (j >= n_groups) return 0;
        const int64_t left = B - row0_of(j);
        return static_cast<int>(left < 0 ? 0 : (left < RW ? left : RW));
    };
    // lane l holds the id of row (l & (RW - 1)) of a group (address clamped: a row past the group repeats one)
    auto lane_row = [&](int j) {
        const int64_t r = row0_of(j) + (lane & (RW - 1));
        return r < B ? r : B - 1;
    };
    auto ids_of = [&](int j) {
        const int64_t r = lane_row(j);
        return a.rows ? a.rows[r] : static_cast<int>(r);
    };
    auto label_of = [&](int j, int id) { return a.labels[a.labels_by_row ? static_cast<int64_t>(id) : lane_row(j)]; };
    auto row_ptr = [&](int id, int col) {
        return reinterpret_cast<const T*>(a.H + static_cast<int64_t>(id) * a.ldh) + col;
    };
    // this lane's prefetch items (row, column) of any group: fixed by the shape
    int pr[kEvalPre], pc[kEvalPre];
#pragma unroll
    for (int k = 0; k < kEvalPre; ++k) {
        const int q = lane + 64 * k;
        pr[k] = q / DW;
        pc[k] = q - pr[k] * DW;
    }

    T pv[kEvalPre];
#pragma unroll
    for (int k = 0; k < kEvalPre; ++k) {
        if constexpr (VEC) pv[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        else pv[k] = 0.f;
    }
    int id_cur = 0, y_cur = 0, id_next = 0;
    if (n_groups > 0) {  // prologue: group 0's ids, rows and labels, group 1's ids
        id_cur = ids_of(0);
        const int n0 = rows_of(0);
        if (n0 > 0) {
#pragma unroll
            for (int k = 0; k < kEvalPre; ++k)
                if (64 * k < RW * DW) pv[k] = *row_ptr(__shfl(id_cur, min(pr[k], n0 - 1), 64), pc[k]);
            y_cur = label_of(0, id_cur);
        }
        if (rows_of(1) > 0) id_next = ids_of(1);
    }

    double acc = 0.0;  // the chunk's NLL sum, wave-uniform (fp32 terms added in double: the sum adds no error)
    int n_cnt = 0, n_bad = 0;
    const int DQ = (DW + 3) / 4;
    const int d_lo = min(DW, dq * DQ), d_hi = min(DW, d_lo + DQ);
    for (int j = 0; j < n_groups; ++j) {
        const int n = rows_of(j), n1 = rows_of(j + 1), n2 = rows_of(j + 2);
        const int64_t row0 = row0_of(j);
        // ---- group j into the tile (its loads were issued one iteration ago)
#pragma unroll
        for (int k = 0; k < kEvalPre; ++k)
            if (pr[k] < n) tile[pr[k] * LDW + pc[k]] = pv[k];
        for (int q0 = 64 * kEvalPre; q0 < n * DW; q0 += 64) {  // rows past the prefetch's reach (every lane shuffles)
            const int q = q0 + lane, r = min(q / DW, n - 1), c = q - (q / DW) * DW;
            const int id = __shfl(id_cur, r, 64);
            if (q < n * DW) tile[r * LDW + c] = *row_ptr(id, c);
        }
        const int y_grp = y_cur;
        // ---- group j + 1's rows and labels, group j + 2's ids: in flight during the compute
        int y_next = 0, id_next2 = 0;
        if (n1 > 0) {
#pragma unroll
            for (int k = 0; k < kEvalPre; ++k)  // (a wave-uniform test: no load for a k past the group's last element)
                if (64 * k < RW * DW) pv[k] = *row_ptr(__shfl(id_next, min(pr[k], n1 - 1), 64), pc[k]);
            y_next = label_of(j + 1, id_next);
        }
        if (n2 > 0) id_next2 = ids_of(j + 2);
        __builtin_amdgcn_wave_barrier();

        if (n > 0) {
            // the group's rows side by side: one read of a Wc element serves them all, and their
            // dependent chains (dot product, shuffles, exp, log) interleave.  Slot q >= n works on a
            // repeated row and writes nothing.
            constexpr int R = kEvalRowsMax;
            const T* e[R];
            float bz[R];
            int bcx[R];
#pragma unroll
            for (int q = 0; q < R; ++q) {
                e[q] = tile + min(q, n - 1) * LDW;
                bz[q] = -INFINITY;
                bcx[q] = INT_MAX;
            }
            for (int c0 = 0; c0 < C; c0 += 16) {
                const int c = c0 + cl;
                const T* wr = reinterpret_cast<const T*>(Wsrc + static_cast<int64_t>(min(c, C - 1)) * wp);
                float p[R];
                if constexpr (VEC) {
                    float4 s4[R];
#pragma unroll
                    for (int q = 0; q < R; ++q) s4[q] = make_float4(0.f, 0.f, 0.f, 0.f);
                    for (int d = d_lo; d < d_hi; ++d) {
                        const float4 wv = wr[d];
#pragma unroll
                        for (int q = 0; q < R; ++q) {
                            const float4 ev = e[q][d];
                            s4[q].x = fmaf(ev.x, wv.x, s4[q].x);
                            s4[q].y = fmaf(ev.y, wv.y, s4[q].y);
                            s4[q].z = fmaf(ev.z, wv.z, s4[q].z);
                            s4[q].w = fmaf(ev.w, wv.w, s4[q].w);
                        }
                    }
#pragma unroll
                    for (int q = 0; q < R; ++q) p[q] = (s4[q].x + s4[q].y) + (s4[q].z + s4[q].w);
                } else {
#pragma unroll
                    for (int q = 0; q < R; ++q) p[q] = 0.f;
                    for (int d = d_lo; d < d_hi; ++d) {
                        const float wv = wr[d];
#pragma unroll
                        for (int q = 0; q < R; ++q) p[q] = fmaf(e[q][d], wv, p[q]);
                    }
                }
#pragma unroll
                for (int q = 0; q < R; ++q) p[q] += __shfl_xor(p[q], 16, 64);
#pragma unroll
                for (int q = 0; q < R; ++q) p[q] += __shfl_xor(p[q], 32, 64);
                const float bias = sB[min(c, C - 1)];
#pragma unroll
                for (int q = 0; q < R; ++q) {
                    const float z = p[q] + bias;
                    if (dq == 0 && c < C && q < n) zbuf[q * CP + c] = z;
                    if (c < C && eval_better(z, c, bz[q], bcx[q])) {
                        bz[q] = z;
                        bcx[q] = c;
                    }
                }
            }
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) {
#pragma unroll
                for (int q = 0; q < R; ++q) {
                    const float oz = __shfl_xor(bz[q], o, 64);
                    const int oc = __shfl_xor(bcx[q], o, 64);
                    if (eval_better(oz, oc, bz[q], bcx[q])) {
                        bz[q] = oz;
                        bcx[q] = oc;
                    }
                }
            }
            // bz[q]: the row's maximum (a NaN makes every logp of the row a NaN, as torch)
            __builtin_amdgcn_wave_barrier();
            float lse[R];
#pragma unroll
            for (int q = 0; q < R; ++q) {
                const float* zr = zbuf + min(q, n - 1) * CP;
                float se = 0.f;
                for (int c = lane; c < C; c += 64) se += expf(zr[c] - bz[q]);
                lse[q] = se;
            }
#pragma unroll
            for (int q = 0; q < R; ++q) lse[q] = logf(wave_sum(lse[q]));
#pragma unroll
            for (int q = 0; q < R; ++q) {
                if (q < n) {
                    const float* zr = zbuf + q * CP;
                    const int64_t i = row0 + q;
                    const float mx = bz[q];
                    if (a.logp) {
                        float* out = a.logp + (static_cast<int64_t>(set) * B + i) * C;
                        for (int c = lane; c < C; c += 64) out[c] = (zr[c] - mx) - lse[q];
                    }
                    const int y = __shfl(y_grp, q, 64);
                    const bool has = static_cast<unsigned>(y) < static_cast<unsigned>(C);
                    if (has) {
                        acc += static_cast<double>(-((zr[y] - mx) - lse[q]));
                        ++n_cnt;
                    } else {
                        ++n_bad;
                    }
                    if (lane == 0) {
                        if (a.pred) a.pred[static_cast<int64_t>(set) * B + i] = bcx[q];
                        if (has) {
                            const int64_t cell = static_cast<int64_t>(y) * C + bcx[q];
                            if (a.L.hist_lds) atomicAdd(hist + cell, 1);
                            else atomicAdd(counts + cell, 1ull);
                        }
                    }
                }
            }
            __builtin_amdgcn_wave_barrier();  // zbuf is rewritten by the next group
        }
        if ((j & (GPC - 1)) == GPC - 1) {  // the chunk's last group: its partial
            if (lane == 0) a.part[static_cast<int64_t>(set) * a.n_chunks + (gw + (j >> gsh) * GW)] = acc;
            acc = 0.0;
        }
        id_cur = id_next;
        id_next = id_next2;
        y_cur = y_next;
    }

    if (lane == 0) {
        if (n_cnt) atomicAdd(cnt, n_cnt);
        if (n_bad) atomicAdd(cnt + 1, n_bad);
    }
    __syncthreads();
    const int CC = C * C;
    if (a.L.hist_lds) {
        // the workgroup's histogram and counters as one slab of plain stores; cls_eval_counts_kernel
        // adds the slabs.  (Flushed with global atomics, every workgroup of a 1 M-row call added
        // into the same few cache lines, and the launch's tail waited for them.)
        int* out = a.slab + (static_cast<int64_t>(set) * gridDim.x + blockIdx.x) * (CC + 2);
        for (int t = tid; t < CC; t += kEvalThreads) out[t] = hist[t];
        if (tid < 2) out[CC + tid] = cnt[tid];
    } else if (tid < 2 && cnt[tid]) {
        atomicAdd(counts + CC + tid, static_cast<unsigned long long>(cnt[tid]));
    }
}

__global__ __launch_bounds__(256) void cls_eval_zero_kernel(unsigned long long* __restrict__ counts, int64_t n) {
    for (int64_t i = blockIdx.x * int64_t(256) + threadIdx.x; i < n; i += int64_t(gridDim.x) * 256) counts[i] = 0ull;
}

// counts[set][t] = Σ over the workgroups' slabs of cell t (integers: any order gives the same sum).
__global__ __launch_bounds__(256) void cls_eval_counts_kernel(int nb, int64_t CC, const int* __restrict__ slab,
                                                              unsigned long long* __restrict__ counts) {
    const int64_t t = blockIdx.x * int64_t(256) + threadIdx.x;
    if (t >= CC + 2) return;
    const int set = blockIdx.y;
    const int* p = slab + static_cast<int64_t>(set) * nb * (CC + 2) + t;
    unsigned long long s = 0;
#pragma unroll 8
    for (int b = 0; b < nb; ++b) s += static_cast<unsigned long long>(p[static_cast<int64_t>(b) * (CC + 2)]);
    counts[set * (CC + 2) + t] = s;
}

// loss[set] = Σ of the set's chunk partials / n_counted, in double and
// rounded to fp32 once: thread-strided in chunk order, then the threads'
// sums in thread order.  0 rows counted: NaN.
__global__ __launch_bounds__(kEvalRedThreads) void cls_eval_loss_kernel(int n_chunks, int64_t CC,
                                                                        const double* __restrict__ part,
                                                                        const unsigned long long* __restrict__ counts,
                                                                        float* __restrict__ loss) {
    __shared__ double red[kEvalRedThreads];
    const int set = blockIdx.x;
    const double* p = part + static_cast<int64_t>(set) * n_chunks;
    double s = 0.0;
    for (int k = threadIdx.x; k < n_chunks; k += kEvalRedThreads) s += p[k];
    red[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int w = 0; w < kEvalRedThreads; ++w) t += red[w];
        const unsigned long long n = counts[set * (CC + 2) + CC];
        loss[set] = n ? static_cast<float>(t / static_cast<double>(n)) : __builtin_nanf("");
    }
}

inline int64_t eval_chunks(int64_t B) { return (B + kEvalChunk - 1) / kEvalChunk; }
// Workgroups per set: a function of B alone (and no result depends on it).
inline int64_t eval_blocks(int64_t B) {
    return std::min<int64_t>(kEvalMaxBlocks, (eval_chunks(B) + kEvalWaves - 1) / kEvalWaves);
}
inline int64_t eval_round16(int64_t x) { return (x + 15) / 16 * 16; }
// The workspace: the loss partials (doubles), then the workgroups' histogram slabs where C·C fits LDS.
inline int64_t eval_part_bytes(int64_t B, int64_t n_sets) { return eval_round16(n_sets * eval_chunks(B) * 8); }
inline int64_t eval_slab_bytes(int64_t B, int64_t C, int64_t n_sets) {
    return C * C <= kEvalHistLds ? eval_round16(n_sets * eval_blocks(B) * (C * C + 2) * 4) : 0;
}

}  // namespace gs

extern "C" {

int64_t gs_cls_eval_wc_lds_floats(void) { return gs::kEvalWcLds; }

int64_t gs_cls_eval_ws_bytes(int64_t B, int64_t D, int64_t C, int64_t n_sets) {
    GS_BYTES_BEGIN
    GS_REQUIRE(B >= 1 && D >= 1 && C >= 1 && n_sets >= 1, GS_EINVAL, "sizes must be >= 1");
    GS_REQUIRE(B < (int64_t(1) << 31) && n_sets < (int64_t(1) << 16), GS_EINVAL, "B < 2^31 and n_sets < 2^16");
    return gs::eval_part_bytes(B, n_sets) + gs::eval_slab_bytes(B, C, n_sets);
    GS_BYTES_END
}

int gs_cls_eval(int64_t B, int64_t D, int64_t C, const float* H, int64_t ldh, const int32_t* rows,
                const int32_t* labels, int32_t labels_by_row, const float* params, int64_t n_sets,
                int64_t set_stride, int32_t* pred, float* logp, float* loss, int64_t* counts, void* ws,
                int64_t ws_bytes, void* stream) {
    GS_API_BEGIN
    using namespace gs;
    GS_REQUIRE(H && labels && params && loss && counts && ws, GS_EINVAL, "NULL mandatory pointer");
    GS_REQUIRE(B >= 1 && D >= 1 && C >= 1 && n_sets >= 1, GS_EINVAL, "sizes must be >= 1");
    GS_REQUIRE(B < (int64_t(1) << 31) && n_sets < (int64_t(1) << 16), GS_EINVAL, "B < 2^31 and n_sets < 2^16");
    GS_REQUIRE(ldh >= D, GS_EINVAL, "ldh < D");
    GS_REQUIRE(C <= 46340 && D <= kEvalLdsFloats, GS_EINVAL, "C·C must fit an int32, D the LDS");
    GS_REQUIRE(set_stride >= C * D + C, GS_EINVAL, "set_stride < C*D + C");
    const int64_t need = gs_cls_eval_ws_bytes(B, D, C, n_sets);
    GS_REQUIRE(need > 0 && ws_bytes >= need, GS_EINVAL, "workspace shorter than gs_cls_eval_ws_bytes");
    GS_REQUIRE(aligned16(ws), GS_EINVAL, "workspace not 16-byte aligned");
    const bool vec_h = D % 4 == 0 && ldh % 4 == 0 && aligned16(H);
    // with D % 4 == 0: every Wc row of every set on a 16-byte boundary.  The stride counts for one set too, so
    // that the load path is a property of (params, set_stride), not of how many sets ride along.
    const bool vec_w = aligned16(params) && set_stride % 4 == 0;
    bool vec = vec_h;
    EvalLayout L = eval_layout(D, C, vec);
    if (vec && !L.wc_lds && !vec_w) {  // Wc is read from memory and its rows are not 16-byte aligned
        vec = false;
        L = eval_layout(D, C, vec);
    }
    GS_REQUIRE(L.rw >= 1, GS_EINVAL, "D + C too large for the workgroup's LDS");
    EvalArgs a;
    a.H = H;
    a.ldh = ldh;
    a.rows = rows;
    a.labels = labels;
    a.labels_by_row = labels_by_row && rows ? 1 : 0;
    a.params = params;
    a.set_stride = set_stride;
    a.B = B;
    a.D = static_cast<int>(D);
    a.C = static_cast<int>(C);
    a.n_chunks = static_cast<int>(eval_chunks(B));
    a.pred = pred;
    a.logp = logp;
    a.counts = reinterpret_cast<unsigned long long*>(counts);
    a.part = static_cast<double*>(ws);
    a.slab = reinterpret_cast<int*>(static_cast<char*>(ws) + eval_part_bytes(B, n_sets));
    a.L = L;
    hipStream_t st = as_stream(stream);
    const int64_t CC = C * C, n_counts = n_sets * (CC + 2);
    const int nb = static_cast<int>(eval_blocks(B));
    if (!L.hist_lds) {  // the counts are added into with integer atomics: zeroed by a launch in front
        cls_eval_zero_kernel<<<dim3(static_cast<unsigned>(std::min<int64_t>((n_counts + 255) / 256, 1024))), 256, 0,
                               st>>>(a.counts, n_counts);
        check_launch("gs_cls_eval: zero");
    }
    const dim3 grid(static_cast<unsigned>(nb), static_cast<unsigned>(n_sets));
    const uint32_t smem = static_cast<uint32_t>(L.floats) * 4u;
    if (vec) cls_eval_rows_kernel<true><<<grid, kEvalThreads, smem, st>>>(a);
    else cls_eval_rows_kernel<false><<<grid, kEvalThreads, smem, st>>>(a);
    check_launch("gs_cls_eval: rows");
    if (L.hist_lds) {
        cls_eval_counts_kernel<<<dim3(static_cast<unsigned>((CC + 2 + 255) / 256), static_cast<unsigned>(n_sets)), 256,
                                 0, st>>>(nb, CC, a.slab, a.counts);
        check_launch("gs_cls_eval: counts");
    }
    cls_eval_loss_kernel<<<dim3(static_cast<unsigned>(n_sets)), kEvalRedThreads, 0, st>>>(
        a.n_chunks, C * C, a.part, a.counts, loss);
    check_launch("gs_cls_eval: loss");
    GS_API_END
}

}  // extern "C"
