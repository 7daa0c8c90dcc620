// The multi-label classifier head: C independent sigmoid outputs per row under
// the binary cross-entropy of torch's binary_cross_entropy_with_logits (mean,
// optional pos_weight), fused forward + backward for training
// (gs_cls_bce_fwd_bwd) and forward only for evaluation (gs_cls_bce_eval).
//   z = E·Wcᵀ + bc
//   l = (1 - y)·z + (1 + (pw - 1)·y)·(log1p(exp(-|z|)) + max(-z, 0))     (no term overflows)
//   loss = Σ l / (B·C)
//   dz = (σ(z)·(1 + (pw - 1)·y) - pw·y) / (B·C);  dE = dz·Wc (relu-masked);  dWc = dzᵀ·E;  dbc = Σ_rows dz
// Targets are hard 0/1 bits: node v owns nW = ceil(C / 32) int32 words, label c
// is bit c % 32 of word c / 32; bits at or above C are never looked at.
//
// Launch shape.  A workgroup of kBceThreads = 256 threads (4 waves) stages Wc
// once, zero-padded to CP = round16(C) labels by D16 = round16(D) columns with
// a row pitch of WP = D16 + 4 floats, then walks the row tiles b, b + G, ... of
// kBceRows = 16 rows (G workgroups, a function of B alone).  Per tile, with
// barriers in between:
//   logits  wave w takes the label groups w, w + 4, ... of 16 labels: z on
//           v_mfma_f32_16x16x4_f32 (A = the tile's rows, B = Wc, both as b128
//           LDS reads: lane quarter q owns the columns 16 ch + 4 q .. + 3 of
//           chunk ch, a fixed permutation of the k order), the loss term and
//           dz on the accumulator registers (lane (j, q) = (lane & 15,
//           lane >> 4) holds rows 4 q .. 4 q + 3 of label c0 + j), dz to an LDS
//           tile [16][ZP = CP + 4]
//   dE      wave w takes the column tiles w, w + 4, ... of 16 columns:
//           dE = dz·Wc (A = the dz tile, B = Wc read by column), masked by the
//           tile's own E and stored from the accumulator (16 lanes = 64 bytes
//           of a row)
//   dWc     the (label group, column tile) pairs, with one extra column tile
//           per label group whose B operand is the constant 1 (its column 0 is
//           dbc), are dealt to the waves in turn; A = the dz tile read in the
//           accumulator's own layout, B = the rows' columns; the accumulators
//           live in registers over all the workgroup's tiles (NT tiles per
//           wave: the kernel is instantiated for NT = 1, 3, 5, 9, 18, 36)
// The pitches keep the scalar operand reads conflict-free: 4·WP and 4·ZP are
// 16 mod 32 banks, so the two lane quarters of a 32-lane half read disjoint
// bank halves.  The next tile's rows (8 floats per thread: D16 <= 128) and
// target words are loaded into registers before the current tile's compute.
//
// Determinism.  Every sum has an order fixed by (B, D, C): the k order of the
// MFMA chains, each lane's loss terms (fp32 per tile, added in double over the
// tiles), one slab of [CP][D16 + 16] partials and one double per workgroup, and
// a second launch that adds the slabs in workgroup order (four consecutive
// quarters, then the quarters in order).  No floating-point atomics.
//
// Budget.  LDS in floats: CP·WP (Wc) + 2·CP (bc, pos_weight) + 16·WP (rows) +
// 16·ZP (dz) + 2·16·nW (targets, predictions) + 3·CP (the evaluation's counts)
// + 16 <= 40960 (160 KiB), and CP/16 · (D16/16 + 1) <= 144 accumulator tiles
// (36 per wave = 144 registers).  D = 128 with C = 128 takes 86 KiB, D = 256
// with C = 128 158 KiB.
//
// The evaluation kernel shares the staging and the logits; its rows are
// gathered by id, the predicted bit is z > 0, and the per-label counts (true
// positives, false positives, false negatives) and the exactly-right rows are
// integer sums over LDS images of the target and prediction words.
#include <algorithm>
#include <cmath>
#include <mutex>

#include "kcommon.hpp"

namespace gs {

constexpr int kBceThreads = 256;
constexpr int kBceWaves = kBceThreads / 64;
constexpr int kBceRows = 16;
constexpr int kBcePre = 8;                    // prefetched row elements per thread
constexpr int kBceMaxBlocks = 512;            // workgroups (a cap on the slabs; the result depends on B, not on it)
constexpr int64_t kBceLdsFloats = 40 * 1024;  // 160 KiB
constexpr int kBceMaxTiles = 144;             // dWc accumulator tiles per workgroup
constexpr int kBceRedThreads = 256;

inline int64_t bce_round16(int64_t x) { return (x + 15) & ~int64_t(15); }

struct BceLayout {
    int ok;
    int D16, CP, WP, ZP, nW, nDT, nCG;
    int oB, oPW, oE, oZ, oY, oP, oCnt, oMisc, floats;
};

inline BceLayout bce_layout(int64_t D, int64_t C) {
    BceLayout L{};
    if (D < 1 || C < 1 || D > 8192 || C > 8192) return L;
    const int64_t D16 = bce_round16(D), CP = bce_round16(C), WP = D16 + 4, ZP = CP + 4, nW = (C + 31) / 32;
    const int64_t oB = CP * WP, oPW = oB + CP, oE = oPW + CP, oZ = oE + kBceRows * WP, oY = oZ + kBceRows * ZP;
    const int64_t oP = oY + kBceRows * nW, oCnt = oP + kBceRows * nW;
    const int64_t oMisc = (oCnt + 3 * CP + 3) & ~int64_t(3), floats = oMisc + 16;
    if (floats > kBceLdsFloats || (CP / 16) * (D16 / 16 + 1) > kBceMaxTiles) return L;
    L.ok = 1;
    L.D16 = static_cast<int>(D16);
    L.CP = static_cast<int>(CP);
    L.WP = static_cast<int>(WP);
    L.ZP = static_cast<int>(ZP);
    L.nW = static_cast<int>(nW);
    L.nDT = static_cast<int>(D16 / 16);
    L.nCG = static_cast<int>(CP / 16);
    L.oB = static_cast<int>(oB);
    L.oPW = static_cast<int>(oPW);
    L.oE = static_cast<int>(oE);
    L.oZ = static_cast<int>(oZ);
    L.oY = static_cast<int>(oY);
    L.oP = static_cast<int>(oP);
    L.oCnt = static_cast<int>(oCnt);
    L.oMisc = static_cast<int>(oMisc);
    L.floats = static_cast<int>(floats);
    return L;
}

inline int64_t bce_tiles(int64_t B) { return (B + kBceRows - 1) / kBceRows; }
inline int64_t bce_blocks(int64_t B) { return std::min<int64_t>(bce_tiles(B), kBceMaxBlocks); }
inline int64_t bce_slab_floats(const BceLayout& L) { return static_cast<int64_t>(L.CP) * (L.D16 + 16); }
inline int64_t bce_part_bytes(int64_t B) { return bce_round16(bce_blocks(B) * 8); }

struct BceArgs {
    const float* X;          // rows: row i of the call is X[ids ? ids[i] : i]
    int64_t ldx;
    const int32_t* ids;
    const int32_t* tids;     // targets of row i: node tids ? tids[i] : i
    const int32_t* targets;  // [*, nW]
    const float* Wc;
    const float* bc;
    const float* pw;         // NULL: ones
    int64_t B;
    int D, C;
    int mask_relu;
    float inv_n;             // 1 / (B·C)
    float* dE;               // [B, D] (training)
    float* slab;             // [blocks][CP][D16 + 16] (training)
    double* lpart;           // [blocks]
    int32_t* pred;           // NULL or [B, nW] (evaluation)
    float* logits;           // NULL or [B, C] (evaluation)
    int* cslab;              // [blocks][3·C + 1] (evaluation)
    BceLayout L;
};

// Wc (zero-padded), bc and pos_weight into the workgroup's LDS.
__device__ __forceinline__ void bce_stage_params(const BceArgs& a, float* sm) {
    const int tid = threadIdx.x, WP = a.L.WP, CP = a.L.CP;
    for (int t = tid; t < CP * WP; t += kBceThreads) {
        const int c = t / WP, d = t - c * WP;
        sm[t] = (c < a.C && d < a.D) ? a.Wc[static_cast<int64_t>(c) * a.D + d] : 0.f;
    }
    for (int t = tid; t < CP; t += kBceThreads) {
        sm[a.L.oB + t] = t < a.C ? a.bc[t] : 0.f;
        sm[a.L.oPW + t] = (t < a.C && a.pw) ? a.pw[t] : 1.f;
    }
}

// A row tile on its way from memory to LDS: the first kBcePre elements per thread and one target word.
struct BceTile {
    float v[kBcePre];
    int y;
};

__device__ __forceinline__ int64_t bce_src_row(const BceArgs& a, int64_t row) {
    return a.ids ? static_cast<int64_t>(a.ids[row]) : row;
}
__device__ __forceinline__ int bce_target_word(const BceArgs& a, int64_t row, int w) {
    const int64_t node = a.tids ? static_cast<int64_t>(a.tids[row]) : row;
    return a.targets[node * a.L.nW + w];
}

__device__ __forceinline__ void bce_tile_issue(const BceArgs& a, int64_t row0, const int (&pr)[kBcePre],
                                               const int (&pc)[kBcePre], BceTile& t) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int k = 0; k < kBcePre; ++k) {
        const int64_t row = row0 + pr[k];
        t.v[k] = 0.f;
        if (pr[k] < kBceRows && row < a.B && pc[k] < a.D) t.v[k] = a.X[bce_src_row(a, row) * a.ldx + pc[k]];
    }
    t.y = 0;
    if (tid < kBceRows * a.L.nW) {
        const int r = tid / a.L.nW, w = tid - r * a.L.nW;
        if (row0 + r < a.B) t.y = bce_target_word(a, row0 + r, w);
    }
}

// The tile into LDS: zero-padded rows [16][WP], the target words [16][nW], the prediction words cleared.
__device__ __forceinline__ void bce_tile_commit(const BceArgs& a, int64_t row0, const int (&pr)[kBcePre],
                                                const int (&pc)[kBcePre], const BceTile& t, float* sm) {
    const int tid = threadIdx.x, WP = a.L.WP, D16 = a.L.D16, nW = a.L.nW;
    float* sE = sm + a.L.oE;
    int* sY = reinterpret_cast<int*>(sm + a.L.oY);
    int* sP = reinterpret_cast<int*>(sm + a.L.oP);
#pragma unroll
    for (int k = 0; k < kBcePre; ++k)
        if (pr[k] < kBceRows) sE[pr[k] * WP + pc[k]] = t.v[k];
    for (int e = tid + kBceThreads * kBcePre; e < kBceRows * D16; e += kBceThreads) {  // D16 > 128: the rest
        const int r = e / D16, c = e - r * D16;
        const int64_t row = row0 + r;
        sE[r * WP + c] = (row < a.B && c < a.D) ? a.X[bce_src_row(a, row) * a.ldx + c] : 0.f;
    }
    if (tid < kBceRows * nW) {
        sY[tid] = t.y;
        sP[tid] = 0;
    }
    for (int e = tid + kBceThreads; e < kBceRows * nW; e += kBceThreads) {  // C > 512: the rest
        const int r = e / nW, w = e - r * nW;
        sY[e] = row0 + r < a.B ? bce_target_word(a, row0 + r, w) : 0;
        sP[e] = 0;
    }
}

// z[row 4 q + reg][label c0 + j] of the tile, without the bias.
__device__ __forceinline__ f32x4 bce_logits(const float* sE, const float* sW, int WP, int nDT, int c0, int j, int q) {
    f32x4 a0 = f32x4{0.f, 0.f, 0.f, 0.f}, a1 = a0;
    const float* ep = sE + j * WP + 4 * q;
    const float* wp = sW + (c0 + j) * WP + 4 * q;
    int ch = 0;
    for (; ch + 1 < nDT; ch += 2) {
        const float4 e0 = *reinterpret_cast<const float4*>(ep + 16 * ch);
        const float4 w0 = *reinterpret_cast<const float4*>(wp + 16 * ch);
        const float4 e1 = *reinterpret_cast<const float4*>(ep + 16 * ch + 16);
        const float4 w1 = *reinterpret_cast<const float4*>(wp + 16 * ch + 16);
        a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(e0.x, w0.x, a0, 0, 0, 0);
        a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(e1.x, w1.x, a1, 0, 0, 0);
        a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(e0.y, w0.y, a0, 0, 0, 0);
        a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(e1.y, w1.y, a1, 0, 0, 0);
        a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(e0.z, w0.z, a0, 0, 0, 0);
        a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(e1.z, w1.z, a1, 0, 0, 0);
        a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(e0.w, w0.w, a0, 0, 0, 0);
        a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(e1.w, w1.w, a1, 0, 0, 0);
    }
    if (ch < nDT) {
        const float4 e0 = *reinterpret_cast<const float4*>(ep + 16 * ch);
        const float4 w0 = *reinterpret_cast<const float4*>(wp + 16 * ch);
        a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(e0.x, w0.x, a0, 0, 0, 0);
        a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(e0.y, w0.y, a0, 0, 0, 0);
        a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(e0.z, w0.z, a0, 0, 0, 0);
        a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(e0.w, w0.w, a0, 0, 0, 0);
    }
    return a0 + a1;
}

// One element's loss term and (unscaled) dz: torch's stable form; e = exp(-|z|) <= 1, so nothing overflows.
__device__ __forceinline__ void bce_elem(float z, bool y, float pw, float& l, float& g) {
    const float e = expf(-fabsf(z));
    const float sp = log1pf(e) + fmaxf(-z, 0.f);  // softplus(-z) = -log σ(z)
    const float r = 1.f / (1.f + e);
    if (y) {
        l = pw * sp;
        g = -pw * ((z >= 0.f ? e : 1.f) * r);  // -pw·(1 - σ(z))
    } else {
        l = z + sp;
        g = (z >= 0.f ? 1.f : e) * r;          // σ(z)
    }
}

// The workgroup's loss partial: the lanes' doubles added by a fixed xor tree, then the waves in order.
__device__ __forceinline__ void bce_loss_partial(double dl, float* sm, int oMisc, double* out) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) dl += __shfl_xor(dl, o, 64);
    double* red = reinterpret_cast<double*>(sm + oMisc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = dl;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int w = 0; w < kBceWaves; ++w) t += red[w];
        *out = t;
    }
}

__device__ __forceinline__ void bce_pre_map(int D16, int (&pr)[kBcePre], int (&pc)[kBcePre]) {
#pragma unroll
    for (int k = 0; k < kBcePre; ++k) {
        const int e = threadIdx.x + kBceThreads * k;
        pr[k] = e / D16;  // >= 16: past the tile
        pc[k] = e - pr[k] * D16;
    }
}

template <int NT>
__global__ __launch_bounds__(kBceThreads) void cls_bce_train_kernel(const BceArgs a) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 15, q = lane >> 4;
    const int WP = a.L.WP, ZP = a.L.ZP, nW = a.L.nW, nDT = a.L.nDT, nCG = a.L.nCG, D = a.D, C = a.C;
    const float* sW = sm;
    const float* sB = sm + a.L.oB;
    const float* sPW = sm + a.L.oPW;
    const float* sE = sm + a.L.oE;
    float* sZ = sm + a.L.oZ;
    const int* sY = reinterpret_cast<const int*>(sm + a.L.oY);
    const int64_t B = a.B;
    const int64_t n_tiles = (B + kBceRows - 1) / kBceRows;
    const int nT = nCG * (nDT + 1);                      // dWc tiles of the workgroup
    const int nt = (nT - wave + kBceWaves - 1) / kBceWaves;  // this wave's (<= NT)

    int pr[kBcePre], pc[kBcePre];
    bce_pre_map(a.L.D16, pr, pc);
    BceTile pre;
    int64_t tile = blockIdx.x;
    if (tile < n_tiles) bce_tile_issue(a, tile * kBceRows, pr, pc, pre);
    bce_stage_params(a, sm);

    f32x4 acc[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    double dl = 0.0;

    for (; tile < n_tiles; tile += gridDim.x) {
        const int64_t row0 = tile * kBceRows;
        bce_tile_commit(a, row0, pr, pc, pre, sm);
        __syncthreads();
        if (tile + gridDim.x < n_tiles) bce_tile_issue(a, (tile + gridDim.x) * kBceRows, pr, pc, pre);

        // ---- logits, loss terms and dz of this wave's label groups
        float lt = 0.f;
        for (int cg = wave; cg < nCG; cg += kBceWaves) {
            const int c0 = 16 * cg, c = c0 + j;
            const f32x4 z4 = bce_logits(sE, sW, WP, nDT, c0, j, q);
            const float bias = sB[c], pw = sPW[c];
            const int wd = c >> 5, bit = c & 31;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 4 * q + r;
                const bool valid = c < C && row0 + row < B;
                const bool y = (sY[row * nW + min(wd, nW - 1)] >> bit) & 1;
                float l, g;
                bce_elem(z4[r] + bias, y, pw, l, g);
                lt += valid ? l : 0.f;
                sZ[row * ZP + c] = valid ? g * a.inv_n : 0.f;
            }
        }
        dl += static_cast<double>(lt);
        __syncthreads();

        // ---- dE = dz·Wc of this wave's column tiles
        for (int dt = wave; dt < nDT; dt += kBceWaves) {
            f32x4 a0 = f32x4{0.f, 0.f, 0.f, 0.f}, a1 = a0;
            const float* zp = sZ + j * ZP + 4 * q;
            const float* wp = sW + (4 * q) * WP + 16 * dt + j;
            for (int cg = 0; cg < nCG; ++cg) {
                const float4 zv = *reinterpret_cast<const float4*>(zp + 16 * cg);
                const float* wr = wp + 16 * cg * WP;
                const float w0 = wr[0], w1 = wr[WP], w2 = wr[2 * WP], w3 = wr[3 * WP];
                a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(zv.x, w0, a0, 0, 0, 0);
                a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(zv.y, w1, a1, 0, 0, 0);
                a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(zv.z, w2, a0, 0, 0, 0);
                a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(zv.w, w3, a1, 0, 0, 0);
            }
            const f32x4 g4 = a0 + a1;
            const int d = 16 * dt + j;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 4 * q + r;
                const float e = sE[row * WP + d];
                if (d < D && row0 + row < B)
                    a.dE[(row0 + row) * D + d] = (a.mask_relu && e <= 0.f) ? 0.f : g4[r];
            }
        }

        // ---- dWc / dbc += dzᵀ·[E | 1] on this wave's tiles
        {
            int cg = 0, dt = wave;
#pragma unroll
            for (int i = 0; i < NT; ++i) {
                while (dt > nDT) {
                    dt -= nDT + 1;
                    ++cg;
                }
                if (i < nt) {
                    const float* zp = sZ + (4 * q) * ZP + 16 * cg + j;
                    const bool ones = dt == nDT;
                    const float* ep = sE + (4 * q) * WP + (ones ? 0 : 16 * dt) + j;
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        const float ev = ones ? 1.f : ep[s * WP];
                        acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(zp[s * ZP], ev, acc[i], 0, 0, 0);
                    }
                }
                dt += kBceWaves;
            }
        }
        __syncthreads();
    }

    // ---- the workgroup's slab [CP][D16 + 16] and its loss partial
    {
        const int SW = a.L.D16 + 16;
        float* out = a.slab + static_cast<int64_t>(blockIdx.x) * a.L.CP * SW;
        int cg = 0, dt = wave;
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            while (dt > nDT) {
                dt -= nDT + 1;
                ++cg;
            }
            if (i < nt) {
#pragma unroll
                for (int r = 0; r < 4; ++r) out[(16 * cg + 4 * q + r) * SW + 16 * dt + j] = acc[i][r];
            }
            dt += kBceWaves;
        }
    }
    bce_loss_partial(dl, sm, a.L.oMisc, a.lpart + blockIdx.x);
}

// dWc, dbc = Σ over the workgroups' slabs, in workgroup order (four consecutive quarters, then the quarters in
// order); the last block adds the loss partials (thread-strided, then the threads in order) and divides by B·C.
__global__ __launch_bounds__(kBceRedThreads) void cls_bce_reduce_kernel(int nb, int D, int C, int D16, int CP,
                                                                        double n_elems,
                                                                        const float* __restrict__ slab,
                                                                        const double* __restrict__ lpart,
                                                                        float* __restrict__ dWc,
                                                                        float* __restrict__ dbc,
                                                                        float* __restrict__ loss) {
    if (blockIdx.x == gridDim.x - 1) {
        __shared__ double red[kBceRedThreads];
        double s = 0.0;
        for (int k = threadIdx.x; k < nb; k += kBceRedThreads) s += lpart[k];
        red[threadIdx.x] = s;
        __syncthreads();
        if (threadIdx.x == 0) {
            double t = 0.0;
            for (int w = 0; w < kBceRedThreads; ++w) t += red[w];
            loss[0] = static_cast<float>(t / n_elems);
        }
        return;
    }
    __shared__ float part[3][64];
    const int per = C * (D + 1), SW = D16 + 16;
    const int p = threadIdx.x >> 6;
    const int t = blockIdx.x * 64 + (threadIdx.x & 63);
    const int tc = min(t, per - 1);
    const int c = tc / (D + 1), d = tc - c * (D + 1);
    const int64_t src = static_cast<int64_t>(c) * SW + (d < D ? d : D16);
    const int64_t stride = static_cast<int64_t>(CP) * SW;
    const int nq = (nb + 3) / 4;
    const int k0 = min(nb, p * nq), k1 = min(nb, k0 + nq);
    float s = 0.f;
#pragma unroll 8
    for (int k = k0; k < k1; ++k) s += slab[k * stride + src];
    if (p > 0) part[p - 1][threadIdx.x & 63] = s;
    __syncthreads();
    if (p == 0 && t < per) {
        s += part[0][threadIdx.x];
        s += part[1][threadIdx.x];
        s += part[2][threadIdx.x];
        if (d < D) dWc[static_cast<int64_t>(c) * D + d] = s;
        else dbc[c] = s;
    }
}

__global__ __launch_bounds__(kBceThreads) void cls_bce_eval_kernel(const BceArgs a) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 15, q = lane >> 4;
    const int WP = a.L.WP, nW = a.L.nW, nDT = a.L.nDT, nCG = a.L.nCG, C = a.C;
    const float* sW = sm;
    const float* sB = sm + a.L.oB;
    const float* sPW = sm + a.L.oPW;
    const float* sE = sm + a.L.oE;
    const int* sY = reinterpret_cast<const int*>(sm + a.L.oY);
    int* sP = reinterpret_cast<int*>(sm + a.L.oP);
    unsigned short* sP16 = reinterpret_cast<unsigned short*>(sP);
    int* sCnt = reinterpret_cast<int*>(sm + a.L.oCnt);
    int* sExact = reinterpret_cast<int*>(sm + a.L.oMisc + 8);
    const int64_t B = a.B;
    const int64_t n_tiles = (B + kBceRows - 1) / kBceRows;

    int pr[kBcePre], pc[kBcePre];
    bce_pre_map(a.L.D16, pr, pc);
    BceTile pre;
    int64_t tile = blockIdx.x;
    if (tile < n_tiles) bce_tile_issue(a, tile * kBceRows, pr, pc, pre);
    bce_stage_params(a, sm);
    for (int t = tid; t < 3 * C; t += kBceThreads) sCnt[t] = 0;
    if (tid == 0) *sExact = 0;

    double dl = 0.0;
    int n_exact = 0;  // threads 0..15: the rows of their index
    for (; tile < n_tiles; tile += gridDim.x) {
        const int64_t row0 = tile * kBceRows;
        bce_tile_commit(a, row0, pr, pc, pre, sm);
        __syncthreads();
        if (tile + gridDim.x < n_tiles) bce_tile_issue(a, (tile + gridDim.x) * kBceRows, pr, pc, pre);

        float lt = 0.f;
        for (int cg = wave; cg < nCG; cg += kBceWaves) {
            const int c0 = 16 * cg, c = c0 + j;
            const f32x4 z4 = bce_logits(sE, sW, WP, nDT, c0, j, q);
            const float bias = sB[c], pw = sPW[c];
            const int wd = c >> 5, bit = c & 31;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 4 * q + r;
                const bool valid = c < C && row0 + row < B;
                const bool y = (sY[row * nW + min(wd, nW - 1)] >> bit) & 1;
                const float z = z4[r] + bias;
                float l, g;
                bce_elem(z, y, pw, l, g);
                lt += valid ? l : 0.f;
                // lane 16 q' + j' of the ballot: row 4 q' + r, label c0 + j'
                const unsigned long long m = __ballot(valid && z > 0.f);
                if (j == 0) sP16[row * (2 * nW) + cg] = static_cast<unsigned short>((m >> (16 * q)) & 0xffffu);
                if (a.logits && valid) a.logits[(row0 + row) * C + c] = z;
            }
        }
        dl += static_cast<double>(lt);
        __syncthreads();

        // ---- the counts from the word images: thread c owns label c; threads 0..15 a row each
        const int rows = static_cast<int>(B - row0 < kBceRows ? B - row0 : kBceRows);
        for (int c = tid; c < C; c += kBceThreads) {
            const int wd = c >> 5, bit = c & 31;
            int tp = 0, fp = 0, fn = 0;
            for (int r = 0; r < rows; ++r) {
                const int y = (sY[r * nW + wd] >> bit) & 1, p = (sP[r * nW + wd] >> bit) & 1;
                tp += p & y;
                fp += p & (y ^ 1);
                fn += (p ^ 1) & y;
            }
            sCnt[3 * c] += tp;
            sCnt[3 * c + 1] += fp;
            sCnt[3 * c + 2] += fn;
        }
        if (tid < rows) {
            bool same = true;
            for (int w = 0; w < nW; ++w) {
                const int left = C - 32 * w;
                const unsigned mask = left >= 32 ? 0xffffffffu : ((1u << left) - 1u);
                same = same && (((static_cast<unsigned>(sY[tid * nW + w]) ^ static_cast<unsigned>(sP[tid * nW + w])) &
                                 mask) == 0u);
            }
            n_exact += same ? 1 : 0;
        }
        if (a.pred)
            for (int e = tid; e < rows * nW; e += kBceThreads) a.pred[row0 * nW + e] = sP[e];
        __syncthreads();
    }

    if (tid < kBceRows && n_exact) atomicAdd(sExact, n_exact);
    __syncthreads();
    int* out = a.cslab + static_cast<int64_t>(blockIdx.x) * (3 * C + 1);
    for (int t = tid; t < 3 * C; t += kBceThreads) out[t] = sCnt[t];
    if (tid == 0) out[3 * C] = *sExact;
    bce_loss_partial(dl, sm, a.L.oMisc, a.lpart + blockIdx.x);
}

// counts[t] = Σ over the workgroups' integer slabs; the last block finishes the loss.
__global__ __launch_bounds__(kBceRedThreads) void cls_bce_eval_reduce_kernel(int nb, int n_counts, double n_elems,
                                                                             const int* __restrict__ cslab,
                                                                             const double* __restrict__ lpart,
                                                                             long long* __restrict__ counts,
                                                                             float* __restrict__ loss) {
    if (blockIdx.x == gridDim.x - 1) {
        __shared__ double red[kBceRedThreads];
        double s = 0.0;
        for (int k = threadIdx.x; k < nb; k += kBceRedThreads) s += lpart[k];
        red[threadIdx.x] = s;
        __syncthreads();
        if (threadIdx.x == 0) {
            double t = 0.0;
            for (int w = 0; w < kBceRedThreads; ++w) t += red[w];
            loss[0] = static_cast<float>(t / n_elems);
        }
        return;
    }
    const int t = blockIdx.x * kBceRedThreads + threadIdx.x;
    if (t >= n_counts) return;
    long long s = 0;
    for (int k = 0; k < nb; ++k) s += cslab[static_cast<int64_t>(k) * n_counts + t];
    counts[t] = s;
}

namespace {

template <int NT>
bool bce_raise() {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(cls_bce_train_kernel<NT>),
                               hipFuncAttributeMaxDynamicSharedMemorySize,
                               static_cast<int>(kBceLdsFloats * 4)) == hipSuccess;
}

// The raised LDS limit of every kernel here, once per device.
void bce_lds_limit() {
    static std::mutex mu;
    static uint64_t done_mask = 0;
    int dev = 0;
    hip_ok(hipGetDevice(&dev), "gs_cls_bce: device");
    std::lock_guard<std::mutex> lock(mu);
    const bool cached = dev >= 0 && dev < 64;
    if (cached && (done_mask >> dev & 1)) return;
    const bool all = bce_raise<1>() && bce_raise<3>() && bce_raise<5>() && bce_raise<9>() && bce_raise<18>() &&
                     bce_raise<36>() &&
                     hipFuncSetAttribute(reinterpret_cast<const void*>(cls_bce_eval_kernel),
                                         hipFuncAttributeMaxDynamicSharedMemorySize,
                                         static_cast<int>(kBceLdsFloats * 4)) == hipSuccess;
    if (!all) fail(GS_EHIP, "gs_cls_bce: cannot raise the kernels' LDS limit");
    if (cached) done_mask |= uint64_t(1) << dev;
}

void bce_check_sizes(int64_t B, int64_t D, int64_t C) {
    GS_REQUIRE(B >= 1 && D >= 1 && C >= 1, GS_EINVAL, "sizes must be >= 1");
    GS_REQUIRE(B < (int64_t(1) << 31), GS_EINVAL, "B < 2^31");
}

}  // namespace

}  // namespace gs

extern "C" {

int gs_cls_bce_supported(int64_t D, int64_t C) { return gs::bce_layout(D, C).ok; }

int64_t gs_cls_bce_ws_bytes(int64_t B, int64_t D, int64_t C) {
    GS_BYTES_BEGIN
    gs::bce_check_sizes(B, D, C);
    const gs::BceLayout L = gs::bce_layout(D, C);
    GS_REQUIRE(L.ok, GS_EINVAL, "D and C too large for the workgroup's LDS (gs_cls_bce_supported)");
    return gs::bce_part_bytes(B) + gs::bce_round16(gs::bce_blocks(B) * gs::bce_slab_floats(L) * 4);
    GS_BYTES_END
}

int64_t gs_cls_bce_eval_ws_bytes(int64_t B, int64_t D, int64_t C) {
    GS_BYTES_BEGIN
    gs::bce_check_sizes(B, D, C);
    GS_REQUIRE(gs::bce_layout(D, C).ok, GS_EINVAL, "D and C too large for the workgroup's LDS (gs_cls_bce_supported)");
    return gs::bce_part_bytes(B) + gs::bce_round16(gs::bce_blocks(B) * (3 * C + 1) * 4);
    GS_BYTES_END
}

int gs_cls_bce_fwd_bwd(int64_t B, int64_t D, int64_t C, const float* E, int64_t lde, const float* Wc,
                       const float* bc, const int32_t* targets, const int32_t* roots, const float* pos_weight,
                       int32_t mask_relu, float* loss, float* dE, float* dWc, float* dbc, void* ws,
                       int64_t ws_bytes, void* stream) {
    GS_API_BEGIN
    using namespace gs;
    GS_REQUIRE(E && Wc && bc && targets && loss && dE && dWc && dbc && ws, GS_EINVAL, "NULL mandatory pointer");
    bce_check_sizes(B, D, C);
    GS_REQUIRE(lde >= D, GS_EINVAL, "lde < D");
    const BceLayout L = bce_layout(D, C);
    GS_REQUIRE(L.ok, GS_EINVAL, "D and C too large for the workgroup's LDS (gs_cls_bce_supported)");
    const int64_t need = gs_cls_bce_ws_bytes(B, D, C);
    GS_REQUIRE(need > 0 && ws_bytes >= need, GS_EINVAL, "workspace shorter than gs_cls_bce_ws_bytes");
    GS_REQUIRE(aligned16(ws), GS_EINVAL, "workspace not 16-byte aligned");
    bce_lds_limit();
    BceArgs a{};
    a.X = E;
    a.ldx = lde;
    a.ids = nullptr;
    a.tids = roots;
    a.targets = targets;
    a.Wc = Wc;
    a.bc = bc;
    a.pw = pos_weight;
    a.B = B;
    a.D = static_cast<int>(D);
    a.C = static_cast<int>(C);
    a.mask_relu = mask_relu ? 1 : 0;
    const double n_elems = static_cast<double>(B) * static_cast<double>(C);
    a.inv_n = static_cast<float>(1.0 / n_elems);
    a.dE = dE;
    a.lpart = static_cast<double*>(ws);
    a.slab = reinterpret_cast<float*>(static_cast<char*>(ws) + bce_part_bytes(B));
    a.L = L;
    hipStream_t st = as_stream(stream);
    const int nb = static_cast<int>(bce_blocks(B));
    const uint32_t smem = static_cast<uint32_t>(L.floats) * 4u;
    const int per_wave = (L.nCG * (L.nDT + 1) + kBceWaves - 1) / kBceWaves;
    if (per_wave <= 1) cls_bce_train_kernel<1><<<dim3(nb), kBceThreads, smem, st>>>(a);
    else if (per_wave <= 3) cls_bce_train_kernel<3><<<dim3(nb), kBceThreads, smem, st>>>(a);
    else if (per_wave <= 5) cls_bce_train_kernel<5><<<dim3(nb), kBceThreads, smem, st>>>(a);
    else if (per_wave <= 9) cls_bce_train_kernel<9><<<dim3(nb), kBceThreads, smem, st>>>(a);
    else if (per_wave <= 18) cls_bce_train_kernel<18><<<dim3(nb), kBceThreads, smem, st>>>(a);
    else cls_bce_train_kernel<36><<<dim3(nb), kBceThreads, smem, st>>>(a);
    check_launch("gs_cls_bce_fwd_bwd: rows");
    const int per = static_cast<int>(C * (D + 1));
    cls_bce_reduce_kernel<<<dim3((per + 63) / 64 + 1), kBceRedThreads, 0, st>>>(
        nb, a.D, a.C, L.D16, L.CP, n_elems, a.slab, a.lpart, dWc, dbc, loss);
    check_launch("gs_cls_bce_fwd_bwd: reduce");
    GS_API_END
}

int gs_cls_bce_eval(int64_t B, int64_t D, int64_t C, const float* H, int64_t ldh, const int32_t* rows,
                    const int32_t* targets, int32_t targets_by_row, const float* Wc, const float* bc,
                    const float* pos_weight, int32_t* pred, float* logits, float* loss, int64_t* counts, void* ws,
                    int64_t ws_bytes, void* stream) {
    GS_API_BEGIN
    using namespace gs;
    GS_REQUIRE(H && Wc && bc && targets && loss && counts && ws, GS_EINVAL, "NULL mandatory pointer");
    bce_check_sizes(B, D, C);
    GS_REQUIRE(ldh >= D, GS_EINVAL, "ldh < D");
    const BceLayout L = bce_layout(D, C);
    GS_REQUIRE(L.ok, GS_EINVAL, "D and C too large for the workgroup's LDS (gs_cls_bce_supported)");
    const int64_t need = gs_cls_bce_eval_ws_bytes(B, D, C);
    GS_REQUIRE(need > 0 && ws_bytes >= need, GS_EINVAL, "workspace shorter than gs_cls_bce_eval_ws_bytes");
    GS_REQUIRE(aligned16(ws), GS_EINVAL, "workspace not 16-byte aligned");
    bce_lds_limit();
    BceArgs a{};
    a.X = H;
    a.ldx = ldh;
    a.ids = rows;
    a.tids = targets_by_row && rows ? rows : nullptr;
    a.targets = targets;
    a.Wc = Wc;
    a.bc = bc;
    a.pw = pos_weight;
    a.B = B;
    a.D = static_cast<int>(D);
    a.C = static_cast<int>(C);
    const double n_elems = static_cast<double>(B) * static_cast<double>(C);
    a.inv_n = static_cast<float>(1.0 / n_elems);
    a.pred = pred;
    a.logits = logits;
    a.lpart = static_cast<double*>(ws);
    a.cslab = reinterpret_cast<int*>(static_cast<char*>(ws) + bce_part_bytes(B));
    a.L = L;
    hipStream_t st = as_stream(stream);
    const int nb = static_cast<int>(bce_blocks(B));
    cls_bce_eval_kernel<<<dim3(nb), kBceThreads, static_cast<uint32_t>(L.floats) * 4u, st>>>(a);
    check_launch("gs_cls_bce_eval: rows");
    const int n_counts = static_cast<int>(3 * C + 1);
    cls_bce_eval_reduce_kernel<<<dim3((n_counts + kBceRedThreads - 1) / kBceRedThreads + 1), kBceRedThreads, 0,
                                 st>>>(nb, n_counts, n_elems, a.cslab, a.lpart,
                                       reinterpret_cast<long long*>(counts), loss);
    check_launch("gs_cls_bce_eval: reduce");
    GS_API_END
}

}  // extern "C"
