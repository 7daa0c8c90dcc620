// Counter-based device sampler: the device form of
// gs_fsample_pack_run (host/fsample.cpp) — the same rule, the same pack, bit
// for bit — with none of the bit-exact sampler's sequential pieces.  Every
// draw is a pure function of (seed, batch_index, hop, frontier slot, draw
// number), so destinations are sampled independently; the frontier union is a
// bitmap over the node ids, which makes "unique, ascending" a popcount scan.
//
// Kernels of a hop before the last (F = F(j-1), n_dst destinations):
//   draw_kernel<false>  32 lanes per destination: lane t computes draw t's
//                       Philox word, the k Floyd steps resolve "already
//                       chosen" with a ballot over the lanes, lane t reads its
//                       neighbour id, keeps it (samp) and marks the bitmap.
//   scan_a/b + compact  popcount scan of the bitmap words (per-block sums, one
//                       small block over the sums, per-block rescan); compact
//                       writes Fj in ascending id order, lid[id] = slot, and
//                       clears the words it read.
//   scan_a/b/c (NBR)    neighbour counts -> nbr_ptr; scan_b also lays the
//                       hop's fields out in the pack (sizes exist only here).
//   lists_kernel        32 lanes per destination: slots via lid, self dropped
//                       (gcn: added once), rank sort of <= 33 slots, nbr /
//                       self into the pack, transposed counts (atomic counts).
//   scan_a/b/c (T)      counts -> tptr.
//   tfill_kernel        every (source, key) into its source's segment at an
//                       atomically claimed place, key = 2r + 1 for "r reads c",
//                       2r for "c is r's self row".  The places are arbitrary;
//                       the keys of one segment are distinct.
//   tsort_kernel        one wave per source: segments <= 64 are rank-sorted by
//                       key and decoded into tidx; longer ones are listed.
//   tlong_kernel        one block per listed source: its distinct keys marked
//                       in an LDS bitmap (262144 keys per pass), scanned and
//                       emitted ascending.
// So atomics count and claim scratch places; the order of everything that
// reaches the pack comes from sorts and scans.  The last hop: a scan of
// min(deg, k) (POS) -> pos_ptr, then draw_kernel<true> writes entries and
// dst_ids.  A scan whose bound is at most kSmallScan (15360) values runs as one
// launch (scan_small_kernel) instead of three; the bitmap's never does.
//
// Every grid is sized by the bounds fixed at create; the kernels read the real
// sizes from the control block.  An overflow of a bound or of the pack sets a
// status (GS_ELIMIT) and the later kernels return; nothing is written past a
// buffer.  No kernel waits on another block.
#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../host/graph.hpp"
#include "../host/philox.hpp"
#include "block_scan.hpp"
#include "dev_host.hpp"
#include "fsample.hpp"
#include "kcommon.hpp"

namespace gs {
namespace fs {

constexpr int kStLimit = 1;           // a frontier or the pack outgrew its bound
constexpr int kStRange = 2;           // a root id outside the graph
constexpr int kStEmpty = 4;           // empty neighbourhood with GS_SAMPLE_FAIL_EMPTY
constexpr int kStBail = kStLimit | kStRange;  // later kernels have nothing valid to read
constexpr int kScanBlock = 1024;      // elements per scan block (256 threads x 4)
constexpr int kSmallScan = 15 * 1024;  // a scan bounded by this is one launch (scan_small_kernel, 60 KiB of LDS)
constexpr int kLongKeys = 262144;     // keys per tlong pass (32 KiB of LDS bits)
constexpr int kLongWords = kLongKeys / 32;

enum { kScanBitmap = 0, kScanNbr = 1, kScanT = 2, kScanPos = 3 };

struct FHop {
    int32_t n_dst, n_pos, n_src, n_nbr, n_empty;
    int32_t off[GS_PK_NFIELDS];
};

struct FCtl {
    int32_t status;
    int32_t at;       // pack elements laid out so far
    int32_t used;     // at + roots, written by finish_kernel
    int32_t n_long;   // sources listed for tlong_kernel
    int32_t tot;      // total of the last scan
    FHop hop[GS_MAX_HOPS];
};

struct P {
    const int64_t* row_ptr;
    const int32_t* col;
    int32_t n_nodes;
    FCtl* ctl;
    uint32_t* bitmap;       // [n_words] one bit per node, all zero between hops
    int32_t n_words;        // multiple of kScanBlock
    int32_t* lid;           // [n_nodes] node -> slot in Fj (this hop's keys only)
    int32_t* F[GS_MAX_HOPS];  // frontiers F0 .. F(L-1)
    int32_t nd_max[GS_MAX_HOPS];
    int32_t* samp;          // sampled neighbour ids, k per destination
    int32_t* cnt;           // sampled entries per destination
    int32_t* nbrcnt;        // neighbourhood size after the self rule
    int32_t* tcnt;          // transposed counts, then claim cursors
    int32_t* traw;          // transposed keys before their sort
    int32_t* longs;         // sources left to tlong_kernel
    int32_t longs_cap;
    int32_t* bsum;          // scan block sums / prefixes
    int32_t* pack;
    int32_t cap;            // pack elements available before the roots
    uint64_t seed, batch_index;
    int32_t gcn;
};

// The lanes of this thread's 32-lane group for which pred holds.
__device__ __forceinline__ uint32_t ballot32(bool pred) {
    return static_cast<uint32_t>(__ballot(pred) >> (threadIdx.x & 32));
}

__device__ __forceinline__ bool bailed(const FCtl* c) {
    __shared__ int s_bail;
    if (threadIdx.x == 0) s_bail = c->status & kStBail;
    __syncthreads();
    return s_bail != 0;
}

// ------------------------------------------------------------------ scans
template <int MODE>
__device__ __forceinline__ int scan_n(const P& p, int hop) {
    if (MODE == kScanBitmap) return p.n_words;
    if (MODE == kScanT) return p.ctl->hop[hop].n_src;
    return p.ctl->hop[hop].n_dst;
}
template <int MODE>
__device__ __forceinline__ int scan_val(const P& p, int hop, int k, int i) {
    if (MODE == kScanBitmap) return __popc(p.bitmap[i]);
    if (MODE == kScanNbr) return p.nbrcnt[i];
    if (MODE == kScanT) return p.tcnt[i];
    const int v = p.F[hop][i];  // kScanPos: the last hop's min(deg, k) per destination
    return static_cast<int>(min(p.row_ptr[v + 1] - p.row_ptr[v], static_cast<int64_t>(k)));
}

// After a scan (one thread): record its total and lay out the fields whose
// sizes it completes.
template <int MODE>
__device__ void scan_done(const P& p, int hop, int run) {
    FCtl* c = p.ctl;
    c->tot = run;
    FHop& h = c->hop[hop];
    int32_t at = c->at;
    auto put = [&](int f, int32_t cnt) {
        h.off[f] = at;
        at += al4(cnt);
    };
    if (MODE == kScanBitmap) {  // |Fj|: the next hop's destinations
        h.n_src = run;
        if (run > p.nd_max[hop + 1]) {
            atomicOr(&c->status, kStLimit);
            c->hop[hop + 1].n_dst = 0;
        } else {
            c->hop[hop + 1].n_dst = run;
        }
    } else if (MODE == kScanNbr) {
        h.n_nbr = run;
        put(GS_PK_NBR_PTR, h.n_dst + 1);
        put(GS_PK_NBR, run);
        put(GS_PK_SELF, h.n_dst);
        put(GS_PK_TPTR, h.n_src + 1);
        put(GS_PK_TIDX, run + h.n_dst);
        if (at > p.cap) atomicOr(&c->status, kStLimit);
        else c->at = at;
    } else if (MODE == kScanT) {
        c->n_long = 0;
    } else {
        h.n_pos = run;
        put(GS_PK_POS_PTR, h.n_dst + 1);
        put(GS_PK_POS, run);
        put(GS_PK_DST_IDS, h.n_dst);
        if (at > p.cap) atomicOr(&c->status, kStLimit);
        else c->at = at;
    }
}

// A scan of at most kSmallScan values in one launch: one block reads the
// values thread-strided into LDS (the last hop's are two dependent gathers
// each: every wave takes an equal share), then scans 15 consecutive values per
// thread; the result of the three-kernel form below.
template <int MODE>
__global__ __launch_bounds__(1024) void scan_small_kernel(P p, int hop, int k) {
    __shared__ int sh[17];
    __shared__ int s_ok;
    __shared__ int vals[kSmallScan];
    FCtl* c = p.ctl;
    if (bailed(c)) return;
    constexpr int kPer = kSmallScan / 1024;
    const int n = min(scan_n<MODE>(p, hop), kSmallScan);  // n <= the launch's bound <= kSmallScan
#pragma unroll
    for (int q = 0; q < kPer; ++q) {
        const int i = threadIdx.x + q * 1024;
        if (i < n) vals[i] = scan_val<MODE>(p, hop, k, i);
    }
    __syncthreads();
    const int i0 = threadIdx.x * kPer;
    int v[kPer], s = 0;
#pragma unroll
    for (int q = 0; q < kPer; ++q) {
        v[q] = i0 + q < n ? vals[i0 + q] : 0;
        s += v[q];
    }
    int total;
    int run = block_excl_scan<16>(s, sh, &total);
    if (threadIdx.x == 0) {
        scan_done<MODE>(p, hop, total);
        s_ok = !(c->status & kStBail);  // the layout may have found the pack too small
    }
    __syncthreads();  // also orders thread 0's offsets before the reads below
    if (!s_ok) return;
    const int field = MODE == kScanNbr ? GS_PK_NBR_PTR : MODE == kScanT ? GS_PK_TPTR : GS_PK_POS_PTR;
    int32_t* out = p.pack + c->hop[hop].off[field];
    if (threadIdx.x == 0) out[n] = total;
#pragma unroll
    for (int q = 0; q < kPer; ++q) {
        if (i0 + q < n) out[i0 + q] = run;
        run += v[q];
    }
}

template <int MODE>
__global__ __launch_bounds__(256) void scan_a_kernel(P p, int hop, int k) {
    __shared__ int sh[5];
    if (MODE != kScanBitmap && bailed(p.ctl)) return;  // the bitmap scans always run: compact clears the words
    const int n = scan_n<MODE>(p, hop);
    const int base = blockIdx.x * kScanBlock;
    if (base >= n) return;
    const int i0 = base + threadIdx.x * 4;
    int s = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q)
        if (i0 + q < n) s += scan_val<MODE>(p, hop, k, i0 + q);
    int total;
    (void)block_excl_scan<4>(s, sh, &total);
    if (threadIdx.x == 0) p.bsum[blockIdx.x] = total;
}

// One block: the block sums' exclusive prefixes in place; thread 0 then
// finishes the scan (scan_done).
template <int MODE>
__global__ __launch_bounds__(1024) void scan_b_kernel(P p, int hop, int nb_max) {
    __shared__ int sh[17];
    FCtl* c = p.ctl;
    if (MODE != kScanBitmap && bailed(c)) return;
    const int n = scan_n<MODE>(p, hop);
    const int nb = (n + kScanBlock - 1) / kScanBlock;
    int run = 0;
    for (int c0 = 0; c0 < nb_max; c0 += 1024) {
        if (c0 >= nb) break;  // block-uniform
        const int i = c0 + threadIdx.x;
        const int v = i < nb ? p.bsum[i] : 0;
        int total;
        const int ex = block_excl_scan<16>(v, sh, &total);
        if (i < nb) p.bsum[i] = run + ex;
        run += total;
    }
    if (threadIdx.x == 0) scan_done<MODE>(p, hop, run);
}

// Exclusive prefixes out[0..n) and out[n] = total into the field's pack slot.
template <int MODE>
__global__ __launch_bounds__(256) void scan_c_kernel(P p, int hop, int k) {
    __shared__ int sh[5];
    if (bailed(p.ctl)) return;
    const int n = scan_n<MODE>(p, hop);
    const int field = MODE == kScanNbr ? GS_PK_NBR_PTR : MODE == kScanT ? GS_PK_TPTR : GS_PK_POS_PTR;
    int32_t* out = p.pack + p.ctl->hop[hop].off[field];
    if (blockIdx.x == 0 && threadIdx.x == 0) out[n] = p.ctl->tot;
    const int base = blockIdx.x * kScanBlock;
    if (base >= n) return;
    const int i0 = base + threadIdx.x * 4;
    int v[4], s = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        v[q] = i0 + q < n ? scan_val<MODE>(p, hop, k, i0 + q) : 0;
        s += v[q];
    }
    int total;
    int run = block_excl_scan<4>(s, sh, &total) + p.bsum[blockIdx.x];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (i0 + q < n) out[i0 + q] = run;
        run += v[q];
    }
}

// The bitmap scan's third pass: Fj ascending, lid, zeroed transposed counts;
// clears every word it read (also on a failed run: the bitmap is all zero
// whenever no hop is in flight).
__global__ __launch_bounds__(256) void compact_kernel(P p, int hop) {
    __shared__ int sh[5];
    const int i0 = blockIdx.x * kScanBlock + threadIdx.x * 4;  // n_words is a multiple of kScanBlock
    uint32_t w[4];
    int s = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        w[q] = p.bitmap[i0 + q];
        s += __popc(w[q]);
    }
    int total;
    int rank = block_excl_scan<4>(s, sh, &total) + p.bsum[blockIdx.x];
    if (total == 0) return;
    const int cap = p.nd_max[hop + 1];
    int32_t* next = p.F[hop + 1];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        uint32_t bits = w[q];
        if (!bits) continue;
        p.bitmap[i0 + q] = 0;
        while (bits) {
            const int id = (i0 + q) * 32 + __ffs(bits) - 1;
            bits &= bits - 1;
            if (rank >= 0 && rank < cap) {
                next[rank] = id;
                p.lid[id] = rank;
                p.tcnt[rank] = 0;
            }
            ++rank;
        }
    }
}

// ------------------------------------------------------------------ draws
__global__ __launch_bounds__(256) void begin_kernel(P p, const int32_t* roots, int n_roots) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i == 0) p.ctl->hop[0].n_dst = n_roots;
    if (i >= n_roots) return;
    const int32_t v = roots[i];
    if (v < 0 || v >= p.n_nodes) atomicOr(&p.ctl->status, kStRange);
    p.F[0][i] = v;
}

// 32 lanes per destination, 8 destinations per block.
template <bool LAST>
__global__ __launch_bounds__(256) void draw_kernel(P p, int hop, int k) {
    __shared__ int s_pos, s_empty;
    FCtl* c = p.ctl;
    if (threadIdx.x == 0) s_pos = s_empty = 0;
    if (bailed(c)) return;  // syncs
    const int n_dst = c->hop[hop].n_dst;
    const int r = blockIdx.x * 8 + (threadIdx.x >> 5), lane = threadIdx.x & 31;
    const bool act = r < n_dst;
    int v = 0, deg = 0;
    int64_t rs = 0;
    if (act) {
        v = p.F[hop][r];
        rs = p.row_ptr[v];
        deg = static_cast<int>(p.row_ptr[v + 1] - rs);
    }
    const int cn = min(deg, k);
    // Floyd: lane t holds draw t's x; step t appends m = deg-k+t when x is
    // already among the t values chosen so far
    int x = 0;
    if (act && deg > k && lane < k)
        x = static_cast<int>(randbelow(static_cast<uint32_t>(deg - k + lane) + 1u,
                                       draw_word(p.seed, p.batch_index, static_cast<uint32_t>(r),
                                                 static_cast<uint32_t>(hop + 1), static_cast<uint32_t>(lane))));
    int chosen = -1;
    for (int t = 0; t < k; ++t) {  // uniform: every lane of the block takes every step
        const int xt = __shfl(x, t, 32);
        const bool hit = ballot32(lane < t && chosen == xt) != 0;
        if (lane == t) chosen = hit ? deg - k + t : xt;
    }
    const int pos = deg <= k ? lane : chosen;
    const bool valid = act && lane < cn;
    if (!LAST) {
        int id = -1;
        if (valid) {
            id = p.col[rs + pos];
            p.samp[static_cast<int64_t>(r) * k + lane] = id;
            atomicOr(&p.bitmap[id >> 5], 1u << (id & 31));
        }
        const int self_in = ballot32(valid && id == v) != 0;
        if (act && lane == 0) {
            atomicOr(&p.bitmap[v >> 5], 1u << (v & 31));
            const int nn = p.gcn ? cn + !self_in : cn - self_in;
            p.cnt[r] = cn;
            p.nbrcnt[r] = nn;
            atomicAdd(&s_pos, cn);
            if (nn == 0) atomicAdd(&s_empty, 1);
        }
    } else {
        const FHop& h = c->hop[hop];
        if (valid) p.pack[h.off[GS_PK_POS] + p.pack[h.off[GS_PK_POS_PTR] + r] + lane] = static_cast<int32_t>(rs + pos);
        if (act && lane == 0) {
            p.pack[h.off[GS_PK_DST_IDS] + r] = v;
            if (!p.gcn && (cn == 0 || (cn == 1 && p.col[rs + pos] == v))) atomicAdd(&s_empty, 1);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (!LAST && s_pos) atomicAdd(&c->hop[hop].n_pos, s_pos);
        if (s_empty) atomicAdd(&c->hop[hop].n_empty, s_empty);
    }
}

// ------------------------------------------------------------------ lists
// 32 lanes per destination: nbr (ascending Fj slots), self, transposed counts.
__global__ __launch_bounds__(256) void lists_kernel(P p, int hop, int k) {
    if (bailed(p.ctl)) return;
    const FHop& h = p.ctl->hop[hop];
    const int r = blockIdx.x * 8 + (threadIdx.x >> 5), lane = threadIdx.x & 31;
    const bool act = r < h.n_dst;
    int v = 0, cn = 0, s = 0, base = 0;
    if (act) {
        v = p.F[hop][r];
        cn = p.cnt[r];
        s = p.lid[v];
        base = p.pack[h.off[GS_PK_NBR_PTR] + r];
    }
    int rk = 0x7fffffff;
    bool valid = false;
    if (act && lane < cn) {
        const int id = p.samp[static_cast<int64_t>(r) * k + lane];
        valid = id != v;
        if (valid) rk = p.lid[id];
    }
    int pos = 0;
    for (int i = 0; i < 32; ++i) pos += __shfl(rk, i, 32) < rk;  // distinct slots: the rank is the place
    const uint32_t below = ballot32(valid && rk < s);
    int32_t* nbr = p.pack + h.off[GS_PK_NBR] + base;
    if (valid) {
        nbr[pos + (p.gcn && s < rk ? 1 : 0)] = rk;
        atomicAdd(&p.tcnt[rk], 1);
    }
    if (act && lane == 0) {
        if (p.gcn) nbr[__popc(below)] = s;
        p.pack[h.off[GS_PK_SELF] + r] = s;
        atomicAdd(&p.tcnt[s], p.gcn ? 2 : 1);
    }
}

// Keys into their source's segment of traw, at places claimed by counting the
// cursor (tcnt, holding the segment's length) down.
__global__ __launch_bounds__(256) void tfill_kernel(P p, int hop) {
    if (bailed(p.ctl)) return;
    const FHop& h = p.ctl->hop[hop];
    const int r = blockIdx.x * 8 + (threadIdx.x >> 5), lane = threadIdx.x & 31;
    if (r >= h.n_dst) return;
    const int32_t* tptr = p.pack + h.off[GS_PK_TPTR];
    const int32_t* nptr = p.pack + h.off[GS_PK_NBR_PTR];
    const int32_t* nbr = p.pack + h.off[GS_PK_NBR];
    const int b = nptr[r], e = nptr[r + 1];
    for (int q = b + lane; q < e; q += 32) {  // <= 33 entries
        const int c = nbr[q];
        p.traw[tptr[c] + atomicSub(&p.tcnt[c], 1) - 1] = 2 * r + 1;
    }
    if (lane == 0) {
        const int c = p.pack[h.off[GS_PK_SELF] + r];
        p.traw[tptr[c] + atomicSub(&p.tcnt[c], 1) - 1] = 2 * r;
    }
}

__device__ __forceinline__ int32_t tkey_decode(int key) { return (key & 1) ? key >> 1 : -((key >> 1) + 1); }

// One wave per source: a segment of <= 64 distinct keys rank-sorted into tidx.
__global__ __launch_bounds__(256) void tsort_kernel(P p, int hop) {
    if (bailed(p.ctl)) return;
    const FHop& h = p.ctl->hop[hop];
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (c >= h.n_src) return;
    const int32_t* tptr = p.pack + h.off[GS_PK_TPTR];
    const int b = tptr[c], len = tptr[c + 1] - b;
    if (len > 64) {
        if (lane == 0) {
            const int i = atomicAdd(&p.ctl->n_long, 1);
            if (i < p.longs_cap) p.longs[i] = c;
            else atomicOr(&p.ctl->status, kStLimit);
        }
        return;
    }
    const int key = lane < len ? p.traw[b + lane] : 0x7fffffff;
    int pos = 0;
    for (int i = 0; i < len; ++i) pos += __shfl(key, i, 64) < key;  // len is wave-uniform
    if (lane < len) p.pack[h.off[GS_PK_TIDX] + b + pos] = tkey_decode(key);
}

// One block per listed source: its keys (all < 2 n_dst) marked in an LDS
// bitmap, kLongKeys per pass, then emitted in ascending order.
__global__ __launch_bounds__(256) void tlong_kernel(P p, int hop, int per_block, int passes_max) {
    __shared__ uint32_t bits[kLongWords];
    __shared__ int sh[5];
    if (bailed(p.ctl)) return;
    const FHop& h = p.ctl->hop[hop];
    const int n_long = min(p.ctl->n_long, p.longs_cap);
    const int32_t* tptr = p.pack + h.off[GS_PK_TPTR];
    int32_t* tidx = p.pack + h.off[GS_PK_TIDX];
    const int krange = 2 * h.n_dst;
    for (int it = 0; it < per_block; ++it) {
        const int li = blockIdx.x + it * gridDim.x;
        if (li >= n_long) break;  // block-uniform
        const int c = p.longs[li];
        const int b = tptr[c], len = tptr[c + 1] - b;
        int done = 0;
        for (int pass = 0; pass < passes_max; ++pass) {
            const int lo = pass * kLongKeys;
            if (lo >= krange) break;
            for (int w = threadIdx.x; w < kLongWords; w += 256) bits[w] = 0;
            __syncthreads();
            for (int e = threadIdx.x; e < len; e += 256) {
                const int key = p.traw[b + e] - lo;
                if (key >= 0 && key < kLongKeys) atomicOr(&bits[key >> 5], 1u << (key & 31));
            }
            __syncthreads();
            constexpr int kPer = kLongWords / 256;  // consecutive words per thread
            int s = 0;
            for (int q = 0; q < kPer; ++q) s += __popc(bits[threadIdx.x * kPer + q]);
            int total;
            int at = done + block_excl_scan<4>(s, sh, &total);
            for (int q = 0; q < kPer; ++q) {
                uint32_t m = bits[threadIdx.x * kPer + q];
                while (m) {
                    const int key = lo + (threadIdx.x * kPer + q) * 32 + __ffs(m) - 1;
                    m &= m - 1;
                    if (at < len) tidx[b + at] = tkey_decode(key);
                    ++at;
                }
            }
            done += total;
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(256) void finish_kernel(P p, const int32_t* roots, int n_roots, int fail_empty,
                                                     int n_hops) {
    FCtl* c = p.ctl;
    if (bailed(c)) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int at = c->at;
    if (i < n_roots) p.pack[at + i] = roots[i];
    if (i == 0) {
        c->used = at + n_roots;
        int empty = 0;
        for (int j = 0; j < n_hops; ++j) empty += c->hop[j].n_empty;
        if (fail_empty && empty) atomicOr(&c->status, kStEmpty);
    }
}

// ------------------------------------------------------------------ handle
struct Fast {
    int32_t n_hops = 0;
    int32_t fanouts[GS_MAX_HOPS] = {};
    int32_t flags = 0;
    int64_t max_roots = 0;
    int64_t nd_max[GS_MAX_HOPS] = {};
    int64_t tidx_max[GS_MAX_HOPS] = {};
    const gs_graph* host_graph = nullptr;
    uint64_t seed = 0;
    P p{};
    int32_t nb_max = 0;  // scan blocks of the largest scan
    // freed after the destructor's wait: ring first (declared last), then mem
    DevArena mem{"fast sampler"};
    RunRing<FCtl> ring;

    ~Fast() { (void)ring.wait_last_if_any(); }
};

Fast* fast_create(const gs_graph* gp, const int32_t* fanouts, int32_t n_hops, int64_t max_roots, int32_t flags) {
    GS_REQUIRE(gp && fanouts, GS_EINVAL, "NULL argument");
    GS_REQUIRE(n_hops >= 1 && n_hops <= GS_MAX_HOPS, GS_EINVAL, "n_hops out of [1, 8]");
    GS_REQUIRE(max_roots >= 1 && max_roots < (int64_t(1) << 24), GS_EINVAL, "max_roots out of range");
    const auto& g = *reinterpret_cast<const gs::Graph*>(gp);
    GS_REQUIRE(g.n_entries < (int64_t(1) << 31) && g.n_nodes < (int64_t(1) << 31) - 32 * kScanBlock, GS_ERANGE,
               "graph too large for int32 entries");
    std::unique_ptr<Fast> f(new Fast());
    f->n_hops = n_hops;
    f->flags = flags;
    f->max_roots = max_roots;
    f->host_graph = gp;
    for (int32_t j = 0; j < n_hops; ++j) {
        f->fanouts[j] = fanouts[j];
        GS_REQUIRE(fanouts[j] >= 1 && fanouts[j] <= 32, GS_EINVAL, "fast sampler: fanouts must be in [1, 32]");
    }
    P& p = f->p;
    int64_t nd = max_roots, samp_max = 1, traw_max = 1, nd_all = 1, src_max = 1;
    for (int32_t j = 0; j < n_hops; ++j) {
        const int64_t k = f->fanouts[j];
        const int64_t npos = nd * std::min<int64_t>(k, g.max_degree);
        GS_REQUIRE(npos + 2 * nd < (int64_t(1) << 30), GS_ERANGE, "sampled entries exceed int32");
        f->nd_max[j] = nd;
        p.nd_max[j] = static_cast<int32_t>(nd);
        nd_all = std::max(nd_all, nd);
        if (j + 1 < n_hops) {
            samp_max = std::max(samp_max, nd * k);
            f->tidx_max[j] = npos + 2 * nd;  // gcn: one more slot per destination, and its self row
            traw_max = std::max(traw_max, f->tidx_max[j]);
            nd = std::min<int64_t>(g.n_nodes, nd + npos);
            src_max = std::max(src_max, nd);
        }
    }
    p.row_ptr = static_cast<const int64_t*>(f->mem.upload(g.row_ptr.data(), g.row_ptr.size() * sizeof(int64_t)));
    p.col = static_cast<const int32_t*>(f->mem.upload(g.col.data(), g.col.size() * sizeof(int32_t)));
    p.n_nodes = static_cast<int32_t>(g.n_nodes);
    const int64_t words = (g.n_nodes + 31) / 32;
    p.n_words = static_cast<int32_t>((words + kScanBlock - 1) / kScanBlock * kScanBlock);
    p.bitmap = f->mem.alloc<uint32_t>(p.n_words);
    hip_ok(hipMemset(p.bitmap, 0, static_cast<size_t>(p.n_words) * sizeof(uint32_t)), "hipMemset(bitmap)");
    p.lid = f->mem.alloc<int32_t>(g.n_nodes);
    for (int32_t j = 0; j < n_hops; ++j) p.F[j] = f->mem.alloc<int32_t>(f->nd_max[j]);
    p.samp = f->mem.alloc<int32_t>(samp_max);
    p.cnt = f->mem.alloc<int32_t>(nd_all);
    p.nbrcnt = f->mem.alloc<int32_t>(nd_all);
    p.tcnt = f->mem.alloc<int32_t>(src_max);
    p.traw = f->mem.alloc<int32_t>(traw_max);
    p.longs_cap = static_cast<int32_t>(traw_max / 65 + 1);  // a listed segment holds > 64 of the keys
    p.longs = f->mem.alloc<int32_t>(p.longs_cap);
    f->nb_max = static_cast<int32_t>(std::max<int64_t>(p.n_words, std::max(nd_all, src_max) + kScanBlock) / kScanBlock);
    p.bsum = f->mem.alloc<int32_t>(f->nb_max + 1);
    p.ctl = f->mem.alloc<FCtl>(1);
    hip_ok(hipMemset(p.ctl, 0, sizeof(FCtl)), "hipMemset");
    p.gcn = (flags & GS_SAMPLE_GCN) ? 1 : 0;
    hip_ok(hipDeviceSynchronize(), "hipDeviceSynchronize");
    return f.release();
}

void fast_destroy(Fast* f) { delete f; }

void fast_set_seed(Fast* f, uint64_t seed) { f->seed = seed; }

int64_t fast_pack_bound(const Fast* f, int64_t n_roots) {
    if (n_roots < 1 || n_roots > f->max_roots) return -1;
    return gs_sample_pack_bound(f->host_graph, n_roots, f->fanouts, f->n_hops) + n_roots;
}

int64_t fast_runs(const Fast* f) { return f->ring.runs(); }

template <int MODE>
static void launch_scan(const P& p, int hop, int k, int64_t n_max, hipStream_t st) {
    if (MODE != kScanBitmap && n_max <= kSmallScan) {
        scan_small_kernel<MODE><<<1, 1024, 0, st>>>(p, hop, k);
        gs::check_launch("fsample scan_small_kernel");
        return;
    }
    const unsigned nb = static_cast<unsigned>((n_max + kScanBlock - 1) / kScanBlock);
    scan_a_kernel<MODE><<<nb, 256, 0, st>>>(p, hop, k);
    gs::check_launch("fsample scan_a_kernel");
    scan_b_kernel<MODE><<<1, 1024, 0, st>>>(p, hop, static_cast<int>(nb));
    gs::check_launch("fsample scan_b_kernel");
    if (MODE != kScanBitmap) {  // the bitmap's third pass is compact_kernel
        scan_c_kernel<MODE><<<nb, 256, 0, st>>>(p, hop, k);
        gs::check_launch("fsample scan_c_kernel");
    }
}

void fast_run_at(Fast* f, int64_t batch_index, const int32_t* roots, int64_t n_roots, int32_t* pack, int64_t cap,
                 hipStream_t st) {
    GS_REQUIRE(roots && pack, GS_EINVAL, "NULL argument");
    GS_REQUIRE(n_roots >= 1 && n_roots <= f->max_roots, GS_EINVAL, "n_roots out of [1, max_roots]");
    GS_REQUIRE(cap >= fast_pack_bound(f, n_roots), GS_EINVAL, "pack buffer below gs_dsampler_pack_bound");
    P p = f->p;
    p.pack = pack;
    p.cap = static_cast<int32_t>(std::min<int64_t>(cap - n_roots, (int64_t(1) << 31) - 1));
    p.seed = f->seed;
    p.batch_index = static_cast<uint64_t>(batch_index);
    const int nr = static_cast<int>(n_roots);
    const unsigned root_blocks = static_cast<unsigned>((n_roots + 255) / 256);
    hip_ok(hipMemsetAsync(p.ctl, 0, sizeof(FCtl), st), "hipMemsetAsync(ctl)");
    begin_kernel<<<root_blocks, 256, 0, st>>>(p, roots, nr);
    gs::check_launch("fsample begin_kernel");
    for (int32_t j = 0; j < f->n_hops; ++j) {
        const int k = f->fanouts[j];
        const int64_t nd = f->nd_max[j];
        const unsigned groups = static_cast<unsigned>((nd + 7) / 8);
        if (j == f->n_hops - 1) {
            launch_scan<kScanPos>(p, j, k, nd, st);
            draw_kernel<true><<<groups, 256, 0, st>>>(p, j, k);
            gs::check_launch("fsample draw_kernel");
            break;
        }
        const int64_t ns = f->nd_max[j + 1];
        draw_kernel<false><<<groups, 256, 0, st>>>(p, j, k);
        gs::check_launch("fsample draw_kernel");
        launch_scan<kScanBitmap>(p, j, k, p.n_words, st);
        compact_kernel<<<static_cast<unsigned>(p.n_words / kScanBlock), 256, 0, st>>>(p, j);
        gs::check_launch("fsample compact_kernel");
        launch_scan<kScanNbr>(p, j, k, nd, st);
        lists_kernel<<<groups, 256, 0, st>>>(p, j, k);
        gs::check_launch("fsample lists_kernel");
        launch_scan<kScanT>(p, j, k, ns, st);
        tfill_kernel<<<groups, 256, 0, st>>>(p, j);
        gs::check_launch("fsample tfill_kernel");
        tsort_kernel<<<static_cast<unsigned>((ns + 3) / 4), 256, 0, st>>>(p, j);
        gs::check_launch("fsample tsort_kernel");
        const int64_t longs_max = f->tidx_max[j] / 65 + 1;
        const int64_t grid = std::min<int64_t>(longs_max, 1024);
        tlong_kernel<<<static_cast<unsigned>(grid), 256, 0, st>>>(p, j, static_cast<int>((longs_max + grid - 1) / grid),
                                                                  static_cast<int>((2 * nd + kLongKeys - 1) / kLongKeys));
        gs::check_launch("fsample tlong_kernel");
    }
    finish_kernel<<<root_blocks, 256, 0, st>>>(p, roots, nr, (f->flags & GS_SAMPLE_FAIL_EMPTY) ? 1 : 0, f->n_hops);
    gs::check_launch("fsample finish_kernel");
    f->ring.record(p.ctl, st);
}

bool fast_run_ready(Fast* f, int64_t run) { return f->ring.ready(run); }

void fast_result_of(Fast* f, int64_t run, int64_t* hop_sizes, int64_t* offsets, int64_t* used) {
    const FCtl& c = f->ring.wait(run);
    if (c.status & kStRange) gs::fail(GS_ERANGE, "node id out of range");
    if (c.status & kStLimit) gs::fail(GS_ELIMIT, "fast sampler: a frontier or the pack outgrew its bound");
    if (c.status & kStEmpty) gs::fail(GS_EEMPTY, "empty neighbourhood");
    report_layout(c, f->n_hops, hop_sizes, offsets, used);
}

}  // namespace fs
}  // namespace gs
