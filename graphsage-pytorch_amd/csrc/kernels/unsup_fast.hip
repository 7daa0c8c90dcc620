// The counter-based extend_nodes on the device: walks, far-list
// negatives and unique_nodes_batch of a batch as a pure function of (seed,
// batch index, nodes), every random word from gs::fs::draw_word
// (host/philox.hpp; hop tag 0xF0 for the walks, 0xF1 for the negatives).  The
// host mirror (host/unsup.cpp, extend_fast_host) states the same rule
// sequentially; the two agree bit for bit.
//
//   fast_walk_kernel     one thread per (node, walk): its WALK_LEN steps into the
//                        walk's fixed candidate slots (-1 = no pair), the kept
//                        pairs counted per node (integer atomicAdd) and their
//                        members marked in the unique bitmap (atomicOr).
//   fast_scan_kernel     exclusive scan of the per-node pair counts (one block).
//   fast_compact_kernel  one wave per node: its candidates, in (walk, step)
//                        order, to the node's offset as (node, other) pairs.
//   balls, masks         unsup_ball.hip's launches; only the ascending order.
//   fast_count_kernel    has_pos and min(num_neg, |far|) per node.
//   fast_neg_kernel      one wave per node: the whole far list, or Floyd's
//                        algorithm — the lanes compute the Philox words of 64
//                        draws at once, the steps run in order with the
//                        "already chosen" test as a ballot over the list in
//                        LDS — and each pick resolved through the chunk prefix
//                        and mask (far_select_kernel's arithmetic).
//   uniq_sum / uniq_scan / uniq_compact   popcount scan of the bitmap words
//                        and the ascending compaction, which clears the words.
//
// Atomics only mark bits and count, so every order that reaches the host comes
// from a scan or from the rule.  Every grid and loop bound is a launch
// argument; no kernel waits for another block.
#include <algorithm>
#include <vector>

#include "../host/graph.hpp"
#include "../host/philox.hpp"
#include "../host/unsup_dev.hpp"
#include "block_scan.hpp"
#include "kcommon.hpp"
#include "unsup_dev_state.hpp"

namespace gs {
namespace {

constexpr int kUniqBlock = 1024;  // bitmap words per scan block: 256 threads x 4 words

__device__ __forceinline__ void mark(uint32_t* bits, int32_t x) { atomicOr(&bits[x >> 5], 1u << (x & 31)); }

__global__ __launch_bounds__(256) void fast_walk_kernel(const int32_t* __restrict__ nodes, int n, int n_walks,
                                                        int walk_len, const int64_t* __restrict__ row_ptr,
                                                        const int32_t* __restrict__ col,
                                                        const uint32_t* __restrict__ train_bits, uint64_t seed,
                                                        uint64_t batch_index, int32_t* __restrict__ cand,
                                                        int32_t* __restrict__ cnt, uint32_t* __restrict__ uniq_bits) {
    const int64_t t = blockIdx.x * int64_t(256) + threadIdx.x;
    if (t >= static_cast<int64_t>(n) * n_walks) return;
    const int r = static_cast<int>(t / n_walks), w = static_cast<int>(t % n_walks);
    const int32_t v = nodes[r];
    int32_t* c = cand + (static_cast<int64_t>(r) * n_walks + w) * walk_len;
    int32_t cur = v;
    int kept = 0;
    bool alive = true;
    for (int j = 0; j < walk_len; ++j) {
        int64_t b = 0, d = 0;
        if (alive) {
            b = row_ptr[cur];
            d = row_ptr[cur + 1] - b;
            alive = d > 0;  // an empty row ends the walk (directed input only)
        }
        if (!alive) {
            c[j] = -1;
            continue;
        }
        const uint32_t word = fs::draw_word(seed, batch_index, static_cast<uint32_t>(r), kFastHopWalk,
                                            static_cast<uint32_t>(w * walk_len + j));
        const int32_t nxt = col[b + fs::randbelow(static_cast<uint32_t>(d), word)];
        const bool keep = nxt != v && ((train_bits[nxt >> 5] >> (nxt & 31)) & 1u);
        c[j] = keep ? nxt : -1;
        if (keep) {
            mark(uniq_bits, nxt);
            ++kept;
        }
        cur = nxt;
    }
    if (kept) {
        atomicAdd(&cnt[r], kept);
        mark(uniq_bits, v);
    }
}

// off[i] = sum of cnt[0..i), *total = the sum: one block, in rounds of 1024.  off may be cnt.
__global__ __launch_bounds__(1024) void fast_scan_kernel(const int32_t* cnt, int32_t* off, int n,
                                                         int64_t* __restrict__ total_out) {
    __shared__ int sh[17];
    int run = 0;
    for (int base = 0; base < n; base += 1024) {
        const int i = base + threadIdx.x;
        const int v = i < n ? cnt[i] : 0;
        int total;
        const int ex = block_excl_scan<16>(v, sh, &total);
        if (i < n) off[i] = run + ex;
        run += total;
    }
    if (threadIdx.x == 0) *total_out = run;
}

__global__ __launch_bounds__(64) void fast_compact_kernel(const int32_t* __restrict__ nodes, int slots,
                                                          const int32_t* __restrict__ cand,
                                                          const int32_t* __restrict__ off, int64_t* __restrict__ out) {
    const int r = blockIdx.x, lane = threadIdx.x;
    const int64_t v = nodes[r];
    const int32_t* c = cand + static_cast<int64_t>(r) * slots;
    int64_t at = off[r];
    for (int base = 0; base < slots; base += 64) {
        const int s = base + lane;
        const int32_t x = s < slots ? c[s] : -1;
        const unsigned long long m = __ballot(x >= 0);
        if (x >= 0) {
            const int64_t q = at + __popcll(m & ((1ull << lane) - 1ull));
            out[2 * q] = v;
            out[2 * q + 1] = x;
        }
        at += __popcll(m);
    }
}

__global__ __launch_bounds__(256) void fast_count_kernel(const int32_t* __restrict__ nodes, int n,
                                                         const int64_t* __restrict__ row_ptr,
                                                         const int32_t* __restrict__ pre, int n_chunks, int num_neg,
                                                         int parts, uint8_t* __restrict__ has,
                                                         int32_t* __restrict__ cnt_neg) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const int32_t v = nodes[r];
    has[r] = (parts & 1) && row_ptr[v + 1] > row_ptr[v];
    cnt_neg[r] = (parts & 2) ? min(num_neg, pre[static_cast<int64_t>(r) * (n_chunks + 1) + n_chunks]) : 0;
}

__global__ __launch_bounds__(64) void fast_neg_kernel(const int32_t* __restrict__ nodes, int n_chunks,
                                                      const unsigned long long* __restrict__ M,
                                                      const int32_t* __restrict__ pre,
                                                      const int32_t* __restrict__ asc, int num_neg, uint64_t seed,
                                                      uint64_t batch_index, const int32_t* __restrict__ cnt,
                                                      const int32_t* __restrict__ off, int64_t* __restrict__ out_all,
                                                      uint32_t* __restrict__ uniq_bits) {
    __shared__ int32_t chosen[kFastMaxNeg];
    const int r = blockIdx.x, lane = threadIdx.x;
    const int k = cnt[r];  // min(num_neg, len) <= kFastMaxNeg
    if (k == 0) return;
    const int64_t v = nodes[r];
    const int32_t* p = pre + static_cast<int64_t>(r) * (n_chunks + 1);
    const unsigned long long* Mr = M + static_cast<int64_t>(r) * n_chunks;
    const int len = p[n_chunks];
    int64_t* out = out_all + 2 * static_cast<int64_t>(off[r]);
    if (lane == 0) mark(uniq_bits, static_cast<int32_t>(v));
    if (len <= num_neg) {  // the whole far list, ascending (k == len)
        for (int c = 0; c < n_chunks; ++c) {
            const unsigned long long m = Mr[c];
            if ((m >> lane) & 1ull) {
                const int q = p[c] + __popcll(m & ((1ull << lane) - 1ull));
                const int32_t x = asc[64 * c + lane];
                out[2 * q] = v;
                out[2 * q + 1] = x;
                mark(uniq_bits, x);
            }
        }
        return;
    }
    // Floyd's algorithm over [0, len): draw t picks x below len - k + t + 1, or len - k + t when x is taken
    for (int base = 0; base < k; base += 64) {
        const int tl = base + lane;
        const uint32_t mine = tl < k ? fs::draw_word(seed, batch_index, static_cast<uint32_t>(r), kFastHopNeg,
                                                     static_cast<uint32_t>(tl))
                                     : 0u;
        const int nb = min(64, k - base);
        for (int i = 0; i < nb; ++i) {
            const int t = base + i;
            const uint32_t word = __shfl(mine, i, 64);
            const uint32_t m = static_cast<uint32_t>(len - k + t);
            const int32_t x = static_cast<int32_t>(fs::randbelow(m + 1u, word));
            bool found = false;
            for (int j0 = 0; j0 < t && !found; j0 += 64) {
                const int j = j0 + lane;
                found = __ballot(j < t && chosen[j] == x) != 0ull;
            }
            if (lane == 0) chosen[t] = found ? static_cast<int32_t>(m) : x;
            __syncthreads();  // one wave: the LDS write before the next step's reads
        }
    }
    for (int t = lane; t < k; t += 64) {
        const int j = chosen[t];
        int lo = 0, hi = n_chunks - 1;  // last chunk with p[c] <= j
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (p[mid] <= j) lo = mid;
            else hi = mid - 1;
        }
        unsigned long long m = Mr[lo];
        for (int s = j - p[lo]; s > 0; --s) m &= m - 1;
        const int32_t x = asc[64 * lo + __ffsll(m) - 1];
        out[2 * t] = v;
        out[2 * t + 1] = x;
        mark(uniq_bits, x);
    }
}

__device__ __forceinline__ int words_pop(const uint32_t* w) {
    return __popc(w[0]) + __popc(w[1]) + __popc(w[2]) + __popc(w[3]);
}

// bsum[b] = set bits of block b's kUniqBlock words.
__global__ __launch_bounds__(256) void uniq_sum_kernel(const uint32_t* __restrict__ bits, int32_t* __restrict__ bsum) {
    __shared__ int sh[5];
    const uint4 q = *reinterpret_cast<const uint4*>(bits + (static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x) * 4);
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
    int total;
    (void)block_excl_scan<4>(words_pop(w), sh, &total);
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// The ids of the set bits, ascending, to out[bsum[b] + rank ..]; the words are cleared.
__global__ __launch_bounds__(256) void uniq_compact_kernel(uint32_t* __restrict__ bits,
                                                           const int32_t* __restrict__ bsum,
                                                           int64_t* __restrict__ out) {
    __shared__ int sh[5];
    const int64_t w0 = (static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x) * 4;
    const uint4 q = *reinterpret_cast<const uint4*>(bits + w0);
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
    const int s = words_pop(w);
    int total;
    int64_t rank = block_excl_scan<4>(s, sh, &total) + bsum[blockIdx.x];
    if (s == 0) return;  // after the block's last barrier
#pragma unroll
    for (int i = 0; i < 4; ++i)
        for (uint32_t m = w[i]; m; m &= m - 1) out[rank++] = (w0 + i) * 32 + (__ffs(m) - 1);
    *reinterpret_cast<uint4*>(bits + w0) = make_uint4(0u, 0u, 0u, 0u);
}

void fast_resident(UnsupDev* d, const Graph& g, const std::vector<uint8_t>& is_train) {
    if (d->row_ptr) return;
    const int64_t n = g.n_nodes;
    const int64_t words = (n + 31) / 32;
    std::vector<uint32_t> tb(static_cast<size_t>(std::max<int64_t>(words, 1)), 0u);
    for (int64_t v = 0; v < n; ++v)
        if (is_train[static_cast<size_t>(v)]) tb[static_cast<size_t>(v >> 5)] |= 1u << (v & 31);
    d->uniq_words = std::max<int64_t>(1, (words + kUniqBlock - 1) / kUniqBlock) * kUniqBlock;
    d->uniq_bits = d->mem.alloc<uint32_t>(d->uniq_words);
    hip_ok(hipMemset(d->uniq_bits, 0, static_cast<size_t>(d->uniq_words) * sizeof(uint32_t)), "hipMemset(unsup fast)");
    d->uniq_bsum = d->mem.alloc<int32_t>(d->uniq_words / kUniqBlock + 1);
    d->train_bits = static_cast<const uint32_t*>(d->mem.upload(tb.data(), tb.size() * sizeof(uint32_t)));
    d->col = static_cast<const int32_t*>(d->mem.upload(g.col.data(), static_cast<size_t>(g.row_ptr[n]) * sizeof(int32_t)));
    d->row_ptr = static_cast<const int64_t*>(d->mem.upload(g.row_ptr.data(), static_cast<size_t>(n + 1) * sizeof(int64_t)));
}

template <typename T>
void grow_to(UnsupDev* d, T*& p, int64_t& cap, int64_t need) {
    if (need <= cap && p) return;
    const int64_t to = std::max<int64_t>(need, cap + cap / 2);
    d->regrow(p, to);
    cap = to;
}

}  // namespace

void unsup_dev_fast_phases(UnsupDev* d, int enable, double* ms) {
    if (ms) std::copy(d->phase_ms, d->phase_ms + kFastPhases, ms);
    d->phases_on = enable != 0;
    if (d->phases_on && !d->ev[0])
        for (hipEvent_t& e : d->ev) hip_ok(hipEventCreate(&e), "hipEventCreate(unsup fast)");
}

void unsup_dev_extend_fast(UnsupDev* d, const Graph& g, const std::vector<uint8_t>& is_train, const FastExtend& a,
                           const std::vector<int64_t>& nodes, std::vector<int64_t>& unique, std::vector<int64_t>& pos,
                           std::vector<int64_t>& neg, std::vector<int64_t>& pos_cnt, std::vector<int64_t>& neg_cnt,
                           std::vector<uint8_t>& has_pos) {
    const int64_t n64 = static_cast<int64_t>(nodes.size());
    unique.clear();
    pos.clear();
    neg.clear();
    pos_cnt.assign(nodes.size(), 0);
    neg_cnt.assign(nodes.size(), 0);
    has_pos.assign(nodes.size(), 0);
    if (n64 == 0) return;  // no nodes: no launch
    const int n = static_cast<int>(n64);
    const bool walks = (a.parts & 1) != 0, negs = (a.parts & 2) != 0;
    const int slots = walks ? a.n_walks * a.walk_len : 0;
    const int64_t kk = negs ? std::min<int64_t>(a.num_neg, d->n_order) : 0;
    fast_resident(d, g, is_train);
    if (n > d->cap_fast_n) {
        const int cap = std::max(n, 64);
        d->regrow(d->f_cnt, 2 * static_cast<int64_t>(cap));
        d->regrow(d->f_off, 2 * static_cast<int64_t>(cap));
        d->regrow(d->f_has, cap);
        d->regrow(d->f_nodes, cap);
        if (!d->f_totals) d->f_totals = d->mem.alloc<int64_t>(4);
        d->cap_fast_n = cap;
    }
    if (negs) unsup_dev_reserve_roots(d, n);  // the ball bitmaps: not for the walks alone
    grow_to(d, d->f_cand, d->cap_cand, n64 * slots);
    grow_to(d, d->f_pos, d->cap_pos, 2 * n64 * slots);
    grow_to(d, d->f_neg, d->cap_neg, 2 * n64 * kk);
    grow_to(d, d->f_uniq, d->cap_uniq, std::min<int64_t>(g.n_nodes, n64 * (1 + slots + kk)));
    const int cap = d->cap_fast_n;
    int32_t *cnt_pos = d->f_cnt, *cnt_neg = d->f_cnt + cap, *off_pos = d->f_off, *off_neg = d->f_off + cap;
    hipStream_t st = d->st;
    const bool timed = d->phases_on;
    auto stamp = [&](int i) {
        if (timed) hip_ok(hipEventRecord(d->ev[i], st), "hipEventRecord(unsup fast)");
    };

    std::vector<int32_t> r32(nodes.begin(), nodes.end());  // alive until the first synchronise
    stamp(0);
    hip_ok(hipMemcpyAsync(d->f_nodes, r32.data(), n * sizeof(int32_t), hipMemcpyHostToDevice, st), "hipMemcpyAsync");
    hip_ok(hipMemsetAsync(d->f_cnt, 0, 2 * static_cast<size_t>(cap) * sizeof(int32_t), st), "hipMemsetAsync");
    if (walks && slots > 0) {
        const int64_t threads = n64 * a.n_walks;
        fast_walk_kernel<<<static_cast<unsigned>((threads + 255) / 256), 256, 0, st>>>(
            d->f_nodes, n, a.n_walks, a.walk_len, d->row_ptr, d->col, d->train_bits, a.seed,
            static_cast<uint64_t>(a.batch_index), d->f_cand, cnt_pos, d->uniq_bits);
        check_launch("fast_walk_kernel");
    }
    fast_scan_kernel<<<1, 1024, 0, st>>>(cnt_pos, off_pos, n, d->f_totals);
    check_launch("fast_scan_kernel");
    if (walks && slots > 0) {
        fast_compact_kernel<<<n, 64, 0, st>>>(d->f_nodes, slots, d->f_cand, off_pos, d->f_pos);
        check_launch("fast_compact_kernel");
    }
    stamp(1);
    if (negs) {
        hip_ok(hipMemcpyAsync(d->roots, d->f_nodes, n * sizeof(int32_t), hipMemcpyDeviceToDevice, st), "hipMemcpyAsync");
        unsup_dev_launch_balls(d, n, a.n_walk_len, false);
    }
    stamp(2);
    if (negs) unsup_dev_launch_masks(d, n, 1, 2);
    stamp(3);
    fast_count_kernel<<<(n + 255) / 256, 256, 0, st>>>(d->f_nodes, n, d->row_ptr, d->pre[1], d->n_chunks,
                                                        static_cast<int>(a.num_neg), a.parts, d->f_has, cnt_neg);
    check_launch("fast_count_kernel");
    fast_scan_kernel<<<1, 1024, 0, st>>>(cnt_neg, off_neg, n, d->f_totals + 1);
    check_launch("fast_scan_kernel");
    if (negs && kk > 0) {
        fast_neg_kernel<<<n, 64, 0, st>>>(d->f_nodes, d->n_chunks, d->M[1], d->pre[1], d->asc_order,
                                           static_cast<int>(a.num_neg), a.seed, static_cast<uint64_t>(a.batch_index),
                                           cnt_neg, off_neg, d->f_neg, d->uniq_bits);
        check_launch("fast_neg_kernel");
    }
    stamp(4);
    const unsigned ub = static_cast<unsigned>(d->uniq_words / kUniqBlock);
    uniq_sum_kernel<<<ub, 256, 0, st>>>(d->uniq_bits, d->uniq_bsum);
    check_launch("uniq_sum_kernel");
    fast_scan_kernel<<<1, 1024, 0, st>>>(d->uniq_bsum, d->uniq_bsum, static_cast<int>(ub), d->f_totals + 2);
    check_launch("fast_scan_kernel");
    uniq_compact_kernel<<<ub, 256, 0, st>>>(d->uniq_bits, d->uniq_bsum, d->f_uniq);
    check_launch("uniq_compact_kernel");
    stamp(5);

    // the sizes, then the arrays: the call's two synchronisations
    std::vector<int32_t> cnt(2 * static_cast<size_t>(n));
    int64_t totals[3] = {0, 0, 0};
    hip_ok(hipMemcpyAsync(cnt.data(), cnt_pos, n * sizeof(int32_t), hipMemcpyDeviceToHost, st), "hipMemcpyAsync");
    hip_ok(hipMemcpyAsync(cnt.data() + n, cnt_neg, n * sizeof(int32_t), hipMemcpyDeviceToHost, st), "hipMemcpyAsync");
    hip_ok(hipMemcpyAsync(has_pos.data(), d->f_has, n, hipMemcpyDeviceToHost, st), "hipMemcpyAsync");
    hip_ok(hipMemcpyAsync(totals, d->f_totals, sizeof(totals), hipMemcpyDeviceToHost, st), "hipMemcpyAsync");
    hip_ok(hipStreamSynchronize(st), "hipStreamSynchronize");
    if (totals[0] > n64 * slots || totals[1] > n64 * kk || totals[2] > d->cap_uniq)
        fail(GS_EHIP, "unsup fast: the device reported more pairs than the batch can have");
    for (int i = 0; i < n; ++i) {
        pos_cnt[static_cast<size_t>(i)] = cnt[static_cast<size_t>(i)];
        neg_cnt[static_cast<size_t>(i)] = cnt[static_cast<size_t>(n + i)];
    }
    pos.resize(static_cast<size_t>(2 * totals[0]));
    neg.resize(static_cast<size_t>(2 * totals[1]));
    unique.resize(static_cast<size_t>(totals[2]));
    auto down = [&](std::vector<int64_t>& v, const int64_t* src) {
        if (!v.empty())
            hip_ok(hipMemcpyAsync(v.data(), src, v.size() * sizeof(int64_t), hipMemcpyDeviceToHost, st), "hipMemcpyAsync");
    };
    down(pos, d->f_pos);
    down(neg, d->f_neg);
    down(unique, d->f_uniq);
    stamp(6);
    hip_ok(hipStreamSynchronize(st), "hipStreamSynchronize");
    if (timed)
        for (int i = 0; i < kFastPhases; ++i) {
            float ms = 0.f;
            hip_ok(hipEventElapsedTime(&ms, d->ev[i], d->ev[i + 1]), "hipEventElapsedTime(unsup fast)");
            d->phase_ms[i] = ms;
        }
}

}  // namespace gs
