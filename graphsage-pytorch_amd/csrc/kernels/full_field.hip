// The L-hop receptive field of a mini-batch, found on the device from the
// forward plan, the transposed plan and the device CSR (train.FullTrainer's
// field path):
//   R_L = nodes,  R_{l-1} = R_l U N_eff(R_l)
// with N_eff the plan's effective neighbourhood (a row's own id skipped; under
// gcn the row itself is in R_l already).
//
// One byte flag per node accumulates the levels (R_{l-1} holds R_l, so the
// flags are never cleared between levels): the roots are flagged, the flags
// are compacted into rows_L / pos_L, the plan's items and split rows are
// filtered to R_L, mark_kernel walks those items -- one wave per (row,
// segment), as the aggregate spreads a hub row over many lane groups -- and
// flags every neighbour, the flags are compacted into rows_{L-1} / pos_{L-1},
// the transposed plan is filtered to R_{L-1}, and so on down to level 0.  The
// last launch takes the flags down again by walking rows_0.
//
// A compaction is three launches -- per-block counts, one workgroup's scan of
// the block counts, a scatter -- so it keeps the input order, it is
// deterministic, and no workgroup waits on another.  What depends on a count
// only the device knows (the marks, the resets) runs on a fixed grid-stride
// grid and reads the count from memory; the host learns the counts once, in
// gs_full_field_counts.  Several lanes may store the same flag value to one
// byte: plain vector stores, no atomics.
#include "full_field.hpp"

#include <algorithm>

namespace gs {

namespace {

constexpr int64_t kAlign = 256;
constexpr int kT = 256;            // threads of a compaction workgroup
constexpr int kE = 8;              // consecutive elements per thread
constexpr int kTile = kT * kE;
constexpr int kStrideGrid = 1024;  // workgroups of a grid-stride launch

int64_t round_up(int64_t b) { return (b + kAlign - 1) / kAlign * kAlign; }

// SRC 0: element i of [0, m) is kept where flags[i] != 0 (the output is i, and pos[i] its index)
// SRC 1: element src[i] is kept where pos[src[i]] >= 0
// SRC 2: the pair src[2 i], src[2 i + 1] is kept where pos[src[2 i]] >= 0
struct CompactArgs {
    const uint8_t* flags;
    const int* src;
    const int* pos;
    int64_t m;
    int* out;
    int* out_pos;
    int* block_counts;  // [nb]: counts, then (after the scan) exclusive prefixes
    int* total;
    int nb;
};

template <int SRC>
__device__ __forceinline__ bool kept(const CompactArgs& a, int64_t i) {
    if (SRC == 0) return a.flags[i] != 0;
    return a.pos[a.src[SRC == 2 ? 2 * i : i]] >= 0;
}

// Exclusive prefix of v over the workgroup's kT threads; *sum receives the workgroup's total.
__device__ __forceinline__ int block_exclusive(int v, int* sum) {
    __shared__ int s[kT];
    const int t = threadIdx.x;
    s[t] = v;
    __syncthreads();
    for (int d = 1; d < kT; d <<= 1) {
        const int add = t >= d ? s[t - d] : 0;
        __syncthreads();
        s[t] += add;
        __syncthreads();
    }
    const int incl = s[t];
    *sum = s[kT - 1];
    __syncthreads();
    return incl - v;
}

template <int SRC>
__global__ __launch_bounds__(kT) void compact_count_kernel(CompactArgs a) {
    const int64_t i0 = blockIdx.x * int64_t(kTile) + threadIdx.x * kE;
    int c = 0;
    for (int k = 0; k < kE; ++k)
        if (i0 + k < a.m) c += kept<SRC>(a, i0 + k);
    int sum;
    block_exclusive(c, &sum);
    if (threadIdx.x == 0) a.block_counts[blockIdx.x] = sum;
}

// One workgroup: block_counts -> exclusive prefixes in place, *total = their sum.
__global__ __launch_bounds__(kT) void compact_scan_kernel(int* block_counts, int nb, int* total) {
    const int per = (nb + kT - 1) / kT;
    const int lo = min(nb, static_cast<int>(threadIdx.x) * per), hi = min(nb, lo + per);
    int c = 0;
    for (int i = lo; i < hi; ++i) c += block_counts[i];
    int sum;
    int off = block_exclusive(c, &sum);
    for (int i = lo; i < hi; ++i) {
        const int v = block_counts[i];
        block_counts[i] = off;
        off += v;
    }
    if (threadIdx.x == 0) *total = sum;
}

template <int SRC>
__global__ __launch_bounds__(kT) void compact_scatter_kernel(CompactArgs a) {
    const int64_t i0 = blockIdx.x * int64_t(kTile) + threadIdx.x * kE;
    bool keep[kE];
    int c = 0;
    for (int k = 0; k < kE; ++k) {
        keep[k] = i0 + k < a.m && kept<SRC>(a, i0 + k);
        c += keep[k];
    }
    int sum;
    int off = a.block_counts[blockIdx.x] + block_exclusive(c, &sum);  // off + c <= the kept total <= m
    for (int k = 0; k < kE; ++k) {
        if (!keep[k]) continue;
        const int64_t i = i0 + k;
        if (SRC == 0) {
            a.out[off] = static_cast<int>(i);
            a.out_pos[i] = off;
        } else if (SRC == 1) {
            a.out[off] = a.src[i];
        } else {
            reinterpret_cast<int2*>(a.out)[off] = reinterpret_cast<const int2*>(a.src)[i];
        }
        ++off;
    }
}

template <int SRC>
void compact(CompactArgs a, hipStream_t st) {
    if (a.m == 0) return;  // the caller zeroed *total
    a.nb = static_cast<int>((a.m + kTile - 1) / kTile);
    compact_count_kernel<SRC><<<dim3(a.nb), kT, 0, st>>>(a);
    compact_scan_kernel<<<dim3(1), kT, 0, st>>>(a.block_counts, a.nb, a.total);
    compact_scatter_kernel<SRC><<<dim3(a.nb), kT, 0, st>>>(a);
}

// flags[nodes[i]] = 1; an id outside [0, n) is ignored.
__global__ __launch_bounds__(kT) void flag_nodes_kernel(const int* __restrict__ nodes, int64_t B, int n,
                                                        uint8_t* __restrict__ flags) {
    const int64_t i = blockIdx.x * int64_t(kT) + threadIdx.x;
    if (i >= B) return;
    const int v = nodes[i];
    if (static_cast<unsigned>(v) < static_cast<unsigned>(n)) flags[v] = 1;
}

// One wave per compacted item (row, segment): every entry of the segment that is not the row's own id
// is flagged.  Column ids were range-checked when the plan was built.
__global__ __launch_bounds__(kT) void mark_kernel(const int* __restrict__ items, const int* __restrict__ n_items_p,
                                                  int64_t cap, const int64_t* __restrict__ row_ptr,
                                                  const int* __restrict__ col, int64_t seg_len,
                                                  uint8_t* __restrict__ flags) {
    const int64_t n_items = min(static_cast<int64_t>(*n_items_p), cap);
    const int lane = threadIdx.x % 64;
    const int64_t stride = int64_t(gridDim.x) * (kT / 64);
    for (int64_t li = blockIdx.x * int64_t(kT / 64) + threadIdx.x / 64; li < n_items; li += stride) {
        const int2 it = reinterpret_cast<const int2*>(items)[li];
        const int node = it.x, seg = it.y;
        const int64_t rb = row_ptr[node], re = row_ptr[node + 1];
        const bool split = re - rb > seg_len;
        const int64_t beg = rb + seg * seg_len;  // seg == 0 unless split
        const int64_t end = split ? min(beg + seg_len, re) : re;
        for (int64_t e = beg + lane; e < end; e += 64) {
            const int c = col[e];
            if (c != node) flags[c] = 1;
        }
    }
}

struct WalkArgs {
    const int* rows[GS_MAX_HOPS + 1];
    int* pos[GS_MAX_HOPS + 1];
    const int* counts;
};

// Level blockIdx.y of an earlier field: pos[rows[i]] = -1 for i < counts[level].
__global__ __launch_bounds__(kT) void reset_pos_kernel(WalkArgs a, int n) {
    const int l = blockIdx.y;
    const int cnt = min(a.counts[l], n);
    const int* rows = a.rows[l];
    int* pos = a.pos[l];
    for (int64_t i = blockIdx.x * int64_t(kT) + threadIdx.x; i < cnt; i += int64_t(gridDim.x) * kT) {
        const int v = rows[i];
        if (static_cast<unsigned>(v) < static_cast<unsigned>(n)) pos[v] = -1;
    }
}

// flags[rows[i]] = 0 for i < *count: the flags leave the build as they entered it.
__global__ __launch_bounds__(kT) void clear_flags_kernel(const int* __restrict__ rows, const int* __restrict__ count,
                                                         int n, uint8_t* __restrict__ flags) {
    const int cnt = min(*count, n);
    for (int64_t i = blockIdx.x * int64_t(kT) + threadIdx.x; i < cnt; i += int64_t(gridDim.x) * kT)
        flags[rows[i]] = 0;
}

unsigned stride_grid(int64_t upper, int per_block) {
    return static_cast<unsigned>(std::max<int64_t>(1, std::min<int64_t>(kStrideGrid, (upper + per_block - 1) / per_block)));
}

void check_plans(const FullPlan& p, const FullPlan& tp, int L) {
    GS_REQUIRE(L >= 1 && L <= GS_MAX_HOPS, GS_EINVAL, "1 to 8 layers");
    GS_REQUIRE(p.n >= 1, GS_EINVAL, "empty graph");
    GS_REQUIRE(!p.transposed && tp.transposed && tp.n == p.n && tp.gcn == p.gcn, GS_EINVAL,
               "tplan must be the forward plan's transpose");
}

}  // namespace

FieldLayout field_layout(const FullPlan& p, const FullPlan& tp, int L) {
    check_plans(p, tp, L);
    FieldLayout lo;
    const int64_t n = p.n;
    const int64_t n_items = static_cast<int64_t>(p.items.size() / 2), n_t_items = static_cast<int64_t>(tp.items.size() / 2);
    int64_t off = 0;
    auto take = [&](int64_t bytes) {
        const int64_t at = off;
        off += round_up(std::max<int64_t>(bytes, 4));
        return at;
    };
    lo.counts = take(GS_FF_NCOUNTS * 4);
    lo.flags = take(n);
    lo.scan_ints = (std::max(std::max(n, n_items), n_t_items) + kTile - 1) / kTile;
    lo.scan = take(lo.scan_ints * 4);
    // the pos maps lie together: a first build clears them with one memset
    for (int l = 0; l <= L; ++l) lo.pos[l] = take(n * 4);
    for (int l = 0; l <= L; ++l) lo.rows[l] = take(n * 4);
    lo.items[0] = lo.split[0] = lo.t_items[0] = lo.t_split[0] = -1;
    for (int l = 1; l <= L; ++l) {
        lo.items[l] = take(n_items * 8);
        lo.split[l] = take(static_cast<int64_t>(p.split_rows.size()) * 4);
        lo.t_items[l] = take(n_t_items * 8);
        lo.t_split[l] = take(static_cast<int64_t>(tp.split_rows.size()) * 4);
    }
    lo.total = off;
    return lo;
}

static void check_field(const FieldLayout& lo, const gs_full_field& f) {
    GS_REQUIRE(f.buf && f.buf_bytes >= lo.total && (reinterpret_cast<uintptr_t>(f.buf) & (kAlign - 1)) == 0, GS_EINVAL,
               "field buffer smaller than gs_full_field_bytes or not 256-byte aligned");
}

FieldLayer field_layer(const FullPlan& p, const FullPlan& tp, const gs_full_field& f, int layer) {
    const FieldLayout lo = field_layout(p, tp, f.n_layers);
    check_field(lo, f);
    GS_REQUIRE(layer >= 1 && layer <= f.n_layers, GS_EINVAL, "layer outside the field's 1 .. n_layers");
    const char* b = static_cast<const char*>(f.buf);
    auto ip = [&](int64_t o) { return reinterpret_cast<const int*>(b + o); };
    FieldLayer fl;
    fl.rows = ip(lo.rows[layer]);
    fl.pos = ip(lo.pos[layer]);
    fl.rows_prev = ip(lo.rows[layer - 1]);
    fl.pos_prev = ip(lo.pos[layer - 1]);
    fl.items = ip(lo.items[layer]);
    fl.split = ip(lo.split[layer]);
    fl.t_items = ip(lo.t_items[layer]);
    fl.t_split = ip(lo.t_split[layer]);
    const int64_t* c = f.counts + GS_FF_LAYER0 + 4 * (layer - 1);
    fl.n = f.counts[layer];
    fl.n_prev = f.counts[layer - 1];
    fl.n_items = c[0];
    fl.n_split = c[1];
    fl.n_t_items = c[2];
    fl.n_t_split = c[3];
    GS_REQUIRE(fl.n >= 1 && fl.n <= fl.n_prev && fl.n_prev <= p.n && fl.n_items >= fl.n &&
                   fl.n_items <= static_cast<int64_t>(p.items.size() / 2) && fl.n_split >= 0 &&
                   fl.n_split <= static_cast<int64_t>(p.split_rows.size()) && fl.n_t_items >= fl.n_prev &&
                   fl.n_t_items <= static_cast<int64_t>(tp.items.size() / 2) && fl.n_t_split >= 0 &&
                   fl.n_t_split <= static_cast<int64_t>(tp.split_rows.size()),
               GS_EINVAL, "the field's counts do not fit its plans (gs_full_field_counts after the build?)");
    return fl;
}

static void field_build(const FullPlan& p, const gs_full_plan_dev& d, const FullPlan& tp, const gs_full_plan_dev& td,
                        const int64_t* row_ptr, const int32_t* col, const int32_t* nodes, int64_t B, int rebuild,
                        const gs_full_field& f, hipStream_t st) {
    const int L = f.n_layers;
    const FieldLayout lo = field_layout(p, tp, L);
    check_field(lo, f);
    const int64_t n = p.n;
    const int64_t n_items = static_cast<int64_t>(p.items.size() / 2), n_t_items = static_cast<int64_t>(tp.items.size() / 2);
    const int64_t n_split = static_cast<int64_t>(p.split_rows.size()), n_t_split = static_cast<int64_t>(tp.split_rows.size());
    GS_REQUIRE(row_ptr && col && nodes && d.items && td.items, GS_EINVAL, "NULL device pointer");
    GS_REQUIRE((n_split == 0 || d.split_rows) && (n_t_split == 0 || td.split_rows), GS_EINVAL, "NULL split_rows");
    GS_REQUIRE(B >= 1 && B <= n, GS_EINVAL, "nodes: 1 to n_nodes ids");
    char* b = static_cast<char*>(f.buf);
    auto ip = [&](int64_t o) { return reinterpret_cast<int*>(b + o); };
    int* counts = ip(lo.counts);
    uint8_t* flags = reinterpret_cast<uint8_t*>(b + lo.flags);
    const int64_t seg_len = std::min<int64_t>(p.seg_len, (int64_t(1) << 31) - 1);

    if (rebuild) {  // the earlier field's maps, by walking its rows; its flags are down already
        WalkArgs w;
        for (int l = 0; l <= GS_MAX_HOPS; ++l) {
            w.rows[l] = ip(lo.rows[std::min(l, L)]);
            w.pos[l] = ip(lo.pos[std::min(l, L)]);
        }
        w.counts = counts;
        reset_pos_kernel<<<dim3(stride_grid(n, kT), L + 1), kT, 0, st>>>(w, static_cast<int>(n));
    } else {
        GS_REQUIRE(hipMemsetAsync(b + lo.pos[0], 0xFF, lo.rows[0] - lo.pos[0], st) == hipSuccess, GS_EHIP, "memset failed");
        GS_REQUIRE(hipMemsetAsync(flags, 0, n, st) == hipSuccess, GS_EHIP, "memset failed");
    }
    GS_REQUIRE(hipMemsetAsync(counts, 0, GS_FF_NCOUNTS * 4, st) == hipSuccess, GS_EHIP, "memset failed");
    flag_nodes_kernel<<<dim3(static_cast<unsigned>((B + kT - 1) / kT)), kT, 0, st>>>(nodes, B, static_cast<int>(n), flags);

    CompactArgs a{};
    a.block_counts = ip(lo.scan);
    auto level = [&](int l) {  // the flags -> rows_l, pos_l, counts[l]
        a.flags = flags;
        a.m = n;
        a.out = ip(lo.rows[l]);
        a.out_pos = ip(lo.pos[l]);
        a.total = counts + l;
        compact<0>(a, st);
    };
    auto filter = [&](const int* src, int64_t m, bool pairs, const int* pos, int64_t out, int slot) {
        a.src = src;
        a.pos = pos;
        a.m = m;
        a.out = ip(out);
        a.total = counts + slot;
        if (pairs) compact<2>(a, st);
        else compact<1>(a, st);
    };
    level(L);
    for (int l = L; l >= 1; --l) {
        const int c0 = GS_FF_LAYER0 + 4 * (l - 1);
        filter(d.items, n_items, true, ip(lo.pos[l]), lo.items[l], c0);
        filter(d.split_rows, n_split, false, ip(lo.pos[l]), lo.split[l], c0 + 1);
        mark_kernel<<<dim3(stride_grid(n_items, kT / 64)), kT, 0, st>>>(ip(lo.items[l]), counts + c0, n_items, row_ptr,
                                                                        col, seg_len, flags);
        level(l - 1);
        filter(td.items, n_t_items, true, ip(lo.pos[l - 1]), lo.t_items[l], c0 + 2);
        filter(td.split_rows, n_t_split, false, ip(lo.pos[l - 1]), lo.t_split[l], c0 + 3);
    }
    clear_flags_kernel<<<dim3(stride_grid(n, kT)), kT, 0, st>>>(ip(lo.rows[0]), counts, static_cast<int>(n), flags);
    check_launch("gs_full_field_build");
}

}  // namespace gs

extern "C" {

int64_t gs_full_field_bytes(const gs_full_plan* plan, const gs_full_plan* tplan, int32_t n_layers) {
    GS_BYTES_BEGIN
    if (!plan || !tplan) return -1;
    return gs::field_layout(*reinterpret_cast<const gs::FullPlan*>(plan),
                            *reinterpret_cast<const gs::FullPlan*>(tplan), n_layers).total;
    GS_BYTES_END
}

int64_t gs_full_field_offset(const gs_full_plan* plan, const gs_full_plan* tplan, int32_t n_layers, int32_t which,
                             int32_t level) {
    GS_BYTES_BEGIN
    if (!plan || !tplan || level < 0 || level > n_layers) return -1;
    const gs::FieldLayout lo = gs::field_layout(*reinterpret_cast<const gs::FullPlan*>(plan),
                                                *reinterpret_cast<const gs::FullPlan*>(tplan), n_layers);
    switch (which) {
        case GS_FF_ROWS: return lo.rows[level];
        case GS_FF_POS: return lo.pos[level];
        case GS_FF_ITEMS: return lo.items[level];
        case GS_FF_SPLIT: return lo.split[level];
        case GS_FF_T_ITEMS: return lo.t_items[level];
        case GS_FF_T_SPLIT: return lo.t_split[level];
        default: return -1;
    }
    GS_BYTES_END
}

int gs_full_field_build(const gs_full_plan* plan, const gs_full_plan_dev* dev, const gs_full_plan* tplan,
                        const gs_full_plan_dev* tdev, const int64_t* row_ptr, const int32_t* col, const int32_t* nodes,
                        int64_t n_nodes, int32_t rebuild, gs_full_field* f, void* stream) {
    GS_API_BEGIN
    GS_REQUIRE(plan && dev && tplan && tdev && f, GS_EINVAL, "NULL argument");
    gs::field_build(*reinterpret_cast<const gs::FullPlan*>(plan), *dev, *reinterpret_cast<const gs::FullPlan*>(tplan),
                    *tdev, row_ptr, col, nodes, n_nodes, rebuild, *f, gs::as_stream(stream));
    GS_API_END
}

int gs_full_field_counts(const gs_full_plan* plan, const gs_full_plan* tplan, gs_full_field* f, void* stream) {
    GS_API_BEGIN
    GS_REQUIRE(plan && tplan && f, GS_EINVAL, "NULL argument");
    const gs::FieldLayout lo = gs::field_layout(*reinterpret_cast<const gs::FullPlan*>(plan),
                                                *reinterpret_cast<const gs::FullPlan*>(tplan), f->n_layers);
    gs::check_field(lo, *f);
    int32_t c[GS_FF_NCOUNTS];
    hipStream_t st = gs::as_stream(stream);
    GS_REQUIRE(hipMemcpyAsync(c, static_cast<const char*>(f->buf) + lo.counts, sizeof(c), hipMemcpyDeviceToHost, st) ==
                   hipSuccess, GS_EHIP, "copy failed");
    GS_REQUIRE(hipStreamSynchronize(st) == hipSuccess, GS_EHIP, "synchronise failed");
    for (int i = 0; i < GS_FF_NCOUNTS; ++i) f->counts[i] = c[i];
    GS_API_END
}

}  // extern "C"
