// Stand-alone sanitizer driver for the full-neighbourhood plan builder
// (csrc/host/full_plan.cpp): a 2000-node CSR with hubs, self loops in the
// first and in later segments, rows of degree 0, 1, seg_len, seg_len + 1 and
// 3 * seg_len + 5, an isolated last node and the highest id as a neighbour,
// planned at several seg_len with gcn on and off; every plan is recounted
// here (items cover each row once, in order; counts, flags, empty rows), its
// transposed plan (gs_full_plan_transpose; the CSR is directed) is checked
// entry by entry with its T_SRC array, the weighted mean's divisors
// (gs_full_plan_edge_denom) are recomputed, and the error paths are taken.
//   make -C graphsage-pytorch_amd/csrc sanitize-full-plan
// builds it with the host sources under -fsanitize=address,undefined (the
// Makefile's ASANFLAGS) and runs it once; it prints one line and exits 0.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../include/graphsage_amd.h"

static uint64_t state = 0x9E3779B97F4A7C15ull;
static uint64_t next_u64() {  // splitmix64
    uint64_t z = (state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "line %d: %s failed\n", __LINE__, #cond); \
            return 1;                                                      \
        }                                                                  \
    } while (0)

template <typename T>
static const T* arr(const gs_full_plan* p, int which) {
    return static_cast<const T*>(gs_full_plan_array(p, which));
}

int main() {
    const int64_t n = 2000;
    std::vector<std::vector<int32_t>> rows(n);
    const int degs[] = {0, 1, 8, 9, 29, 64, 65, 197, 1500};
    for (int64_t v = 0; v + 1 < n; ++v) {
        const int d = v < 90 ? degs[v % 9] : static_cast<int>(next_u64() % 12);
        for (int e = 0; e < d; ++e) rows[v].push_back(static_cast<int32_t>(next_u64() % n));
        std::sort(rows[v].begin(), rows[v].end());
        rows[v].erase(std::unique(rows[v].begin(), rows[v].end()), rows[v].end());
        rows[v].erase(std::remove(rows[v].begin(), rows[v].end(), static_cast<int32_t>(v)), rows[v].end());
    }
    rows[4].insert(rows[4].begin() + 2, 4);     // self loop in the first segment
    rows[8].push_back(8);                       // ... and in the last one of a hub
    rows[7].insert(rows[7].begin() + 100, 7);
    rows[100] = {100};                          // nothing but a self loop
    rows[5].push_back(static_cast<int32_t>(n - 1));
    std::vector<int64_t> row_ptr(n + 1, 0);
    std::vector<int32_t> col;
    for (int64_t v = 0; v < n; ++v) {
        col.insert(col.end(), rows[v].begin(), rows[v].end());
        row_ptr[v + 1] = static_cast<int64_t>(col.size());
    }
    int64_t plans = 0, items_total = 0;
    const int64_t seg_lens[] = {1, 8, 64, 100000, 0};
    for (int64_t seg_len : seg_lens)
        for (int gcn = 0; gcn < 2; ++gcn) {
            gs_full_plan* p = nullptr;
            if (gs_full_plan_create(row_ptr.data(), col.data(), n, gcn, seg_len, &p) != GS_OK) {
                std::fprintf(stderr, "plan: %s\n", gs_last_error());
                return 1;
            }
            int64_t dims[GS_FP_NDIMS];
            CHECK(gs_full_plan_dims(p, dims) == GS_OK);
            const int64_t sl = dims[GS_FP_SEG_LEN];
            CHECK(dims[GS_FP_N_NODES] == n && dims[GS_FP_N_ENTRIES] == row_ptr[n] && sl >= 1);
            const int32_t* items = arr<int32_t>(p, GS_FP_ITEMS);
            const int64_t* item_ptr = arr<int64_t>(p, GS_FP_ITEM_PTR);
            const int64_t* slot_ptr = arr<int64_t>(p, GS_FP_SLOT_PTR);
            const int64_t* split_ptr = arr<int64_t>(p, GS_FP_SPLIT_PTR);
            const int32_t* split_rows = arr<int32_t>(p, GS_FP_SPLIT_ROWS);
            const int32_t* cnt = arr<int32_t>(p, GS_FP_COUNT);
            const uint8_t* self_loop = arr<uint8_t>(p, GS_FP_SELF_LOOP);
            const int32_t* empty_rows = arr<int32_t>(p, GS_FP_EMPTY_ROWS);
            int64_t it = 0, slots = 0, n_split = 0, n_empty = 0;
            for (int64_t v = 0; v < n; ++v) {
                const int64_t deg = row_ptr[v + 1] - row_ptr[v];
                CHECK(item_ptr[v] == it && slot_ptr[v] == slots && split_ptr[v] == n_split);
                int64_t covered = 0;
                int32_t s = 0;
                do {  // a row without entries keeps one empty item
                    CHECK(it < dims[GS_FP_N_ITEMS] && items[2 * it] == v && items[2 * it + 1] == s);
                    covered += std::min<int64_t>(sl, deg - covered);
                    ++it, ++s;
                } while (covered < deg);
                const int64_t n_self = std::count(rows[v].begin(), rows[v].end(), static_cast<int32_t>(v));
                CHECK(self_loop[v] == (n_self != 0));
                const int64_t c = gcn ? deg + (n_self == 0) : deg - n_self;
                CHECK(cnt[v] == c);
                if (c == 0) {
                    CHECK(n_empty < dims[GS_FP_N_EMPTY] && empty_rows[n_empty] == v);
                    ++n_empty;
                }
                if (deg > sl) {
                    CHECK(n_split < dims[GS_FP_N_SPLIT] && split_rows[n_split] == v);
                    ++n_split;
                    slots += s;
                }
            }
            CHECK(it == dims[GS_FP_N_ITEMS] && item_ptr[n] == it && slots == dims[GS_FP_N_SLOTS]);
            CHECK(n_split == dims[GS_FP_N_SPLIT] && n_empty == dims[GS_FP_N_EMPTY]);
            CHECK(gcn ? n_empty == 0 : n_empty >= 2);  // the isolated node and the self-loop-only row
            items_total += it;
            ++plans;
            // the transposed plan (gs_full_plan_transpose): every kept entry (v, u) of this directed CSR turns up
            // once in row u, rows ascending, v itself exactly once under gcn; counts are the forward plan's
            gs_full_plan* t = nullptr;
            CHECK(gs_full_plan_transpose(p, row_ptr.data(), col.data(), seg_len, &t) == GS_OK);
            int64_t tdims[GS_FP_NDIMS];
            CHECK(gs_full_plan_dims(t, tdims) == GS_OK && tdims[GS_FP_N_NODES] == n && tdims[GS_FP_SEG_LEN] == sl);
            const int64_t* trp = arr<int64_t>(t, GS_FP_T_ROW_PTR);
            const int32_t* tcol = arr<int32_t>(t, GS_FP_T_COL);
            const int32_t* tcnt = arr<int32_t>(t, GS_FP_COUNT);
            const int64_t* titem_ptr = arr<int64_t>(t, GS_FP_ITEM_PTR);
            const int64_t* tsrc = arr<int64_t>(t, GS_FP_T_SRC);
            CHECK(tsrc != nullptr && arr<int64_t>(p, GS_FP_T_SRC) == nullptr);
            CHECK(arr<int64_t>(p, GS_FP_T_ROW_PTR) == nullptr && arr<int32_t>(p, GS_FP_T_COL) == nullptr);
            int64_t kept = 0;
            for (int64_t v = 0; v < n; ++v) {
                kept += gcn;
                for (int32_t u : rows[v]) kept += u != v;
                CHECK(tcnt[v] == cnt[v]);
            }
            CHECK(trp[0] == 0 && trp[n] == kept && tdims[GS_FP_N_ENTRIES] == kept && tdims[GS_FP_N_EMPTY] == 0);
            for (int64_t u = 0; u < n; ++u) {
                const int64_t deg = trp[u + 1] - trp[u];
                CHECK(deg >= 0 && titem_ptr[u + 1] - titem_ptr[u] == (deg == 0 ? 1 : (deg - 1) / sl + 1));
                int64_t own = 0;
                for (int64_t e = trp[u]; e < trp[u + 1]; ++e) {
                    const int32_t v = tcol[e];
                    CHECK(v >= 0 && v < n && (e == trp[u] || tcol[e - 1] <= v));
                    own += v == u;
                    // T_SRC: the forward entry behind this one, in v's row and naming u; -1: the self entry gcn added
                    const int64_t src = tsrc[e];
                    if (src < 0) CHECK(gcn && v == u && !self_loop[u]);
                    else CHECK(src >= row_ptr[v] && src < row_ptr[v + 1] && col[src] == u);
                    CHECK(v == u || std::find(rows[v].begin(), rows[v].end(), static_cast<int32_t>(u)) != rows[v].end());
                }
                CHECK(own == gcn);
            }
            // the weighted mean's divisor: the double sum of a row's effective weights, rounded once
            std::vector<float> w(col.size()), sw(n), den(n, -1.f);
            for (size_t e = 0; e < w.size(); ++e) w[e] = 0.25f + static_cast<float>(next_u64() % 1000) / 256.f;
            for (int64_t v = 0; v < n; ++v) sw[v] = 0.5f + static_cast<float>(v % 7);
            CHECK(gs_full_plan_edge_denom(p, row_ptr.data(), col.data(), w.data(), sw.data(), den.data()) == GS_OK);
            for (int64_t v = 0; v < n; ++v) {
                double sum = 0.0;
                for (int64_t e = row_ptr[v]; e < row_ptr[v + 1]; ++e)
                    if (gcn || col[e] != v) sum += w[e];
                if (gcn && !self_loop[v]) sum += sw[v];
                CHECK(den[v] == static_cast<float>(sum));
            }
            CHECK(gs_full_plan_edge_denom(t, trp, tcol, w.data(), nullptr, den.data()) == GS_EINVAL);  // transposed
            CHECK(gs_full_plan_edge_denom(p, row_ptr.data(), col.data(), w.data(), nullptr, nullptr) == GS_EINVAL);
            gs_full_plan* tt = nullptr;
            CHECK(gs_full_plan_transpose(t, trp, tcol, seg_len, &tt) == GS_EINVAL);  // already transposed
            CHECK(gs_full_plan_transpose(p, row_ptr.data(), col.data(), seg_len, nullptr) == GS_EINVAL);
            gs_full_plan_destroy(t);
            gs_full_plan_destroy(p);
        }
    // error paths: a column id out of range, a decreasing row pointer, NULL out
    gs_full_plan* p = nullptr;
    std::vector<int32_t> bad_col = col;
    bad_col[3] = static_cast<int32_t>(n);
    CHECK(gs_full_plan_create(row_ptr.data(), bad_col.data(), n, 0, 8, &p) == GS_ERANGE);
    std::vector<int64_t> bad_ptr = row_ptr;
    bad_ptr[10] = bad_ptr[9] - 1;
    CHECK(gs_full_plan_create(bad_ptr.data(), col.data(), n, 0, 8, &p) == GS_EINVAL);
    CHECK(gs_full_plan_create(row_ptr.data(), col.data(), n, 0, 8, nullptr) == GS_EINVAL);
    CHECK(gs_full_plan_create(row_ptr.data(), col.data(), 0, 1, 8, &p) == GS_OK);  // the empty graph
    int64_t dims[GS_FP_NDIMS];
    CHECK(gs_full_plan_dims(p, dims) == GS_OK && dims[GS_FP_N_ITEMS] == 0);
    gs_full_plan_destroy(p);
    gs_full_plan_destroy(nullptr);
    std::printf("full_plan_sanitize OK: %lld plans, %lld items\n", static_cast<long long>(plans),
                static_cast<long long>(items_total));
    return 0;
}
