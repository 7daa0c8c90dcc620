// Stand-alone sanitizer driver for the counter-based extend's host mirror
// (csrc/host/unsup.cpp, gs_unsup_extend_fast with no device attached): the
// 3001-node graph of tests/fast_extend_cases.py (ring lattice with self loops,
// a star of 500, a path, ten 4-cliques, isolated nodes) under its three train
// sets, at the batch sizes, num_neg values, ball depths, walk shapes and parts
// the tests use — including n = 0, num_neg = 0, an empty far list and, on the
// path with forward edges only, a dead-end walk — plus the fetch, the loss plan
// and the error paths.
//   make -C graphsage-pytorch_amd/csrc sanitize-unsup-fast
// builds it with the host sources under -fsanitize=address,undefined (the
// Makefile's ASANFLAGS) and runs it once; it prints one line and exits 0.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../include/graphsage_amd.h"

static int die(const char* what) {
    std::fprintf(stderr, "%s: %s\n", what, gs_last_error());
    return 1;
}

// One extend, fetched into buffers of exactly the reported sizes (a write past them is a heap overflow), then
// the loss plan into a buffer of exactly `used` elements.  Returns a checksum, or -1.
static int64_t extend(gs_unsup* u, uint64_t seed, int64_t bi, const std::vector<int64_t>& nodes, int64_t num_neg,
                      int32_t parts, int64_t* flag) {
    int64_t sizes[4];
    if (gs_unsup_extend_fast(u, seed, bi, nodes.data(), static_cast<int64_t>(nodes.size()), num_neg, parts, 3, sizes) !=
        GS_OK)
        return -1;
    std::vector<int64_t> uniq(sizes[0]), pos(2 * sizes[1]), neg(2 * sizes[2]), pc(nodes.size()), nc(nodes.size());
    std::vector<uint8_t> hp(nodes.size());
    if (gs_unsup_fetch(u, uniq.data(), pos.data(), neg.data(), pc.data(), nc.data(), hp.data()) != GS_OK) return -1;
    int64_t sum = sizes[3];
    for (auto x : uniq) sum += x;
    for (auto x : pos) sum += x;
    for (auto x : neg) sum += x;
    for (size_t i = 0; i < nodes.size(); ++i) sum += pc[i] + nc[i] + hp[i];
    int64_t dims[6], used = 0;
    if (gs_unsup_loss_plan(u, nullptr, 0, dims, &used) != GS_OK) return -1;
    if (parts == 3) {
        std::vector<int32_t> plan(used);
        if (gs_unsup_loss_plan(u, plan.data(), used, dims, &used) != GS_OK) return -1;
        for (auto x : plan) sum += x;
    }
    if (flag) *flag = sizes[3];
    return sum;
}

int main() {
    const int64_t n = 3001, lattice = 2400;
    std::vector<int64_t> src, dst;
    for (int64_t v = 0; v < lattice; ++v) {
        src.push_back(v), dst.push_back((v + 1) % lattice);
        src.push_back(v), dst.push_back((v + 2) % lattice);
    }
    for (int64_t v : {3, 100, 700, 1500, 2399}) src.push_back(v), dst.push_back(v);
    for (int64_t v = 2401; v <= 2899; ++v) src.push_back(2400), dst.push_back(v);
    for (int64_t v = 2900; v < 2949; ++v) src.push_back(v), dst.push_back(v + 1);
    for (int64_t c = 0; c < 10; ++c)
        for (int i = 0; i < 4; ++i)
            for (int j = i + 1; j < 4; ++j) src.push_back(2950 + 4 * c + i), dst.push_back(2950 + 4 * c + j);
    gs_graph* g = nullptr;
    if (gs_graph_build(src.data(), dst.data(), static_cast<int64_t>(src.size()), n, 2, &g) != GS_OK) return die("graph");

    std::vector<int64_t> train[3];
    for (int64_t i = 0; i < n; ++i)
        if (i % 3) train[0].push_back(i);
    for (int64_t i = 2401; i <= 2460; ++i) train[1].push_back(i);
    for (int64_t i = 10; i < lattice; i += 80) train[1].push_back(i);
    for (int64_t i = 2401; i <= 2440; ++i) train[2].push_back(i);

    const int64_t batch_sizes[] = {0, 1, 64, 65, 130}, num_negs[] = {0, 1, 6, 64, 65, 100, 1024};
    const int32_t walk_shapes[][2] = {{6, 1}, {0, 1}, {3, 2}}, depths[] = {0, 1, 5};
    const int64_t fixed[] = {2450, 2995, 2450, 300, 2400, 2405, 2949, 2900, 2950, 3, 2399, 10, 11, 2990, 2460, 2461};
    int64_t runs = 0, checksum = 0;
    uint64_t lcg = 12345;
    for (int t = 0; t < 3; ++t)
        for (const auto& ws : walk_shapes)
            for (int32_t depth : depths) {
                if (t != 1 && (ws[0] != 6 || depth != 5)) continue;  // the reference's constants on T_A and T_C
                gs_unsup* u = nullptr;
                if (gs_unsup_create(g, train[t].data(), static_cast<int64_t>(train[t].size()), ws[0], ws[1], depth, &u) !=
                    GS_OK)
                    return die("create");
                for (int64_t B : batch_sizes)
                    for (int64_t k : num_negs)
                        for (int32_t parts = 1; parts <= 3; ++parts) {
                            if (parts != 3 && (B != 65 || (k != 6 && k != 100))) continue;
                            std::vector<int64_t> nodes(B);
                            for (int64_t i = 0; i < B; ++i) {
                                lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
                                nodes[i] = i < 16 && B > 1 ? fixed[i] : static_cast<int64_t>((lcg >> 33) % n);
                            }
                            const int64_t s = extend(u, 824 + runs, runs + (B == 64 ? (int64_t(1) << 33) : 0), nodes, k,
                                                     parts, nullptr);
                            if (s < 0) return die("extend");
                            checksum += s;
                            ++runs;
                        }
                gs_unsup_destroy(u);
            }
    {  // an empty far list: T_C, a star node with neither kind of pair turns the subset flag off
        gs_unsup* u = nullptr;
        if (gs_unsup_create(g, train[2].data(), static_cast<int64_t>(train[2].size()), 6, 1, 5, &u) != GS_OK)
            return die("create");
        int64_t flag = 1;
        if (extend(u, 3, 0, {2405, 2450, 100}, 6, 3, &flag) < 0 || flag != 0) return die("empty far list");
        // error paths
        const int64_t bad[1] = {n}, ok[1] = {5};
        int64_t sizes[4];
        int good = gs_unsup_extend_fast(u, 1, 1, ok, 1, 1025, 3, 1, sizes) == GS_EINVAL;
        good &= gs_unsup_extend_fast(u, 1, 1, ok, 1, -1, 3, 1, sizes) == GS_ERANGE;
        good &= gs_unsup_extend_fast(u, 1, 1, bad, 1, 6, 3, 1, sizes) == GS_ERANGE;
        good &= gs_unsup_extend_fast(u, 1, 1, ok, 1, 6, 4, 1, sizes) == GS_EINVAL;
        good &= gs_unsup_extend_fast(u, 1, 1, nullptr, 1, 6, 3, 1, sizes) == GS_EINVAL;
        gs_unsup_destroy(u);
        gs_unsup* w = nullptr;
        if (gs_unsup_create(g, train[1].data(), static_cast<int64_t>(train[1].size()), 257, 256, 5, &w) != GS_OK)
            return die("create");
        good &= gs_unsup_extend_fast(w, 1, 1, ok, 1, 6, 3, 1, sizes) == GS_EINVAL;
        gs_unsup_destroy(w);
        if (!good) {
            std::fprintf(stderr, "an error path returned the wrong status\n");
            return 1;
        }
        ++runs;
    }
    gs_graph_destroy(g);
    {  // the path's edges forward only: 2949 is a dead end, every walk from 2947 stops there
        std::vector<int64_t> rp(n + 1, 0);
        std::vector<int32_t> col;
        std::vector<uint32_t> slot;
        std::vector<uint8_t> lg(n, 3), dirty(n, 0);
        for (int64_t v = 0; v < n; ++v) {
            if (v >= 2900 && v < 2949) {
                col.push_back(static_cast<int32_t>(v + 1));
                slot.push_back(static_cast<uint32_t>((v + 1) & 7));
            }
            rp[v + 1] = static_cast<int64_t>(col.size());
        }
        gs_graph* dg = nullptr;
        if (gs_graph_from_tables(n, rp.data(), col.data(), slot.data(), lg.data(), dirty.data(), &dg) != GS_OK)
            return die("directed graph");
        std::vector<int64_t> tr;
        for (int64_t v = 2900; v <= 2949; v += 2) tr.push_back(v);
        gs_unsup* u = nullptr;
        if (gs_unsup_create(dg, tr.data(), static_cast<int64_t>(tr.size()), 3, 4, 2, &u) != GS_OK) return die("create");
        const int64_t s = extend(u, 5, 1, {2947, 2949, 2900, 5}, 6, 3, nullptr);
        if (s < 0) return die("dead-end walk");
        int64_t pc[4];
        if (gs_unsup_fetch(u, nullptr, nullptr, nullptr, pc, nullptr, nullptr) != GS_OK || pc[0] != 3 || pc[1] != 0 ||
            pc[2] != 6 || pc[3] != 0) {
            std::fprintf(stderr, "dead-end walk: pair counts %lld %lld %lld %lld\n", (long long)pc[0], (long long)pc[1],
                         (long long)pc[2], (long long)pc[3]);
            return 1;
        }
        checksum += s;
        ++runs;
        gs_unsup_destroy(u);
        gs_graph_destroy(dg);
    }
    std::printf("unsup_fast_sanitize: %lld runs, checksum %lld, clean\n", static_cast<long long>(runs),
                static_cast<long long>(checksum));
    return 0;
}
