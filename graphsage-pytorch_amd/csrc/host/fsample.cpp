// Counter-based neighbour sampler, host mirror: uniform
// without-replacement sampling as a pure function of (graph, seed,
// batch_index, roots, fanouts, flags), with no sampler state.  It writes the
// pack layout of gs_sample_pack_run; only the choice of each k-subset, the
// order of its positions and the frontier order (ascending node id instead of
// CPython set order) differ from the bit-exact sampler.  Sequential C++: this
// is the statement of the rule the device kernels (kernels/fsample.hip) are
// checked against, and a CPU entry point of its own.
//
// Per destination in slot r of F(j-1), row length deg, fanout k (1..32):
//   deg <= k : positions 0..deg-1 in row order, no draw
//   else     : Floyd's algorithm; for t = 0..k-1, m = deg-k+t,
//              x = randbelow(m+1, word(r, j, t)); append m if x is already
//              chosen, else x
// Fj = sampled neighbours ∪ F(j-1), unique, ascending.
#include <algorithm>
#include <cstring>
#include <vector>

#include "common.hpp"
#include "graph.hpp"
#include "philox.hpp"

namespace gs {
namespace fs {

// positions of one destination into pos[<= 32]; returns their count
static int32_t draw_row(uint64_t seed, uint64_t batch_index, uint32_t r, uint32_t hop, int64_t deg, int32_t k,
                        int32_t* pos) {
    if (deg <= k) {
        for (int32_t t = 0; t < deg; ++t) pos[t] = t;
        return static_cast<int32_t>(deg);
    }
    for (int32_t t = 0; t < k; ++t) {
        const int32_t m = static_cast<int32_t>(deg - k + t);
        const int32_t x = static_cast<int32_t>(
            randbelow(static_cast<uint32_t>(m) + 1u, draw_word(seed, batch_index, r, hop, static_cast<uint32_t>(t))));
        bool chosen = false;
        for (int32_t i = 0; i < t; ++i) chosen |= pos[i] == x;
        pos[t] = chosen ? m : x;
    }
    return k;
}

}  // namespace fs
}  // namespace gs

extern "C" {

int gs_philox4x32(const uint32_t* ctr, const uint32_t* key, uint32_t* out) {
    GS_API_BEGIN
    GS_REQUIRE(ctr && key && out, GS_EINVAL, "NULL argument");
    gs::fs::philox4x32_10(ctr, key, out);
    GS_API_END
}

int gs_fsample_pack_run(const gs_graph* gp, uint64_t seed, int64_t batch_index, const int64_t* roots, int64_t n_roots,
                        const int32_t* fanouts, int32_t n_hops, int32_t flags, int32_t* buf, int64_t cap,
                        int64_t* hop_sizes, int64_t* offsets, int64_t* used) {
    GS_API_BEGIN
    GS_REQUIRE(gp && roots && fanouts && buf && hop_sizes && offsets && used, GS_EINVAL, "NULL argument");
    GS_REQUIRE(n_hops >= 1 && n_hops <= GS_MAX_HOPS, GS_EINVAL, "n_hops out of [1, 8]");
    GS_REQUIRE(n_roots >= 1, GS_EINVAL, "empty nodes_batch");
    GS_REQUIRE(!(flags & ~(GS_SAMPLE_GCN | GS_SAMPLE_FAIL_EMPTY)), GS_EINVAL, "unsupported flag");
    for (int32_t j = 0; j < n_hops; ++j)
        GS_REQUIRE(fanouts[j] >= 1 && fanouts[j] <= 32, GS_EINVAL, "fanouts must be in [1, 32]");
    const auto& g = *reinterpret_cast<const gs::Graph*>(gp);
    GS_REQUIRE(g.n_entries < (int64_t(1) << 31) && g.n_nodes < (int64_t(1) << 31), GS_ERANGE,
               "graph too large for int32 pack entries");
    const int64_t bound = gs_sample_pack_bound(gp, n_roots, fanouts, n_hops);
    GS_REQUIRE(bound >= 0 && cap >= bound, GS_EINVAL, "buffer below gs_sample_pack_bound");
    for (int64_t i = 0; i < n_roots; ++i)
        GS_REQUIRE(roots[i] >= 0 && roots[i] < g.n_nodes, GS_ERANGE, "node id out of range");
    const bool gcn = flags & GS_SAMPLE_GCN;
    const uint64_t bi = static_cast<uint64_t>(batch_index);

    for (int64_t i = 0; i < GS_MAX_HOPS * GS_PK_NFIELDS; ++i) offsets[i] = -1;
    int64_t at = 0;
    auto put = [&](int32_t j, int f, int64_t n) {
        offsets[j * GS_PK_NFIELDS + f] = at;
        int32_t* p = buf + at;
        at += (n + 3) & ~int64_t(3);  // every array 16-byte aligned
        GS_REQUIRE(at + n_roots <= cap, GS_EINVAL, "pack exceeds its bound");
        return p;
    };

    std::vector<int32_t> frontier(roots, roots + n_roots), next, ids, cnt, tcur;
    std::vector<int32_t> lid(static_cast<size_t>(g.n_nodes), -1);  // node -> slot in Fj (this hop's keys only)
    std::vector<uint8_t> mark(static_cast<size_t>(g.n_nodes), 0);
    int64_t n_empty = 0;
    for (int32_t j = 0; j < n_hops; ++j) {
        const int32_t k = fanouts[j];
        const int64_t nd = static_cast<int64_t>(frontier.size());
        const bool last = j == n_hops - 1;
        int32_t pos[32];
        hop_sizes[4 * j] = nd;
        if (last) {
            int32_t* pptr = put(j, GS_PK_POS_PTR, nd + 1);
            int64_t total = 0;
            for (int64_t r = 0; r < nd; ++r) {
                pptr[r] = static_cast<int32_t>(total);
                total += std::min<int64_t>(g.degree(frontier[r]), k);
            }
            pptr[nd] = static_cast<int32_t>(total);
            int32_t* ent = put(j, GS_PK_POS, total);
            int32_t* dst = put(j, GS_PK_DST_IDS, nd);
            for (int64_t r = 0; r < nd; ++r) {
                const int32_t v = frontier[r];
                const int64_t rs = g.row_ptr[v];
                const int32_t c = gs::fs::draw_row(seed, bi, static_cast<uint32_t>(r), j + 1, g.degree(v), k, pos);
                for (int32_t t = 0; t < c; ++t) ent[pptr[r] + t] = static_cast<int32_t>(rs + pos[t]);
                dst[r] = v;
                if (!gcn) n_empty += c == 0 || (c == 1 && g.col[rs + pos[0]] == v);
            }
            hop_sizes[4 * j + 1] = total;
            hop_sizes[4 * j + 2] = hop_sizes[4 * j + 3] = -1;
            break;
        }
        // sampled neighbour ids per destination (k per slot), the union's marks
        ids.resize(static_cast<size_t>(nd * k));
        cnt.resize(static_cast<size_t>(nd));
        int64_t n_pos = 0;
        for (int64_t r = 0; r < nd; ++r) {
            const int32_t v = frontier[r];
            const int64_t rs = g.row_ptr[v];
            const int32_t c = gs::fs::draw_row(seed, bi, static_cast<uint32_t>(r), j + 1, g.degree(v), k, pos);
            cnt[r] = c;
            n_pos += c;
            mark[v] = 1;
            for (int32_t t = 0; t < c; ++t) {
                const int32_t u = g.col[rs + pos[t]];
                ids[r * k + t] = u;
                mark[u] = 1;
            }
        }
        // Fj ascending; the marks are cleared on the way (only marked bytes are touched again below)
        next.clear();
        for (int64_t v = 0; v < g.n_nodes; ++v)
            if (mark[v]) {
                lid[v] = static_cast<int32_t>(next.size());
                next.push_back(static_cast<int32_t>(v));
                mark[v] = 0;
            }
        const int64_t ns = static_cast<int64_t>(next.size());
        // neighbour lists in Fj slots, ascending; self dropped (gcn: kept once)
        int32_t* nptr = put(j, GS_PK_NBR_PTR, nd + 1);
        int64_t n_nbr = 0;
        for (int64_t r = 0; r < nd; ++r) {
            nptr[r] = static_cast<int32_t>(n_nbr);
            bool self_in = false;
            for (int32_t t = 0; t < cnt[r]; ++t) self_in |= ids[r * k + t] == frontier[r];
            const int64_t n = gcn ? cnt[r] + !self_in : cnt[r] - self_in;
            if (n == 0) ++n_empty;
            n_nbr += n;
        }
        nptr[nd] = static_cast<int32_t>(n_nbr);
        int32_t* nbr = put(j, GS_PK_NBR, n_nbr);
        int32_t* self = put(j, GS_PK_SELF, nd);
        int32_t* tptr = put(j, GS_PK_TPTR, ns + 1);
        int32_t* tidx = put(j, GS_PK_TIDX, n_nbr + nd);
        for (int64_t r = 0; r < nd; ++r) {
            const int32_t v = frontier[r];
            int32_t* out = nbr + nptr[r];
            int32_t n = 0;
            for (int32_t t = 0; t < cnt[r]; ++t)
                if (ids[r * k + t] != v) out[n++] = lid[ids[r * k + t]];
            if (gcn) out[n++] = lid[v];
            std::sort(out, out + n);
            self[r] = lid[v];
        }
        // transposed lists: per source ascending r, a row's -(r+1) before its r
        std::fill(tptr, tptr + ns + 1, 0);
        for (int64_t e = 0; e < n_nbr; ++e) ++tptr[nbr[e] + 1];
        for (int64_t r = 0; r < nd; ++r) ++tptr[self[r] + 1];
        for (int64_t c = 0; c < ns; ++c) tptr[c + 1] += tptr[c];
        tcur.assign(tptr, tptr + ns);
        for (int64_t r = 0; r < nd; ++r) {
            tidx[tcur[self[r]]++] = static_cast<int32_t>(-(r + 1));
            for (int32_t e = nptr[r]; e < nptr[r + 1]; ++e) tidx[tcur[nbr[e]]++] = static_cast<int32_t>(r);
        }
        hop_sizes[4 * j + 1] = n_pos;
        hop_sizes[4 * j + 2] = ns;
        hop_sizes[4 * j + 3] = n_nbr;
        frontier.swap(next);
    }
    if (n_empty && (flags & GS_SAMPLE_FAIL_EMPTY)) gs::fail(GS_EEMPTY, "empty neighbourhood");
    int32_t* r32 = buf + at;  // roots (int32) right after the pack
    for (int64_t i = 0; i < n_roots; ++i) r32[i] = static_cast<int32_t>(roots[i]);
    *used = at + n_roots;
    GS_API_END
}

}  // extern "C"
