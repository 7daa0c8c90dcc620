// The device half of a gs_unsup (host/unsup_dev.hpp): its resident arrays and
// per-call buffers, shared by the two translation units that launch on it —
// unsup_ball.hip (the balls, the far masks and the exact path's picks) and
// unsup_fast.hip (the counter-based extend).
// Included by .hip files only.
#pragma once

#include "dev_host.hpp"

namespace gs {

constexpr int kFastPhases = 6;  // walks, balls, masks, negatives, unique, copy-back

struct UnsupDev {
    int64_t n_nodes = 0;
    int n_order = 0, n_chunks = 0;
    DevArena mem{"unsup dev"};
    const int64_t* t_ptr = nullptr;  // transposed CSR (in-neighbours) for the pulls
    const int32_t* t_col = nullptr;
    int32_t* copy_order = nullptr;  // list(set(train).copy())
    int32_t* asc_order = nullptr;   // sorted(set(train))
    int32_t* set_order = nullptr;   // list(set(train))
    int cap_roots = 0;
    unsigned long long *S = nullptr, *E = nullptr, *X = nullptr;
    int32_t* roots = nullptr;
    int64_t* counts = nullptr;  // [2][cap_roots]
    unsigned long long* M[3] = {};
    int32_t* pre[3] = {};
    int cap_req = 0;
    int32_t *req_r = nullptr, *req_j = nullptr, *picks = nullptr;
    int cap_lists = 0;
    int64_t cap_list_out = 0;
    int32_t* list_balls = nullptr;
    int64_t* list_base = nullptr;
    int32_t* list_out = nullptr;
    uint8_t* req_kind = nullptr;
    hipStream_t st = nullptr;

    // The counter-based extend (unsup_fast.hip).  Resident from its first call:
    // the forward CSR (the walks index rows in their own order), the train
    // bitmap and the all-zero unique bitmap.
    const int64_t* row_ptr = nullptr;
    const int32_t* col = nullptr;
    const uint32_t* train_bits = nullptr;  // [(n_nodes + 31) / 32]
    uint32_t* uniq_bits = nullptr;         // [uniq_words], all zero between calls
    int32_t* uniq_bsum = nullptr;          // [uniq_words / kUniqBlock + 1]
    int64_t uniq_words = 0;                // a multiple of the scan block
    int cap_fast_n = 0;
    int32_t *f_cnt = nullptr, *f_off = nullptr;  // [2][n] pair counts, [2][n] offsets
    uint8_t* f_has = nullptr;                    // [n]
    int32_t* f_nodes = nullptr;                  // [n] the batch's ids
    int64_t* f_totals = nullptr;                 // {P, N, U}
    int64_t cap_cand = 0, cap_pos = 0, cap_neg = 0, cap_uniq = 0;
    int32_t* f_cand = nullptr;                           // [n][n_walks * walk_len] walk candidates, -1 = none
    int64_t *f_pos = nullptr, *f_neg = nullptr, *f_uniq = nullptr;  // pairs (a, b) flattened; ascending ids
    bool phases_on = false;
    hipEvent_t ev[kFastPhases + 1] = {};
    double phase_ms[kFastPhases] = {};

    // A grown buffer replaces the old one, which is freed at once: every call
    // ends with a stream synchronise, so no launch still reads it.
    template <typename T>
    void regrow(T*& p, int64_t n) {
        if (p) mem.release(p);
        p = nullptr;
        p = mem.alloc<T>(n);
    }
    ~UnsupDev() {  // `mem` frees the buffers after this body
        if (st) (void)hipStreamSynchronize(st);
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
        if (st) (void)hipStreamDestroy(st);
    }
};

// The launches of one batch's balls on d->st (unsup_ball.hip), roots already in
// d->roots and the buffers reserved (unsup_dev_reserve_roots).  launch_balls:
// the two memsets, seed, `hops` pulls and, when `counts`, the ball sizes into
// d->counts.  launch_masks: the far masks and chunk prefixes of the orders
// lo .. hi - 1 (0 copy, 1 ascending, 2 set order).  Neither synchronises.
void unsup_dev_reserve_roots(UnsupDev* d, int n);
void unsup_dev_launch_balls(UnsupDev* d, int n, int hops, bool counts);
void unsup_dev_launch_masks(UnsupDev* d, int n, int lo, int hi);

}  // namespace gs
