#pragma once
// Host image of the full-neighbourhood aggregate's work plan (full_plan.cpp).
#include <cstdint>
#include <memory>
#include <vector>

#include "common.hpp"

namespace gs {

struct FullPlan {
    int64_t n = 0, seg_len = 0, n_entries = 0;
    bool gcn = false;
    std::vector<int32_t> items;       // [n_items][2]: (row, segment)
    std::vector<int64_t> item_ptr;    // [n + 1]: first item of each row
    std::vector<int64_t> slot_ptr;    // [n + 1]: partial slots before each row (split rows own one per item)
    std::vector<int64_t> split_ptr;   // [n + 1]: split rows before each row
    std::vector<int32_t> split_rows;  // rows of more than seg_len entries, ascending
    std::vector<int32_t> cnt;         // [n]: effective neighbour count
    std::vector<uint8_t> self_loop;   // [n]: the row holds its own id
    std::vector<int32_t> empty_rows;  // rows with cnt == 0, ascending
    // A transposed plan (full_plan_transpose) owns its CSR: row u lists the destinations v whose effective
    // neighbourhood holds u, ascending.  Its cnt is the forward plan's (the MEAN divisor of each destination),
    // self_loop is all zero and empty_rows stays empty.
    bool transposed = false;
    std::vector<int64_t> t_row_ptr;   // [n + 1]
    std::vector<int32_t> t_col;       // [t_row_ptr[n]]
    std::vector<int64_t> t_src;       // [t_row_ptr[n]]: the forward entry behind each one, -1: the self entry gcn added
};

// Throws gs::Error; seg_len <= 0: no row is split.
FullPlan* full_plan_build(const int64_t* row_ptr, const int32_t* col, int64_t n, int gcn, int64_t seg_len);
// Rows of [row0, row0 + n_rows) with an empty effective neighbourhood.
// The plan of the backward aggregate: the transpose of (row_ptr, col) under fwd's effective-neighbourhood
// rules, cut into segments of seg_len (<= 0: no row is split).  (row_ptr, col) must be the CSR fwd was built from.
FullPlan* full_plan_transpose(const FullPlan& fwd, const int64_t* row_ptr, const int32_t* col, int64_t seg_len);
int64_t full_plan_empty_in(const FullPlan& p, int64_t row0, int64_t n_rows);

}  // namespace gs
