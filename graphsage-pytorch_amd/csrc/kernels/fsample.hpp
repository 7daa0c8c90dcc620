// Counter-based device sampler (fsample.hip) as the gs_dsampler
// entry points (dsample.hip) and the runner reach it: a GS_DSAMPLER_FAST
// handle owns one Fast and forwards to it.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../host/common.hpp"

namespace gs {
namespace fs {

struct Fast;

Fast* fast_create(const gs_graph* g, const int32_t* fanouts, int32_t n_hops, int64_t max_roots, int32_t flags);
void fast_destroy(Fast* f);
void fast_set_seed(Fast* f, uint64_t seed);
int64_t fast_pack_bound(const Fast* f, int64_t n_roots);
void fast_run_at(Fast* f, int64_t batch_index, const int32_t* roots, int64_t n_roots, int32_t* pack, int64_t cap,
                 hipStream_t st);
int64_t fast_runs(const Fast* f);
// run < 0: the last run.  Waits for that run and reports it as
// gs_sample_pack_run would (throws its error).
void fast_result_of(Fast* f, int64_t run, int64_t* hop_sizes, int64_t* offsets, int64_t* used);
bool fast_run_ready(Fast* f, int64_t run);  // run number `run` has finished (no wait)

}  // namespace fs
}  // namespace gs
