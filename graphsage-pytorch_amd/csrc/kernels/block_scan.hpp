// Wave and block prefix sums shared by the device samplers' kernels
// (dsample.hip, dsample_union.hip, fsample.hip).
#pragma once

#include "kcommon.hpp"

namespace gs {

__device__ __forceinline__ int32_t al4(int32_t n) { return (n + 3) & ~3; }

__device__ __forceinline__ int warp_incl_scan(int v) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(v, o, 64);
        if ((threadIdx.x & 63) >= o) v += t;
    }
    return v;
}
__device__ __forceinline__ float warp_incl_scan(float v) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float t = __shfl_up(v, o, 64);
        if ((threadIdx.x & 63) >= o) v += t;
    }
    return v;
}

// Exclusive scan of one value per thread over a block of NW waves; returns
// the thread's exclusive prefix, *total the block's sum.  sh: NW + 1 values.
template <int NW, typename T>
__device__ __forceinline__ T block_excl_scan(T v, T* sh, T* total) {
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const T inc = warp_incl_scan(v);
    if (lane == 63) sh[w] = inc;
    __syncthreads();
    if (threadIdx.x == 0) {
        T run = T(0);
        for (int q = 0; q < NW; ++q) {
            const T t = sh[q];
            sh[q] = run;
            run += t;
        }
        sh[NW] = run;
    }
    __syncthreads();
    const T out = sh[w] + inc - v;
    *total = sh[NW];
    __syncthreads();
    return out;
}

}  // namespace gs
