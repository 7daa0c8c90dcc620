// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3",
// SC'11) and the draw rule of the counter-based sampler, shared
// by the host mirror (host/fsample.cpp) and the device kernels
// (kernels/fsample.hip): one definition, so both sides state the same rule.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GS_HD __host__ __device__ __forceinline__
#define GS_UNROLL _Pragma("unroll")
#else
#define GS_HD inline
#define GS_UNROLL
#endif

namespace gs {
namespace fs {

GS_HD void philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
    uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3];
    uint32_t k0 = key[0], k1 = key[1];
    GS_UNROLL
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = static_cast<uint64_t>(0xD2511F53u) * c0;
        const uint64_t p1 = static_cast<uint64_t>(0xCD9E8D57u) * c2;
        const uint32_t n0 = static_cast<uint32_t>(p1 >> 32) ^ c1 ^ k0;
        const uint32_t n1 = static_cast<uint32_t>(p1);
        const uint32_t n2 = static_cast<uint32_t>(p0 >> 32) ^ c3 ^ k1;
        const uint32_t n3 = static_cast<uint32_t>(p0);
        c0 = n0;
        c1 = n1;
        c2 = n2;
        c3 = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0;
    out[1] = c1;
    out[2] = c2;
    out[3] = c3;
}

// The random word of draw t of the destination in slot r of F(hop - 1),
// hop 1-based: counter (r, hop << 24 | t / 4, batch_index), output word t % 4.
GS_HD uint32_t draw_word(uint64_t seed, uint64_t batch_index, uint32_t r, uint32_t hop, uint32_t t) {
    const uint32_t ctr[4] = {r, (hop << 24) | (t >> 2), static_cast<uint32_t>(batch_index),
                             static_cast<uint32_t>(batch_index >> 32)};
    const uint32_t key[2] = {static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32)};
    uint32_t out[4];
    philox4x32_10(ctr, key, out);
    return out[t & 3];
}

// floor(word * n / 2^32): in [0, n), each value within n / 2^32 of uniform.
GS_HD uint32_t randbelow(uint32_t n, uint32_t word) {
    return static_cast<uint32_t>((static_cast<uint64_t>(word) * n) >> 32);
}

}  // namespace fs
}  // namespace gs
