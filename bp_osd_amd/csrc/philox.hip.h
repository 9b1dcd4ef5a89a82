// philox.hip.h -- the project's counter-based random stream (include/bposd_mi355x.h "Random stream"): Philox4x32-10, the
// uniform it is turned into, and the bit interleave the samplers pack their ballots with.  Shared by the kernels of the
// two Monte-Carlo engines (mc_kernels.hip.h, dem_kernels.hip.h); the host restatement is bp_osd_amd/sim.py.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bposd_rng {

// ---- Philox4x32-10 (Salmon et al., Random123)
struct Philox4 {
    uint32_t v[4];
};

__host__ __device__ inline Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)c0 * 0xD2511F53u;
        const uint64_t p1 = (uint64_t)c2 * 0xCD9E8D57u;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return Philox4{{c0, c1, c2, c3}};
}

// numpy's legacy recipe for a double in [0, 1): 27 + 26 bits, exact in fp64
__host__ __device__ inline double uniform53(uint32_t hi, uint32_t lo) {
    return ((double)(hi >> 5) * 67108864.0 + (double)(lo >> 6)) * (1.0 / 9007199254740992.0);
}

// bit i of x -> bit 2i of the result (x: 32 bits)
__device__ inline uint64_t spread_bits(uint64_t x) {
    x = (x | (x << 16)) & 0x0000FFFF0000FFFFull;
    x = (x | (x << 8)) & 0x00FF00FF00FF00FFull;
    x = (x | (x << 4)) & 0x0F0F0F0F0F0F0F0Full;
    x = (x | (x << 2)) & 0x3333333333333333ull;
    x = (x | (x << 1)) & 0x5555555555555555ull;
    return x;
}

}  // namespace bposd_rng
