// dem_kernels.hip.h -- the kernels of the detector-error-model Monte-Carlo engine (gfx950, wave64): everything of a DEM
// batch that is not a decode.  dem_sample_kernel draws the fault mechanisms of a batch from the project's counter-based
// stream (philox.hip.h, the one mc_sample_kernel draws from) and forms the detector row H . f and the
// true observable row L . f of every shot; dem_score_kernel holds the three decoded observable sets against the true one
// and reduces a batch to five integers and a failure count per observable.  DESIGN.md 4.11 has the stream, the shapes and
// the byte counts; the host restatement is bp_osd_amd/sim.py (philox_uniforms) < priors.
//
// Scatter, not gather.  mc_sample_kernel walks the CSR rows of its check matrices against the packed error row: nnz(H) LDS
// reads per shot whatever fired.  A DEM has heavy rows and small priors, so here the faults that fired walk their COLUMN of
// H stacked on L and flip one bit per entry: sum_i p_i . colweight_i LDS operations per shot on average.  XOR commutes, so
// the row does not depend on the order in which the lanes arrive.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "philox.hip.h"

namespace bposd_dem_dev {

using namespace bposd_rng;  // philox4x32_10, uniform53, spread_bits

constexpr int DEM_THREADS = 256;  // 4 waves
constexpr int DEM_WAVES = DEM_THREADS / 64;
constexpr int DEM_SCORE_THREADS = 256;

struct DemSampleParams {
    long long B;
    unsigned long long first_shot;  // global index of row 0
    uint32_t key0, key1;            // seed, low and high word
    int N, fw;                      // fault mechanisms, ceil(N / 64)
    int dw, ow;                     // ceil(M / 64) detector words, ceil(k / 64) observable words of a row
    const double* priors;           // [N], as given
    // CSC of H stacked on L: entries col_ptr[i] .. col_ptr[i + 1] of col_bits are the bits fault i flips in the shot's
    // accumulator row -- detector r is bit r, observable j is bit 64 * dw + j (ascending within a column)
    const int *col_ptr, *col_bits;
    unsigned long long* faults;       // [B][fw]
    unsigned long long* detectors;    // [B][dw]: the layout of bposd_decode_batch_packed, padding bits zero
    unsigned long long* observables;  // [B][ow]
    // weighted sampling only (dem_sample_kernel<true>; the plain instance reads neither): `priors` is then the row the faults
    // are drawn against, incr[i] the 2^-32 units of log-weight a fired fault i adds, logw[b] their sum over shot b's faults
    const long long* incr;  // [N]
    long long* logw;        // [B]
};

// every entry of one fault's column: one LDS XOR of a single bit each.  32-bit operations: an entry flips one bit, so the
// narrower atomic does the same work on one bank instead of two, and little-endian dword 2w / 2w + 1 are the halves of
// 64-bit word w, so the row is read back as the packed words the outputs want.
__device__ inline void dem_flip_column(unsigned* acc, const int* __restrict__ col_ptr, const int* __restrict__ col_bits, int i) {
    const int hi = col_ptr[i + 1];
    for (int e = col_ptr[i]; e < hi; ++e) {
        const int bit = col_bits[e];
        atomicXor(&acc[bit >> 5], 1u << (bit & 31));
    }
}

// WEIGHTED: importance sampling.  The draw is the same; every shot also leaves the integer sum of
// incr[i] over its fired faults.  Each lane sums its own faults across its chunks, the wave reduces the 64 sums as 64-bit
// values (so a carry between the halves is the adder's business) and one lane adds the wave's sum to one more 64-bit word
// behind the shot's accumulator row with one LDS atomic.  The word goes out and is cleared with the row: no barrier of its
// own.  Integer sums do not depend on arrival order, so logw is bit-exact like the rows.
template <bool WEIGHTED>
__global__ __launch_bounds__(DEM_THREADS) void dem_sample_kernel(DemSampleParams P) {
    // [2][dw + ow] accumulator rows ([2][dw + ow + 1] when WEIGHTED).  Two of them, used in turn, make one barrier per shot
    // enough: behind the barrier of
    // shot t every thread writes out and clears its own words of row t & 1 while the faults of shot t + 1 already flip bits
    // of the other row, whose words were cleared behind the barrier of shot t - 1 -- that is, in front of the barrier of shot t.
    extern __shared__ unsigned long long dem_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rw = P.dw + P.ow;
    const int rs = WEIGHTED ? rw + 1 : rw;  // words of a row in LDS
    const int chunks = (P.N + 127) >> 7;  // a wave step covers 128 faults: lane l draws the pair (2l, 2l + 1) of it
    for (int w = threadIdx.x; w < 2 * rs; w += DEM_THREADS) dem_lds[w] = 0;
    __syncthreads();

    int turn = 0;
    for (long long b = blockIdx.x; b < P.B; b += gridDim.x, turn ^= 1) {
        unsigned long long* row = dem_lds + (size_t)turn * rs;
        unsigned* acc = (unsigned*)row;
        const unsigned long long s = P.first_shot + (unsigned long long)b;
        const uint32_t s_lo = (uint32_t)s, s_hi = (uint32_t)(s >> 32);
        long long lw = 0;  // this lane's share of the shot's log-weight
        for (int ch = wave; ch < chunks; ch += DEM_WAVES) {
            const int pair = ch * 64 + lane;
            const int i0 = 2 * pair, i1 = i0 + 1;
            bool f0 = false, f1 = false;
            if (i0 < P.N) {
                const Philox4 o = philox4x32_10(s_lo, s_hi, (uint32_t)pair, 0u, P.key0, P.key1);
                f0 = uniform53(o.v[0], o.v[1]) < P.priors[i0];
                if (i1 < P.N) f1 = uniform53(o.v[2], o.v[3]) < P.priors[i1];
            }
            // ballot bit l = fault 2l (even) / 2l + 1 (odd) of the chunk: interleave into the chunk's two words
            const unsigned long long be = __ballot(f0), bo = __ballot(f1);
            if (lane < 2) {
                const int w = 2 * ch + lane;
                if (w < P.fw) {
                    const int sh = 32 * lane;
                    P.faults[(size_t)b * P.fw + w] = spread_bits((be >> sh) & 0xffffffffull) | (spread_bits((bo >> sh) & 0xffffffffull) << 1);
                }
            }
            if (f0) dem_flip_column(acc, P.col_ptr, P.col_bits, i0);
            if (f1) dem_flip_column(acc, P.col_ptr, P.col_bits, i1);
            if constexpr (WEIGHTED) {
                if (f0) lw += P.incr[i0];
                if (f1) lw += P.incr[i1];
            }
        }
        if constexpr (WEIGHTED) {
            if (wave < chunks) {  // (wave-uniform: the lanes of a wave that drew are all here)
                for (int d = 32; d; d >>= 1) lw += __shfl_xor(lw, d);
                if (lane == 0 && lw) atomicAdd(&row[rw], (unsigned long long)lw);
            }
        }
        __syncthreads();  // the row is complete
        for (int w = threadIdx.x; w < rs; w += DEM_THREADS) {
            const unsigned long long v = row[w];
            row[w] = 0;  // for shot t + 2
            if (w < P.dw) P.detectors[(size_t)b * P.dw + w] = v;
            else if (!WEIGHTED || w < rw) P.observables[(size_t)b * P.ow + (w - P.dw)] = v;
            else P.logw[b] = (long long)v;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
struct DemScoreParams {
    long long B;
    int k, ow, dw;                               // observables, ceil(k / 64), ceil(M / 64)
    const unsigned long long* detectors;         // [B][dw]
    const unsigned long long* truth;             // [B][ow]: L . faults
    const unsigned long long *bp, *osd0, *osdw;  // [B][ow]: L . correction, as decoded
    const uint8_t* conv;                         // [B]
    uint8_t* flags;                              // [B]: bit 0 bp wrong, 1 osd0 wrong, 2 osdw wrong, 3 no detector fired
    int* counters;                               // [5]: bp converged, bp / osd0 / osdw success, shots with no detector fired
    int* obs_fail;                               // [k]: osdw failures per observable
};

// One thread per shot: a shot is a few words.  Counts are formed per wave from ballots, summed per workgroup in LDS and
// leave as one integer atomic per counter per workgroup; sums of integers do not depend on arrival order.
__global__ __launch_bounds__(DEM_SCORE_THREADS) void dem_score_kernel(DemScoreParams P) {
    __shared__ int wg_count[5];
    if (threadIdx.x < 5) wg_count[threadIdx.x] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    int mine[5] = {0, 0, 0, 0, 0};  // lane 0's share
    for (long long base = (long long)blockIdx.x * DEM_SCORE_THREADS; base < P.B; base += (long long)gridDim.x * DEM_SCORE_THREADS) {
        const long long b = base + threadIdx.x;  // (uniform trip count: the ballots below want whole waves)
        bool conv = false, ok_bp = false, ok_0 = false, ok_w = false, quiet = false;
        if (b < P.B) {
            const size_t o = (size_t)b * P.ow;
            unsigned long long d_bp = 0, d_0 = 0, d_w = 0, any = 0;
            for (int w = 0; w < P.ow; ++w) {
                const unsigned long long t = P.truth[o + w];
                d_bp |= P.bp[o + w] ^ t;
                d_0 |= P.osd0[o + w] ^ t;
                const unsigned long long x = P.osdw[o + w] ^ t;
                d_w |= x;
                for (unsigned long long r = x; r; r &= r - 1) {  // failures are rare
                    const int j = 64 * w + __ffsll((long long)r) - 1;
                    if (j < P.k) atomicAdd(&P.obs_fail[j], 1);
                }
            }
            for (int w = 0; w < P.dw; ++w) any |= P.detectors[(size_t)b * P.dw + w];
            conv = P.conv[b] != 0;
            quiet = any == 0;
            ok_bp = conv && d_bp == 0;
            ok_0 = d_0 == 0;
            ok_w = d_w == 0;
            P.flags[b] = (uint8_t)((d_bp != 0 ? 1 : 0) | (d_0 != 0 ? 2 : 0) | (d_w != 0 ? 4 : 0) | (quiet ? 8 : 0));
        }
        const int c0 = __popcll(__ballot(conv)), c1 = __popcll(__ballot(ok_bp)), c2 = __popcll(__ballot(ok_0)),
                  c3 = __popcll(__ballot(ok_w)), c4 = __popcll(__ballot(quiet));
        mine[0] += c0;
        mine[1] += c1;
        mine[2] += c2;
        mine[3] += c3;
        mine[4] += c4;
    }
    if (lane == 0)
        for (int i = 0; i < 5; ++i)
            if (mine[i]) atomicAdd(&wg_count[i], mine[i]);
    __syncthreads();
    if (threadIdx.x < 5 && wg_count[threadIdx.x]) atomicAdd(&P.counters[threadIdx.x], wg_count[threadIdx.x]);
}

}  // namespace bposd_dem_dev
