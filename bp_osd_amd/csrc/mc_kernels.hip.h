// mc_kernels.hip.h -- the Monte-Carlo harness's own kernels (gfx950, wave64): everything of a css_decode_sim batch that
// is not a decode.  mc_sample_kernel draws the errors of a batch from the project's counter-based stream and computes
// both syndromes; mc_score_kernel does the logical checks of the three decoder outputs and reduces a batch to seven
// integers.  DESIGN.md "Monte-Carlo engine" has the stream definition, the shapes and the byte counts; the host
// restatement of the stream is bp_osd_amd/sim.py (philox4x32_10, philox_uniforms), which the tests hold these against.
//
// One workgroup of MC_THREADS threads works on one shot at a time (grid-stride over the batch): a wave's __ballot is one
// packed word, the packed error rows stay in LDS for the syndrome pass, and nothing of size B x N x 8 bytes exists.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "philox.hip.h"

namespace bposd_mc_dev {

constexpr int MC_THREADS = 256;  // 4 waves
constexpr int MC_WAVES = MC_THREADS / 64;

using namespace bposd_rng;  // philox4x32_10, uniform53, spread_bits

struct McSampleParams {
    long long B;
    unsigned long long first_shot;  // global index of row 0
    uint32_t key0, key1;            // seed, low and high word
    int n, words;                   // qubits, ceil(n / 64)
    const double* thr;              // [3][n]: t1 = pz, t2 = pz + px, t3 = px + py + pz (fp64, computed on the host)
    // hx (mx rows) acts on error_z, hz (mz rows) on error_x
    int mx, mz, swx, swz;           // swx = ceil(mz / 64) words of a packed synd_x row, swz = ceil(mx / 64)
    const int *hx_rp, *hx_ci, *hz_rp, *hz_ci;
    unsigned long long *err_x, *err_z;    // [B][words]
    uint8_t *synd_x, *synd_z;             // [B][mz], [B][mx]
    unsigned long long *psynd_x, *psynd_z;  // [B][swx], [B][swz]
};

// parity of the bits of `row` (LDS, packed) at the columns of one CSR row
__device__ inline unsigned csr_parity(const unsigned long long* row, const int* __restrict__ ci, int lo, int hi) {
    unsigned p = 0;
    for (int e = lo; e < hi; ++e) {
        const int c = ci[e];
        p ^= (unsigned)(row[c >> 6] >> (c & 63));
    }
    return p & 1u;
}

// checks [0, m) of one sector: byte row and packed row of the syndrome (every thread of the workgroup takes part)
__device__ inline void syndrome_pass(const unsigned long long* row, const int* __restrict__ rp, const int* __restrict__ ci, int m,
                                     uint8_t* out_bytes, unsigned long long* out_words) {
    const int lane = threadIdx.x & 63;
    for (int base = 0; base < m; base += MC_THREADS) {  // uniform trip count: the ballot below wants whole waves
        const int c = base + (int)threadIdx.x;
        unsigned bit = 0;
        if (c < m) {
            bit = csr_parity(row, ci, rp[c], rp[c + 1]);
            out_bytes[c] = (uint8_t)bit;
        }
        const unsigned long long word = __ballot(bit);
        if (lane == 0 && (c & ~63) < m) out_words[c >> 6] = word;
    }
}

__global__ __launch_bounds__(MC_THREADS) void mc_sample_kernel(McSampleParams P) {
    extern __shared__ unsigned long long mc_lds[];  // [2][words]: error_x row, error_z row
    unsigned long long* row_x = mc_lds;
    unsigned long long* row_z = mc_lds + P.words;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int chunks = (P.n + 127) >> 7;  // a wave step covers 128 qubits: lane l draws the pair (2l, 2l + 1) of it
    const double* __restrict__ t1 = P.thr;
    const double* __restrict__ t2 = P.thr + P.n;
    const double* __restrict__ t3 = P.thr + 2 * (size_t)P.n;

    for (long long b = blockIdx.x; b < P.B; b += gridDim.x) {
        const unsigned long long s = P.first_shot + (unsigned long long)b;
        const uint32_t s_lo = (uint32_t)s, s_hi = (uint32_t)(s >> 32);
        for (int ch = wave; ch < chunks; ch += MC_WAVES) {
            const int pair = ch * 64 + lane;
            const int i0 = 2 * pair, i1 = i0 + 1;
            bool ex0 = false, ez0 = false, ex1 = false, ez1 = false;
            if (i0 < P.n) {
                const Philox4 o = philox4x32_10(s_lo, s_hi, (uint32_t)pair, 0u, P.key0, P.key1);
                const double u0 = uniform53(o.v[0], o.v[1]);
                const bool z = u0 < t1[i0], x = t1[i0] <= u0 && u0 < t2[i0], y = t2[i0] <= u0 && u0 < t3[i0];
                ez0 = z || y;
                ex0 = x || y;
                if (i1 < P.n) {
                    const double u1 = uniform53(o.v[2], o.v[3]);
                    const bool z1 = u1 < t1[i1], x1 = t1[i1] <= u1 && u1 < t2[i1], y1 = t2[i1] <= u1 && u1 < t3[i1];
                    ez1 = z1 || y1;
                    ex1 = x1 || y1;
                }
            }
            // ballot bit l = qubit 2l (even) / 2l + 1 (odd) of the chunk: interleave into the chunk's two words
            const unsigned long long bxe = __ballot(ex0), bxo = __ballot(ex1), bze = __ballot(ez0), bzo = __ballot(ez1);
            if (lane < 2) {
                const int w = 2 * ch + lane;
                if (w < P.words) {
                    const int sh = 32 * lane;
                    const unsigned long long wx = spread_bits((bxe >> sh) & 0xffffffffull) | (spread_bits((bxo >> sh) & 0xffffffffull) << 1);
                    const unsigned long long wz = spread_bits((bze >> sh) & 0xffffffffull) | (spread_bits((bzo >> sh) & 0xffffffffull) << 1);
                    row_x[w] = wx;
                    row_z[w] = wz;
                    P.err_x[(size_t)b * P.words + w] = wx;
                    P.err_z[(size_t)b * P.words + w] = wz;
                }
            }
        }
        __syncthreads();
        syndrome_pass(row_z, P.hx_rp, P.hx_ci, P.mx, P.synd_z + (size_t)b * P.mx, P.psynd_z + (size_t)b * P.swz);
        syndrome_pass(row_x, P.hz_rp, P.hz_ci, P.mz, P.synd_x + (size_t)b * P.mz, P.psynd_x + (size_t)b * P.swx);
        __syncthreads();  // the rows are overwritten by the next shot
    }
}

// ---------------------------------------------------------------------------------------------------------------------
struct McScoreParams {
    long long B;
    int n, words, k;
    const unsigned long long *err_x, *err_z;  // [B][words]
    const uint8_t* dec[6];                    // byte rows [B][n]: bp x, bp z, osd0 x, osd0 z, osdw x, osdw z
    const uint8_t *conv_x, *conv_z;           // [B]
    const unsigned long long *lzT, *lxT;      // logicals, packed and transposed: [words][k] (lz is held against residual_x)
    uint8_t* flags;                           // [B]: bit 0/1 bp fail x/z, 2/3 osd0, 4/5 osdw
    int* counters;  // [7]: converge x, converge z, bp / osd0 / osdw success, smallest failing weight osd0 / osdw
};

// eight 0/1 bytes -> eight bits (byte j -> bit j)
__device__ inline unsigned pack8(uint64_t q) { return (unsigned)(((q & 0x0101010101010101ull) * 0x0102040810204080ull) >> 56); }

__global__ __launch_bounds__(MC_THREADS) void mc_score_kernel(McScoreParams P) {
    extern __shared__ unsigned long long mc_lds[];  // [6][words] residual rows, then 6 weights + 1 flag word (ints)
    unsigned long long* res = mc_lds;
    int* wt = (int*)(mc_lds + 6 * (size_t)P.words);  // [6] popcounts, [6] = fail flags
    const int row_bytes = P.words * 8;
    const int full = P.n >> 3;  // 8-byte groups wholly inside a row
    int acc[7] = {0, 0, 0, 0, 0, 0x7fffffff, 0x7fffffff};  // thread 0's share of the counters

    for (long long b = blockIdx.x; b < P.B; b += gridDim.x) {
        if (threadIdx.x < 7) wt[threadIdx.x] = 0;
        // residuals error ^ decoding, packed on the fly: one 8-byte load of a decoder row makes one byte of a packed row
        const uint8_t* ex = (const uint8_t*)(P.err_x + (size_t)b * P.words);
        const uint8_t* ez = (const uint8_t*)(P.err_z + (size_t)b * P.words);
        uint8_t* res_b = (uint8_t*)res;
        for (int j = threadIdx.x; j < row_bytes; j += MC_THREADS) {  // byte j of the six packed rows: six loads in flight per thread
            unsigned bits[6] = {0, 0, 0, 0, 0, 0};
            unsigned e_x = 0, e_z = 0;
            if (j < full) {
                uint64_t q[6];
#pragma unroll
                for (int r = 0; r < 6; ++r)
                    __builtin_memcpy(&q[r], P.dec[r] + (size_t)b * P.n + 8 * (size_t)j, 8);  // rows start at any byte: unaligned load
                e_x = ex[j];
                e_z = ez[j];
#pragma unroll
                for (int r = 0; r < 6; ++r) bits[r] = pack8(q[r]);
            } else if (8 * j < P.n) {  // the last, partial group of a row: byte by byte, never past the row's end
                e_x = ex[j];
                e_z = ez[j];
#pragma unroll
                for (int r = 0; r < 6; ++r) {
                    const uint8_t* d = P.dec[r] + (size_t)b * P.n;
                    for (int i = 8 * j; i < P.n; ++i) bits[r] |= (unsigned)(d[i] & 1) << (i & 7);
                }
            }
#pragma unroll
            for (int r = 0; r < 6; ++r) res_b[r * row_bytes + j] = (uint8_t)(bits[r] ^ ((r & 1) ? e_z : e_x));
        }
        __syncthreads();
        // logical checks: task (row r, logical k) = parity of popcount(l_k & residual_r); then the six weights
        const int checks = 6 * P.k;
        for (int t = threadIdx.x; t < checks + 6 * P.words; t += MC_THREADS) {
            if (t < checks) {
                const int r = t / P.k, k = t - r * P.k;
                const unsigned long long* __restrict__ L = (r & 1) ? P.lxT : P.lzT;  // residual_z against lx, residual_x against lz
                const unsigned long long* row = res + (size_t)r * P.words;
                unsigned long long a = 0;
                for (int w = 0; w < P.words; ++w) a ^= L[(size_t)w * P.k + k] & row[w];
                if (__popcll(a) & 1) atomicOr(&wt[6], 1 << r);
            } else {
                const int u = t - checks;
                const int c = __popcll(res[u]);
                if (c) atomicAdd(&wt[u / P.words], c);
            }
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            const int f = wt[6];
            const int cx = P.conv_x[b] != 0, cz = P.conv_z[b] != 0;
            P.flags[b] = (uint8_t)f;
            acc[0] += cx;
            acc[1] += cz;
            acc[2] += (cx && cz && !(f & 3)) ? 1 : 0;
#pragma unroll
            for (int o = 1; o < 3; ++o) {  // osd0, osdw
                const int fx = (f >> (2 * o)) & 1, fz = (f >> (2 * o + 1)) & 1;
                if (fx | fz) {
                    const int w = fx ? wt[2 * o] : wt[2 * o + 1];
                    acc[4 + o] = min(acc[4 + o], w);
                } else {
                    acc[2 + o] += 1;
                }
            }
        }
        __syncthreads();  // wt and the residual rows are reused by the next shot
    }
    if (threadIdx.x == 0) {  // one integer atomic per counter per workgroup: sums and minima do not depend on arrival order
        for (int i = 0; i < 5; ++i)
            if (acc[i]) atomicAdd(&P.counters[i], acc[i]);
        for (int i = 5; i < 7; ++i)
            if (acc[i] != 0x7fffffff) atomicMin(&P.counters[i], acc[i]);
    }
}

}  // namespace bposd_mc_dev
