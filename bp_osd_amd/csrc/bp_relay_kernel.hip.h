// bp_relay_kernel.hip.h -- Relay-BP: min-sum legs with a memory term per bit.
//
// The flooding min-sum of the other BP kernels, run as a chain of legs.  In leg r the bit pass starts its sums not at the
// prior l0[j] but at  lam = (1 - g[j]) * l0[j] + g[j] * M[j],  g = gammas[r] and M[j] the bit's posterior of the previous
// iteration (two products rounded separately, then one add: build with -ffp-contract=off).  A leg ends at its first
// solution (H * dec == syndrome) or after leg_iters[r] iterations; the next leg keeps M and, with leg_init = 0, resets every
// bit->check message to the prior.  The lightest of the first stop_after solutions is the result (integer weights, a tie
// keeps the earlier one).  Shots without a solution leave the last decisions and go to the OSD list with M as their LLRs.
//
// One persistent workgroup per shot on the atomic queue; degrees are run-time loop bounds and messages are indexed by CSR
// edge, as in bp_anydeg_kernel.hip.h, whose check and bit passes these are (same association order, same rounding).  The
// convergence test is a pass of its own behind the bit pass, not folded into the next check pass: with leg_init = 1 the
// next leg starts from the bit->check messages, which a speculative check pass would have overwritten.
//   LDS = true : messages, prefixes, M and the leg's two per-bit factors live in LDS (bp_relay_lds_bytes fits the CU)
//   LDS = false: they live in a per-workgroup slice of the lane's workspace; LDS holds the decision bytes only
// The leg's factors are formed once per leg: G[j] = g[j] and A[j] = (1 - g[j]) * l0[j], so the bit pass costs one multiply
// and one add more than plain min-sum.  The best solution is a second byte row in LDS, its weight a register every thread
// holds; both are touched only when a solution is found.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bp_kernel.hip.h"

namespace bposd {

constexpr int BPR_MAXNT = 1024;

struct BpRelayParams {
    int m, n, E;
    long long B;
    double ms_scaling;
    int osd_enabled;
    int packed_io;  // as BpParams::packed_io
    int legs, stop_after, leg_init;
    const double* __restrict__ gammas;    // [legs, n]
    const int* __restrict__ leg_iters;    // [legs]
    const uint8_t* __restrict__ synd;
    const double* __restrict__ llr0;      // [n]
    const uint8_t* __restrict__ sel;      // [B, n] nullable
    const double* __restrict__ llr0_alt;  // [n]
    const double* __restrict__ llr0_rows; // [B, n] nullable
    const int* __restrict__ rp;           // CSR indptr [m + 1]
    const int* __restrict__ ci;           // CSR indices [E]
    const int* __restrict__ cp;           // CSC indptr [n + 1]
    const int* __restrict__ ce;           // [E] CSR edge ids of a column, ascending row
    double* __restrict__ ws;              // LDS = false: [gridDim.x][2 * E + 3 * n]
    uint8_t* __restrict__ out_bp;
    uint8_t* __restrict__ out_osd0;
    uint8_t* __restrict__ out_osdw;
    uint8_t* __restrict__ out_conv;
    int* __restrict__ out_iters;
    double* __restrict__ out_llr;
    double* __restrict__ llr_ws;
    int* __restrict__ osd_list;
    int* __restrict__ counters;
    unsigned long long* __restrict__ iter_total;
    int* __restrict__ tail_flag;
    int* __restrict__ out_solutions;      // [B]
    int* __restrict__ out_best_leg;       // [B]
    long long* __restrict__ out_weight;   // [B]
};

// doubles per workgroup: messages | prefixes | M | A | G
__host__ __device__ inline size_t bp_relay_doubles(int n, int E) { return 2 * (size_t)E + 3 * (size_t)n; }
// decision bytes | best solution | syndrome bytes | 32 control bytes
__host__ __device__ inline size_t bp_relay_byte_part(int m, int n) {
    return 2 * (size_t)((n + 15) & ~15) + (size_t)((m + 15) & ~15) + 32;
}
// LDS of the instance that keeps everything on the CU
__host__ __device__ inline size_t bp_relay_lds_bytes(int m, int n, int E) { return 8 * bp_relay_doubles(n, E) + bp_relay_byte_part(m, n); }

// integer weight of a bit: its prior LLR in units of 2^-32, clamped so that 32767 of them cannot overflow an int64
__device__ __forceinline__ long long bp_relay_weight(double l0) {
    double x = l0;
    if (x < -32768.0) x = -32768.0;
    if (x > 32768.0) x = 32768.0;
    return (long long)__builtin_rint(x * 4294967296.0);
}

// Does any thread of the workgroup hold `v`?  One barrier, no static LDS (the kernel may take the whole CU's): two flag words
// used in turn; thread 0 clears the one the next use takes, and the caller has a barrier between any two uses.
__device__ __forceinline__ bool bp_relay_any(volatile int* flags, int& phase, bool v, int tid) {
    volatile int* f = flags + (phase & 1);
    if (v) *f = 1;
    __syncthreads();
    const bool r = *f != 0;
    ++phase;
    if (tid == 0) flags[phase & 1] = 0;
    return r;
}

template <bool LDS>
__global__ __launch_bounds__(BPR_MAXNT) void bp_relay_kernel(const BpRelayParams P) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int m = P.m, n = P.n, E = P.E;
    const int tid = threadIdx.x, NT = blockDim.x;
    double* msg = LDS ? reinterpret_cast<double*>(smem) : P.ws + (size_t)blockIdx.x * bp_relay_doubles(n, E);
    double* pre = msg + E;
    double* M = pre + E;
    double* A = M + n;
    double* G = A + n;
    unsigned char* dec = smem + (LDS ? 8 * bp_relay_doubles(n, E) : 0);
    unsigned char* best = dec + ((n + 15) & ~15);
    unsigned char* syb = best + ((n + 15) & ~15);
    int* sh = reinterpret_cast<int*>(syb + ((m + 15) & ~15));                          // [0] queue index, [1] list slot
    unsigned long long* wsum = reinterpret_cast<unsigned long long*>(sh + 2);          // weight of the solution just found
    volatile int* flags = sh + 4;                                                      // bp_relay_any
    int phase = 0;
    if (tid == 0) flags[0] = flags[1] = 0;  // (published by the first barrier of the queue loop)

    for (;;) {
        if (tid == 0) {
            sh[0] = atomicAdd(&P.counters[0], 1);
            *wsum = 0ull;
        }
        __syncthreads();
        const long long s = sh[0];
        if (s >= P.B) {
            if (s == P.B && tid == 0 && P.tail_flag) *(volatile int*)P.tail_flag = 1;
            break;
        }
        bool nz = false;
        for (int c = tid; c < m; c += NT) {
            const bool b = bp_synd_bit(P.synd, P.packed_io, s, m, c);
            syb[c] = b ? 1 : 0;
            nz |= b;
        }
        // every edge's bit->check message starts at the prior; M = prior; decisions = 0
        for (int i = tid; i < n; i += NT) {
            const double l0 = bp_shot_prior(P, s, n, i);
            for (int k = P.cp[i]; k < P.cp[i + 1]; ++k) msg[P.ce[k]] = l0;
            dec[i] = 0;
            M[i] = l0;
        }
        const bool zero = !bp_relay_any(flags, phase, nz, tid);  // all-zero syndrome: zeros, converge = true, BP not run

        int t = 0, found = 0, best_leg = -1;
        long long best_w = 0;
        if (!zero) {
#pragma clang loop unroll(disable)
            for (int r = 0; r < P.legs; ++r) {
                // ---------------- the leg's factors, once; messages back to the prior unless the legs hand them on
                const double* __restrict__ gr = P.gammas + (size_t)r * n;
                const bool reset = r > 0 && P.leg_init == 0;
                for (int i = tid; i < n; i += NT) {
                    const double l0 = bp_shot_prior(P, s, n, i);
                    const double g = gr[i];
                    G[i] = g;
                    A[i] = (1.0 - g) * l0;
                    if (reset)
                        for (int k = P.cp[i]; k < P.cp[i + 1]; ++k) msg[P.ce[k]] = l0;
                }
                __syncthreads();
                const int li = P.leg_iters[r];
                bool sol = false;
#pragma clang loop unroll(disable)
                for (int k = 0; k < li; ++k) {
                    ++t;
                    const double alpha = alpha_for_iteration(P.ms_scaling, t);
                    // ---------------- check pass (min-sum), as bp_anydeg_kernel
                    for (int c = tid; c < m; c += NT) {
                        const int e0 = P.rp[c], e1 = P.rp[c + 1];
                        double mn = __DBL_MAX__;
                        bool par = syb[c] != 0;
                        for (int e = e0; e < e1; ++e) {
                            const double v = msg[e];
                            pre[e] = mn;
                            mn = min_abs(mn, v);
                            par ^= (v <= 0.0);  // a zero counts as negative
                        }
                        double suf = __DBL_MAX__;
                        for (int e = e1 - 1; e >= e0; --e) {
                            const double v = msg[e];
                            const double mag = min_pos(pre[e], suf);
                            msg[e] = flip_sign(mag * alpha, par ^ (v <= 0.0));
                            suf = min_abs(suf, v);
                        }
                    }
                    __syncthreads();
                    // ---------------- bit pass: the sums start at lam instead of the prior
                    for (int i = tid; i < n; i += NT) {
                        const int k0 = P.cp[i], k1 = P.cp[i + 1];
                        const double gm = G[i] * M[i];
                        double acc = A[i] + gm;
                        for (int q = k0; q < k1; ++q) {
                            const int e = P.ce[q];
                            pre[e] = acc;
                            acc += msg[e];
                        }
                        M[i] = acc;
                        dec[i] = (acc <= 0.0) ? 1 : 0;
                        double suf = 0.0;
                        for (int q = k1 - 1; q >= k0; --q) {
                            const int e = P.ce[q];
                            const double cm = msg[e];
                            msg[e] = pre[e] + suf;
                            suf += cm;
                        }
                    }
                    __syncthreads();
                    // ---------------- H * dec == syndrome ?
                    bool mis = false;
                    for (int c = tid; c < m; c += NT) {
                        unsigned int dpar = syb[c];
                        for (int e = P.rp[c]; e < P.rp[c + 1]; ++e) dpar ^= dec[P.ci[e]];
                        mis |= dpar != 0u;
                    }
                    sol = !bp_relay_any(flags, phase, mis, tid);
                    if (sol) break;
                }
                if (sol) {  // the rare path: weigh the solution, keep it if it is lighter than the best so far
                    long long w = 0;
                    for (int i = tid; i < n; i += NT)
                        if (dec[i]) w += bp_relay_weight(bp_shot_prior(P, s, n, i));
                    for (int off = 32; off > 0; off >>= 1) w += __shfl_down(w, off);
                    if ((tid & 63) == 0) atomicAdd(wsum, (unsigned long long)w);
                    __syncthreads();
                    const long long wt = (long long)*(volatile unsigned long long*)wsum;
                    if (found == 0 || wt < best_w) {
                        for (int i = tid; i < n; i += NT) best[i] = dec[i];
                        best_w = wt;
                        best_leg = r;
                    }
                    ++found;
                    __syncthreads();
                    if (tid == 0) *wsum = 0ull;
                    if (found == P.stop_after) break;
                }
            }
        }

        // ---- results (as the other flooding kernels)
        const bool conv = zero || found > 0;
        const bool to_osd = (!conv) && P.osd_enabled;
        const unsigned char* row = found > 0 ? best : dec;
        if (tid == 0) {
            if (to_osd) {
                const int slot = atomicAdd(&P.counters[1], 1);
                P.osd_list[slot] = (int)s;
                sh[1] = slot;
            }
            if (P.out_conv) P.out_conv[s] = conv ? 1 : 0;
            if (P.out_iters) P.out_iters[s] = t;
            if (t) atomicAdd(P.iter_total, (unsigned long long)t);
            P.out_solutions[s] = found;
            P.out_best_leg[s] = best_leg;
            P.out_weight[s] = best_w;
        }
        __syncthreads();
        const int slot = to_osd ? sh[1] : 0;
        for (int i = tid; i < n; i += NT) {
            const size_t o = (size_t)s * n + i;
            const double llr = M[i];
            if (!P.packed_io) {
                const uint8_t b = row[i];
                if (P.out_bp) P.out_bp[o] = b;
                if (!to_osd) {
                    P.out_osdw[o] = b;
                    if (P.out_osd0) P.out_osd0[o] = b;
                }
            }
            if (to_osd) P.llr_ws[(size_t)slot * n + i] = llr;
            if (P.out_llr) P.out_llr[o] = llr;
        }
        if (P.packed_io) {  // the row's bytes are in LDS: one thread forms each 64-bit word
            const int wpn = (n + 63) >> 6;
            for (int w = tid; w < wpn; w += NT) {
                unsigned long long v = 0ull;
                const int hi = min(64, n - 64 * w);
                for (int b = 0; b < hi; ++b) v |= (unsigned long long)(row[64 * w + b] & 1) << b;
                const size_t o = (size_t)s * wpn + w;
                if (P.out_bp) ((unsigned long long*)P.out_bp)[o] = v;
                if (!to_osd) {
                    ((unsigned long long*)P.out_osdw)[o] = v;
                    if (P.out_osd0) ((unsigned long long*)P.out_osd0)[o] = v;
                }
            }
        }
        __syncthreads();
    }
}

}  // namespace bposd
