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
// edge, as in bp_anydeg_kernel.hip.h: both take their check and bit sweeps, the queue take, the start of a shot and the results
// protocol (bytes or packed words) from bp_csr.hip.h; the bit sweep starts at lam here and at the prior there.  The
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

#include "bp_csr.hip.h"

namespace bposd {

constexpr int BPR_MAXNT = 1024;

struct BpRelayParams {
    BpShotIo io;  // (max_iter and ps_clip are not read: the legs carry the iteration counts, and relay is min-sum)
    BpCsrGraph g;
    int legs, stop_after, leg_init;
    const double* __restrict__ gammas;    // [legs, n]
    const int* __restrict__ leg_iters;    // [legs]
    double* __restrict__ ws;              // LDS = false: [gridDim.x][2 * E + 3 * n]
    int* __restrict__ out_solutions;      // [B]
    int* __restrict__ out_best_leg;       // [B]
    long long* __restrict__ out_weight;   // [B]
};

// doubles per workgroup: messages | prefixes | M | A | G
__host__ __device__ inline size_t bp_relay_doubles(int n, int E) { return 2 * (size_t)E + 3 * (size_t)n; }
// decision bytes | best solution | syndrome bytes | 32 control bytes
__host__ __device__ inline size_t bp_relay_byte_part(int m, int n) {
    return 2 * bp_csr_row_bytes(n) + bp_csr_row_bytes(m) + 32;
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
    const BpShotIo& io = P.io;
    const BpCsrGraph& g = P.g;
    const int m = io.m, n = io.n, E = g.E;
    const int tid = threadIdx.x, NT = blockDim.x;
    double* msg = LDS ? reinterpret_cast<double*>(smem) : P.ws + (size_t)blockIdx.x * bp_relay_doubles(n, E);
    double* pre = msg + E;
    double* M = pre + E;
    double* A = M + n;
    double* G = A + n;
    unsigned char* dec = smem + (LDS ? 8 * bp_relay_doubles(n, E) : 0);
    unsigned char* best = dec + bp_csr_row_bytes(n);
    unsigned char* syb = best + bp_csr_row_bytes(n);
    int* ctl = reinterpret_cast<int*>(syb + bp_csr_row_bytes(m));                      // bp_csr_take / bp_csr_finish
    unsigned long long* wsum = reinterpret_cast<unsigned long long*>(ctl + 2);         // weight of the solution just found
    volatile int* flags = ctl + 4;                                                     // bp_relay_any
    int phase = 0;
    if (tid == 0) flags[0] = flags[1] = 0;  // (published by the first barrier of the queue loop)

    for (;;) {
        if (tid == 0) *wsum = 0ull;
        const long long s = bp_csr_take(io, io.tail_flag, ctl, tid);
        if (s < 0) break;
        // every edge's bit->check message starts at the prior; M = prior; decisions = 0; the syndrome's bytes go to LDS
        const bool nz = bp_csr_start(io, g, s, io.packed_io, msg, dec, M, syb, tid, NT);
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
                    const double l0 = bp_shot_prior(io, s, n, i);
                    const double gm = gr[i];
                    G[i] = gm;
                    A[i] = (1.0 - gm) * l0;
                    if (reset) bp_csr_set_bit_edges(g, msg, i, l0);
                }
                __syncthreads();
                const int li = P.leg_iters[r];
                bool sol = false;
#pragma clang loop unroll(disable)
                for (int k = 0; k < li; ++k) {
                    ++t;
                    const double alpha = alpha_for_iteration(io.ms_scaling, t);
                    // ---------------- check pass (min-sum)
                    for (int c = tid; c < m; c += NT) bp_csr_minsum_check(msg, pre, g.rp[c], g.rp[c + 1], syb[c] != 0, alpha, [](int) {});
                    __syncthreads();
                    // ---------------- bit pass: the sums start at lam instead of the prior
                    for (int i = tid; i < n; i += NT) {
                        const double gm = G[i] * M[i];
                        const double acc = bp_csr_bit_sweep(g.ce, msg, pre, g.cp[i], g.cp[i + 1], A[i] + gm);
                        M[i] = acc;
                        dec[i] = (acc <= 0.0) ? 1 : 0;
                    }
                    __syncthreads();
                    // ---------------- H * dec == syndrome ?
                    const bool mis = bp_csr_mismatch(g, dec, m, tid, NT, [&](int c) { return syb[c]; });
                    sol = !bp_relay_any(flags, phase, mis, tid);
                    if (sol) break;
                }
                if (sol) {  // the rare path: weigh the solution, keep it if it is lighter than the best so far
                    long long w = 0;
                    for (int i = tid; i < n; i += NT)
                        if (dec[i]) w += bp_relay_weight(bp_shot_prior(io, s, n, i));
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

        if (tid == 0) {
            P.out_solutions[s] = found;
            P.out_best_leg[s] = best_leg;
            P.out_weight[s] = best_w;
        }
        bp_csr_finish(io, s, io.packed_io, zero || found > 0, t, found > 0 ? best : dec, M, ctl, tid, NT);
    }
}

}  // namespace bposd
