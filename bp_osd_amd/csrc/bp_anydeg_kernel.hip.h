// bp_anydeg_kernel.hip.h -- flooding-schedule BP for parity-check matrices of ANY row / column weight.
//
// The tuned kernels are compiled for check degrees <= 16 and bit degrees <= 8 (what sparse quantum codes have); the
// reference's decoder (ldpc's, /root/reference/src/bposd/__init__.py:1) has no such limit, and classical LDPC / BCH-like
// matrices handed to `bposd_decoder` exceed it.  This kernel serves those: same algorithm, arithmetic order and
// convergence bookkeeping as bp_kernel.hip.h / bp_large_kernel.hip.h (rows a3-a7 of SURVEY.md §8), degrees are run-time
// loop bounds.  One 256-thread workgroup per syndrome (persistent, atomic queue); messages live in a per-workgroup slice
// of a global workspace indexed by CSR edge id; a thread walks checks c = tid, tid + 256, ... and bits likewise.
//   check pass, two sweeps over the check's edges: forward stores the prefix (running minimum of |b2c|, or running
//     product of tanh(b2c / 2)) of every edge in a second array and accumulates the sign parity; backward combines it with
//     the running suffix and overwrites the edge's message in place.  The candidate syndrome of the previous bit pass'
//     decisions is accumulated in the same forward sweep (the flooding kernels keep an incremental bitmap instead).
//   bit pass, two sweeps over the bit's edges in ascending check order: forward stores the prefix sums (prior included),
//     backward adds the suffix sums -- prefix(d) + suffix(d) as the reference forms them.
// Built for completeness and exactness (tests/test_gpu_parity.py compares LLR bits with the oracle), not tuned.
// The queue take, the start of a shot, the min-sum check sweep, the bit sweep, the parity of a check and the results protocol
// are those of bp_csr.hip.h, shared with bp_serial_kernel and bp_relay_kernel; here are the flooding schedule with its
// speculative check pass (whose forward sweep gathers the candidate syndrome through the helper's per-edge hook; the iteration
// behind the last bit pass only takes the parity) and the product-sum check update.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bp_csr.hip.h"
#include "portable_math.h"

namespace bposd {

constexpr int BPA_NT = 256;
constexpr int BPA_PACKED = 0;  // launched with byte rows only (native_packed() in internal.h)

struct BpAnyParams {
    BpShotIo io;
    BpCsrGraph g;
    int bp_method;  // 0 product-sum, 1 min-sum
    int ps_form;    // product-sum evaluation order (portable_math.h: pm_ps_tanh_half)
    double* __restrict__ msg_ws;   // [gridDim.x][3 * E]: messages | prefixes | tanh values (product-sum)
    double* __restrict__ llr_tmp;  // [gridDim.x][n]
};

__host__ __device__ inline size_t bp_anydeg_lds_bytes(int n) { return bp_csr_row_bytes(n) + 8 * 4; }

__global__ __launch_bounds__(BPA_NT) void bp_anydeg_kernel(const BpAnyParams P) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const BpShotIo& io = P.io;
    const BpCsrGraph& g = P.g;
    const int m = io.m, n = io.n;
    const int tid = threadIdx.x;
    unsigned char* dec = smem;
    int* ctl = reinterpret_cast<int*>(smem + bp_csr_row_bytes(n));
    double* msg = P.msg_ws + (size_t)blockIdx.x * 3 * g.E;
    double* pre = msg + g.E;
    double* thv = pre + g.E;
    double* llrt = P.llr_tmp + (size_t)blockIdx.x * n;

    for (;;) {
        const long long s = bp_csr_take(io, io.tail_flag, ctl, tid);
        if (s < 0) break;
        const auto synd_of = [&](int c) { return bp_synd_bit(io.synd, BPA_PACKED, s, m, c) ? 1u : 0u; };
        const bool zero = !__syncthreads_or(bp_csr_start(io, g, s, BPA_PACKED, msg, dec, llrt, nullptr, tid, BPA_NT));

        int it_done = 0;
        bool conv = zero;
        if (!zero) {
#pragma clang loop unroll(disable)
            for (int it = 1;; ++it) {
                const bool last = it > io.max_iter;  // only the convergence test of the last bit pass is left
                const double alpha = alpha_for_iteration(io.ms_scaling, it);
                // ---------------- check pass (a4 / a5), speculative; candidate syndrome of the previous decisions
                bool mis = false;
                if (last) mis = bp_csr_mismatch(g, dec, m, tid, BPA_NT, synd_of);
                else
                    for (int c = tid; c < m; c += BPA_NT) {
                        const int e0 = g.rp[c], e1 = g.rp[c + 1];
                        const bool sbit = synd_of(c) != 0u;
                        unsigned int dpar = sbit ? 1u : 0u;
                        if (P.bp_method == 1) {
                            bp_csr_minsum_check(msg, pre, e0, e1, sbit, alpha, [&](int e) { dpar ^= dec[g.ci[e]]; });
                        } else {
                            double t = 1.0;
                            for (int e = e0; e < e1; ++e) {
                                dpar ^= dec[g.ci[e]];
                                pre[e] = t;
                                const double th = pm_ps_tanh_half(msg[e], P.ps_form);
                                thv[e] = th;
                                t *= th;
                            }
                            t = 1.0;
                            const double sg = sbit ? -1.0 : 1.0;
                            for (int e = e1 - 1; e >= e0; --e) {
                                const double x = pre[e] * t;
                                double o = sg * pm_ps_log_ratio(x, P.ps_form);
                                if (io.ps_clip > 0.0) {  // the comparisons are false for NaN, as on the CPU
                                    if (o > io.ps_clip) o = io.ps_clip;
                                    if (o < -io.ps_clip) o = -io.ps_clip;
                                }
                                msg[e] = o;
                                t *= thv[e];
                            }
                        }
                        mis |= dpar != 0u;
                    }
                const bool any_mis = __syncthreads_or(mis) != 0;  // (also publishes the check pass' messages)
                if (last) {
                    conv = !any_mis;
                    it_done = io.max_iter;
                    break;
                }
                if (!any_mis) {
                    conv = true;
                    it_done = it - 1;
                    break;
                }
                // ---------------- bit pass: posterior, decision, bit -> check (a6 / a7)
                for (int i = tid; i < n; i += BPA_NT) {
                    const double t = bp_csr_bit_sweep(g.ce, msg, pre, g.cp[i], g.cp[i + 1], bp_shot_prior(io, s, n, i));
                    llrt[i] = t;
                    dec[i] = (t <= 0.0) ? 1 : 0;
                }
                __syncthreads();
            }
        }
        bp_csr_finish(io, s, BPA_PACKED, conv, it_done, dec, llrt, ctl, tid, BPA_NT);
    }
}

}  // namespace bposd
