// bp_serial_kernel.hip.h -- belief propagation with the SERIAL schedule (`schedule="serial"` of
// the ldpc v2 decoder; the reference itself never passes it -- css_decode_sim.py:444-463 -- so this path is built for
// API completeness and exactness, not tuned like the flooding kernels).
//
// Serial schedule: inside an iteration the bits are visited in ascending index and every bit sees the messages the bits
// before it have just written.  Bit j depends on an earlier bit i only if the two share a check, so the host sorts the
// bits into LEVELS (level(j) = 1 + max level of the earlier bits that share a check with j): bits of one level touch
// disjoint sets of checks, run in parallel, and give bit for bit what the sequential sweep gives.  One workgroup decodes
// one syndrome at a time (persistent, atomic queue); the E bit->check messages live in a per-workgroup slice of a global
// workspace indexed by CSR edge id (levels are separated by __syncthreads(): workgroup-scope release / acquire, the
// waves share the CU's L1); hard decisions sit in LDS for the convergence test after every sweep.
//
// Per bit (the CPU restatement under tests' checker directory walks the same steps): LLR := prior; for its checks top to
// bottom: message := f(current bit->check messages of the check's OTHER edges); bit->check := LLR (prefix); LLR +=
// message.  Decision = (LLR <= 0).  Then bottom to top: bit->check += suffix sum.  fp64, no contraction.
// That per-edge "all other edges" check update and the level loop are this kernel's own; the queue take, the start of a shot,
// the candidate-syndrome test and the results protocol are those of bp_csr.hip.h, shared with bp_anydeg_kernel and
// bp_relay_kernel.  The launch passes no tail flag: the kernel could report its tail, the host path does not ask it to yet.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bp_csr.hip.h"
#include "portable_math.h"

namespace bposd {

constexpr int BPS_NT = 256;
constexpr int BPS_MAXDV = 8;
constexpr int BPS_PACKED = 0;  // launched with byte rows only (native_packed() in internal.h)

struct BpSerialParams {
    BpShotIo io;  // (io.tail_flag is null: this kernel's launch does not report its tail)
    BpCsrGraph g;
    int bp_method;  // 0 product-sum, 1 min-sum
    int ps_form;    // product-sum evaluation order (portable_math.h: pm_ps_tanh_half)
    int nlevels;
    const int* __restrict__ erow;      // [E] row of a CSR edge
    const int* __restrict__ lvl_ptr;   // [nlevels + 1]
    const int* __restrict__ lvl_bits;  // [n] bits by level, ascending inside a level
    double* __restrict__ msg_ws;       // [gridDim.x][E] bit->check messages
    double* __restrict__ llr_tmp;      // [gridDim.x][n]
};

__host__ __device__ inline size_t bp_serial_lds_bytes(int n) { return bp_csr_row_bytes(n) + 8 * 4; }

__global__ __launch_bounds__(BPS_NT) void bp_serial_kernel(const BpSerialParams P) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const BpShotIo& io = P.io;
    const BpCsrGraph& g = P.g;
    const int m = io.m, n = io.n;
    const int tid = threadIdx.x;
    unsigned char* dec = smem;
    int* ctl = reinterpret_cast<int*>(smem + bp_csr_row_bytes(n));
    double* b2c = P.msg_ws + (size_t)blockIdx.x * g.E;
    double* llrt = P.llr_tmp + (size_t)blockIdx.x * n;

    for (;;) {
        const long long s = bp_csr_take(io, nullptr, ctl, tid)  /* no tail report yet: launch_bp_serial */;
        if (s < 0) break;
        const auto synd_of = [&](int c) { return bp_synd_bit(io.synd, BPS_PACKED, s, m, c) ? 1u : 0u; };
        const bool zero = !__syncthreads_or(bp_csr_start(io, g, s, BPS_PACKED, b2c, dec, llrt, nullptr, tid, BPS_NT));  // (A.2)

        int it_done = 0;
        bool conv = zero;
        if (!zero) {
#pragma clang loop unroll(disable)
            for (int it = 1; it <= io.max_iter; ++it) {
                const double alpha = alpha_for_iteration(io.ms_scaling, it);
                for (int lv = 0; lv < P.nlevels; ++lv) {
                    const int lo = P.lvl_ptr[lv], hi = P.lvl_ptr[lv + 1];
                    for (int q = lo + tid; q < hi; q += BPS_NT) {
                        const int i = P.lvl_bits[q];
                        const double l0 = bp_shot_prior(io, s, n, i);
                        double llr = l0;
                        double c2b[BPS_MAXDV];
                        const int k0 = g.cp[i], deg = g.cp[i + 1] - k0;
                        for (int d = 0; d < deg; ++d) {
                            const int e = g.ce[k0 + d], c = P.erow[e];
                            const int g0 = g.rp[c], g1 = g.rp[c + 1];
                            double msg;
                            if (P.bp_method == 0) {
                                double prod = 1.0;
                                for (int j = g0; j < g1; ++j)
                                    if (j != e) prod *= pm_ps_tanh_half(b2c[j], P.ps_form);
                                msg = (synd_of(c) ? -1.0 : 1.0) * pm_ps_log_ratio(prod, P.ps_form);
                                if (io.ps_clip > 0.0) {
                                    if (msg > io.ps_clip) msg = io.ps_clip;
                                    if (msg < -io.ps_clip) msg = -io.ps_clip;
                                }
                            } else {
                                const unsigned int sb = synd_of(c);  // (loaded here, needed behind the loop)
                                int sgn = 0;
                                double temp = __DBL_MAX__;
                                for (int j = g0; j < g1; ++j) {
                                    if (j == e) continue;
                                    const double v = b2c[j];
                                    const double a = fabs(v);
                                    if (a < temp) temp = a;
                                    if (v <= 0.0) sgn += 1;
                                }
                                const double message_sign = ((sgn + sb) & 1) ? -1.0 : 1.0;
                                msg = alpha * message_sign * temp;
                            }
                            c2b[d] = msg;
                            b2c[e] = llr;  // prefix from the top of the column (prior included)
                            llr += msg;
                        }
                        llrt[i] = llr;
                        dec[i] = (llr <= 0.0) ? 1 : 0;
                        double temp = 0.0;  // suffix from the bottom of the column
                        for (int d = deg - 1; d >= 0; --d) {
                            const int e = g.ce[k0 + d];
                            b2c[e] += temp;
                            temp += c2b[d];
                        }
                    }
                    __syncthreads();
                }
                // candidate syndrome of this sweep's decisions against the input syndrome
                it_done = it;
                if (!__syncthreads_or(bp_csr_mismatch(g, dec, m, tid, BPS_NT, synd_of))) {
                    conv = true;
                    break;
                }
            }
        }
        bp_csr_finish(io, s, BPS_PACKED, conv, it_done, dec, llrt, ctl, tid, BPS_NT);
    }
}

}  // namespace bposd
