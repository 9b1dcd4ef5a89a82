// bp_csr.hip.h -- what the three "complete and exact, not tuned" BP kernels share: bp_anydeg_kernel (any degree),
// bp_serial_kernel (serial schedule) and bp_relay_kernel (relay mode).  All three index messages by CSR edge, run one
// persistent workgroup per shot on the atomic queue and keep the hard decisions as a byte row in LDS; each of them is a
// schedule on top of the parameter blocks and the helpers below, and every rule here is written once: the queue take, the
// start of a shot, the min-sum check sweep, the bit sweep, the candidate-syndrome test and the results protocol the OSD
// kernels and lsd_kernel read.  The helpers are inlined into their caller and take messages as plain pointers, so a kernel
// that keeps them in LDS (bp_relay_kernel<true>) still addresses them with ds_ instructions; the thread count is an argument
// (a constant in two kernels, blockDim.x in relay).  Arithmetic and association order are those of bp_kernel.hip.h.
// The tuned kernels (bp_local, bp_class, bp_kernel, bp_large) do not use this header: their parameter structs are frozen.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bp_kernel.hip.h"

namespace bposd {

// The shot-level fields every BP kernel takes, named as in BpParams (bp_kernel.hip.h has the comments).
// Outputs in front of inputs: the inputs then sit next to the graph tables and a kernel's own pointers, with which the iteration
// loops use them.  The kernels are at their scalar-register ceiling, and with the outputs in between bp_serial_kernel restores
// 28 spilled scalars per bit of a level instead of 18 (12 in the flat struct it had before; profiles/bp_csr_core_rates.txt).
struct BpShotIo {
    int m, n;
    long long B;
    int max_iter;
    double ms_scaling;
    double ps_clip;
    int osd_enabled;
    int packed_io;
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
    const uint8_t* __restrict__ synd;
    const double* __restrict__ llr0;
    const uint8_t* __restrict__ sel;
    const double* __restrict__ llr0_alt;
    const double* __restrict__ llr0_rows;
};

struct BpCsrGraph {
    int E;
    const int* __restrict__ rp;  // CSR indptr [m + 1]
    const int* __restrict__ ci;  // CSR indices [E]
    const int* __restrict__ cp;  // CSC indptr [n + 1]
    const int* __restrict__ ce;  // [E] CSR edge ids of a column, ascending row
};

// decision bytes of a shot, padded to 16, in front of whatever else a kernel keeps in LDS
__host__ __device__ inline size_t bp_csr_row_bytes(int n) { return (size_t)((n + 15) & ~15); }

// The loops of bp_csr_start and bp_csr_finish run once per shot and index by thread.  Their addresses do not change from shot to
// shot, so the compiler computes them once per kernel and holds them through every iteration loop in between (8 VGPRs in
// bp_anydeg_kernel, a wave per SIMD).  Behind this opaque copy of the thread index they are formed where they are used.
__device__ __forceinline__ int bp_csr_per_shot_tid(int tid) {
    asm volatile("" : "+v"(tid));
    return tid;
}

// The queue take: the next shot, or -1 when the queue is empty (the workgroup that finds it just empty reports the tail to
// tail_flag, nullable).  ctl: two LDS words of the workgroup, [0] queue index, [1] OSD list slot (bp_csr_finish).  One barrier.
// tail_flag here and `packed` below (the form of the syndrome and result rows, BpParams::packed_io) are arguments, not read from
// io: a kernel that is launched with one value only passes the constant and carries neither the other path nor its registers.
__device__ __forceinline__ long long bp_csr_take(const BpShotIo& io, int* tail_flag, int* ctl, int tid) {
    if (tid == 0) ctl[0] = atomicAdd(&io.counters[0], 1);
    __syncthreads();
    const long long s = ctl[0];
    if (s < io.B) return s;
    if (s == io.B && tid == 0 && tail_flag) *(volatile int*)tail_flag = 1;
    return -1;
}

// every edge of bit i: bit->check message := v
__device__ __forceinline__ void bp_csr_set_bit_edges(const BpCsrGraph& g, double* msg, int i, double v) {
    for (int k = g.cp[i]; k < g.cp[i + 1]; ++k) msg[g.ce[k]] = v;
}

// The start of a shot (a3): every edge's bit->check message and llr[] start at the prior, decisions = 0.  Returns whether one
// of the thread's syndrome bits is set (all-zero syndrome: zeros, converge = true, BP not run); syb, where not null, receives
// the syndrome as bytes.
__device__ __forceinline__ bool bp_csr_start(const BpShotIo& io, const BpCsrGraph& g, long long s, int packed, double* msg,
                                             unsigned char* dec, double* llr, unsigned char* syb, int tid, int nt) {
    tid = bp_csr_per_shot_tid(tid);
    bool nz = false;
    for (int c = tid; c < io.m; c += nt) {
        const bool b = bp_synd_bit(io.synd, packed, s, io.m, c);
        if (syb) syb[c] = b ? 1 : 0;
        nz |= b;
    }
    for (int i = tid; i < io.n; i += nt) {
        const double l0 = bp_shot_prior(io, s, io.n, i);
        bp_csr_set_bit_edges(g, msg, i, l0);
        dec[i] = 0;
        llr[i] = l0;
    }
    return nz;
}

// Min-sum update of one check's edges [e0, e1), in place (a4 / a5): forward, the running minimum of |b2c| in front of every
// edge goes to pre[] and the sign parity is accumulated (sbit = the check's syndrome bit); backward, it meets the running
// suffix.  edge(e) is called once per edge in the forward sweep.
template <class Edge>
__device__ __forceinline__ void bp_csr_minsum_check(double* msg, double* pre, int e0, int e1, bool sbit, double alpha, Edge edge) {
    double t = __DBL_MAX__;
    bool par = sbit;
    for (int e = e0; e < e1; ++e) {
        edge(e);
        const double v = msg[e];
        pre[e] = t;
        t = min_abs(t, v);
        par ^= (v <= 0.0);  // a zero counts as negative, as in the reference
    }
    double suf = __DBL_MAX__;
    for (int e = e1 - 1; e >= e0; --e) {
        const double v = msg[e];
        const double mag = min_pos(pre[e], suf);
        msg[e] = flip_sign(mag * alpha, par ^ (v <= 0.0));
        suf = min_abs(suf, v);
    }
}

// Bit update of one bit's edges ce[k0 .. k1), in place (a6 / a7), in ascending check order: forward stores the prefix sums
// ((start + c[0]) + ...) + c[d-1], backward adds the suffix sums ((0.0 + c[D-1]) + ...) + c[d+1].  Returns the posterior.
__device__ __forceinline__ double bp_csr_bit_sweep(const int* ce, double* msg, double* pre, int k0, int k1, double start) {
    double t = start;
    for (int k = k0; k < k1; ++k) {
        const int e = ce[k];
        pre[e] = t;
        t += msg[e];
    }
    double suf = 0.0;
    for (int k = k1 - 1; k >= k0; --k) {
        const int e = ce[k];
        const double cm = msg[e];
        msg[e] = pre[e] + suf;
        suf += cm;
    }
    return t;
}

// parity of check c under the decisions, started at its syndrome bit (0 / 1): 0 where H * dec agrees with the syndrome
// (an integer from the start: from a bool the compiler no longer runs four edges of the loop at a time)
__device__ __forceinline__ unsigned int bp_csr_check_parity(const BpCsrGraph& g, const unsigned char* dec, int c, unsigned int sbit) {
    unsigned int par = sbit;
    for (int e = g.rp[c]; e < g.rp[c + 1]; ++e) par ^= dec[g.ci[e]];
    return par;
}

// The thread's half of H * dec == syndrome: does one of its checks disagree?  synd_of(c) = the check's syndrome bit, 0 / 1.  The
// workgroup reduction stays with the kernel (__syncthreads_or costs static LDS, which relay cannot spare).
template <class SyndOf>
__device__ __forceinline__ bool bp_csr_mismatch(const BpCsrGraph& g, const unsigned char* dec, int m, int tid, int nt, SyndOf synd_of) {
    bool mis = false;
    for (int c = tid; c < m; c += nt) mis |= bp_csr_check_parity(g, dec, c, synd_of(c)) != 0u;
    return mis;
}

// The results of shot s, as every OSD kernel and lsd_kernel expect them: a shot that did not converge takes a slot of the OSD
// list (where OSD is on) and leaves its LLRs there; the others write all three result rows.  row: the decisions, bytes in LDS;
// llr: n doubles; ctl as in bp_csr_take.  Rows are bytes, or 64-bit words where the call is packed: one thread forms each word
// from the byte row.  Ends with the barrier behind which row, llr and ctl may be written again.
__device__ __forceinline__ void bp_csr_finish(const BpShotIo& io, long long s, int packed, bool conv, int iters,
                                              const unsigned char* row, const double* llr, int* ctl, int tid, int nt) {
    tid = bp_csr_per_shot_tid(tid);
    const int n = io.n;
    const bool to_osd = (!conv) && io.osd_enabled;
    if (tid == 0) {
        if (to_osd) {
            const int slot = atomicAdd(&io.counters[1], 1);
            io.osd_list[slot] = (int)s;
            ctl[1] = slot;
        }
        if (io.out_conv) io.out_conv[s] = conv ? 1 : 0;
        if (io.out_iters) io.out_iters[s] = iters;
        if (iters) atomicAdd(io.iter_total, (unsigned long long)iters);
    }
    __syncthreads();
    const int slot = to_osd ? ctl[1] : 0;
    for (int i = tid; i < n; i += nt) {
        const size_t o = (size_t)s * n + i;
        if (!packed) {
            const uint8_t b = row[i];
            if (io.out_bp) io.out_bp[o] = b;
            if (!to_osd) {
                io.out_osdw[o] = b;
                if (io.out_osd0) io.out_osd0[o] = b;
            }
        }
        if (to_osd) io.llr_ws[(size_t)slot * n + i] = llr[i];
        if (io.out_llr) io.out_llr[o] = llr[i];
    }
    if (packed) {
        const int wpn = (n + 63) >> 6;
        for (int w = tid; w < wpn; w += nt) {
            unsigned long long v = 0ull;
            const int hi = min(64, n - 64 * w);
            for (int b = 0; b < hi; ++b) v |= (unsigned long long)(row[64 * w + b] & 1) << b;
            const size_t o = (size_t)s * wpn + w;
            if (io.out_bp) ((unsigned long long*)io.out_bp)[o] = v;
            if (!to_osd) {
                ((unsigned long long*)io.out_osdw)[o] = v;
                if (io.out_osd0) ((unsigned long long*)io.out_osd0)[o] = v;
            }
        }
    }
    __syncthreads();
}

}  // namespace bposd
