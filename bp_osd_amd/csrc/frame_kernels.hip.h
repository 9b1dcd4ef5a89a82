// frame_kernels.hip.h -- Pauli-frame propagation of the elementary faults of a Clifford circuit (bposd_frame_* of
// include/bposd_mi355x.h), and the reduction of the resulting detector / observable rows to columns.
//
// Bit-sliced: a uint64 word holds one bit of 64 consecutive faults, bit j of word w belongs to fault 64 w + j.  A chunk of
// nw words keeps x[Q][nw], z[Q][nw], D[M][nw], O[k][nw] in HBM, word index innermost, zeroed by the launcher.  One thread
// of frame_propagate_kernel owns one word: it walks the op table once, injects those of its 64 faults that sit in front
// of the op, applies the op to the words of the qubits it names, and at a measurement XORs the flip word into the rows of
// the detectors and observables that hold the measurement.  Threads never communicate: no barrier, no LDS, no atomic, and
// every word is read and written by one thread only.  The op table and the measurement tables are wave-uniform reads.
//
// The faults are sorted by position, so a word's frame is zero before its first fault, and the first word of a wave has the
// earliest first fault of the wave: the wave starts at that op.  Lanes whose first fault comes later apply the ops in
// between to zero words, which changes nothing.
//
// frame_propagate_layered_kernel is the same walk with up to FRAME_GROUP ops in flight: grp[t] says how many ops from t on
// act on disjoint qubits, hold no measurement, and are disjoint from the faults that sit between them (the launcher works
// that out per call: a memory-experiment circuit is layers of such ops with noise behind each gate).  The loads of a group
// are issued before its first store, so the thread waits for one global-memory round trip per group, not per op; the
// faults inside a group are injected behind it, which their disjointness makes the same frame.
//
// frame_count_kernel / frame_fill_kernel: one wave per word, lane j = fault 64 w + j.  The rows are read at a wave-uniform
// address and zero words are skipped; count gives the set rows per fault, fill writes their indices in ascending order at
// the offsets a prefix sum of the counts gave: count, prefix, fill, no slot is grabbed and the output is deterministic.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace bposd_frame_dev {

// opcodes of the op table (BPOSD_FRAME_OP_* of the public header)
enum { OP_R = 0, OP_RX = 1, OP_M = 2, OP_MX = 3, OP_MR = 4, OP_MRX = 5, OP_H = 6, OP_S = 7, OP_CX = 8, OP_CZ = 9, OP_COUNT = 10 };

constexpr int FRAME_THREADS = 256;
constexpr int FRAME_GROUP = 4;

typedef unsigned long long u64;

struct FramePropagateParams {
    const int* ops;          // [T][3]: opcode, a, b
    const int* meas_before;  // [T + 1]: measurements in front of op t
    int T;
    const int *md_ptr, *md_idx;  // measurement -> detector rows (CSR over measurements)
    const int *mo_ptr, *mo_idx;  // measurement -> observable rows
    const int* grp;              // [T], frame_propagate_layered_kernel only: ops from t on that go as one group, 1 .. FRAME_GROUP
    const int *f_pos, *f_qa, *f_qb;  // [F], sorted by pos
    const uint8_t* f_pauli;          // [F]: pa | pb << 2
    long long F;
    long long word0;  // first word of the chunk
    int nw;           // words of the chunk: the row stride of x, z, D, O
    u64 *x, *z, *D, *O;
};

__device__ __forceinline__ void frame_inject(const FramePropagateParams& P, long long c, size_t w) {
    const u64 bit = 1ull << (c & 63);
    const int pauli = P.f_pauli[c];
    const size_t a = (size_t)P.f_qa[c] * P.nw + w;
    if (pauli & 1) P.x[a] ^= bit;
    if (pauli & 2) P.z[a] ^= bit;
    const int qb = P.f_qb[c];
    if (qb >= 0) {
        const size_t b = (size_t)qb * P.nw + w;
        if (pauli & 4) P.x[b] ^= bit;
        if (pauli & 8) P.z[b] ^= bit;
    }
}

// A measurement: the flip word goes into the rows that hold measurement mi.
__device__ __forceinline__ void frame_measure(const FramePropagateParams& P, int op, size_t a, size_t ld, size_t w, int mi) {
    const u64 flip = (op == OP_M || op == OP_MR) ? P.x[a] : P.z[a];
    for (int e = P.md_ptr[mi]; e < P.md_ptr[mi + 1]; ++e) P.D[(size_t)P.md_idx[e] * ld + w] ^= flip;
    for (int e = P.mo_ptr[mi]; e < P.mo_ptr[mi + 1]; ++e) P.O[(size_t)P.mo_idx[e] * ld + w] ^= flip;
    if (op == OP_MR || op == OP_MRX) {
        P.x[a] = 0;
        P.z[a] = 0;
    }
}

__global__ __launch_bounds__(FRAME_THREADS) void frame_propagate_kernel(const FramePropagateParams P) {
    const int wi = blockIdx.x * FRAME_THREADS + threadIdx.x;
    if (wi >= P.nw) return;
    const size_t w = (size_t)wi;
    const size_t ld = (size_t)P.nw;
    // the wave's first word is a live one (wi >= its index), and holds the earliest fault of the wave
    const int wave_word = __builtin_amdgcn_readfirstlane(wi & ~63);
    const int t0 = __builtin_amdgcn_readfirstlane(P.f_pos[64 * (P.word0 + wave_word)]);
    long long c = 64 * (P.word0 + wi);
    const long long end = c + 64 < P.F ? c + 64 : P.F;
    int next = c < end ? P.f_pos[c] : 0x7fffffff;
    int mi = P.meas_before[t0 < P.T ? t0 : P.T];
    for (int t = t0; t < P.T; ++t) {
        while (next == t) {
            frame_inject(P, c, w);
            ++c;
            next = c < end ? P.f_pos[c] : 0x7fffffff;
        }
        const int op = P.ops[3 * (size_t)t], qa = P.ops[3 * (size_t)t + 1], qb = P.ops[3 * (size_t)t + 2];
        const size_t a = (size_t)qa * ld + w, b = (size_t)qb * ld + w;
        switch (op) {
            case OP_H: {
                const u64 xa = P.x[a], za = P.z[a];
                P.x[a] = za;
                P.z[a] = xa;
                break;
            }
            case OP_S:
                P.z[a] ^= P.x[a];
                break;
            case OP_CX: {
                const u64 xa = P.x[a], zb = P.z[b];
                P.x[b] ^= xa;
                P.z[a] ^= zb;
                break;
            }
            case OP_CZ: {
                const u64 xa = P.x[a], xb = P.x[b];
                P.z[a] ^= xb;
                P.z[b] ^= xa;
                break;
            }
            case OP_R:
            case OP_RX:
                P.x[a] = 0;
                P.z[a] = 0;
                break;
            default:  // M, MX, MR, MRX
                frame_measure(P, op, a, ld, w, mi);
                ++mi;
                break;
        }
    }
    // (faults at pos == T are never injected: nothing is measured behind them)
}

__global__ __launch_bounds__(FRAME_THREADS) void frame_propagate_layered_kernel(const FramePropagateParams P) {
    const int wi = blockIdx.x * FRAME_THREADS + threadIdx.x;
    if (wi >= P.nw) return;
    const size_t w = (size_t)wi;
    const size_t ld = (size_t)P.nw;
    const int wave_word = __builtin_amdgcn_readfirstlane(wi & ~63);
    const int t0 = __builtin_amdgcn_readfirstlane(P.f_pos[64 * (P.word0 + wave_word)]);
    long long c = 64 * (P.word0 + wi);
    const long long end = c + 64 < P.F ? c + 64 : P.F;
    int next = c < end ? P.f_pos[c] : 0x7fffffff;
    int mi = P.meas_before[t0 < P.T ? t0 : P.T];
    int t = t0;
    while (t < P.T) {
        while (next <= t) {  // in front of op t, or inside the group that ended there
            frame_inject(P, c, w);
            ++c;
            next = c < end ? P.f_pos[c] : 0x7fffffff;
        }
        const int n = P.grp[t];
        const int op0 = P.ops[3 * (size_t)t];
        if (op0 >= OP_M && op0 <= OP_MRX) {  // (a measurement is a group of its own)
            frame_measure(P, op0, (size_t)P.ops[3 * (size_t)t + 1] * ld + w, ld, w, mi);
            ++mi;
            ++t;
            continue;
        }
        int op[FRAME_GROUP];
        size_t a[FRAME_GROUP], b[FRAME_GROUP];
        u64 xa[FRAME_GROUP], za[FRAME_GROUP], xb[FRAME_GROUP], zb[FRAME_GROUP];
#pragma unroll
        for (int i = 0; i < FRAME_GROUP; ++i) {
            if (i >= n) break;
            op[i] = P.ops[3 * (size_t)(t + i)];
            a[i] = (size_t)P.ops[3 * (size_t)(t + i) + 1] * ld + w;
            b[i] = (op[i] == OP_CX || op[i] == OP_CZ) ? (size_t)P.ops[3 * (size_t)(t + i) + 2] * ld + w : a[i];
            xa[i] = P.x[a[i]];
            za[i] = P.z[a[i]];
            xb[i] = P.x[b[i]];
            zb[i] = P.z[b[i]];
        }
#pragma unroll
        for (int i = 0; i < FRAME_GROUP; ++i) {
            if (i >= n) break;
            switch (op[i]) {
                case OP_H:
                    P.x[a[i]] = za[i];
                    P.z[a[i]] = xa[i];
                    break;
                case OP_S:
                    P.z[a[i]] = za[i] ^ xa[i];
                    break;
                case OP_CX:
                    P.x[b[i]] = xb[i] ^ xa[i];
                    P.z[a[i]] = za[i] ^ zb[i];
                    break;
                case OP_CZ:
                    P.z[a[i]] = za[i] ^ xb[i];
                    P.z[b[i]] = zb[i] ^ xa[i];
                    break;
                default:  // R, RX
                    P.x[a[i]] = 0;
                    P.z[a[i]] = 0;
                    break;
            }
        }
        t += n;
    }
}

// Rows [rows][nw] of a chunk; one wave (one workgroup of 64) per word.
struct FrameRowsParams {
    const u64 *D, *O;
    int M, k, nw;
    long long fault0, F;  // first fault of the chunk, faults in all
    int *cnt_h, *cnt_l;         // [64 nw], count: out
    const int *off_h, *off_l;   // [64 nw], fill: where a fault's indices start in idx_h / idx_l
    int *idx_h, *idx_l;
};

__device__ __forceinline__ int frame_count_rows(const u64* rows, int n, size_t ld, size_t w, int lane) {
    int cnt = 0;
    int r = 0;
    for (; r + 4 <= n; r += 4) {
        const u64 a0 = rows[(size_t)r * ld + w], a1 = rows[(size_t)(r + 1) * ld + w], a2 = rows[(size_t)(r + 2) * ld + w], a3 = rows[(size_t)(r + 3) * ld + w];
        if ((a0 | a1 | a2 | a3) == 0) continue;
        cnt += (int)((a0 >> lane) & 1) + (int)((a1 >> lane) & 1) + (int)((a2 >> lane) & 1) + (int)((a3 >> lane) & 1);
    }
    for (; r < n; ++r) cnt += (int)((rows[(size_t)r * ld + w] >> lane) & 1);
    return cnt;
}

__device__ __forceinline__ void frame_fill_rows(const u64* rows, int n, size_t ld, size_t w, int lane, int* idx, int off) {
    for (int r = 0; r < n; ++r) {
        const u64 a = rows[(size_t)r * ld + w];
        if (a == 0) continue;
        if ((a >> lane) & 1) idx[off++] = r;
    }
}

__global__ __launch_bounds__(64) void frame_count_kernel(const FrameRowsParams P) {
    const size_t w = blockIdx.x;
    const int lane = threadIdx.x;
    const int ch = frame_count_rows(P.D, P.M, (size_t)P.nw, w, lane);
    const int cl = frame_count_rows(P.O, P.k, (size_t)P.nw, w, lane);
    if (P.fault0 + 64 * (long long)w + lane >= P.F) return;  // a padding bit of the last word: no fault, and no entry
    P.cnt_h[64 * w + lane] = ch;
    P.cnt_l[64 * w + lane] = cl;
}

__global__ __launch_bounds__(64) void frame_fill_kernel(const FrameRowsParams P) {
    const size_t w = blockIdx.x;
    const int lane = threadIdx.x;
    if (P.fault0 + 64 * (long long)w + lane >= P.F) return;
    frame_fill_rows(P.D, P.M, (size_t)P.nw, w, lane, P.idx_h, P.off_h[64 * w + lane]);
    frame_fill_rows(P.O, P.k, (size_t)P.nw, w, lane, P.idx_l, P.off_l[64 * w + lane]);
}

}  // namespace bposd_frame_dev
