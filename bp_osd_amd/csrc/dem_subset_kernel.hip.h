// dem_subset_kernel.hip.h -- the fixed-weight sampler of the detector-error-model engine (gfx950, wave64): a shot whose fault
// set is not a Bernoulli row but a set of exactly w of the n mechanisms of a support (bposd_dem_set_subset).
// Global shot s is either the set of colexicographic rank s (ENUMERATE) or a uniformly drawn one (RANDOM, Floyd's algorithm
// on the project's Philox stream).  The outputs are those of dem_sample_kernel: packed fault row, H . f, L . f, and with an
// increment table the integer sum of incr over the set.  The host restatement is bp_osd_amd.dem.fault_subsets.
//
// One wave per shot.  A shot's work is w <= 64 columns, not N draws, so a workgroup per shot would leave three waves idle:
// here every wave of a workgroup owns an LDS row (dw + ow accumulator words, then fw fault words) and walks shots of its own
// grid-stride.  Lane l < w holds element l of the set, flips its column with dem_flip_column and sets its fault bit; the
// wave writes its row out with coalesced word stores and clears it.
//
// Ordering.  The rows are wave-private, so no workgroup barrier is needed, and the hardware runs one wave's LDS operations
// in the order it issued them.  What must still be said is that the compiler keeps that order: the flips are relaxed atomics
// of 32 bits and the read-back is a plain load of 64, of other lanes' work.  subset_row_fence() is a release and an acquire
// fence of WAVEFRONT scope around a wave barrier (a scheduling barrier: no instruction): every lane's atomics are ordered in
// front of every lane's loads behind it, and the loads and clearing stores of one shot in front of the next shot's atomics.
// Wavefront is the scope of the sharing; a wider one would make the other waves' traffic wait for nothing.
#pragma once
#include "dem_kernels.hip.h"

namespace bposd_dem_dev {

constexpr int DEM_SUBSET_ENUMERATE = 1, DEM_SUBSET_RANDOM = 2;  // BPOSD_DEM_SUBSET_* of the public header
constexpr int DEM_SUBSET_MAX_WEIGHT = 64;                        // one lane per element

struct DemSubsetParams {
    long long B;
    unsigned long long first_shot;  // global index of row 0: the rank (ENUMERATE) or the stream's shot (RANDOM)
    uint32_t key0, key1;            // seed, low and high word
    int mode, w;                    // DEM_SUBSET_*, 0 <= w <= min(n, 64)
    int n;                          // size of the support
    int N, fw, dw, ow;
    const int* support;             // [n] ascending fault indices: position c of a set is fault support[c]
    // ENUMERATE only: binom[(j - 1) * (n + 1) + c] = C(c, j) for j = 1 .. w, c = 0 .. n, saturated at 2^64 - 1 (a rank is
    // below 2^63, so a saturated entry compares as the true one would)
    const unsigned long long* binom;
    const int *col_ptr, *col_bits;  // as DemSampleParams
    unsigned long long* faults;       // [B][fw]
    unsigned long long* detectors;    // [B][dw]
    unsigned long long* observables;  // [B][ow]
    const long long* incr;            // [N] or NULL
    long long* logw;                  // [B], written iff incr
};

__device__ inline void subset_row_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Element `lane` of the set of colex rank r (wave-uniform) among the w-subsets of n positions; lanes >= w get -1.
// For j = w .. 1: c_j = the largest c with C(c, j) <= r, found by a 64-ary search over [j - 1, c_{j+1} - 1] (C(j - 1, j) = 0
// <= r, so the low end always passes, and C(., j) does not decrease, so the ballot is a prefix of ones).
__device__ inline int subset_unrank(const DemSubsetParams& P, unsigned long long r, int lane) {
    int mine = -1;
    int top = P.n - 1;  // r < C(n, w): c_w <= n - 1
    for (int j = P.w; j >= 1; --j) {
        const unsigned long long* row = P.binom + (size_t)(j - 1) * (size_t)(P.n + 1);
        int lo = j - 1, hi = top;
        while (true) {
            const int span = hi - lo + 1;
            const int step = (span + 63) >> 6;  // 1 once span <= 64
            const long long c = (long long)lo + (long long)lane * step;
            const bool pass = c <= hi && row[c] <= r;
            const int last = __popcll(__ballot(pass)) - 1;  // >= 0: lane 0 tests lo
            const int nlo = lo + last * step;
            hi = min(hi, nlo + step - 1);
            lo = nlo;
            if (step == 1) break;
        }
        r -= row[lo];
        if (lane == j - 1) mine = lo;
        top = lo - 1;
    }
    return mine;
}

// Element `lane` of the set Floyd's algorithm draws for shot s; lanes >= w get -1.  Lane i computes the draw of step i (two
// steps share a Philox block); the steps are then resolved in order: step i takes j = n - w + i if its draw is already in the
// set, else the draw.
__device__ inline int subset_floyd(const DemSubsetParams& P, unsigned long long s, int lane) {
    unsigned long long t = 0;
    if (lane < P.w) {
        const Philox4 o = philox4x32_10((uint32_t)s, (uint32_t)(s >> 32), (uint32_t)(lane >> 1), 1u, P.key0, P.key1);
        const bool odd = lane & 1;  // (selects, not an index: a register array indexed by a variable goes to scratch)
        const unsigned long long u = (unsigned long long)(odd ? o.v[2] : o.v[0]) | ((unsigned long long)(odd ? o.v[3] : o.v[1]) << 32);
        t = __umul64hi(u, (unsigned long long)(P.n - P.w + lane) + 1ull);
    }
    int mine = -1;
    for (int i = 0; i < P.w; ++i) {
        const int ti = __shfl((int)t, i);  // (t <= j < n < 2^31)
        const bool taken = __ballot(lane < i && mine == ti) != 0ull;
        if (lane == i) mine = taken ? P.n - P.w + i : ti;
    }
    return mine;
}

__global__ __launch_bounds__(DEM_THREADS) void dem_subset_kernel(DemSubsetParams P) {
    extern __shared__ unsigned long long subset_lds[];  // [DEM_WAVES][dw + ow + fw]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rw = P.dw + P.ow, rs = rw + P.fw;
    unsigned long long* row = subset_lds + (size_t)wave * rs;
    unsigned* acc = (unsigned*)row;
    unsigned* fbits = (unsigned*)(row + rw);
    for (int x = lane; x < rs; x += 64) row[x] = 0;
    subset_row_fence();

    const long long stride = (long long)gridDim.x * DEM_WAVES;
    for (long long b = (long long)blockIdx.x * DEM_WAVES + wave; b < P.B; b += stride) {  // (wave-uniform)
        const unsigned long long s = P.first_shot + (unsigned long long)b;
        const int pos = P.mode == DEM_SUBSET_ENUMERATE ? subset_unrank(P, s, lane) : subset_floyd(P, s, lane);
        long long lw = 0;
        if (pos >= 0) {
            const int i = P.support[pos];
            dem_flip_column(acc, P.col_ptr, P.col_bits, i);
            atomicOr(&fbits[i >> 5], 1u << (i & 31));
            if (P.incr) lw = P.incr[i];
        }
        if (P.incr) {  // 64-bit adds: a carry between the halves is the adder's business
            for (int d = 32; d; d >>= 1) lw += __shfl_xor(lw, d);
            if (lane == 0) P.logw[b] = lw;
        }
        subset_row_fence();  // the row is complete
        for (int x = lane; x < rs; x += 64) {
            const unsigned long long v = row[x];
            row[x] = 0;
            if (x < P.dw) P.detectors[(size_t)b * P.dw + x] = v;
            else if (x < rw) P.observables[(size_t)b * P.ow + (x - P.dw)] = v;
            else P.faults[(size_t)b * P.fw + (x - rw)] = v;
        }
        subset_row_fence();  // cleared in front of the next shot's flips
    }
}

}  // namespace bposd_dem_dev
