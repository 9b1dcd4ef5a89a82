// fault_sums_kernel.hip.h -- per-fault sums over selected shots of a detector-error-model batch (gfx950, wave64): for the
// packed fault rows f_b of a batch and a list of selected rows b_0 < b_1 < ... with one 32-bit multiplier v_s each,
//     counts[i] = sum_s f_{b_s}[i]          sums[i] = sum_s v_s f_{b_s}[i]          (64-bit integers, i = 0 .. N - 1)
// -- the statistic a cross-entropy fit of the sampling row needs (the likelihood-weighted frequency of every fault among the
// failing shots), formed where the rows are: N numbers come down in place of the rows.  DESIGN.md 4.16 has the definition
// and the byte counts; the host restatement is bp_osd_amd/_dem_base.py (fault_sums_batch).
//
// Scatter, like dem_sample_kernel: the cost is the set bits of the selected rows, not rows x N.  A workgroup owns a column
// tile (blockIdx.x) and a chunk of the row list (blockIdx.y) and keeps the tile's accumulators in LDS; a wave takes a row,
// lane l word tile + l of it (one coalesced 512-byte read), and every set bit is one 32-bit LDS add (and one 64-bit LDS add of
// the row's multiplier).  Behind one barrier the non-zero accumulators go to the global 64-bit arrays with returnless atomic
// adds.  Everything is an integer add: the result does not depend on the order of arrival, nor on the grid.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bposd_fault_sums_dev {

constexpr int FS_THREADS = 256;  // 4 waves, a selected row each
constexpr int FS_WAVES = FS_THREADS / 64;
constexpr int FS_TILE_WORDS = 64;                  // words of a row per column tile: one per lane
constexpr int FS_TILE_COLS = 64 * FS_TILE_WORDS;   // 4096 faults: 16 KB of counts and 32 KB of sums in LDS

struct FaultSumsParams {
    long long rows;                    // selected rows, or an upper bound of them where `count` is given
    const int* count;                  // the device's own count of listed rows (HarvestState::count), or NULL
    const int* list;                   // [rows]: the selected rows, ascending; NULL: row s is s
    int N, fw;                         // fault mechanisms, ceil(N / 64)
    const unsigned long long* faults;  // [.][fw], padding bits zero
    const uint32_t* mult;              // [rows]: the multiplier of slot s (WEIGHTED only)
    unsigned long long* counts;        // [N], cleared in front of the launch
    unsigned long long* sums;          // [N], likewise (WEIGHTED only)
};

// Accumulator of bit j of the tile's word l.  The rotation by l spreads one bit position over the banks: with the plain index
// 64 l + j the lanes of a wave that walk the same bit of their words (a dense row) would all meet in bank j.
__device__ inline int fs_slot(int l, int j) { return 64 * l + ((j + l) & 63); }

template <bool WEIGHTED>
__global__ __launch_bounds__(FS_THREADS) void fault_sums_kernel(FaultSumsParams P) {
    __shared__ unsigned cnt[FS_TILE_COLS];
    __shared__ unsigned long long sum[WEIGHTED ? FS_TILE_COLS : 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long total = P.count ? (long long)*P.count : P.rows;
    // the chunk of this workgroup: the row list in gridDim.y equal runs (a chunk holds fewer than 2^31 rows: cnt cannot wrap)
    const long long per = (total + gridDim.y - 1) / gridDim.y;
    const long long lo = per * blockIdx.y, hi = lo + per < total ? lo + per : total;
    if (lo >= hi) return;  // (the whole workgroup)
    for (int e = threadIdx.x; e < FS_TILE_COLS; e += FS_THREADS) {
        cnt[e] = 0;
        if constexpr (WEIGHTED) sum[e] = 0;
    }
    __syncthreads();

    const int w = blockIdx.x * FS_TILE_WORDS + lane;  // this lane's word of a row
    for (long long s = lo + wave; s < hi; s += FS_WAVES) {
        const long long b = P.list ? (long long)P.list[s] : s;
        unsigned long long v = 0;
        if constexpr (WEIGHTED) v = P.mult[s];  // one load per row (the same address in every lane)
        unsigned long long m = w < P.fw ? P.faults[(size_t)b * P.fw + w] : 0ull;
        for (; m; m &= m - 1) {
            const int slot = fs_slot(lane, __ffsll((long long)m) - 1);
            atomicAdd(&cnt[slot], 1u);
            if constexpr (WEIGHTED) atomicAdd(&sum[slot], v);
        }
    }
    __syncthreads();  // the tile's accumulators are complete

    for (int e = threadIdx.x; e < FS_TILE_COLS; e += FS_THREADS) {
        const int l = e >> 6;
        const int i = blockIdx.x * FS_TILE_COLS + 64 * l + ((e - l) & 63);  // fs_slot, inverted
        const unsigned c = cnt[e];
        if (c == 0 || i >= P.N) continue;  // (a fault that never fired adds nothing to either array)
        atomicAdd(&P.counts[i], (unsigned long long)c);
        if constexpr (WEIGHTED) {
            const unsigned long long t = sum[e];
            if (t) atomicAdd(&P.sums[i], t);
        }
    }
}

}  // namespace bposd_fault_sums_dev
