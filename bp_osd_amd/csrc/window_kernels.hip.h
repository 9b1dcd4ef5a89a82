// window_kernels.hip.h -- the kernels of the sliding-window engine (gfx950, wave64): everything of a windowed decode that is
// not a decode.  window_step_kernel sits between the decodes of windows w - 1 and w: it commits the faults window w - 1
// decided -- XORs their columns of H stacked on L out of the shot's running detector row and into its observable row, sets
// their bits of the correction row -- and gathers the detectors of window w from the running row into the syndrome row
// that window's decoder reads.  window_score_kernel holds the decoded observables against the true ones and reduces a
// batch to four integers and a failure count per observable.  DESIGN.md 4.12 has the definition and the byte counts; the
// host restatement is bp_osd_amd/window.py (_Model.decode_host).
//
// Scatter, as in dem_sample_kernel: a committed fault walks its column of the stacked CSC (bposd_dem_tables) and flips one
// bit per entry of the staged row in LDS.  XOR and OR commute, so every row is exact whatever the arrival order.  Only the
// words of the detector row that this step can touch are staged -- the host computes the range [w_lo, w_hi) per step -- so
// the work of a step does not grow with the number of rounds of the experiment.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bposd_window_dev {

constexpr int WIN_THREADS = 256;  // 4 waves
constexpr int WIN_WAVES = WIN_THREADS / 64;
constexpr int WIN_SCORE_THREADS = 256;

struct WindowStepParams {
    long long B;
    int dw, ow, fw;    // ceil(M / 64) detector words, ceil(k / 64) observable words, ceil(N / 64) fault words of a global row
    int w_lo, w_hi;    // the detector words this step stages: every committed column's detector entries and every gathered
                       // detector lie in [64 w_lo, 64 w_hi)
    // the stacked CSC of bposd_dem_tables: detector r is bit r, observable j is bit 64 * dw + j
    const int *col_ptr, *col_bits;
    // commit of the previous window (n_commit = 0: none): entry c is position commit_pos[c] of the decoded row and global
    // fault commit_fault[c]; its correction bit lives in staged correction word commit_slot[c], which is global word
    // corr_words[commit_slot[c]] of the row (n_corr distinct words, ascending)
    int n_commit, n_corr;
    const int *commit_pos, *commit_fault, *commit_slot, *corr_words;
    const void* decoded;  // [B] rows of the previous window's osdw output: decoded_cols bytes, or ceil(decoded_cols / 64) words
    int decoded_cols, decoded_packed;
    const uint8_t* prev_conv;  // [B] converge byte and iteration count of the previous window's decode
    const int* prev_iters;
    // gather of the next window (n_gather = 0: none): syndrome bit r = running bit gather_det[r]
    int n_gather;
    const int* gather_det;
    void* syndrome;  // [B] rows: n_gather bytes, or ceil(n_gather / 64) words with zero padding bits
    int syndrome_packed;
    unsigned long long* running;      // [B][dw]   in / out
    unsigned long long* observables;  // [B][ow]   in / out
    unsigned long long* correction;   // [B][fw]   in / out, or null: not wanted
    uint8_t* conv_all;                // [B]       in / out: BP converged in every window so far
    int* iters;                       // [B]       in / out: iterations summed over the windows so far
};

// dwords of LDS a step needs: the staged detector words, the observable words and the staged correction words
__host__ __device__ inline size_t window_step_lds_bytes(int w_lo, int w_hi, int ow, int n_corr) {
    return sizeof(unsigned long long) * ((size_t)(w_hi - w_lo) + (size_t)ow + (size_t)n_corr);
}

// every entry of one fault's column, dem_flip_column's way: one 32-bit LDS XOR of a single bit each.  The staged row holds
// detector words [w_lo, w_hi) and behind them the observable words, so bit positions are moved down by the words left out;
// an entry outside the staged range (the host's range rules them out) is skipped, never written.
__device__ inline void window_flip_column(unsigned* acc, const WindowStepParams& P, int i) {
    const int hi = P.col_ptr[i + 1];
    const int det_bits = 64 * P.dw, lo_bit = 64 * P.w_lo, span = 64 * (P.w_hi - P.w_lo);
    for (int e = P.col_ptr[i]; e < hi; ++e) {
        const int bit = P.col_bits[e];
        int at;
        if (bit < det_bits) {
            at = bit - lo_bit;
            if (at < 0 || at >= span) continue;
        } else {
            at = bit - det_bits;
            if (at >= 64 * P.ow) continue;
            at += span;
        }
        atomicXor(&acc[at >> 5], 1u << (at & 31));
    }
}

// One workgroup per shot, grid-stride.  Per shot: stage -> barrier -> commit -> barrier -> write back and gather -> barrier.
__global__ __launch_bounds__(WIN_THREADS) void window_step_kernel(WindowStepParams P) {
    extern __shared__ unsigned long long win_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nd = P.w_hi - P.w_lo;  // staged detector words
    const int nrow = nd + P.ow;      // ... and the observable words behind them
    unsigned long long* const row = win_lds;
    unsigned long long* const cor = win_lds + nrow;  // [n_corr]
    const int dec_words = (P.decoded_cols + 63) >> 6, syn_words = (P.n_gather + 63) >> 6;

    for (long long b = blockIdx.x; b < P.B; b += gridDim.x) {
        for (int w = threadIdx.x; w < nrow; w += WIN_THREADS)
            row[w] = w < nd ? P.running[(size_t)b * P.dw + P.w_lo + w] : P.observables[(size_t)b * P.ow + (w - nd)];
        for (int w = threadIdx.x; w < P.n_corr; w += WIN_THREADS) cor[w] = 0;
        __syncthreads();

        if (P.n_commit > 0) {
            unsigned* const acc = (unsigned*)row;
            unsigned* const cacc = (unsigned*)cor;
            for (int c = threadIdx.x; c < P.n_commit; c += WIN_THREADS) {
                const int j = P.commit_pos[c];
                bool set;
                if (P.decoded_packed)
                    set = (((const unsigned long long*)P.decoded)[(size_t)b * dec_words + (j >> 6)] >> (j & 63)) & 1ull;
                else
                    set = ((const uint8_t*)P.decoded)[(size_t)b * P.decoded_cols + j] & 1;
                if (set) {
                    const int f = P.commit_fault[c];
                    window_flip_column(acc, P, f);
                    if (P.correction) atomicOr(&cacc[2 * P.commit_slot[c] + ((f >> 5) & 1)], 1u << (f & 31));
                }
            }
            __syncthreads();  // the rows are complete
            for (int w = threadIdx.x; w < nrow; w += WIN_THREADS) {
                if (w < nd) P.running[(size_t)b * P.dw + P.w_lo + w] = row[w];
                else P.observables[(size_t)b * P.ow + (w - nd)] = row[w];
            }
            if (P.correction)  // commit sets are disjoint, so a bit is set once; a word may hold bits of earlier windows
                for (int w = threadIdx.x; w < P.n_corr; w += WIN_THREADS) {
                    const unsigned long long v = cor[w];
                    if (v) P.correction[(size_t)b * P.fw + P.corr_words[w]] |= v;
                }
        }
        if (threadIdx.x == 0) {  // the previous window's decode joins the shot's totals
            if (P.prev_conv) P.conv_all[b] = (uint8_t)((P.conv_all[b] != 0 && P.prev_conv[b] != 0) ? 1 : 0);
            if (P.prev_iters) P.iters[b] += P.prev_iters[b];
        }

        // gather: lane l of a wave takes syndrome bit 64 * word + l; one ballot is the packed word
        for (int gw = wave; gw < syn_words; gw += WIN_WAVES) {
            const int r = 64 * gw + lane;
            bool bit = false;
            if (r < P.n_gather) {
                const int at = P.gather_det[r] - 64 * P.w_lo;
                if (at >= 0 && at < 64 * nd) bit = (row[at >> 6] >> (at & 63)) & 1ull;
            }
            const unsigned long long word = __ballot(bit);
            if (P.syndrome_packed) {
                if (lane == 0) ((unsigned long long*)P.syndrome)[(size_t)b * syn_words + gw] = word;
            } else if (r < P.n_gather) {
                ((uint8_t*)P.syndrome)[(size_t)b * P.n_gather + r] = bit ? 1 : 0;
            }
        }
        __syncthreads();  // the staged row is free for the workgroup's next shot
    }
}

// ---------------------------------------------------------------------------------------------------------------------
struct WindowScoreParams {
    long long B;
    int k, ow, dw;                         // observables, ceil(k / 64), ceil(M / 64)
    const unsigned long long* detectors;   // [B][dw]: the detector rows as sampled
    const unsigned long long* residual;    // [B][dw]: the running rows behind the last window
    const unsigned long long* truth;       // [B][ow]: L . faults
    const unsigned long long* decoded;     // [B][ow]: L . correction
    const uint8_t* conv_all;               // [B]
    uint8_t* flags;                        // [B]: bit 0 observables wrong, bit 1 residual not zero, bit 3 no detector fired
    int* counters;                         // [4]: converged in every window, success, residual not zero, no detector fired
    int* obs_fail;                         // [k]: failures per observable
};

// One thread per shot, dem_score_kernel's way: counts per wave from ballots, per workgroup in LDS, one integer atomic per
// counter per workgroup.
__global__ __launch_bounds__(WIN_SCORE_THREADS) void window_score_kernel(WindowScoreParams P) {
    __shared__ int wg_count[4];
    if (threadIdx.x < 4) wg_count[threadIdx.x] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    int mine[4] = {0, 0, 0, 0};  // lane 0's share
    for (long long base = (long long)blockIdx.x * WIN_SCORE_THREADS; base < P.B; base += (long long)gridDim.x * WIN_SCORE_THREADS) {
        const long long b = base + threadIdx.x;  // (uniform trip count: the ballots below want whole waves)
        bool conv = false, ok = false, dirty = false, quiet = false;
        if (b < P.B) {
            const size_t o = (size_t)b * P.ow;
            unsigned long long diff = 0, any = 0, left = 0;
            for (int w = 0; w < P.ow; ++w) {
                const unsigned long long x = P.decoded[o + w] ^ P.truth[o + w];
                diff |= x;
                for (unsigned long long r = x; r; r &= r - 1) {  // failures are rare
                    const int j = 64 * w + __ffsll((long long)r) - 1;
                    if (j < P.k) atomicAdd(&P.obs_fail[j], 1);
                }
            }
            for (int w = 0; w < P.dw; ++w) {
                any |= P.detectors[(size_t)b * P.dw + w];
                left |= P.residual[(size_t)b * P.dw + w];
            }
            conv = P.conv_all[b] != 0;
            ok = diff == 0;
            dirty = left != 0;
            quiet = any == 0;
            P.flags[b] = (uint8_t)((ok ? 0 : 1) | (dirty ? 2 : 0) | (quiet ? 8 : 0));
        }
        mine[0] += __popcll(__ballot(conv));
        mine[1] += __popcll(__ballot(ok));
        mine[2] += __popcll(__ballot(dirty));
        mine[3] += __popcll(__ballot(quiet));
    }
    if (lane == 0)
        for (int i = 0; i < 4; ++i)
            if (mine[i]) atomicAdd(&wg_count[i], mine[i]);
    __syncthreads();
    if (threadIdx.x < 4 && wg_count[threadIdx.x]) atomicAdd(&P.counters[threadIdx.x], wg_count[threadIdx.x]);
}

}  // namespace bposd_window_dev
