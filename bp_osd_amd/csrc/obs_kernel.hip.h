// obs_kernel.hip.h -- logical observables of a batch of decoder rows (gfx950, wave64): for every shot and every present
// row set (osdw, osd0, bp) the k bits  parity(popcount(L_j & row))  as ceil(k / 64) packed words.  It is what a caller of
// a decoder asks of a correction -- which observables does it flip -- computed behind the OSD kernel on the rows the lane
// holds, so that k bits per shot leave the device instead of n.  DESIGN.md "Observables" has the mapping and the byte counts.
//
// The shape is that of mc_score_kernel / syndrome_pass (mc_kernels.hip.h): one workgroup of OBS_THREADS threads works on one
// shot at a time (grid-stride over the batch), the shot's rows are staged packed in LDS (byte rows are packed on the way
// in), thread t takes logical base + t, and one wave's __ballot is one output word.  L is stored transposed and packed,
// [words][k], so that the threads of a wave read consecutive words; it stays in LDS for the whole grid-stride loop where it
// fits OBS_TABLE_LDS_BUDGET and is read from global memory (L2-resident: every workgroup reads the same table) otherwise.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bposd_obs_dev {

constexpr int OBS_THREADS = 256;  // 4 waves
constexpr int OBS_SETS = 3;       // osdw, osd0, bp
constexpr int OBS_MAX_N = 32768;  // rows up to the library's largest code (n <= 32767) and any caller-owned rows up to this
constexpr int OBS_MAX_WORDS = OBS_MAX_N / 64;
constexpr int OBS_MAX_K = 4096;
// LDS a workgroup may spend on the table.  With the staged rows of the largest code this is 76 KB: two workgroups still
// share a CU's 160 KB, and the tables of the codes the project decodes today fit many times over ([[1922,50]]: 12.4 KB).
constexpr size_t OBS_TABLE_LDS_BUDGET = 64 * 1024;
constexpr size_t OBS_LDS_PER_CU = 160 * 1024;
static_assert(OBS_TABLE_LDS_BUDGET + OBS_SETS * OBS_MAX_WORDS * sizeof(unsigned long long) <= OBS_LDS_PER_CU / 2,
              "table budget + row staging: two workgroups per CU");

struct ObsParams {
    long long B;
    int n, words;        // bits of a row, ceil(n / 64)
    int k, kw;           // observables, ceil(k / 64)
    int packed;          // rows are [B][words] words (padding bits zero), else [B][n] bytes
    int table_in_lds;    // the host's decision: words * k * 8 <= OBS_TABLE_LDS_BUDGET
    const unsigned long long* table;    // [words][k]
    const void* rows[OBS_SETS];         // null: that set is absent
    unsigned long long* out[OBS_SETS];  // [B][kw]
};

inline size_t obs_table_bytes(int words, int k) { return (size_t)words * (size_t)k * sizeof(unsigned long long); }
inline bool obs_table_fits_lds(int words, int k) { return obs_table_bytes(words, k) <= OBS_TABLE_LDS_BUDGET; }
inline size_t obs_lds_bytes(int words, int k) {
    return OBS_SETS * (size_t)words * sizeof(unsigned long long) + (obs_table_fits_lds(words, k) ? obs_table_bytes(words, k) : 0);
}

// eight 0/1 bytes -> eight bits (byte j -> bit j)
__device__ inline unsigned obs_pack8(uint64_t q) { return (unsigned)(((q & 0x0101010101010101ull) * 0x0102040810204080ull) >> 56); }

__global__ __launch_bounds__(OBS_THREADS) void obs_kernel(ObsParams P) {
    extern __shared__ unsigned long long obs_lds[];  // [OBS_SETS][words] staged rows, then (table_in_lds) [words][k]
    unsigned long long* stage = obs_lds;
    const unsigned long long* __restrict__ T = P.table;
    if (P.table_in_lds) {
        unsigned long long* t_lds = obs_lds + OBS_SETS * (size_t)P.words;
        const int cells = P.words * P.k;
        for (int i = threadIdx.x; i < cells; i += OBS_THREADS) t_lds[i] = P.table[i];
        T = t_lds;  // (the first shot's barrier below publishes it)
    }
    const int lane = threadIdx.x & 63;
    const int row_bytes = P.words * 8;
    const int full = P.n >> 3;  // 8-byte groups wholly inside a byte row
    const bool have0 = P.rows[0] != nullptr, have1 = P.rows[1] != nullptr, have2 = P.rows[2] != nullptr;

    for (long long b = blockIdx.x; b < P.B; b += gridDim.x) {
#pragma unroll
        for (int s = 0; s < OBS_SETS; ++s) {
            if (!P.rows[s]) continue;
            if (P.packed) {
                const unsigned long long* src = (const unsigned long long*)P.rows[s] + (size_t)b * P.words;
                for (int w = threadIdx.x; w < P.words; w += OBS_THREADS) stage[s * P.words + w] = src[w];
            } else {
                // one 8-byte load of a byte row makes one byte of the packed row
                const uint8_t* src = (const uint8_t*)P.rows[s] + (size_t)b * P.n;
                uint8_t* dst = (uint8_t*)(stage + s * P.words);
                for (int j = threadIdx.x; j < row_bytes; j += OBS_THREADS) {
                    unsigned bits = 0;
                    if (j < full) {
                        uint64_t q;
                        __builtin_memcpy(&q, src + 8 * (size_t)j, 8);  // rows start at any byte: unaligned load
                        bits = obs_pack8(q);
                    } else if (8 * j < P.n) {  // the last, partial group of a row: byte by byte, never past the row's end
                        for (int i = 8 * j; i < P.n; ++i) bits |= (unsigned)(src[i] & 1) << (i & 7);
                    }
                    dst[j] = (uint8_t)bits;
                }
            }
        }
        __syncthreads();
        for (int base = 0; base < P.k; base += OBS_THREADS) {  // uniform trip count: the ballots below want whole waves
            const int j = base + (int)threadIdx.x;
            unsigned long long a0 = 0, a1 = 0, a2 = 0;
            if (j < P.k) {
                for (int w = 0; w < P.words; ++w) {
                    const unsigned long long t = T[(size_t)w * P.k + j];
                    if (have0) a0 ^= t & stage[w];
                    if (have1) a1 ^= t & stage[P.words + w];
                    if (have2) a2 ^= t & stage[2 * P.words + w];
                }
            }
            const bool store = lane == 0 && (j & ~63) < P.k;  // (bits of logicals >= k are zero: padding)
            if (have0) {
                const unsigned long long word = __ballot(__popcll(a0) & 1);
                if (store) P.out[0][(size_t)b * P.kw + (j >> 6)] = word;
            }
            if (have1) {
                const unsigned long long word = __ballot(__popcll(a1) & 1);
                if (store) P.out[1][(size_t)b * P.kw + (j >> 6)] = word;
            }
            if (have2) {
                const unsigned long long word = __ballot(__popcll(a2) & 1);
                if (store) P.out[2][(size_t)b * P.kw + (j >> 6)] = word;
            }
        }
        __syncthreads();  // the staged rows are overwritten by the next shot
    }
}

}  // namespace bposd_obs_dev
