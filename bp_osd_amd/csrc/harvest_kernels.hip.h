// harvest_kernels.hip.h -- the failing shots of a Monte-Carlo batch, kept on the device (gfx950, wave64): behind the scorer
// of a detector-error-model engine (dem_score_kernel, window_score_kernel) the shots whose flag byte says "observables wrong
// on a correction that reproduces the syndrome" are listed in shot order, the residual  fault row XOR correction row  of
// every listed shot is formed and weighed, the rows of the first K listed shots are kept, and so is the residual of the
// lightest one.  Such a residual has H r = 0 and L r != 0: an undetected logical fault set, and its weight bounds the
// model's fault distance from above.  DESIGN.md 4.14 has the definition and the byte counts; the host restatement is
// bp_osd_amd/_dem_base.py (harvest_batch).
//
// Three launches on the engine's stream, none of which the host waits for on its own:
//   harvest_list_kernel   B flag bytes -> the selected rows, ascending, and their count.  One workgroup: an ordered
//                         compaction wants a prefix over everything in front of a row, and B bytes are a few tiles.
//   harvest_rows_kernel   one wave per listed shot: XOR, popcount, the rows of slots below K, the lightest (weight, row).
//   harvest_min_kernel    the lightest row's residual and the triple (count, min weight, min row).
// Everything is integer and nothing depends on arrival order: slots come from prefix sums, the lightest shot from a 64-bit
// minimum of (weight << 32) | row, which also settles a tie for the lowest row.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bposd_harvest_dev {

constexpr int LIST_THREADS = 1024;                // 16 waves, one workgroup
constexpr int LIST_BYTES = 16;                    // flag bytes per thread and tile: one 128-bit load
constexpr int LIST_TILE = LIST_THREADS * LIST_BYTES;  // 16384 rows
constexpr int ROWS_THREADS = 256;                 // 4 waves, a listed shot each
constexpr int ROWS_WAVES = ROWS_THREADS / 64;
constexpr int MIN_THREADS = 256;
constexpr unsigned long long NO_KEY = ~0ull;

// What the three kernels share in device memory between launches.
struct HarvestState {
    unsigned long long min_key;  // least (weight << 32) | row over the listed shots, NO_KEY while there is none
    int count;                   // listed shots
};

struct HarvestParams {
    long long B;
    int N, fw;                        // fault mechanisms, ceil(N / 64)
    int flag_mask, flag_want;         // row b is selected when (flags[b] & flag_mask) == flag_want
    long long max_rows;               // K: rows of residual_out / faults_out
    const uint8_t* flags;             // [B]
    const unsigned long long* faults; // [B][fw], padding bits zero
    // the corrections in the decoder's form: [B][fw] words (padding bits zero), or [B][N] bytes of which bit 0 counts
    const void* corr;
    int corr_packed;
    HarvestState* state;
    int* list;                        // [B]: the selected rows, ascending
    int* weight;                      // [B]: popcount of the residual, per slot of list
    unsigned long long* residual_out; // [max_rows][fw]
    unsigned long long* faults_out;   // [max_rows][fw]
    unsigned long long* min_residual; // [fw]
    int* triple;                      // [3]: count, min weight, min row (-1, -1 when nothing is listed)
};

// eight 0/1 bytes -> eight bits (byte j -> bit j), the way obs_kernel and mc_score_kernel pack a byte row
__device__ inline unsigned long long harvest_pack8(uint64_t q) { return ((q & 0x0101010101010101ull) * 0x0102040810204080ull) >> 56; }

// word w of shot b's correction row
__device__ inline unsigned long long harvest_corr_word(const HarvestParams& P, int b, int w) {
    if (P.corr_packed) return ((const unsigned long long*)P.corr)[(size_t)b * P.fw + w];
    const uint8_t* src = (const uint8_t*)P.corr + (size_t)b * P.N;  // rows start at any byte: unaligned loads
    const int lo = 64 * w;
    const int n = min(64, P.N - lo);  // >= 1: w < fw
    unsigned long long word = 0;
    int j = 0;
    for (; j + 8 <= n; j += 8) {
        uint64_t q;
        __builtin_memcpy(&q, src + lo + j, 8);
        word |= harvest_pack8(q) << j;
    }
    for (; j < n; ++j) word |= (unsigned long long)(src[lo + j] & 1) << j;  // the last, partial group: never past the row's end
    return word;
}

// ---------------------------------------------------------------------------------------------------------------------
// Thread t of the one workgroup takes the 16 flag bytes at tile + 16 t: rows ascend with the thread index, so a row's slot
// is (rows listed by earlier tiles) + (selected bytes of the threads in front of it) + (selected bytes in front of it in
// its own 16).  The middle term comes from ballots: the count c of a thread has five bits, bit i of every lane is one
// ballot, and sum_i 2^i popcount(ballot_i & lanes below) is the exclusive prefix of c in the wave; the 16 wave totals meet
// in LDS.  Two LDS rows used in turn make one barrier per tile enough.
__global__ __launch_bounds__(LIST_THREADS) void harvest_list_kernel(HarvestParams P) {
    __shared__ int wave_total[2][LIST_THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1;
    const unsigned mask = (unsigned)P.flag_mask, want = (unsigned)P.flag_want;
    int base = 0;  // rows listed by the tiles in front (uniform)
    int turn = 0;
    for (long long tile = 0; tile < P.B; tile += LIST_TILE, turn ^= 1) {
        const long long first = tile + (long long)LIST_BYTES * threadIdx.x;
        unsigned sel = 0;  // bit j: row first + j is selected
        if (first + LIST_BYTES <= P.B) {
            const uint4 v = *(const uint4*)(P.flags + first);  // (the block is 256-byte aligned, first a multiple of 16)
            const unsigned q[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < LIST_BYTES; ++j) sel |= (((q[j >> 2] >> (8 * (j & 3))) & mask) == want ? 1u : 0u) << j;
        } else {
            for (int j = 0; j < LIST_BYTES && first + j < P.B; ++j) sel |= ((P.flags[first + j] & mask) == want ? 1u : 0u) << j;
        }
        const int c = __popc(sel);
        int in_wave = 0, total = 0;
#pragma unroll
        for (int i = 0; i < 5; ++i) {  // c <= 16
            const unsigned long long bal = __ballot((c >> i) & 1);
            in_wave += __popcll(bal & below) << i;
            total += __popcll(bal) << i;
        }
        if (lane == 0) wave_total[turn][wave] = total;
        __syncthreads();
        int in_front = 0, tile_total = 0;
#pragma unroll
        for (int v = 0; v < LIST_THREADS / 64; ++v) {
            const int t = wave_total[turn][v];
            in_front += v < wave ? t : 0;
            tile_total += t;
        }
        int slot = base + in_front + in_wave;
        for (unsigned m = sel; m; m &= m - 1) P.list[slot++] = (int)(first + (__ffs(m) - 1));
        base += tile_total;
    }
    if (threadIdx.x == 0) {
        P.state->count = base;
        P.state->min_key = NO_KEY;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// One wave per listed shot (grid-stride over the slots): lane l takes words l, l + 64, ... of the fault row and of the
// correction row.  The weight of every listed shot goes out, the rows of the slots below K; the least key is reduced in the
// wave, then in the workgroup, and leaves as one 64-bit atomic minimum per workgroup that listed anything.
__global__ __launch_bounds__(ROWS_THREADS) void harvest_rows_kernel(HarvestParams P) {
    __shared__ unsigned long long wave_key[ROWS_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int count = P.state->count;
    unsigned long long key = NO_KEY;  // (the same in every lane of a wave)
    for (long long s = (long long)blockIdx.x * ROWS_WAVES + wave; s < count; s += (long long)gridDim.x * ROWS_WAVES) {
        const int b = P.list[s];
        const bool keep = s < P.max_rows;
        int wt = 0;
        for (int w = lane; w < P.fw; w += 64) {
            const unsigned long long f = P.faults[(size_t)b * P.fw + w];
            const unsigned long long r = f ^ harvest_corr_word(P, b, w);
            wt += __popcll(r);
            if (keep) {
                P.residual_out[(size_t)s * P.fw + w] = r;
                P.faults_out[(size_t)s * P.fw + w] = f;
            }
        }
        for (int d = 32; d; d >>= 1) wt += __shfl_xor(wt, d);
        if (lane == 0) P.weight[s] = wt;
        const unsigned long long k = ((unsigned long long)(unsigned)wt << 32) | (unsigned)b;
        key = k < key ? k : key;
    }
    if (lane == 0) wave_key[wave] = key;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int v = 1; v < ROWS_WAVES; ++v) key = wave_key[v] < key ? wave_key[v] : key;
        if (key != NO_KEY) atomicMin(&P.state->min_key, key);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// One workgroup: the residual of the lightest row is formed again from its two rows (it need not be among the first K), and
// the triple goes where the batch's counters go.
__global__ __launch_bounds__(MIN_THREADS) void harvest_min_kernel(HarvestParams P) {
    const unsigned long long key = P.state->min_key;
    const int count = P.state->count;
    const bool any = count > 0 && key != NO_KEY;
    const int b = (int)(unsigned)(key & 0xffffffffull);
    for (int w = threadIdx.x; w < P.fw; w += MIN_THREADS)
        P.min_residual[w] = any ? P.faults[(size_t)b * P.fw + w] ^ harvest_corr_word(P, b, w) : 0ull;
    if (threadIdx.x == 0) {
        P.triple[0] = count;
        P.triple[1] = any ? (int)(key >> 32) : -1;
        P.triple[2] = any ? b : -1;
    }
}

}  // namespace bposd_harvest_dev
