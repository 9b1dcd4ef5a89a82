// lsd_kernel.hip.h -- LSD: localized statistics decoding of the shots BP left open.
//
// The definition is the synchronous one of bp_osd_amd/lsd.py (lsd_decode_reference) and of the comment at bposd_set_lsd:
// every unsatisfied check starts as a cluster; in a round every invalid cluster selects the first free bit in the OSD
// stage's column order among the bits next to its checks, all selected bits join at once with their checks, clusters that
// meet merge, and every cluster that changed is eliminated afresh.  The result does not depend on the order clusters are
// visited in, so the mapping below is free.
//
// One wave (a workgroup of 64 threads) per listed shot, on an atomic queue over the BP stage's list.
//   LDS      uf[m]    16 bits per check: 0xFFFF = in no cluster, else its parent in a union-find forest over check indices
//                     (flattened after the merges of every round, so between rounds uf[c] IS the cluster of check c)
//            lrow[m]  16 bits per check: scratch of a sparse set (never cleared: entry v of check c counts only if
//                     v < count and list[v] == c) -- the local row of a check during an elimination, and the duplicate test
//                     when the changed clusters of a round are listed
//            taken    1 bit per bit: the bit is in a cluster;   xsol  1 bit per bit: the solution so far
//            one elimination: LSD_MAXC rows of LSD_WPR 64-bit words, row r in lane r & 63 (LSD_RPL rows per lane), pivots
//            by ballot as in osd_wave_kernel; the cluster's bits sorted into column order by counting
//   global   per workgroup (P.ws): inv[m] the invalid clusters, sel[m] the bit each selected, jb[n] the joined bits
// A cluster's members are not kept: its bits are the joined bits whose first check lies in it, its checks the checks of
// those bits (every check of a cluster with a bit is next to one of its bits: a seed check selected a neighbour).
// Loop bounds: at most n rounds (every round joins a bit), every inner loop over a count fixed before it starts.
//
// lsd_kernel<false> is LSD-0.  lsd_kernel<true> (method lsd_cs / lsd_e, or min_free_bits > 0) adds, in `if constexpr (HO)`
// blocks only: a valid cluster with fewer than min_free free columns and fewer than grow_limit bits stays on the inv / sel
// list and selects like an invalid one (with nothing to select it is finished); a cluster that finishes is swept while its
// reduced rows still sit in LDS -- one candidate per lane, 64 at a time, every lane walking the cluster's bits in ascending
// bit index (perm, built by counting as cbs is) and adding the bit's cost (1.0 where the OSD stage counts bits, so one loop
// serves both weights) where its candidate sets the bit; the lightest (weight, candidate index) over lanes and rounds goes
// into a second bitmap xw.  A cluster that merges later is eliminated and swept again over all its bits, so at the end xw
// holds the final clusters' rows.  LDS of the sweep: prow[p] the pivot row of column position p (LSD_NONE: a free column),
// fcol the free column positions in order, perm; the costs by column position take the place of the sort keys (ck).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bp_kernel.hip.h"

namespace bposd {

constexpr int LSD_NT = 64;     // one wave
constexpr int LSD_RPL = 4;     // rows per lane of an elimination
constexpr int LSD_WPR = 4;     // 64-bit words per row
constexpr int LSD_MAXC = LSD_NT * LSD_RPL;  // checks of a cluster: the ceiling of max_cluster_checks
constexpr int LSD_MAXB = 64 * LSD_WPR;      // bits of a cluster: the ceiling of max_cluster_bits
constexpr unsigned short LSD_NONE = 0xFFFFu;

struct LsdParams {
    int m, n;
    int packed_io;    // as BpParams::packed_io: the syndromes and all four row outputs
    int tie_policy;   // the OSD stage's: ties of the LLRs by ascending (0) or descending (1) bit index
    int max_bits, max_checks;
    int osd_follows;  // 1: a shot that is not solved goes to list2; 0 (osd_off): it gets BP's decisions, llr <= 0
    const uint8_t* __restrict__ synd;
    const int* __restrict__ rp;   // CSR indptr [m + 1]
    const int* __restrict__ ci;   // CSR indices [E]
    const int* __restrict__ cp;   // CSC indptr [n + 1]
    const int* __restrict__ cr;   // CSC row indices [E], ascending within a column
    const double* __restrict__ llr_ws;  // [list slot][n]
    const int* __restrict__ osd_list;   // the BP stage's list
    const int* __restrict__ counters;   // the BP stage's: [1] = entries of osd_list
    int* __restrict__ lsd_counters;     // [1] entries of list2, [2] the OSD kernels' queue over it, [3] this kernel's queue
    int* __restrict__ list2;
    double* __restrict__ llr_ws2;       // [list2 slot][n]
    uint8_t* __restrict__ out_osd0;     // nullable
    uint8_t* __restrict__ out_osdw;
    uint8_t* __restrict__ cmp_osd0;     // nullable: the rows again at [list slot of osd_list]
    uint8_t* __restrict__ cmp_osdw;
    int* __restrict__ st_status;        // [B] each
    int* __restrict__ st_rounds;
    int* __restrict__ st_clusters;
    int* __restrict__ st_maxbits;
    int* ws;                            // [gridDim.x][lsd_ws_ints]
    // ---- lsd_kernel<true> only
    int method, order;                  // 0 lsd_0, 1 lsd_cs, 2 lsd_e
    int min_free, grow_limit;
    int e_msb_first;                    // the handle's osd_e_bit_order
    const double* __restrict__ cost;       // as OsdParams: null = the OSD stage counts bits
    const uint8_t* __restrict__ sel;
    const double* __restrict__ cost_alt;
    const double* __restrict__ cost_rows;
    int* __restrict__ st_maxfree;       // [B] each
    int* __restrict__ st_improved;
};

// inv | sel | jb, and for lsd_kernel<true> the free columns of every finished cluster at its root check
__host__ __device__ inline size_t lsd_ws_ints(int m, int n, bool ho = false) { return (ho ? 3 : 2) * (size_t)m + (size_t)n; }
__host__ __device__ inline size_t lsd_pad8(size_t x) { return (x + 7) & ~(size_t)7; }
// uf | lrow | taken | xsol | syn | rows | keys | cb | cbs | cc | pivcol | rsy | used | 16 control ints
// lsd_kernel<true> appends: xw | prow | fcol | perm
__host__ __device__ inline size_t lsd_lds_bytes(int m, int n, bool ho = false) {
    return (ho ? 8 * (size_t)((n + 63) / 64) + 3 * 2 * (size_t)LSD_MAXB : 0) + 2 * lsd_pad8(2 * (size_t)m) + lsd_pad8(4 * (size_t)((n + 31) / 32)) + 8 * (size_t)((n + 63) / 64) + lsd_pad8(4 * (size_t)((m + 31) / 32)) +
           8 * (size_t)LSD_MAXC * LSD_WPR + 8 * (size_t)LSD_MAXB + 3 * 2 * (size_t)LSD_MAXB + 2 * (size_t)LSD_MAXC + 2 * (size_t)LSD_MAXC + 64;
}

// does bit a (LLR la) come before bit b in the OSD stage's column order?
__device__ __forceinline__ bool lsd_before(double la, int a, double lb, int b, int tie) {
    return la < lb || (la == lb && (tie ? a > b : a < b));
}

// the first bit in column order over the wave (i < 0: the lane has none); every lane gets the result
__device__ __forceinline__ int lsd_wave_first(double l, int i, int tie) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double ol = __shfl_xor(l, off);
        const int oi = __shfl_xor(i, off);
        if (oi >= 0 && (i < 0 || lsd_before(ol, oi, l, i, tie))) { l = ol; i = oi; }
    }
    return i;
}

__device__ __forceinline__ int lsd_lanes_below(unsigned long long bal, int lane) {
    return __popcll(bal & ((1ull << lane) - 1ull));
}

// the free column positions candidate c sets, as a mask over column positions (the enumeration of the OSD stage: osd_kernel.hip.h)
__device__ __forceinline__ void lsd_candidate(int c, int method, int w, int kp, int msb, const unsigned short* fcol, unsigned long long F[LSD_WPR]) {
#pragma unroll
    for (int x = 0; x < LSD_WPR; ++x) F[x] = 0ull;
    int t0 = -1, t1 = -1;
    unsigned int pat = 0u;
    if (c < 0) return;
    if (method == 2) pat = (unsigned int)c + 1u;
    else if (c < kp) t0 = c;
    else {  // pairs a < b < w, a outer
        int q = c - kp, a = 0;
        while (q >= w - 1 - a) { q -= w - 1 - a; ++a; }
        t0 = a;
        t1 = a + 1 + q;
    }
    for (int b = 0; b < (method == 2 ? w : 2); ++b) {
        int t;
        if (method == 2) t = ((pat >> b) & 1u) ? (msb ? w - 1 - b : b) : -1;
        else t = b == 0 ? t0 : t1;
        if (t < 0) continue;
        const int p = fcol[t];
#pragma unroll
        for (int x = 0; x < LSD_WPR; ++x) F[x] |= (p >> 6) == x ? 1ull << (p & 63) : 0ull;
    }
}

// does the candidate with the free columns F set the bit at column position p?
__device__ __forceinline__ bool lsd_candidate_bit(int p, const unsigned short* prow, const unsigned long long* rows, const unsigned char* rsy,
                                                  const unsigned long long F[LSD_WPR]) {
    const int r = prow[p];
    if (r == LSD_NONE) {
        unsigned long long f = 0ull;
#pragma unroll
        for (int x = 0; x < LSD_WPR; ++x) f |= (p >> 6) == x ? F[x] : 0ull;
        return (f >> (p & 63)) & 1ull;
    }
    unsigned long long acc = 0ull;
#pragma unroll
    for (int x = 0; x < LSD_WPR; ++x) acc ^= rows[r * LSD_WPR + x] & F[x];
    return ((__popcll(acc) ^ rsy[r]) & 1) != 0;
}

template <bool HO>
__global__ __launch_bounds__(LSD_NT) void lsd_kernel(const LsdParams P) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int m = P.m, n = P.n, lane = threadIdx.x, tie = P.tie_policy;
    const int wpn = (n + 63) >> 6, tw = (n + 31) >> 5, sw = (m + 31) >> 5;
    unsigned char* q8 = smem;
    unsigned short* uf = reinterpret_cast<unsigned short*>(q8);   q8 += lsd_pad8(2 * (size_t)m);
    unsigned short* lrow = reinterpret_cast<unsigned short*>(q8); q8 += lsd_pad8(2 * (size_t)m);
    unsigned int* taken = reinterpret_cast<unsigned int*>(q8);    q8 += lsd_pad8(4 * (size_t)tw);
    unsigned int* xsol = reinterpret_cast<unsigned int*>(q8);     q8 += 8 * (size_t)wpn;
    unsigned int* syn = reinterpret_cast<unsigned int*>(q8);      q8 += lsd_pad8(4 * (size_t)sw);
    unsigned long long* rows = reinterpret_cast<unsigned long long*>(q8); q8 += 8 * (size_t)LSD_MAXC * LSD_WPR;
    double* ck = reinterpret_cast<double*>(q8);                   q8 += 8 * (size_t)LSD_MAXB;
    unsigned short* cb = reinterpret_cast<unsigned short*>(q8);   q8 += 2 * (size_t)LSD_MAXB;   // a cluster's bits as found
    unsigned short* cbs = reinterpret_cast<unsigned short*>(q8);  q8 += 2 * (size_t)LSD_MAXB;   // ... in column order
    unsigned short* pivcol = reinterpret_cast<unsigned short*>(q8); q8 += 2 * (size_t)LSD_MAXB; // (LSD_MAXC == LSD_MAXB entries)
    unsigned short* cc = reinterpret_cast<unsigned short*>(q8);   q8 += 2 * (size_t)LSD_MAXC;   // a cluster's checks
    unsigned char* rsy = q8;                                      q8 += LSD_MAXC;               // syndrome bit of a row
    unsigned char* used = q8;                                     q8 += LSD_MAXC;               // the row is a pivot row
    int* sh = reinterpret_cast<int*>(q8);                         q8 += 64;
    unsigned int* xw = reinterpret_cast<unsigned int*>(q8);       q8 += 8 * (size_t)wpn;        // (HO) the sweep's rows
    unsigned short* prow = reinterpret_cast<unsigned short*>(q8); q8 += 2 * (size_t)LSD_MAXB;
    unsigned short* fcol = reinterpret_cast<unsigned short*>(q8); q8 += 2 * (size_t)LSD_MAXB;
    unsigned short* perm = reinterpret_cast<unsigned short*>(q8);
    int* inv = P.ws + (size_t)blockIdx.x * lsd_ws_ints(m, n, HO);
    int* sel = inv + m;
    int* jb = sel + m;
    int* cfree = jb + n;  // (HO)

    for (;;) {
        if (lane == 0) sh[0] = atomicAdd(&P.lsd_counters[3], 1);
        __syncthreads();
        const int slot = sh[0];
        if (slot >= P.counters[1]) break;
        const long long s = P.osd_list[slot];
        const double* __restrict__ llr = P.llr_ws + (size_t)slot * n;

        for (int c = lane; c < m; c += LSD_NT) uf[c] = LSD_NONE;
        for (int w = lane; w < tw; w += LSD_NT) taken[w] = 0u;
        for (int w = lane; w < 2 * wpn; w += LSD_NT) xsol[w] = 0u;
        if constexpr (HO)
            for (int w = lane; w < 2 * wpn; w += LSD_NT) xw[w] = 0u;
        for (int w = lane; w < sw; w += LSD_NT) {
            unsigned int v = 0u;
            for (int b = 0; b < 32 && 32 * w + b < m; ++b) v |= (bp_synd_bit(P.synd, P.packed_io, s, m, 32 * w + b) ? 1u : 0u) << b;
            syn[w] = v;
        }
        __syncthreads();

        // ---- every unsatisfied check is a cluster of its own and selects among the bits of its row
        int ninv = 0;
        for (int base = 0; base < m; base += LSD_NT) {
            const int c = base + lane;
            const bool seed = c < m && ((syn[c >> 5] >> (c & 31)) & 1u);
            const unsigned long long bal = __ballot(seed);
            if (seed) {
                const int pos = ninv + lsd_lanes_below(bal, lane);
                int best = -1;
                double bl = 0.0;
                for (int e = P.rp[c]; e < P.rp[c + 1]; ++e) {
                    const int j = P.ci[e];
                    const double l = llr[j];
                    if (best < 0 || lsd_before(l, j, bl, best, tie)) { best = j; bl = l; }
                }
                uf[c] = (unsigned short)c;
                inv[pos] = c;
                sel[pos] = best;
            }
            ninv += __popcll(bal);
        }
        __syncthreads();

        int status = 0, rounds = 0, maxb = 0, nj = 0;
#pragma clang loop unroll(disable)
        for (int round = 0; round < n && ninv > 0; ++round) {
            // ---- an invalid cluster without a bit to select: the syndrome is outside the column space
            bool none = false;
            for (int k = lane; k < ninv; k += LSD_NT) none |= sel[k] < 0;
            if (__ballot(none) != 0ull) { status = 2; break; }
            ++rounds;
            // ---- all selected bits join; a bit brings its checks, clusters that meet in a check merge (lower index wins)
            if (lane == 0) {
                int njl = nj;
                for (int k = 0; k < ninv; ++k) {
                    const int j = sel[k];
                    int e = inv[k];
                    while (uf[e] != e) e = uf[e];
                    const unsigned int bit = 1u << (j & 31);
                    if (!(taken[j >> 5] & bit)) {
                        taken[j >> 5] |= bit;
                        jb[njl++] = j;
                    }
                    for (int q = P.cp[j]; q < P.cp[j + 1]; ++q) {
                        const int c = P.cr[q];
                        if (uf[c] == LSD_NONE) { uf[c] = (unsigned short)e; continue; }
                        int r = c;
                        while (uf[r] != r) r = uf[r];
                        if (r == e) continue;
                        const int lo = min(r, e), hi = max(r, e);
                        uf[hi] = (unsigned short)lo;
                        e = lo;
                    }
                }
                sh[1] = njl;
            }
            __syncthreads();
            nj = sh[1];
            // ---- flatten: uf[c] = the cluster of c (a walk that meets a parent written meanwhile meets an ancestor)
            for (int c = lane; c < m; c += LSD_NT) {
                if (uf[c] == LSD_NONE) continue;
                int r = c;
                while (uf[r] != r) r = uf[r];
                uf[c] = (unsigned short)r;
            }
            __syncthreads();
            // ---- the clusters that changed: the roots of the invalid ones, each once (in place: slot nn <= the slot read)
            int nn = 0;
            for (int base = 0; base < ninv; base += LSD_NT) {
                const int k = base + lane;
                const bool has = k < ninv;
                const int r = has ? uf[inv[k]] : 0;
                __syncthreads();
                const int v = lrow[r];
                const bool fresh = has && !(v < nn && inv[v] == r);
                __syncthreads();
                if (fresh) lrow[r] = (unsigned short)(0x8000 | lane);
                __syncthreads();
                const bool win = fresh && lrow[r] == (unsigned short)(0x8000 | lane);
                const unsigned long long bal = __ballot(win);
                __syncthreads();
                if (win) {
                    const int idx = nn + lsd_lanes_below(bal, lane);
                    inv[idx] = r;
                    lrow[r] = (unsigned short)idx;
                }
                nn += __popcll(bal);
                __syncthreads();
            }
            // ---- every changed cluster: members, caps, elimination; an invalid one stays listed with its next selection
            int nkeep = 0;
            bool over = false;
#pragma clang loop unroll(disable)
            for (int k = 0; k < nn; ++k) {
                const int R = inv[k];
                __syncthreads();
                int nb = 0;
                for (int base = 0; base < nj; base += LSD_NT) {
                    const int t = base + lane;
                    const int j = t < nj ? jb[t] : 0;
                    const bool mine = t < nj && uf[P.cr[P.cp[j]]] == R;
                    const unsigned long long bal = __ballot(mine);
                    const int idx = nb + lsd_lanes_below(bal, lane);
                    if (mine && idx < LSD_MAXB) {
                        cb[idx] = (unsigned short)j;
                        ck[idx] = llr[j];
                    }
                    nb += __popcll(bal);
                }
                maxb = max(maxb, nb);
                if (nb > P.max_bits) { over = true; continue; }
                __syncthreads();
                for (int t = lane; t < nb; t += LSD_NT) {  // column order by counting the bits in front
                    const int j = cb[t];
                    const double l = ck[t];
                    int rk = 0;
                    for (int u = 0; u < nb; ++u) rk += (u != t && lsd_before(ck[u], cb[u], l, j, tie)) ? 1 : 0;
                    cbs[rk] = (unsigned short)j;
                }
                __syncthreads();
                // the checks of the cluster's bits, each once: a lane claims a check by writing its tag, the survivor lists it
                int ncc = 0;
                bool overc = false;
                for (int base = 0; base < nb && !overc; base += LSD_NT) {
                    const int t = base + lane;
                    const int j = t < nb ? cbs[t] : 0;
                    const int q0 = t < nb ? P.cp[j] : 0, deg = t < nb ? P.cp[j + 1] - q0 : 0;
                    for (int q = 0; __ballot(q < deg) != 0ull; ++q) {
                        const bool has = q < deg;
                        const int c = has ? P.cr[q0 + q] : 0;
                        const int v = lrow[c];
                        const bool fresh = has && !(v < min(ncc, LSD_MAXC) && cc[v] == c);
                        __syncthreads();
                        if (fresh) lrow[c] = (unsigned short)(0x8000 | lane);
                        __syncthreads();
                        const bool win = fresh && lrow[c] == (unsigned short)(0x8000 | lane);
                        const unsigned long long bal = __ballot(win);
                        __syncthreads();
                        const int idx = ncc + lsd_lanes_below(bal, lane);
                        if (win && idx < LSD_MAXC) {
                            cc[idx] = (unsigned short)c;
                            lrow[c] = (unsigned short)idx;
                        }
                        ncc += __popcll(bal);
                        __syncthreads();
                        if (ncc > P.max_checks) { overc = true; break; }
                    }
                }
                if (overc) { over = true; continue; }
                // ---- H[checks, bits in column order] | s[checks], a row per check
                for (int r = lane; r < ncc; r += LSD_NT) {
#pragma unroll
                    for (int w = 0; w < LSD_WPR; ++w) rows[r * LSD_WPR + w] = 0ull;
                    const int c = cc[r];
                    rsy[r] = (unsigned char)((syn[c >> 5] >> (c & 31)) & 1u);
                    used[r] = 0;
                }
                __syncthreads();
                for (int t = lane; t < nb; t += LSD_NT) {
                    const int j = cbs[t];
                    for (int q = P.cp[j]; q < P.cp[j + 1]; ++q)
                        atomicOr(reinterpret_cast<unsigned int*>(rows + lrow[P.cr[q]] * LSD_WPR) + (t >> 5), 1u << (t & 31));
                }
                __syncthreads();
                // ---- Gauss-Jordan over the columns in order: the first free row with the column's bit is its pivot
                const int rpl = (ncc + LSD_NT - 1) / LSD_NT;
#pragma clang loop unroll(disable)
                for (int p = 0; p < nb; ++p) {
                    const int w = p >> 6, sft = p & 63;
                    int piv = -1;
                    for (int i = 0; i < rpl; ++i) {
                        const int r = i * LSD_NT + lane;
                        const bool h = r < ncc && !used[r] && ((rows[r * LSD_WPR + w] >> sft) & 1ull);
                        const unsigned long long bal = __ballot(h);
                        if (bal) { piv = i * LSD_NT + __ffsll((long long)bal) - 1; break; }
                    }
                    if (piv < 0) continue;
                    unsigned long long pr[LSD_WPR];
#pragma unroll
                    for (int x = 0; x < LSD_WPR; ++x) pr[x] = rows[piv * LSD_WPR + x];
                    const unsigned char ps = rsy[piv];
                    for (int i = 0; i < rpl; ++i) {
                        const int r = i * LSD_NT + lane;
                        if (r < ncc && r != piv && ((rows[r * LSD_WPR + w] >> sft) & 1ull)) {
#pragma unroll
                            for (int x = 0; x < LSD_WPR; ++x) rows[r * LSD_WPR + x] ^= pr[x];
                            rsy[r] ^= ps;
                        }
                    }
                    if (lane == 0) {
                        used[piv] = 1;
                        pivcol[piv] = (unsigned short)p;
                    }
                    __syncthreads();
                }
                bool bad = false;
                for (int r = lane; r < ncc; r += LSD_NT) bad |= !used[r] && rsy[r];
                const bool valid = __ballot(bad) == 0ull;
                bool keep = !valid;
                int nfree = 0;
                if (valid) {  // the solution on the greedy column basis replaces whatever its bits held
                    for (int t = lane; t < nb; t += LSD_NT) atomicAnd(&xsol[cbs[t] >> 5], ~(1u << (cbs[t] & 31)));
                    __syncthreads();
                    for (int r = lane; r < ncc; r += LSD_NT)
                        if (used[r] && rsy[r]) {
                            const int j = cbs[pivcol[r]];
                            atomicOr(&xsol[j >> 5], 1u << (j & 31));
                        }
                    if constexpr (HO) {  // free = bits - pivots; short of free columns and below the growth limit: unfinished
                        int npiv = 0;
                        for (int base = 0; base < ncc; base += LSD_NT) npiv += __popcll(__ballot(base + lane < ncc && used[base + lane]));
                        nfree = nb - npiv;
                        keep = nfree < P.min_free && nb < P.grow_limit;
                    }
                }
                if (keep) {  // the first free bit in column order next to one of its checks
                    int best = -1;
                    double bl = 0.0;
                    for (int r = lane; r < ncc; r += LSD_NT) {
                        const int c = cc[r];
                        for (int e = P.rp[c]; e < P.rp[c + 1]; ++e) {
                            const int j = P.ci[e];
                            if ((taken[j >> 5] >> (j & 31)) & 1u) continue;
                            const double l = llr[j];
                            if (best < 0 || lsd_before(l, j, bl, best, tie)) { best = j; bl = l; }
                        }
                    }
                    best = lsd_wave_first(bl, best, tie);
                    if constexpr (HO) keep = !valid || best >= 0;  // a valid cluster with nothing to select is finished
                    if (keep) {
                        if (lane == 0) {
                            inv[nkeep] = R;
                            sel[nkeep] = best;
                        }
                        ++nkeep;
                    }
                }
                if constexpr (HO) {
                    if (!keep) {  // finished: the sweep over its reduced rows
                        __syncthreads();
                        for (int t = lane; t < nb; t += LSD_NT) prow[t] = LSD_NONE;
                        __syncthreads();
                        for (int r = lane; r < ncc; r += LSD_NT)
                            if (used[r]) prow[pivcol[r]] = (unsigned short)r;
                        __syncthreads();
                        int kp = 0;
                        for (int base = 0; base < nb; base += LSD_NT) {
                            const int t = base + lane;
                            const bool f = t < nb && prow[t] == LSD_NONE;
                            const unsigned long long bal = __ballot(f);
                            if (f) fcol[kp + lsd_lanes_below(bal, lane)] = (unsigned short)t;
                            kp += __popcll(bal);
                        }
                        if (lane == 0) cfree[R] = kp;
                        int bc = -1;
                        const int w = min(P.order, kp);
                        if (P.method != 0 && kp > 0) {
                            for (int t = lane; t < nb; t += LSD_NT) {  // ascending bit index by counting; the costs by column position
                                const int j = cbs[t];
                                int rk = 0;
                                for (int u = 0; u < nb; ++u) rk += cbs[u] < j ? 1 : 0;
                                perm[rk] = (unsigned short)t;
                                double cj = 1.0;
                                if (P.cost) {
                                    cj = P.cost[j];
                                    if (P.cost_rows) cj = P.cost_rows[(size_t)s * n + j];
                                    else if (P.sel && P.sel[(size_t)s * n + j] != 0) cj = P.cost_alt[j];
                                }
                                ck[t] = cj;
                            }
                            __syncthreads();
                            const int ncand = P.method == 1 ? kp + w * (w - 1) / 2 : (1 << w) - 1;
                            double bw = 0.0;
#pragma clang loop unroll(disable)
                            for (int base = -LSD_NT; base < ncand; base += LSD_NT) {  // (the first pass weighs the baseline, candidate -1)
                                const int c = base < 0 ? -1 : base + lane;
                                unsigned long long F[LSD_WPR];
                                lsd_candidate(c < ncand ? c : -1, P.method, w, kp, P.e_msb_first, fcol, F);
                                double wgt = 0.0;
#pragma clang loop unroll(disable)
                                for (int i = 0; i < nb; ++i) {
                                    const int p = perm[i];
                                    if (lsd_candidate_bit(p, prow, rows, rsy, F)) wgt += ck[p];
                                }
                                if (base < 0) bw = wgt;
                                else if (c < ncand && wgt < bw) { bw = wgt; bc = c; }
                            }
#pragma unroll
                            for (int off = 32; off > 0; off >>= 1) {  // the lightest; ties to the lower candidate index
                                const double ow = __shfl_xor(bw, off);
                                const int oc = __shfl_xor(bc, off);
                                if (ow < bw || (ow == bw && oc < bc)) { bw = ow; bc = oc; }
                            }
                        }
                        for (int t = lane; t < nb; t += LSD_NT) atomicAnd(&xw[cbs[t] >> 5], ~(1u << (cbs[t] & 31)));
                        __syncthreads();
                        unsigned long long F[LSD_WPR];
                        lsd_candidate(bc, P.method, w, kp, P.e_msb_first, fcol, F);
                        for (int t = lane; t < nb; t += LSD_NT)
                            if (lsd_candidate_bit(t, prow, rows, rsy, F)) atomicOr(&xw[cbs[t] >> 5], 1u << (cbs[t] & 31));
                    }
                }
                __syncthreads();
            }
            ninv = nkeep;
            __syncthreads();
            if (over) { status = 1; break; }
        }
        if (status == 0 && ninv > 0) status = 2;  // (not reached: every round joins a bit)

        int ncl = 0;
        for (int base = 0; base < m; base += LSD_NT) {
            const int c = base + lane;
            ncl += __popcll(__ballot(c < m && uf[c] == (unsigned short)c));
        }
        // ---- results
        const bool solved = status == 0;
        if constexpr (HO) {
            __syncthreads();
            int maxf = 0;
            bool diff = false;
            if (solved) {
                for (int c = lane; c < m; c += LSD_NT)
                    if (uf[c] == (unsigned short)c) maxf = max(maxf, cfree[c]);
                for (int w = lane; w < 2 * wpn; w += LSD_NT) diff |= xw[w] != xsol[w];
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) maxf = max(maxf, __shfl_xor(maxf, off));
            const bool any_diff = __ballot(diff) != 0ull;
            if (lane == 0) {
                P.st_maxfree[s] = maxf;
                P.st_improved[s] = any_diff ? 1 : 0;
            }
        }
        if (lane == 0) {
            P.st_status[s] = status;
            P.st_rounds[s] = rounds;
            P.st_clusters[s] = ncl;
            P.st_maxbits[s] = maxb;
            if (!solved && P.osd_follows) {
                const int k2 = atomicAdd(&P.lsd_counters[1], 1);
                P.list2[k2] = (int)s;
                sh[2] = k2;
            }
        }
        __syncthreads();
        if (!solved && P.osd_follows) {  // the OSD kernels index their LLR rows by the slot of the list they walk
            double* __restrict__ dst = P.llr_ws2 + (size_t)sh[2] * n;
            for (int i = lane; i < n; i += LSD_NT) dst[i] = llr[i];
        } else {
            if (!solved) {  // no OSD stage: BP's decisions
                for (int w = lane; w < 2 * wpn; w += LSD_NT) {
                    unsigned int v = 0u;
                    for (int b = 0; b < 32 && 32 * w + b < n; ++b) v |= (llr[32 * w + b] <= 0.0 ? 1u : 0u) << b;
                    xsol[w] = v;
                    if constexpr (HO) xw[w] = v;
                }
                __syncthreads();
            }
            uint8_t* const outs[4] = {P.out_osdw, P.out_osd0, P.cmp_osdw, P.cmp_osd0};
            for (int o = 0; o < 4; ++o) {
                if (!outs[o]) continue;
                const size_t row = o < 2 ? (size_t)s : (size_t)slot;
                const unsigned int* const src = (HO && (o & 1) == 0) ? xw : xsol;  // (HO) osdw: the sweep's rows
                if (P.packed_io) {
                    for (int w = lane; w < wpn; w += LSD_NT)
                        ((unsigned long long*)outs[o])[row * wpn + w] = (unsigned long long)src[2 * w] | ((unsigned long long)src[2 * w + 1] << 32);
                } else {
                    for (int i = lane; i < n; i += LSD_NT) outs[o][row * n + i] = (uint8_t)((src[i >> 5] >> (i & 31)) & 1u);
                }
            }
        }
        __syncthreads();
    }
}

// The rows of the shots OSD rewrote, again at their slot of the BP stage's list (host-pointer calls patch the caller's
// arrays from these compact copies): one workgroup per listed shot that lsd_kernel did not solve.
__global__ __launch_bounds__(256) void lsd_compact_kernel(const int* __restrict__ list, const int* __restrict__ counters,
                                                          const int* __restrict__ status, size_t row_bytes,
                                                          const uint8_t* __restrict__ out_osdw, const uint8_t* __restrict__ out_osd0,
                                                          uint8_t* __restrict__ cmp_osdw, uint8_t* __restrict__ cmp_osd0) {
    const int nlist = counters[1];
    for (int k = blockIdx.x; k < nlist; k += gridDim.x) {
        const size_t s = (size_t)list[k];
        if (status[s] == 0) continue;
        for (size_t i = threadIdx.x; i < row_bytes; i += blockDim.x) {
            if (cmp_osdw) cmp_osdw[(size_t)k * row_bytes + i] = out_osdw[s * row_bytes + i];
            if (cmp_osd0) cmp_osd0[(size_t)k * row_bytes + i] = out_osd0[s * row_bytes + i];
        }
    }
}

}  // namespace bposd
