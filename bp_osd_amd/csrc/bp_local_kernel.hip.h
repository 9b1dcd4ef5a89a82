// bp_local_kernel.hip.h -- min-sum BP for (3,6)-regular codes with one third of the messages kept in registers.
//
// bp_kernel.hip.h moves every message through LDS twice per iteration (check -> bit, bit -> check) and is
// bound by LDS bandwidth (ds_write_b64 6.1 cycles, ds_read_b64 2.95 cycles per wave -- tools/microbench).
// For a code with check degree 6, bit degree 3 and n = 2m the host finds an assignment "every check OWNS two
// of its six neighbouring bits, every bit is owned by exactly one check" (a perfect b-matching; it exists for
// every (3,6)-biregular graph).  The thread that runs a check also runs its two owned bits, so the message on
// the edge (check, owned bit) never leaves that thread's registers: 2 of a check's 6 edges and 1 of a bit's 3
// edges are LOCAL; LDS carries 4m instead of 6m messages (32 instead of 48 bytes per check and direction).
//
// Exactness.  The min-sum check update is order-independent (exact minima of the other five magnitudes, sign
// parity), so a check may list its two local edges last.  The bit update is NOT (fp64 sums: prefix from the
// top of the column including the prior, suffix from the bottom -- SURVEY.md Appendix A.3), so the local
// message has to enter the sums at the position dl in {0,1,2} its check has among the bit's three checks in
// ascending order.  The host therefore sorts checks into 64-position groups (a wave = one group per owned
// check) whose slot-b bits share one dl wherever it can.  The code is wave-uniform and never changes (0, 1, 2:
// straight-line code, instruction for instruction the arithmetic of bp_kernel; 3: a mixed group, the operands are
// routed by per-lane selects), so it is decided once, outside the iteration loop: the loop exists as one body per
// key of a group's two codes (local_keys.h), the host puts groups of equal key into the same wave, and a wave whose
// groups differ runs a generic body with one switch per group -- except the wave (uniform key PAIRKEY, mixed group) of an
// instance compiled with that PAIRKEY, which has a straight-line body of its own (the host launches the instance its
// layout's wave table asks for).  The position count MP is a compile-time power of two, as in bp_kernel, so LDS offsets
// are instruction immediates.
//
// Everything else -- persistent workgroups on an atomic queue, in-place messages, incremental convergence
// bitmap, outputs, OSD hand-off -- is the scheme of bp_kernel.hip.h (rows a3-a7), except the convergence test itself:
// bp_kernel's waves each look at their own bitmap words and agree through flag words and a barrier (which makes its
// check pass speculative); here every wave reads the WHOLE bitmap (MP/64 b64 words, one per lane, one ds_read_b64) at
// the top of an iteration and decides for itself -- no flag word, no aggregation, no check pass whose result is dropped.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bp_kernel.hip.h"
#include "local_keys.h"
#include "local_park.h"

namespace bposd {

struct BpLocalParams {
    int m, n;
    long long B;
    int max_iter;
    double ms_scaling;
    int osd_enabled;
    int mp;                               // positions = blockDim.x * CPT (multiple of 64)
    const uint8_t* __restrict__ synd;     // [B, m]
    const double* __restrict__ llr0;      // [n]
    const uint8_t* __restrict__ sel;      // [B, n] nullable
    const double* __restrict__ llr0_alt;  // [n]
    const int* __restrict__ pos_chk;      // [mp]      check at position p, -1 = padding
    const int* __restrict__ pos_bit;      // [2 * mp]  entry b*mp + p: b-th owned bit of position p, -1 = padding
    const int* __restrict__ pos_alo;      // [2 * mp]  LDS slot (k * mp + p') of the bit's edge to the check after its owner (cyclically)
    const int* __restrict__ pos_ahi;      // [2 * mp]  ... to the check after that one
    const int* __restrict__ pos_dl;       // [2 * mp]  position dl of the owner among the bit's three checks
    const int* __restrict__ grp_dl;       // [2 * mp / 64]  entry b*(mp/64) + g: dl if the whole group shares it, else 3
    uint8_t* __restrict__ out_bp;
    uint8_t* __restrict__ out_osd0;
    uint8_t* __restrict__ out_osdw;
    uint8_t* __restrict__ out_conv;
    int* __restrict__ out_iters;
    double* __restrict__ out_llr;
    double* __restrict__ llr_ws;
    double* __restrict__ llr_tmp;          // [gridDim.x][n] LLRs of the syndrome a workgroup is on, written only when they
                                           // will be read: in the last iteration, or every iteration if out_llr is set
    int* __restrict__ osd_list;
    int* __restrict__ counters;
    unsigned long long* __restrict__ iter_total;
    int* __restrict__ tail_flag;  // nullable, host-visible: set to 1 by the workgroup that finds the queue empty (the tail begins)
    int packed_io;  // 1: packed syndromes in, packed result rows out (bp_kernel.hip.h: BpParams::packed_io)
    const double* __restrict__ llr0_rows;  // [B, n] nullable: this shot's own priors (wins over sel); behind the others, so that none of them moves
    // park at drain (local_park.h): the first launch of a call parks unfinished shots once its queue is dry, the second
    // launch (resume = 1, park_on_dry = 0) takes the records from a queue of their own and finishes them
    unsigned char* __restrict__ park;  // [gridDim.x] records of bposd_local_park::layout(mp).bytes; null unless a launch parks or resumes
    int park_on_dry;                   // bposd_local_park::Mode
    int resume;
};

__host__ __device__ inline size_t bp_local_lds_bytes(int mp) {
    // 4 LDS edges per position (+ dummy slot) + mismatch bitmap + control words
    return ((size_t)4 * mp + 2) * 8 + (size_t)(mp / 32 + 2) * 4 + 8 * 4;
}

// A bit's three checks in ascending index order have ranks 0, 1, 2; its owner has rank DL.  X is the message of the
// check that follows the owner cyclically (rank DL+1 mod 3), Y the one after (rank DL+2 mod 3): the roles are tied to
// the owner, not to the index order, which keeps the LDS access pattern of structured codes regular across the
// wrap-around of their circulants.  The sums run in rank order.
// The reference starts the suffix sums at 0.0 ("temp = 0; b2c += temp; temp += c2b", bottom edge first).  Two of its
// additions are identities and are not executed here: pre2 + 0.0 (== pre2 unless pre2 is -0.0) and 0.0 + c2 (== c2
// unless c2 is -0.0, in which case the +0.0 it would give differs from c2 only in the sign of a zero that is then added
// to pre1 / to c1 + pre0).  A prefix is -0.0 only if the prior is, and a prior log((1 - p) / p) never is (log(1) = +0.0);
// with non-negative-zero prefixes x + (+0.0) == x + (-0.0) bit for bit.  tests/test_gpu_parity.py compares LLR bits.
template <int DL>
__device__ __forceinline__ void bit_update(double l0, double R, double X, double Y, double& llr, double& oR, double& oX,
                                           double& oY) {
    const double c0 = DL == 0 ? R : (DL == 1 ? Y : X);
    const double c1 = DL == 0 ? X : (DL == 1 ? R : Y);
    const double c2 = DL == 0 ? Y : (DL == 1 ? X : R);
    const double pre0 = l0;  // prefix from the top of the column (prior included)
    const double pre1 = pre0 + c0;
    const double pre2 = pre1 + c1;
    llr = pre2 + c2;
    const double o2 = pre2;            // + suffix 0.0
    const double o1 = pre1 + c2;       // + suffix (0.0 + c2)
    const double o0 = pre0 + (c2 + c1);
    oR = DL == 0 ? o0 : (DL == 1 ? o1 : o2);
    oX = DL == 0 ? o1 : (DL == 1 ? o2 : o0);
    oY = DL == 0 ? o2 : (DL == 1 ? o0 : o1);
}

// mixed group: the same sums with the operands routed per lane
__device__ __forceinline__ void bit_update_mixed(int dlv, double l0, double R, double X, double Y, double& llr, double& oR,
                                                 double& oX, double& oY) {
    const bool d0 = dlv == 0, d1 = dlv == 1;
    const double c0 = d0 ? R : (d1 ? Y : X);
    const double c1 = d0 ? X : (d1 ? R : Y);
    const double c2 = d0 ? Y : (d1 ? X : R);
    const double pre0 = l0;
    const double pre1 = pre0 + c0;
    const double pre2 = pre1 + c1;
    llr = pre2 + c2;
    const double o2 = pre2;
    const double o1 = pre1 + c2;
    const double o0 = pre0 + (c2 + c1);
    oR = d0 ? o0 : (d1 ? o1 : o2);
    oX = d0 ? o1 : (d1 ? o2 : o0);
    oY = d0 ? o2 : (d1 ? o0 : o1);
}

// table entry at a uniform base + per-lane byte offset; the offset is made opaque at the point of use so that the
// address is formed there (hoisted out of the syndrome loop it would occupy a 64-bit register pair per table row)
__device__ __forceinline__ int bpl_table_load(const int* base, unsigned int lane_off, unsigned int const_off) {
    asm volatile("" : "+v"(lane_off));
    return *(const int*)((const char*)base + (lane_off + const_off));
}

// Kernel arguments that are read once per syndrome or less often (tables, output pointers, the queue) are fetched from the
// kernarg segment where they are used -- s_load from the scalar cache -- instead of being held in ~50 SGPRs for the
// lifetime of the kernel: the 64-VGPR build had run out of SGPRs and of lanes in its SGPR-spill register.
// CONTRACT: bp_local_kernel takes exactly ONE explicit argument, the BpLocalParams struct BY VALUE -- it then sits at offset 0 of the
// kernarg segment and bpl_args() may read it there.  A second kernel parameter, or the struct passed by pointer, would make these
// reads return garbage without a diagnostic; a -DBPOSD_DEBUG build traps on the first workgroup if the two views disagree.
static_assert(__is_trivially_copyable(BpLocalParams) && alignof(BpLocalParams) <= 8, "BpLocalParams is copied into the kernarg segment as it is");
typedef const __attribute__((address_space(4))) BpLocalParams* bpl_args_ptr;
__device__ __forceinline__ bpl_args_ptr bpl_args() {
    bpl_args_ptr a = (bpl_args_ptr)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(a));
    return a;
}

template <int V>
struct bpl_int {
    static constexpr int value = V;
};

// the instances launch_bp_local.hip selects without a variant being asked for (and their packed-I/O forms)
__host__ __device__ constexpr bool bpl_specialised(int cpt, int mpt, int minw, bool early) {
    return !early && ((cpt == 1 && mpt == 1024 && minw == 8) || (cpt == 2 && mpt == 1024 && (minw == 8 || minw == 6)) || (cpt == 2 && mpt == 2048 && minw == 4));
}

// CPT: checks per thread (each with its two owned bits); MPT: positions (power of two) = blockDim.x * CPT;
// EARLY: the check pass requests the LDS messages of all its checks before it computes the first one (the LDS accesses
// are volatile, i.e. issued in program order: without this the read latency is exposed once per check)
// UPRIOR: every bit has the same prior (uniform channel, no per-shot channel): it lives in a scalar register pair
// PACKED: the packed-I/O form (BpLocalParams::packed_io) as a compile-time switch: the byte form is then instruction for
// instruction what it was before the packed form existed (as a run-time switch it cost the headline launch 1.2 %, same-box A/B)
// PAIRKEY: -1, or the uniform key k of the one (k, mixed) wave this instance has a loop body for (local_keys.h: pair keys).
// The host picks the instance from the layout's wave table; any other wave of unequal groups runs the generic body.
template <int CPT, int MPT, int MINW, bool EARLY, bool UPRIOR, bool PACKED = false, int PAIRKEY = -1, bool RESUME = false>
__global__ __launch_bounds__(MPT / CPT, MINW) void bp_local_kernel(const BpLocalParams P) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    // (m and n are read where they are used, like the other per-syndrome arguments: held next to B as one four-dword load,
    // the register allocation left a dead 16-byte spill slot behind -- a private segment -- first in the PAIRKEY instances'
    // byte form, then in the plain headline instance as well)
    const int m = bpl_args()->m, n = bpl_args()->n;
#ifdef BPOSD_DEBUG
    if (blockIdx.x == 0 && threadIdx.x == 0 && (bpl_args()->m != P.m || bpl_args()->counters != P.counters)) __builtin_trap();
#endif
    constexpr int NT = MPT / CPT;
    constexpr int MP = MPT;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    constexpr int NB = 2 * CPT;  // owned bits per thread

    double* msg_plain = reinterpret_cast<double*>(smem);
    msg_ptr msg = (msg_ptr)msg_plain;
    unsigned int* diffw = reinterpret_cast<unsigned int*>(msg_plain + (size_t)4 * MP + 2);
    int* sh = reinterpret_cast<int*>(diffw + (MP / 32 + 2));  // control words: [0], [1] the park words (by chunk parity), [2] the queue ticket, [3] the OSD / park slot
    const unsigned int diffw_base = (unsigned int)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)diffw;

    // ---- per-thread graph tables
    // Padding positions (no check, no bits) need no predicate anywhere in the iteration loop: the host wires the two
    // "bits" of a padding position to that position's own four LDS slots, i.e. a closed toy graph of one check and two
    // bits, three edges each, with a zero syndrome bit and a positive prior.  All its messages stay positive for ever
    // (they grow; sums of positive numbers never produce a NaN), its bits never change their decision and its check
    // never mismatches.  Only the stores that leave the workgroup (LLRs, results) test pos_bit >= 0.
    // alo / ahi: LDS BYTE addresses of the two non-local edges of an owned bit (one register each for the hot path AND
    // the rare decision-flip path, which recovers the position from the address; a slot index kept next to its byte
    // address cost the default build 84 B/lane of scratch and a scratch reload on the loop's critical path)
    typedef __attribute__((address_space(3))) unsigned char* lds_bytes;
    const unsigned int msg_base = (unsigned int)(uintptr_t)(lds_bytes)smem;
    unsigned int alo[NB], ahi[NB];
    int dl[NB];                // the groups' dl codes: they only form the keys below, none is live in the iteration loop
    unsigned int dlpack = 0u;  // 2 bits per owned bit: its dl (needed per lane only in mixed groups)
    double l0[UPRIOR ? 1 : NB];
    if (UPRIOR) {  // into a scalar register pair
        const double v = bpl_args()->llr0[0];
        l0[0] = __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)), __builtin_amdgcn_readfirstlane(__double2loint(v)));
    }
#define BPL_L0(r) l0[UPRIOR ? 0 : (r)]
#define BPL_AT(a) ((msg_ptr)(uintptr_t)(a))
    // r-th owned bit of this thread (-1 = padding): a uniform base plus a 32-bit byte offset per lane, so the loads outside
    // the iteration loop need no 64-bit per-lane pointers (which the 64-VGPR build kept in scratch)
#define BPL_BIT(r) bpl_table_load(bpl_args()->pos_bit, (unsigned int)tid * 4u, (unsigned int)((((r) & 1) * MP + ((r) >> 1) * NT) * 4))
#pragma unroll
    for (int j = 0; j < CPT; ++j) {
        const int p = tid + j * NT;
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int r = 2 * j + b;
            if (!UPRIOR) {
                const int bit = BPL_BIT(r);
                l0[r] = bit >= 0 ? bpl_args()->llr0[bit] : 1.0;  // (UPRIOR: the host has checked that the prior is > 0)
            }
            alo[r] = msg_base + 8u * (unsigned int)bpl_args()->pos_alo[b * MP + p];
            ahi[r] = msg_base + 8u * (unsigned int)bpl_args()->pos_ahi[b * MP + p];
            dl[r] = __builtin_amdgcn_readfirstlane(bpl_args()->grp_dl[b * (MP >> 6) + (p >> 6)]);  // uniform per wave
            dlpack |= (unsigned int)bpl_args()->pos_dl[b * MP + p] << (2 * r);
        }
    }

    // key of each of the wave's groups, and of the wave: the groups' common key if they share one (the host pairs groups of
    // equal key into a wave: local_layout::pair_groups), else -1 = the generic body.  Constant for the kernel's lifetime.
    int gkey[CPT];
#pragma unroll
    for (int j = 0; j < CPT; ++j) gkey[j] = bposd_local_keys::group_key(dl[2 * j], dl[2 * j + 1]);
    int wkey = gkey[0];
#pragma unroll
    for (int j = 1; j < CPT; ++j) wkey = (gkey[j] == wkey) ? wkey : -1;
    constexpr int PKEY = bposd_local_keys::pair_key(PAIRKEY);  // -1: the instance has no pair body
    static_assert(PKEY < 0 || (CPT == 2 && bpl_specialised(CPT, MPT, MINW, EARLY)), "a pair body is for two groups per wave");
    if constexpr (PKEY >= 0) {
        if (gkey[0] == PAIRKEY && gkey[CPT - 1] == bposd_local_keys::kMixedKey) wkey = PKEY;
    }
    // instances that auto-selection takes get a loop body per key; the A/B variants run the generic body
    constexpr bool SPEC = bpl_specialised(CPT, MPT, MINW, EARLY);

    const int want_llr_s = __builtin_amdgcn_readfirstlane(bpl_args()->out_llr != nullptr ? 1 : 0);
    // tested from ONE scalar register wherever it is needed (as a loop-invariant condition it became a lane mask plus a
    // vector register that went to scratch)
    auto want_llr = [&]() -> bool {
        int w = want_llr_s;
        asm volatile("" : "+s"(w));
        return w != 0;
    };
    // The whole mismatch bitmap in one LDS read: lane l gets b64 word l mod MP/64 (the lanes past MP/64 read the same words
    // again -- a broadcast -- so no lane needs a mask or a select), and it is zero iff no lane holds a set bit.  Every wave
    // reads the same words after the same barrier, so every wave takes the same exit without further synchronisation.
    // The address is formed where it is used (no register live across the loop).
    static_assert(MP % 64 == 0 && MP / 64 <= 64 && ((MP / 64) & (MP / 64 - 1)) == 0, "one bitmap word per lane");
    auto bitmap_word = [&]() -> unsigned long long {
        unsigned int a = (unsigned int)tid;
        asm volatile("" : "+v"(a));
        return *(const volatile __attribute__((address_space(3))) unsigned long long*)(uintptr_t)(diffw_base + ((a & (unsigned int)(MP / 64 - 1)) << 3));
    };
    auto bitmap_is_zero = [&](unsigned long long w) -> bool {
        asm volatile("" : "+v"(w));  // (waited for here, behind whatever was issued after the read)
        return __ballot(w != 0ull) == 0ull;
    };
    // ---- park at drain (local_park.h)
    // The keyed, pair and generic loops run in chunks of CH iterations: iterate() returns at a chunk boundary and the
    // per-syndrome code below enters it again, or parks the shot.
    constexpr int CH = bposd_local_park::kChunk;
    constexpr bposd_local_park::Layout PARK = bposd_local_park::layout(MP);
    static_assert((4 * MP) % NT == 0 && NT <= MP && NT >= MP / 32 && NT >= 2, "the park record is copied in whole rounds of the workgroup");
    for (;;) {
        // both park words are cleared where the ticket is published (the barrier below is between this and their first read)
        if (tid == 0) {
            int t;
            if (RESUME) {
                // The continuation takes the records first (ticket >= 0; the first launch has ended: its record count is
                // final), then whatever the first launch left in the call's queue (ticket = -1 - shot): nothing where it
                // parked because the queue was dry, the rest of the batch where every workgroup was made to park before.
                t = atomicAdd(&bpl_args()->counters[bposd_local_park::kResumeHead], 1);
                if (t >= bpl_args()->counters[bposd_local_park::kParkCount]) t = -1 - atomicAdd(&bpl_args()->counters[0], 1);
            } else t = atomicAdd(&bpl_args()->counters[0], 1);
            sh[2] = t;
            int zero = 0;
            asm volatile("" : "+v"(zero));  // (made here: as a loop invariant the pair of zeros went to scratch)
            sh[0] = zero;
            sh[1] = zero;
        }
        __syncthreads();
        const int ticket = __builtin_amdgcn_readfirstlane(sh[2]);
        const unsigned char* rec = nullptr;  // the record this workgroup restores
        const bool resume = RESUME && ticket >= 0;
        long long s;
        if (resume) {
            rec = bpl_args()->park + (size_t)ticket * PARK.bytes;
            const long long sv = *(const long long*)(rec + PARK.shot);
            s = ((long long)__builtin_amdgcn_readfirstlane((int)(sv >> 32)) << 32) | (unsigned int)__builtin_amdgcn_readfirstlane((int)sv);
        } else {
            s = RESUME ? -1 - ticket : ticket;
            if (s >= P.B) {
                // the chunk loop of the host-pointer API launches the next chunk's kernels when this one's tail begins
                if (s == P.B && tid == 0 && bpl_args()->tail_flag) *(volatile int*)bpl_args()->tail_flag = 1;
                break;
            }
        }

        // ---- syndrome bits of my checks; the mismatch bitmap (indexed by position) starts as the syndrome
        bool sbit[CPT];
#pragma unroll
        for (int j = 0; j < CPT; ++j) {
            const int c = bpl_table_load(bpl_args()->pos_chk, (unsigned int)tid * 4u, (unsigned int)(j * NT * 4));
            sbit[j] = (c >= 0) ? (PACKED ? bp_synd_bit(bpl_args()->synd, 1, s, m, c) : ((bpl_args()->synd[(size_t)s * m + c] & 1) != 0)) : false;
            const unsigned long long bal = __ballot(sbit[j]);
            if (lane == 0 && !resume) {  // (a restored shot brings its bitmap)
                const int w0 = ((wave << 6) + j * NT) >> 5;
                diffw[w0] = (unsigned int)bal;
                diffw[w0 + 1] = (unsigned int)(bal >> 32);
            }
        }
        if (!UPRIOR && bpl_args()->llr0_rows) {  // a channel of its own for every shot: row s of the caller's priors
#pragma unroll
            for (int j = 0; j < CPT; ++j)
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    const int i = BPL_BIT(2 * j + b);
                    if (i >= 0) l0[2 * j + b] = bpl_args()->llr0_rows[(size_t)s * n + i];
                }
        } else if (!UPRIOR && bpl_args()->sel) {
#pragma unroll
            for (int j = 0; j < CPT; ++j)
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    const int i = BPL_BIT(2 * j + b);
                    if (i >= 0) l0[2 * j + b] = bpl_args()->sel[(size_t)s * n + i] ? bpl_args()->llr0_alt[i] : bpl_args()->llr0[i];
                }
        }
        // ---- a3: every edge's bit->check message starts at the prior (two in LDS, one in a register)
#define BPL_LLRT (bpl_args()->llr_tmp + (size_t)blockIdx.x * n)
        double loc[NB];
        unsigned int decmask = 0u;  // bit r: hard decision of my r-th bit
        int it_cur = 1;             // the iteration the shot goes on from
        if (!resume) {
#pragma unroll
            for (int r = 0; r < NB; ++r) {
                double lp = BPL_L0(r);
                if (UPRIOR) asm volatile("" : "+s"(lp));  // copied from the scalar pair here, not kept in a vector pair
                loc[r] = lp;
                *BPL_AT(alo[r]) = lp;
                *BPL_AT(ahi[r]) = lp;
            }
        } else {
            // ---- the shot as its record holds it: messages, bitmap, local messages, decisions, the iteration to go on from
            // (a uniform base plus a 32-bit byte offset per lane, formed here: see bpl_table_load; volatile, as the LDS side is:
            // one element in flight, not 4 * CPT register pairs)
            unsigned int t8 = (unsigned int)tid * 8u;
            asm volatile("" : "+v"(t8));
#pragma unroll
            for (int q = 0; q < 4 * MP / NT; ++q) msg[tid + q * NT] = *(const volatile double*)(rec + (t8 + (unsigned int)(PARK.msg + (size_t)q * NT * 8)));
            if (tid < 2) msg[4 * MP + tid] = *(const volatile double*)(rec + (t8 + (unsigned int)(PARK.msg + (size_t)4 * MP * 8)));
            if (tid < MP / 32) *(volatile __attribute__((address_space(3))) unsigned int*)(uintptr_t)(diffw_base + (t8 >> 1)) = *(const unsigned int*)(rec + ((t8 >> 1) + (unsigned int)PARK.bitmap));
#pragma unroll
            for (int r = 0; r < NB; ++r) loc[r] = *(const double*)(rec + (t8 + (unsigned int)(PARK.loc + (size_t)r * NT * 8)));
            decmask = *(const unsigned int*)(rec + ((t8 >> 1) + (unsigned int)PARK.dec));
            it_cur = __builtin_amdgcn_readfirstlane(*(const int*)(rec + PARK.iter));
        }
        if (want_llr()) {  // a syndrome that needs no iteration reports the priors
#pragma unroll
            for (int r = 0; r < NB; ++r) {
                const int i = BPL_BIT(r);
                double lp = BPL_L0(r);
                if (UPRIOR) asm volatile("" : "+s"(lp));
                if (i >= 0) BPL_LLRT[i] = lp;
            }
        }
        __syncthreads();

        int it_done = 0;
        // the zero syndrome (an int in one scalar register, not a lane mask); a restored shot is tested at the top of the
        // iteration it goes on from, as it would have been without the park
        int conv = (!resume && bitmap_is_zero(bitmap_word())) ? 1 : 0;
        // The iteration loop, as a body per (KEY, LLR).  KEY >= 0: every group of the wave has this key (local_keys.h) and the
        // bit pass is straight-line code (a pair key: group 0 has the uniform key, group 1 the mixed one); KEY < 0: the generic
        // body, one switch per group on its key.  LLR: the body that
        // stores the posterior LLRs (every iteration if out_llr is set, else the last one only); the body without them runs
        // one chunk, iterations it0 .. min(max_iter, it0 + CH) - 1, and holds no test of max_iter.  Returns 1 once conv /
        // it_done are final.
        // Convergence: the bitmap is final at the barrier that ends a bit pass, and the top of iteration `it` tests all of it
        // (bitmap_word): zero means the decisions of iteration it - 1 satisfy the syndrome.  The test is a ballot, so the exit
        // is a scalar branch, and it is the same in every wave.  Nobody writes the bitmap between that barrier and the next
        // barrier a wave that stays in the loop passes (the one after the check pass), and a wave that leaves passes the two
        // barriers of the result section before the next syndrome's bits are written: the slowest wave has read by then.
        auto iterate = [&](auto key_c, auto llr_c, const int it0) __attribute__((always_inline)) -> int {
            constexpr int KEY = decltype(key_c)::value;
            constexpr bool LLR = decltype(llr_c)::value;
            const int max_iter = bpl_args()->max_iter;  // (read here: hoisted out of the syndrome loop it and the tests on it occupy scalar registers)
            // the body without LLR stores runs one chunk: it returns 0 at the boundary it0 + CH, or at max_iter as before
            const int lim = (max_iter - it0 > CH) ? it0 + CH : max_iter;
#pragma clang loop unroll(disable)
            for (int it = it0; LLR || it < lim; ++it) {
                asm volatile("; bpl_body key=%0 llr=%1" ::"n"(KEY), "n"((int)LLR));  // names the loop in the ISA listing (tools/isa_loop_count.py)
                // the bitmap read, then the first check's message loads (all checks' if EARLY), then the test: its LDS round
                // trip overlaps the loads, which a converged syndrome discards (LDS accesses are volatile: issued in this order)
                const unsigned long long bw = bitmap_word();
                double vl[EARLY ? CPT : 1][4];
#pragma unroll
                for (int j = 0; j < (EARLY ? CPT : 1); ++j)
#pragma unroll
                    for (int k = 0; k < 4; ++k) vl[j][k] = msg[(tid + j * NT) + k * MP];
                if (bitmap_is_zero(bw)) {  // converged by the decisions of iteration it - 1
                    conv = 1;
                    it_done = it - 1;
                    return 1;
                }
                if (LLR && it > max_iter) {  // the test after the last bit pass has failed
                    it_done = max_iter;
                    return 1;
                }
                // =================== check -> bit pass (a4) ===========
                const unsigned long long alpha_u = alpha_bits_for_iteration(P.ms_scaling, it);  // scalar instructions
                const int alpha_lo = (int)(unsigned int)alpha_u, alpha_hi = (int)(unsigned int)(alpha_u >> 32), nalpha_hi = alpha_hi ^ (int)0x80000000;
#pragma unroll
                for (int j = 0; j < CPT; ++j) {
                    msg_ptr mc = msg + (tid + j * NT);
                    double v[6];
#pragma unroll
                    for (int k = 0; k < 4; ++k) v[k] = (EARLY || j == 0) ? vl[EARLY ? j : 0][k] : mc[k * MP];
                    v[4] = loc[2 * j];
                    v[5] = loc[2 * j + 1];
                    double pre[6], suf[6];
                    pre[0] = __DBL_MAX__;
#pragma unroll
                    for (int k = 1; k < 6; ++k) pre[k] = min_abs(pre[k - 1], v[k - 1]);
                    suf[5] = __DBL_MAX__;
#pragma unroll
                    for (int k = 4; k >= 0; --k) suf[k] = min_abs(suf[k + 1], v[k + 1]);
                    // signs: a message counts as negative when b2c <= 0 (a zero too, as in the reference); the outgoing
                    // message is mag * ((-1)^(syndrome + #negatives + own) * alpha).  The sign rides on the multiplier:
                    // one select of alpha's high word per edge (mag * (-alpha) == -(mag * alpha) bit for bit).
                    bool neg[6];
                    bool par = sbit[j];
#pragma unroll
                    for (int k = 0; k < 6; ++k) {
                        neg[k] = (v[k] <= 0.0);
                        par ^= neg[k];
                    }
#pragma unroll
                    for (int k = 0; k < 6; ++k) {
                        const double mag = (k == 0) ? suf[0] : (k == 5 ? pre[5] : min_pos(pre[k], suf[k]));
                        const double sa = __hiloint2double((par ^ neg[k]) ? nalpha_hi : alpha_hi, alpha_lo);
                        const double o = mag * sa;
                        if (k < 4) mc[k * MP] = o;
                        else loc[2 * j + (k - 4)] = o;
                    }
                }
                __syncthreads();
                // ============ bit pass: posterior, decision, bit -> check (a6 / a7) ============
                // the two LDS messages of every owned bit: all of them up front (latency hidden inside the thread), or,
                // for the register-capped high-occupancy variant, one group (two bits) at a time
#ifndef BPOSD_BPL_BATCH
#define BPOSD_BPL_BATCH 2
#endif
                constexpr int BATCH = (MINW >= 8 && NB > 2) ? BPOSD_BPL_BATCH : NB;
                static_assert(BATCH % 2 == 0 && NB % BATCH == 0, "the bit pass loads the messages of whole groups");
                double X[NB], Y[NB];
                // one owned bit with its dl (3: per lane) as a compile-time constant: sums, stores, decision update
                auto bit_step = [&](const int r, auto dl_c) __attribute__((always_inline)) {
                    constexpr int DL = decltype(dl_c)::value;
                    double oR, oX, oY, t;
                    if constexpr (DL == 3) bit_update_mixed((int)((dlpack >> (2 * r)) & 3u), BPL_L0(r), loc[r], X[r], Y[r], t, oR, oX, oY);
                    else bit_update<DL>(BPL_L0(r), loc[r], X[r], Y[r], t, oR, oX, oY);
                    if (LLR) {
                        const int bi = BPL_BIT(r);
                        if (bi >= 0) BPL_LLRT[bi] = t;
                    }
                    loc[r] = oR;
                    *BPL_AT(alo[r]) = oX;
                    *BPL_AT(ahi[r]) = oY;
                    const unsigned int dnew = (t <= 0.0) ? 1u : 0u;
                    if (dnew != ((decmask >> r) & 1u)) {  // (a padding bit never gets here: see the tables above)
                        decmask ^= 1u << r;
                        unsigned int pa = alo[r], pb = ahi[r];
                        asm volatile("" : "+v"(pa), "+v"(pb));  // keep the rare path's address arithmetic in the branch
                        const int ca = (int)((pa - msg_base) >> 3) & (MP - 1), cb = (int)((pb - msg_base) >> 3) & (MP - 1);
                        const int co = tid + (r >> 1) * NT;  // slot = k * MP + position
                        atomicXor(&diffw[ca >> 5], 1u << (ca & 31));
                        atomicXor(&diffw[cb >> 5], 1u << (cb & 31));
                        atomicXor(&diffw[co >> 5], 1u << (co & 31));
                    }
                };
                auto group_step = [&](const int j, auto gk_c) __attribute__((always_inline)) {
                    constexpr int GK = decltype(gk_c)::value;
                    bit_step(2 * j, bpl_int<bposd_local_keys::key_dl(GK, 0)>{});
                    bit_step(2 * j + 1, bpl_int<bposd_local_keys::key_dl(GK, 1)>{});
                };
#pragma unroll
                for (int j = 0; j < CPT; ++j) {
                    if ((2 * j) % BATCH == 0) {
#pragma unroll
                        for (int q = 2 * j; q < 2 * j + BATCH; ++q) {
                            X[q] = *BPL_AT(alo[q]);
                            Y[q] = *BPL_AT(ahi[q]);
                        }
                    }
                    if constexpr (KEY >= 0) {
                        if (j == 0) group_step(j, bpl_int<bposd_local_keys::body_group_key(KEY, 0)>{});
                        else group_step(j, bpl_int<bposd_local_keys::body_group_key(KEY, 1)>{});
                    } else {
                        switch (gkey[j]) {  // wave-uniform; both bits of the group inside one arm
                            case 0: group_step(j, bpl_int<0>{}); break;
                            case 1: group_step(j, bpl_int<1>{}); break;
                            case 2: group_step(j, bpl_int<2>{}); break;
                            case 5: group_step(j, bpl_int<5>{}); break;
                            case 6: group_step(j, bpl_int<6>{}); break;
                            case 10: group_step(j, bpl_int<10>{}); break;
                            default: group_step(j, bpl_int<bposd_local_keys::kMixedKey>{}); break;
                        }
                    }
                }
                __syncthreads();
            }
            return 0;
        };
        int done = 0;  // (an int in one scalar register, not a lane mask) 1: conv / it_done are final, 2: the shot parks
        if (!conv) {
            // the body is chosen here, once per syndrome, from a scalar register; every wave of the workgroup passes the same
            // barriers and leaves at the same iteration whichever body it runs
            int it_llr = 1;  // (out_llr set: every iteration stores LLRs, the LLR body runs from the start)
            if (!want_llr()) {
                int wk = wkey;
                asm volatile("" : "+s"(wk));
              for (;;) {  // one chunk per trip: the same switch, entered again at the boundary
                if constexpr (SPEC) {
                    switch (wk) {
                        case 0: done = iterate(bpl_int<0>{}, bpl_int<0>{}, it_cur); break;
                        case 1: done = iterate(bpl_int<1>{}, bpl_int<0>{}, it_cur); break;
                        case 2: done = iterate(bpl_int<2>{}, bpl_int<0>{}, it_cur); break;
                        case 5: done = iterate(bpl_int<5>{}, bpl_int<0>{}, it_cur); break;
                        case 6: done = iterate(bpl_int<6>{}, bpl_int<0>{}, it_cur); break;
                        case 10: done = iterate(bpl_int<10>{}, bpl_int<0>{}, it_cur); break;
                        case bposd_local_keys::kMixedKey: done = iterate(bpl_int<bposd_local_keys::kMixedKey>{}, bpl_int<0>{}, it_cur); break;
                        default:  // the instance's pair key, if it has one; else the generic body
                            if (PKEY >= 0 && wk == PKEY) done = iterate(bpl_int<(PKEY >= 0 ? PKEY : -1)>{}, bpl_int<0>{}, it_cur);
                            else done = iterate(bpl_int<-1>{}, bpl_int<0>{}, it_cur);
                            break;
                    }
                } else done = iterate(bpl_int<-1>{}, bpl_int<0>{}, it_cur);
                asm volatile("" : "+s"(done));
                it_llr = bpl_args()->max_iter;
                if (done || it_llr - it_cur < CH) break;  // finished, or what is left is the last iteration's (the LLR body's)
                // ---- a chunk boundary: the body has run iterations it_cur .. it_cur + CH - 1 and the shot is not finished
                it_cur += CH;
                const int pmode = bpl_args()->park_on_dry;
                if (pmode) {
                    // Why every wave takes the same exit.  The word read at the end of chunk c, sh[c & 1], was written at the end
                    // of chunk c - 1 (or cleared with the ticket), and every wave has passed the 2 * CH barriers of chunk c since;
                    // its next write comes at the end of chunk c + 1, behind the barriers of that chunk, which no wave passes
                    // before all have read here.  At least one barrier lies between a word's write and its read and between that
                    // read and its next write, so all waves read the same value -- with no barrier of the park's own and nobody
                    // waiting for anybody.  A shot parks at most two chunks after the queue ran dry.
                    // The queue head is loaded here, by thread 0, and not a chunk earlier: held across the chunk it is a 65th
                    // vector register (44 B/lane of scratch in the headline instance).  Wave 0 waits for the load once per CH
                    // iterations -- and only shots past iteration CH get here at all.
                    const int chunk = (it_cur - 1) / CH - 1;  // the chunk that has ended (a shot of a parking launch starts at iteration 1)
                    const int parkw = __builtin_amdgcn_readfirstlane(*(volatile int*)&sh[chunk & 1]);
                    if (tid == 0) sh[(chunk + 1) & 1] = (__hip_atomic_load(&bpl_args()->counters[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= P.B) ? 1 : 0;
                    if (parkw != 0 || pmode == bposd_local_park::kForce) {
                        done = 2;  // the record is written in front of the result section
                        break;
                    }
                }
              }
                it_llr = it_llr > 1 ? it_llr : 1;
            }
            if (!done) iterate(bpl_int<-1>{}, bpl_int<1>{}, it_llr);
        }

        // ---- results
        if (done == 2) {
            // ---- park: the shot's state goes into a record and the workgroup leaves (it draws no ticket again,
            // so a launch writes at most gridDim.x records).  Every wave is behind the barrier that ended the
            // chunk's last bit pass: messages and bitmap are final.
            if (tid == 0) sh[3] = atomicAdd(&bpl_args()->counters[bposd_local_park::kParkCount], 1);
            __syncthreads();
            unsigned char* prec = bpl_args()->park + (size_t)__builtin_amdgcn_readfirstlane(sh[3]) * PARK.bytes;
            // (a uniform base plus a 32-bit byte offset per lane, formed here: see bpl_table_load; volatile, as the
            // LDS side is: one element in flight, not 4 * CPT register pairs)
            unsigned int t8 = (unsigned int)tid * 8u;
            asm volatile("" : "+v"(t8));
#pragma unroll
            for (int q = 0; q < 4 * MP / NT; ++q) *(volatile double*)(prec + (t8 + (unsigned int)(PARK.msg + (size_t)q * NT * 8))) = msg[tid + q * NT];
            if (tid < 2) *(volatile double*)(prec + (t8 + (unsigned int)(PARK.msg + (size_t)4 * MP * 8))) = msg[4 * MP + tid];
            if (tid < MP / 32) *(unsigned int*)(prec + ((t8 >> 1) + (unsigned int)PARK.bitmap)) = *(const volatile __attribute__((address_space(3))) unsigned int*)(uintptr_t)(diffw_base + (t8 >> 1));
#pragma unroll
            for (int r = 0; r < NB; ++r) *(double*)(prec + (t8 + (unsigned int)(PARK.loc + (size_t)r * NT * 8))) = loc[r];
            *(unsigned int*)(prec + ((t8 >> 1) + (unsigned int)PARK.dec)) = decmask;
            if (tid == 0) {
                *(long long*)(prec + PARK.shot) = s;
                *(int*)(prec + PARK.iter) = it_cur;
            }
            return;
        }
        const bool to_osd = (!conv) && bpl_args()->osd_enabled;
        if (tid == 0) {
            if (to_osd) {
                const int slot = atomicAdd(&bpl_args()->counters[1], 1);
                bpl_args()->osd_list[slot] = (int)s;
                sh[3] = slot;
            }
            if (bpl_args()->out_conv) bpl_args()->out_conv[s] = conv ? 1 : 0;
            if (bpl_args()->out_iters) bpl_args()->out_iters[s] = it_done;
            if (it_done) atomicAdd(bpl_args()->iter_total, (unsigned long long)it_done);
        }
        __syncthreads();
        const int slot = to_osd ? sh[3] : 0;
        constexpr bool packed = PACKED;
        if (packed)  // result rows as 64-bit words through an LDS bitmap (the messages are dead)
            bp_store_packed_rows<NB>((unsigned int*)smem, tid, NT, n, s, to_osd, (unsigned long long*)bpl_args()->out_bp,
                                     (unsigned long long*)bpl_args()->out_osd0, (unsigned long long*)bpl_args()->out_osdw,
                                     [&](int r) { return BPL_BIT(r); }, [&](int r) { return ((decmask >> r) & 1u) != 0u; });
#pragma unroll
        for (int r = 0; r < NB; ++r) {
            const int i = BPL_BIT(r);
            if (i >= 0) {
                const size_t o = (size_t)s * n + i;
                const uint8_t b = (uint8_t)((decmask >> r) & 1u);
                if (!packed) {
                    if (bpl_args()->out_bp) bpl_args()->out_bp[o] = b;
                    if (!to_osd) {
                        bpl_args()->out_osdw[o] = b;
                        if (bpl_args()->out_osd0) bpl_args()->out_osd0[o] = b;
                    }
                }
                if (to_osd) bpl_args()->llr_ws[(size_t)slot * n + i] = BPL_LLRT[i];
                if (want_llr()) bpl_args()->out_llr[o] = BPL_LLRT[i];
            }
        }
        __syncthreads();
    }
}

#undef BPL_L0
#undef BPL_AT
#undef BPL_BIT
#undef BPL_LLRT

}  // namespace bposd
