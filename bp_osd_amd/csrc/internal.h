// internal.h -- host-side state shared by the translation units of libbposd_mi355x.so (not part of the C-ABI).
// bposd_capi.hip holds creation, the one BP + OSD launch pair every decode ends in (decode_device_impl) and the device-pointer
// calls, decode_host.hip the host-pointer calls with their chunk plan, host_tables.hip table construction and the layout
// searches; every launch_*.hip holds the instantiations and launch code of one kernel family, so that the families compile in
// parallel (bp_osd_amd/build.py).  The any-degree, serial and relay kernels (launch_bp_misc.hip, launch_bp_relay.hip) are three
// schedules on one core, bp_csr.hip.h: its parameter blocks, and the queue, sweep and results helpers.
// Every device block, page-locked block, stream and event below is held by an owning type of owned.h: deleting a handle frees
// all of it, and a resource added to Lane, CallRecord or bposd_handle needs no line anywhere else.
#pragma once
#include "../../include/bposd_mi355x.h"
#include "../../include/bposd_mi355x_debug.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "local_park.h"      // park at drain of the local-edge BP kernel: counter block, record layout, the rule
#include "bp_kernel.hip.h"   // BpParams, bp_lds_bytes (templates only: nothing is instantiated by including it)
#include "bp_csr.hip.h"      // BpShotIo, BpCsrGraph of the CSR-edge kernels (inlined helpers only)
#include "osd_kernel.hip.h"  // OsdParams
#include "owned.h"           // DeviceGuard, DevBuf, DevArray, PinnedBuf, Stream, Event

// Per-call state.  A handle owns BPOSD_LANES of these and alternates between them: consecutive decode calls (and the
// chunks of one host-pointer call) run on different HIP streams with their own workspaces, so the persistent
// workgroups of call k + 1 pick up the CUs that call k's last max_iter stragglers and its OSD kernel leave idle.
constexpr int BPOSD_LANES = 4;  // large codes (HBM-resident workspaces of several GB per lane) use two of them
constexpr int BPOSD_MAX_CHUNKS = 16;  // chunks of one host-pointer call (bposd_decode_batch)

struct Lane {
    Stream stream;
    // The OSD kernel of a call runs on a stream of its own at the highest priority (ordered behind the call's BP kernel
    // and in front of whatever follows on `stream` by events): its few, fat workgroups otherwise queue behind the full
    // grid of the NEXT call's BP kernel for every CU that frees up and take many times their own run time.
    Stream osd_stream;
    Event ev_bp, ev_osd;
    Event ev_park;  // park at drain: orders the continuation launch (on osd_stream) between the lane's two streams
    Event ev_done;  // both kernels of the lane's last (non-lean) call have ended
    bool done_recorded = false;
    PinnedBuf h_stage;  // page-locked, device-visible staging for small host-pointer calls (zero-copy path)
    Event ev_up;        // host-pointer calls: this lane's chunk has been uploaded (uploads go one at a time, in
                        // chunk order: the first chunk's kernels then start after one chunk's copy time)
    DevBuf bpl_msg, bpl_llr;  // large BP workspaces (bpl_llr also serves the local-edge kernel: LLRs of the current syndrome)
    DevBuf bpl_park;          // local-edge kernel, park at drain (local_park.h): one record per workgroup of the BP grid
    bool osd_recorded = false;  // ev_osd has been recorded at least once
    DevBuf osdl_ws;           // large OSD workspaces (matrix, sort keys, pivots, weights) carved from one allocation
    DevBuf osd_rows_ws;       // OSD kernel's per-workgroup spill area for finished row words
    DevBuf llr_ws, osd_list, io_synd, io_osdw, io_osd0, io_bp, io_conv, io_iters, io_llr, io_sel;
    // host-pointer calls with a channel row per shot (bposd_decode_batch_rows): the chunk's prior and weight rows, [chunk][n]
    // doubles each, and the page-locked block the host converts the caller's probabilities into before the upload
    DevBuf io_l0rows, io_costrows;
    PinnedBuf h_rows;
    // host-pointer calls: the outputs are downloaded on a copy stream of the lane's own right after the BP kernel (event-
    // ordered), the rows the OSD kernel rewrites come from compact copies [list slot][n] once it has run
    DevBuf io_cmp0, io_cmpw;
    // bit-packed host I/O (bposd_decode_batch_packed): packed syndromes in, packed rows out, packed compact OSD rows
    DevBuf io_psynd, io_posdw, io_posd0, io_pbp, io_pcmp;
    Stream copy_stream;
    Event ev_copy;                   // the chunk's downloads have left the lane's io buffers
    PinnedBuf h_list;                // page-locked copy of the chunk's OSD list (syndrome index per slot, ints)
    bool copy_pending = false;
    DevArray<long long> d_osd_dbg;   // diagnostics (BPOSD_OSD_DEBUG=1): phase timestamps
    DevArray<int> d_counters;        // 4 ints, the 64-bit iteration total (these 32 bytes go into the call record), and the park
                                     // words of the local-edge kernel behind them (local_park.h: kCounterBytes)
    // per-shot channel of a device-pointer call (bposd_decode_batch_select_device): priors and weights of the alternative
    // channel, 2n doubles, copied from a page-locked staging block on the lane's own stream -- consecutive select calls
    // overlap like plain ones (the first version drained every lane and made two blocking copies per call)
    DevArray<double> d_alt;
    PinnedBuf h_alt;
    Event ev_alt;                    // the staging block has been read
    bool alt_busy = false;
    PinnedBuf h_tail;                // one int, page-locked, device-visible: the BP kernel of this lane's current call has entered its tail
    // host-pointer observables calls (bposd_decode_batch_observables): the chunk's observable words, [chunk][ceil(k/64)] each
    DevBuf io_obsw, io_obs0, io_obsbp;
    // relay mode (bposd_set_relay): per-shot solutions (int), best leg (int) and weight (int64) of the lane's last call,
    // and that call's batch size; -1: the lane's last call did not run in relay mode (bposd_relay_stats)
    DevBuf relay_sol, relay_leg, relay_wt;
    long long relay_B = -1;
    // LSD mode (bposd_set_lsd): status | rounds | clusters | max_bits, [B] ints each, of the lane's last call and that call's
    // batch size (-1: the lane's last call had no LSD stage); the list of the shots lsd_kernel handed on with their LLR rows
    // [second-list slot][n]; the kernel's per-workgroup scratch; the second list's counters (lsd_kernel.hip.h)
    DevBuf lsd_stat, lsd_list2, lsd_llr2, lsd_ws;
    long long lsd_B = -1;
    int lsd_words = 4;  // words per shot of that call: 4 (lsd_kernel<false>) or 6 (lsd_kernel<true>: + max_free | improved)
    DevArray<int> d_lsd_counters;
};

// What bposd_last_timing reports: one record per kernel pair launched by the last call (one per chunk for a
// host-pointer call).  Events and the pinned counter copies live in the handle so that records outlive lane reuse.
struct CallRecord {
    Event ev[3];
    PinnedBuf h_counters;  // 4 ints, and behind them the 64-bit iteration total (the layout of Lane::d_counters)
    int* counters() const { return h_counters.as<int>(); }
    unsigned long long* iter_total() const { return (unsigned long long*)(counters() + 4); }
    bool ran_osd = false;
    bool recorded = false;  // the counters (and, when timed, the events) have been recorded at least once
    bool timed = false;     // the three events bracket the kernels of this record (not on the lean small-call path)
    Event ev_obs[2];        // an observables call: around obs_kernel, which runs behind ev[2] (bposd_debug_obs_timing)
    bool ran_obs = false;
};

struct bposd_handle {
    // lives where `new` put it: DecodeCall points into lanes[] and the record arrays
    bposd_handle() = default;
    bposd_handle(const bposd_handle&) = delete;
    bposd_handle& operator=(const bposd_handle&) = delete;
    bposd_config cfg{};
    int device = 0;
    Lane lanes[BPOSD_LANES];
    int nlanes = BPOSD_LANES; // lanes this handle cycles through
    int next_lane = 0;
    CallRecord lane_rec[BPOSD_LANES];  // device-pointer calls: the record of the last call queued on each lane
    CallRecord rec[BPOSD_MAX_CHUNKS];  // host-pointer calls: one record per chunk
    int nrec = 0;             // > 0: the last call was a host-pointer call of that many chunks
    int last_lane = 0;        // lane of the last device-pointer call
    int num_cu = 0;
    size_t lds_per_cu = 160 * 1024;
    int m = 0, n = 0, E = 0;
    int dc_max = 0, dv_max = 0;
    bool regular = false;
    // local-edge BP kernel (bp_local_kernel.hip.h): available for (3,6)-regular codes with n = 2m, min-sum
    bool local_ok = false;
    int local_mp = 0;
    long long local_passes = 0;  // modelled ds_read_b64 cycles of the bit pass in the chosen layout (floor: 4 * MP / 32)
    long long local_wcycles = 0; // modelled ds_write_b64 cycles of the bit pass (floor: 6 * 4 * MP / 64)
    DevArray<int> d_lpos_chk, d_lpos_bit, d_lpos_alo, d_lpos_ahi, d_lgrp_dl, d_lpos_dl;
    // class BP kernel (bp_class_kernel.hip.h): every check has the same degree, bit degrees inside one compiled range
    bool bp_any = false;  // degrees beyond the compiled kernels: bp_anydeg_kernel.hip.h (run-time degree loops, messages in HBM)
    bool class_ok = false;
    int class_dclo = 0, class_dc = 0, class_dvlo = 0, class_dvhi = 0, class_mp = 0, class_nt = 0;
    long class_read_cycles = 0, class_write_cycles = 0, class_read_floor = 0, class_write_floor = 0;  // modelled, one bit pass
    DevArray<int> d_cpos_chk, d_cpos_bit, d_cbit_slot, d_cgrp_deg, d_cgrp_cdeg;
    bool large = false;   // beyond the register-resident OSD kernel: HBM-resident matrix, device rank probe
    bool bp_hbm = false;  // BP messages do not fit one CU's LDS either: HBM-resident BP kernel
    int max_iter = 0;
    int rank = 0, kprime = 0, ncand = 0;
    bool probs_uniform = true;
    int bp_variant = 0;
    int last_bp_kernel = -1;  // BPOSD_BP_KERNEL_* of the last BP launch
    int osd_variant = 0;      // 0 auto, 1 = one workgroup per elimination (osd_kernel), 2 = one wave per elimination where it applies
    int last_osd_kernel = -1; // 0 none yet, 1 osd_kernel, 2 osd_wave_kernel, 3 osd_large_kernel
    int32_t last_bp_inst[6] = {-1, 0, 0, 0, 0, 0};   // bposd_debug_last_instance: the instance the last launch_* template launched
    int32_t last_osd_inst[6] = {-1, 0, 0, 0, 0, 0};
    int local_pair_key = -1;    // PAIRKEY of the bp_local_kernel instance this layout's (uniform, mixed) wave wants (local_layout::wave_plan), -1 none
    int last_bp_pair_key = -1;  // bposd_debug_last_pair_key: PAIRKEY of the last bp_local_kernel launch (-1: the plain instance)
    int park_mode = 0;          // bposd_debug_set_park: bposd_local_park::UserMode (BPOSD_PARK in the environment wins)
    // host copies
    std::vector<int> rp, ci;
    std::vector<double> probs;
    // device tables
    DevArray<int> d_rp, d_ci;
    DevArray<int> d_chk_deg, d_var_deg, d_var_pos, d_pos_bit, d_var_ck;
    int large_form = 0;  // form of the last bp_large_kernel launch: 0 per-edge messages (product-sum), 1 check records in the workspace, 2 per-check data in LDS
    int tab_np = 0;
    long layout_cost = 0, layout_cost_natural = 0, layout_cost_ideal = 0;  // simulated LDS cycles of the bit pass
    DevArray<double> d_llr0;
    DevArray<double> d_cost;  // log(1/p_i): OSD-W weights of the ldpc-v2 weight function
    DevArray<double> d_llr0_alt, d_cost_alt;  // alternative channel of the two-valued per-shot form
    bool fp_weights = false;   // non-uniform (or degenerate) channel: candidate weights need the fp64 sums
    // serial schedule (cfg.schedule == 1): CSC view and level lists
    DevArray<int> d_cp, d_ce, d_erow, d_lvl_ptr, d_lvl_bits;
    int nlevels = 0;
    int tab_dc = 0, tab_dv = 0, tab_mp = 0;  // layout the tables were built for
    bool have_timing = false;
    bool async_pending = false;        // a device-pointer call may still be running on some lane
    std::string err;
    // logical observables (bposd_set_observables): L transposed and packed, [ceil(n/64)][obs_k] words; obs_k = 0: none set
    DevArray<unsigned long long> d_obs_table;
    int obs_k = 0;
    // relay mode (bposd_set_relay): relay_legs = 0 is off; gammas [legs][n], iterations per leg [legs]
    int relay_legs = 0, relay_stop = 1, relay_init = 0;
    int relay_lane = 0;  // lane of the last relay launch (bposd_relay_stats with lane = -1)
    DevArray<double> d_relay_gammas;
    DevArray<int> d_relay_iters;
    // LSD mode (bposd_set_lsd): lsd_kernel between the BP and the OSD stage; H by column (build_tables_lsd)
    bool lsd_on = false;
    int lsd_max_bits = 0, lsd_max_checks = 0;
    // bposd_set_lsd_order: 0 lsd_0, 1 lsd_cs, 2 lsd_e; a sweep or growth for free bits selects lsd_kernel<true>
    int lsd_method = 0, lsd_order = 0, lsd_min_free = 0, lsd_grow_limit = 256;
    long long lsd_launches[2] = {0, 0};  // launches of lsd_kernel<false> / <true> (bposd_debug_lsd_launches)
    int lsd_lane = 0;  // lane of the last LSD launch (bposd_lsd_stats with lane = -1)
    DevArray<int> d_lsd_cp, d_lsd_cr;
};

// One BP + OSD launch pair: what it needs beyond the handle's per-code state.  The entry point that makes the call fills
// it in and every function below takes it by const reference; nothing per-call is kept in the handle.  Host state only:
// never a kernel argument.
struct DecodeCall {
    Lane* lane = nullptr;              // the lane the pair is enqueued on
    CallRecord* rec = nullptr;         // what bposd_last_timing reads back (null: the rank probe, which records nothing)
    hipStream_t osd_stream = nullptr;  // stream the OSD kernel goes to: the lane's osd_stream, its main stream for a lean call
    long long batch_hint = 0;          // > 0: a chunk of a host call of that many syndromes (kernel variants are chosen for the call)
    uint8_t *cmp_osd0 = nullptr, *cmp_osdw = nullptr;  // compact OSD rows of the chunk (host-pointer calls)
    bool bp_only = false;              // BP's outputs only (bposd_posterior_llr): no OSD kernel
    bool lane_alt = false;             // the alternative channel comes from the lane's buffers (bposd_decode_batch_select_device)
    bool packed = false;               // the kernels read packed syndromes and write packed result rows
    bool tail_gate = false;            // a chunk of a synchronous host-pointer call: its BP kernel reports its tail
    bool lean = false;                 // the small host-pointer call: one stream, no events (decode_device_impl)
    bool device_ptr = false;           // a device-pointer call (take_next_lane; the asynchronous host-pointer forms clear it)
};

namespace bposd_host {

int fail(bposd_handle* h, int code, const char* fmt, ...) __attribute__((format(printf, 3, 4)));

#define HIP_TRY(h, expr)                                                                       \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess)                                                                  \
            return bposd_host::fail(h, BPOSD_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), \
                                    __FILE__, __LINE__);                                       \
    } while (0)

// bposd_debug_last_instance: family code, the instance's template integers, packed-I/O flag
inline void note_instance(int32_t (&dst)[6], int family, int a, int b, int c, int d, bool packed) {
    const int32_t v[6] = {family, a, b, c, d, packed ? 1 : 0};
    std::copy(v, v + 6, dst);
}

// The shot-level fields of a BP launch, from the BpParams decode_device_impl fills into the parameter block of the kernel
// that runs: BpShotIo (bp_csr.hip.h) for the three CSR-edge kernels, BpClassParams, BpLargeParams.  By name: the tuned
// kernels' structs keep the field order they were measured with.  The one list of these fields on the host side.
template <class Dst>
inline void copy_shot_fields(Dst& d, const bposd::BpParams& P) {
    d.m = P.m; d.n = P.n; d.B = P.B; d.max_iter = P.max_iter; d.ms_scaling = P.ms_scaling; d.ps_clip = P.ps_clip;
    d.osd_enabled = P.osd_enabled; d.packed_io = P.packed_io;
    d.synd = P.synd; d.llr0 = P.llr0; d.sel = P.sel; d.llr0_alt = P.llr0_alt; d.llr0_rows = P.llr0_rows;
    d.out_bp = P.out_bp; d.out_osd0 = P.out_osd0; d.out_osdw = P.out_osdw; d.out_conv = P.out_conv; d.out_iters = P.out_iters;
    d.out_llr = P.out_llr; d.llr_ws = P.llr_ws; d.osd_list = P.osd_list; d.counters = P.counters; d.iter_total = P.iter_total;
    d.tail_flag = P.tail_flag;
}
inline bposd::BpCsrGraph csr_graph(const bposd_handle* h) { return bposd::BpCsrGraph{h->E, h->d_rp, h->d_ci, h->d_cp, h->d_ce}; }

int sync_all_lanes(bposd_handle* h);
int set_max_lds(bposd_handle* h, const void* kernel, size_t lds);
int cached_occupancy(bposd_handle* h, const void* kernel, int nt, size_t lds, int* out);
int ensure(bposd_handle* h, DevBuf& b, size_t bytes);
int ensure_lanes(bposd_handle* h, DevBuf Lane::*member, size_t bytes);
int grow_lanes(bposd_handle* h, DevBuf Lane::*member, size_t bytes, bool* drained);  // as ensure_lanes, draining the calls in flight first
int ensure_pinned(bposd_handle* h, PinnedBuf& b, size_t bytes, unsigned flags);  // as ensure(): freed, then allocated anew

// ---- table construction (host_tables.hip)
int upload_ints(bposd_handle* h, DevArray<int>& dst, const std::vector<int>& v);  // (a table that exists is freed first)
int build_tables(bposd_handle* h, int DC, int DV, int MP, int NT, int VPT);  // bp_kernel (rebuilt by launch_bp when the shape changes)
int build_tables_local(bposd_handle* h);  // sets local_ok
int build_tables_class(bposd_handle* h);  // sets class_ok
int build_tables_large(bposd_handle* h, int DV, int MP);
int build_tables_serial(bposd_handle* h);
int ensure_csc_tables(bposd_handle* h);  // d_cp / d_ce of the CSR-edge kernels, built (behind the calls in flight) if the handle has none
int build_tables_lsd(bposd_handle* h);  // d_lsd_cp, d_lsd_cr
struct DegPair { int dc, dv; };
bool pick_pair(int dc, int dv, DegPair* out);  // the compiled bp_kernel degree pair that covers (dc, dv)
int gf2_rank_host(int m, int n, const std::vector<int>& rp, const std::vector<int>& ci);
int upload_priors(bposd_handle* h);
int64_t first_bad_prob(const double* probs, int64_t count);  // index + 1 of the first value outside [0, 1] (NaN included), 0: none
int64_t channel_tables(const double* probs, int64_t count, double* prior_llr, double* cost);  // bposd_channel_tables
int probe_rank_large(bposd_handle* h, const DecodeCall& call, int* rank);
int num_candidates(const bposd_handle* h);

// ---- LDS-resident BP kernel: workgroup shapes (launch_bp_lds.hip)
bool is_reg63(const bposd_handle* h);
int shape_cpt(int shape);
int shape_threads(const bposd_handle* h, int shape);
int pick_shape(const bposd_handle* h);

// ---- kernel launches, one translation unit per family
int launch_bp(bposd_handle* h, const DecodeCall& call, bposd::BpParams& P);              // launch_bp_lds.hip    (bp_kernel)
int launch_bp_local(bposd_handle* h, const DecodeCall& call, const bposd::BpParams& P);  // launch_bp_local.hip  (bp_local_kernel)
int launch_bp_class(bposd_handle* h, const DecodeCall& call, const bposd::BpParams& P);  // launch_bp_class.hip  (bp_class_kernel)
bool class_preferred(const bposd_handle* h);
int launch_bp_large(bposd_handle* h, const DecodeCall& call, const bposd::BpParams& P);  // launch_bp_misc.hip   (bp_large_kernel)
int launch_bp_serial(bposd_handle* h, const DecodeCall& call, const bposd::BpParams& P); //                      (bp_serial_kernel)
int launch_bp_any(bposd_handle* h, const DecodeCall& call, const bposd::BpParams& P);    //                      (bp_anydeg_kernel)
int launch_bp_relay(bposd_handle* h, const DecodeCall& call, const bposd::BpParams& P);  // launch_bp_relay.hip  (bp_relay_kernel)
int bp_serial_max_dv();
size_t bp_large_lds_need(int m, int n);
int launch_osd(bposd_handle* h, const DecodeCall& call, const bposd::OsdParams& P, long long B);  // launch_osd.hip (osd_kernel, osd_wave_kernel)
int osd_words(int n);
int launch_osd_large(bposd_handle* h, const DecodeCall& call, const bposd::OsdParams& P, long long B, int* d_rank_out);  // launch_osd_large.hip
int osd_large_maxspan(bool cs);
// ---- LSD mode (launch_lsd.hip: lsd_kernel, lsd_compact_kernel)
int lsd_max_bits();
int lsd_max_checks();
size_t lsd_lds_need(int m, int n, bool higher_order);
bool lsd_higher_order(const bposd_handle* h);  // does the handle's LSD mode run lsd_kernel<true>?
int launch_lsd(bposd_handle* h, const DecodeCall& call, bposd::OsdParams& Q, long long B, bool osd_follows);
int launch_lsd_compact(bposd_handle* h, const DecodeCall& call, const bposd::OsdParams& Q, const int* bp_list, const int* bp_counters,
                       uint8_t* cmp_osd0, uint8_t* cmp_osdw, long long B);
// ---- logical observables (launch_obs.hip: obs_kernel)
int obs_max_k();
int observable_table(const int32_t* indptr, const int32_t* indices, int k, int n, uint64_t* table, std::string* why);
int launch_obs(bposd_handle* h, hipStream_t st, const void* const rows[3], bool packed, long long B, uint64_t* const out[3]);
// do the kernels this handle runs read packed syndromes / write packed rows themselves (else unpack / pack kernels surround them)?
inline bool native_packed(const bposd_handle* h) {
    // (forced local-edge variants 16 .. 26 have no packed instantiation; the LDS and class kernels switch at run time)
    return !h->bp_any && h->cfg.schedule == 0 && h->bp_variant != 64 && !(h->bp_variant >= 16 && h->bp_variant <= 26);
}

// ---- the decode calls (bposd_capi.hip), as the host-pointer paths (decode_host.hip) use them
// Device-side I/O of one kernel pair: rows of bytes, or of little-endian 64-bit words where the call is packed.  The same
// struct names the caller's arrays of a host-pointer call (null: that output is not wanted).
struct IoPtrs {
    const uint8_t* synd = nullptr;
    const uint8_t* sel = nullptr;
    uint8_t *osdw = nullptr, *osd0 = nullptr, *bp = nullptr, *conv = nullptr;
    int32_t* iters = nullptr;
    double* llr = nullptr;
    // a channel of its own for every syndrome (bposd_decode_batch_rows*): rows [B, n] of prior LLRs and of OSD-W weights
    // as bposd_channel_tables makes them; cost_rows is null where neither the OSD stage nor an LSD sweep weighs candidates
    const double* llr0_rows = nullptr;
    const double* cost_rows = nullptr;
};
// The outputs of an observables decode: rows of ceil(k / 64) words, flags and iteration counts (host or device memory).
struct ObsOut {
    uint64_t *osdw = nullptr, *osd0 = nullptr, *bp = nullptr;
    uint8_t* conv = nullptr;
    int32_t* iters = nullptr;
};
bool stage_weighs_candidates(const bposd_handle* h);  // does the OSD stage, or the sweep of LSD mode, rank candidates by the channel's weights?
int check_batch(bposd_handle* h, int64_t B, const void* synd, const void* osdw);  // every decode entry point, before anything is enqueued
int check_observables(bposd_handle* h);
DecodeCall take_next_lane(bposd_handle* h);  // a stand-alone call on the handle's next lane, record 0 of a new "last call"
int decode_device_impl(bposd_handle* h, const DecodeCall& call, const IoPtrs& io, int64_t B);  // one BP + one OSD launch, `io` in device memory
int obs_reserve(bposd_handle* h, size_t cap, const ObsOut& out, bool host, bool synd_packed);
int decode_obs_impl(bposd_handle* h, DecodeCall call, const void* d_synd, bool synd_packed, int64_t B, const ObsOut& out);
int check_alt_channel(bposd_handle* h, const double* alt);
int upload_alt_channel(bposd_handle* h, const double* alt);
// rows of 0/1 bytes <-> rows of 64-bit words on a stream (pack_rows_kernel, unpack_rows_kernel); wg_per_cu caps the grid
int launch_pack(bposd_handle* h, hipStream_t st, const uint8_t* d_bytes, long long B, int n, unsigned long long* d_words, int wg_per_cu = 2);
int launch_unpack(bposd_handle* h, hipStream_t st, const unsigned long long* d_words, long long B, int n, uint8_t* d_bytes);

// ---- host-pointer calls (decode_host.hip)
size_t row_bytes(int bits, bool packed);  // one row of `bits` entries: bytes, or 64-bit words
IoPtrs lane_ptrs(const Lane& L, bool words, const IoPtrs& host);  // the lane's row buffers of either form, for the outputs `host` names
// The chunks of a synchronous host-pointer call of B syndromes: chunk c is [lo[c], lo[c + 1]), `capacity` the largest.
struct HostChunkPlan {
    int count = 0;
    long long capacity = 0;
    long long lo[BPOSD_MAX_CHUNKS + 1] = {};
};
HostChunkPlan host_chunk_plan(long long B, int n, bool per_shot_rows, int nlanes, int num_cu, bool large, bool taper);

// The osdw rows of the last observables decode (bposd_decode_batch_observables_device) and their form: decode_obs_impl
// leaves them in the buffers of the lane the call took, packed words [B][ceil(n / 64)] where the kernels are packed, bytes
// [B][n] otherwise.  They are final behind the event the caller records on that lane after the call, and they stay until
// the next call that takes that lane.
struct ObsRows {
    const void* osdw;
    bool packed;
};
inline ObsRows last_obs_rows(const bposd_handle* h) {
    const Lane& L = h->lanes[h->last_lane];
    const bool native = native_packed(h);
    return ObsRows{native ? L.io_posdw.p : L.io_osdw.p, native};
}

}  // namespace bposd_host
