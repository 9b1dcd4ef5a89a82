// launch_bp_local.h -- the launch of one bp_local_kernel instance, shared by the translation units that instantiate the
// family: launch_bp_local.hip (the plain instances and the dispatch) and launch_bp_local_pair_k*.hip (the instances with a
// body for one (uniform key, mixed) wave, one unit per key so that no unit compiles longer than the plain one).
#pragma once
#include "internal.h"

#include "bp_local_kernel.hip.h"

namespace bposd_host {

template <int CPT, int MP, int MINW, bool EARLY, bool UPRIOR, bool PACKED, int PAIRKEY = -1>
static int launch_bp_local_tp(bposd_handle* h, const DecodeCall& call, const bposd::BpLocalParams& L) {
    using namespace bposd;
    auto k = bp_local_kernel<CPT, MP, MINW, EARLY, UPRIOR, PACKED, PAIRKEY>;
    const int nt = MP / CPT;
    const size_t lds = bp_local_lds_bytes(L.mp);
    { int rc_lds = set_max_lds(h, (const void*)k, lds); if (rc_lds) return rc_lds; }
    int wg_per_cu = 1;
    { int rc_occ = cached_occupancy(h, (const void*)k, nt, lds, &wg_per_cu); if (rc_occ) return rc_occ; }
    if (getenv("BPOSD_DEBUG_OCC")) fprintf(stderr, "[bposd] local-edge BP kernel: %d threads, %zu B LDS, %d workgroups per CU, PAIRKEY %d\n", nt, lds, wg_per_cu, PAIRKEY);
    wg_per_cu = std::max(1, std::min(wg_per_cu, 8));
    long long grid = std::min<long long>(L.B, (long long)h->num_cu * wg_per_cu);
    if (grid < 1) grid = 1;
    int rc = ensure_lanes(h, &Lane::bpl_llr, sizeof(double) * (size_t)grid * h->n);
    if (rc) return rc;
    BpLocalParams Lq = L;
    Lq.llr_tmp = (double*)call.lane->bpl_llr.p;
    // park at drain (local_park.h) exists for the instances auto-selection takes: launch_bp_local has applied the rest of the rule
    constexpr bool can_park = bpl_specialised(CPT, MP, MINW, EARLY);
    if (!can_park) Lq.park_on_dry = bposd_local_park::kOff;
    if (Lq.park_on_dry) {
        if ((rc = ensure_lanes(h, &Lane::bpl_park, bposd_local_park::layout(MP).bytes * (size_t)grid))) return rc;
        Lq.park = (unsigned char*)call.lane->bpl_park.p;
    }
    note_instance(h->last_bp_inst, BPOSD_BP_KERNEL_LOCAL, CPT, MP, MINW, EARLY, PACKED);
    h->last_bp_pair_key = PAIRKEY;
    hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(nt), lds, call.lane->stream, Lq);
    HIP_TRY(h, hipGetLastError());
    if constexpr (can_park) {
        if (Lq.park_on_dry) {
            // The continuation: the same kernel's RESUME instance directly behind the first launch, same shape and grid,
            // persistent over the park records.  Events are all that lies between the two.  It goes to the call's
            // HIGH-PRIORITY stream (the one the OSD kernel follows on): the slots the first launch frees at the drain
            // otherwise go to workgroups of the other lane's BP grid that are still undispatched, the continuation then
            // starts only when THAT grid drains, and the pipeline settles a phase later (seen once in eight runs of the
            // headline: 22.5 instead of 21.2 ms per step, kernel_ms.bp 36 ms).  The lane's main stream waits for it, so
            // everything recorded there afterwards -- the timing event, ev_bp -- covers both launches.
            auto kr = bp_local_kernel<CPT, MP, MINW, EARLY, UPRIOR, PACKED, PAIRKEY, true>;
            { int rc_lds = set_max_lds(h, (const void*)kr, lds); if (rc_lds) return rc_lds; }
            Lq.park_on_dry = bposd_local_park::kOff;
            Lq.resume = 1;
            // BPOSD_PARK_ORDER=1 (A/B): the continuation lets the previous lane's OSD kernel go first
            static const char* order_env = getenv("BPOSD_PARK_ORDER");
            if (order_env && order_env[0] == '1') {
                Lane& prev = h->lanes[((int)(call.lane - h->lanes) + h->nlanes - 1) % h->nlanes];
                if (&prev != call.lane && prev.osd_recorded) HIP_TRY(h, hipStreamWaitEvent(call.lane->stream, prev.ev_osd, 0));
            }
            hipStream_t cs = call.osd_stream ? call.osd_stream : call.lane->stream;
            if (cs != call.lane->stream) {
                HIP_TRY(h, hipEventRecord(call.lane->ev_park, call.lane->stream));
                HIP_TRY(h, hipStreamWaitEvent(cs, call.lane->ev_park, 0));
            }
            hipLaunchKernelGGL(kr, dim3((unsigned)grid), dim3(nt), lds, cs, Lq);
            HIP_TRY(h, hipGetLastError());
            if (cs != call.lane->stream) {
                HIP_TRY(h, hipEventRecord(call.lane->ev_park, cs));
                HIP_TRY(h, hipStreamWaitEvent(call.lane->stream, call.lane->ev_park, 0));
            }
        }
    }
    return 0;
}

// The instances with a pair body exist for the two-checks-per-thread shapes auto-selection takes, byte and packed forms:
enum BplPairShape { kBplPair1024x8U = 0, kBplPair1024x6 = 1, kBplPair2048x4 = 2 };  // <2,1024,8,false,true> <2,1024,6,false,false> <2,2048,4,false,false>
// defined in launch_bp_local_pair_k<KEY>.hip for the six uniform keys of local_keys.h
template <int KEY>
int launch_bp_local_pair(bposd_handle* h, const DecodeCall& call, const bposd::BpLocalParams& L, int shape);

}  // namespace bposd_host
