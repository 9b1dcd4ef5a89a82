// launch_bp_local.hip -- bp_local_kernel ((3,6)-regular codes with n = 2m, min-sum): launch
// One translation unit of libbposd_mi355x.so: the kernels of this family are instantiated here and nowhere else.
#include "launch_bp_local.h"

using namespace bposd;
using namespace bposd_host;

namespace bposd_host {
// the packed-I/O form exists for the instances auto-selection takes (internal.h: native_packed() asks for bp_variant == 0)
template <int CPT, int MP, int MINW, bool EARLY, bool UPRIOR = false>
static int launch_bp_local_t(bposd_handle* h, const DecodeCall& call, const BpLocalParams& L) {
    constexpr bool has_packed = !EARLY && ((CPT == 1 && MP == 1024 && MINW == 8) || (CPT == 2 && MP == 1024 && (MINW == 8 || MINW == 6)) || MP == 2048);
    if constexpr (has_packed) {
        if (L.packed_io) return launch_bp_local_tp<CPT, MP, MINW, EARLY, UPRIOR, true>(h, call, L);
    } else {
        if (L.packed_io) return fail(h, BPOSD_ERR_UNSUPPORTED, "this BP kernel variant has no packed-I/O form");
    }
    return launch_bp_local_tp<CPT, MP, MINW, EARLY, UPRIOR, false>(h, call, L);
}

// the instance whose pair body serves this layout's (uniform key, mixed) wave, for the shapes auto-selection takes
static int launch_bp_local_pair_any(bposd_handle* h, const DecodeCall& call, const BpLocalParams& L, int shape) {
    switch (h->local_pair_key) {
        case 0: return launch_bp_local_pair<0>(h, call, L, shape);
        case 1: return launch_bp_local_pair<1>(h, call, L, shape);
        case 2: return launch_bp_local_pair<2>(h, call, L, shape);
        case 5: return launch_bp_local_pair<5>(h, call, L, shape);
        case 6: return launch_bp_local_pair<6>(h, call, L, shape);
        case 10: return launch_bp_local_pair<10>(h, call, L, shape);
    }
    return fail(h, BPOSD_ERR_UNSUPPORTED, "no bp_local_kernel instance with a pair body for key %d", h->local_pair_key);
}

int launch_bp_local(bposd_handle* h, const DecodeCall& call, const BpParams& P) {
    BpLocalParams L{};
    L.m = P.m; L.n = P.n; L.B = P.B; L.max_iter = P.max_iter; L.ms_scaling = P.ms_scaling; L.osd_enabled = P.osd_enabled;
    L.mp = h->local_mp;
    L.synd = P.synd; L.llr0 = P.llr0; L.sel = P.sel; L.llr0_alt = P.llr0_alt; L.llr0_rows = P.llr0_rows;
    L.pos_chk = h->d_lpos_chk; L.pos_bit = h->d_lpos_bit; L.pos_alo = h->d_lpos_alo; L.pos_ahi = h->d_lpos_ahi;
    L.grp_dl = h->d_lgrp_dl; L.pos_dl = h->d_lpos_dl;
    L.out_bp = P.out_bp; L.out_osd0 = P.out_osd0; L.out_osdw = P.out_osdw; L.out_conv = P.out_conv; L.out_iters = P.out_iters;
    L.out_llr = P.out_llr; L.llr_ws = P.llr_ws; L.osd_list = P.osd_list; L.counters = P.counters; L.iter_total = P.iter_total; L.tail_flag = P.tail_flag; L.packed_io = P.packed_io;
    // a chunked host call counts as a whole; at most 40000 syndromes are a small call (below)
    const long long work = call.batch_hint > 0 ? call.batch_hint : L.B;
    const bool small_call = h->bp_variant == 0 && work <= 40000;
    // ---- park at drain (local_park.h: park_rule).  "Another lane has work in flight" is asked of the streams themselves.
    {
        int user_mode = h->park_mode;
        static const char* park_env = getenv("BPOSD_PARK");
        if (park_env && park_env[0] == 'f') user_mode = bposd_local_park::kAlways;
        else if (park_env && park_env[0] == '1') user_mode = bposd_local_park::kAuto;
        else if (park_env && park_env[0] == '0') user_mode = bposd_local_park::kNever;
        bool other_busy = false;
        if (user_mode == bposd_local_park::kAuto && !small_call && call.device_ptr && !call.lean && !call.tail_gate && P.osd_enabled && !P.out_llr) {
            for (int l = 0; l < h->nlanes && !other_busy; ++l) {
                const Lane& o = h->lanes[l];
                if (&o == call.lane) continue;
                other_busy = hipStreamQuery(o.stream) == hipErrorNotReady || hipStreamQuery(o.osd_stream) == hipErrorNotReady;
            }
            if (hipPeekAtLastError() == hipErrorNotReady) (void)hipGetLastError();  // (a stream that is not ready is no error of this call; anything else stays)
        }
        L.park_on_dry = bposd_local_park::park_rule(user_mode, call.device_ptr, call.lean, call.tail_gate, P.out_llr != nullptr, P.osd_enabled != 0,
                                                    /*specialised=*/true /* (launch_bp_local_tp knows) */, other_busy, small_call);
    }
    // auto-selection launches the instance that has a body for the layout's (uniform key, mixed) wave, if it has one; a
    // variant asked for by number is the plain instance (generic body for that wave)
    const bool pair = h->bp_variant == 0 && h->local_pair_key >= 0;
    if (h->local_mp == 2048) return pair ? launch_bp_local_pair_any(h, call, L, kBplPair2048x4) : launch_bp_local_t<2, 2048, 4, false>(h, call, L);  // 1024 threads, one workgroup per CU
    if (h->bp_variant == 17) return launch_bp_local_t<2, 1024, 8, false>(h, call, L);   // 512 threads, <= 64 VGPRs: 4 workgroups per CU
    if (h->bp_variant == 18) return launch_bp_local_t<1, 1024, 8, false>(h, call, L);   // 1024 threads, <= 64 VGPRs: 2 workgroups per CU
    if (h->bp_variant == 19) return launch_bp_local_t<4, 1024, 4, true>(h, call, L);    // 256 threads, <= 128 VGPRs: 4 workgroups per CU
    if (h->bp_variant == 20) return launch_bp_local_t<2, 1024, 6, true>(h, call, L);    // as the default with early check-pass loads
    if (h->bp_variant == 21) return launch_bp_local_t<4, 1024, 3, true>(h, call, L);    // 256 threads, <= 168 VGPRs: 3 workgroups per CU
    // one finite positive prior for every bit: it can live in scalar registers (positive: the padding positions share it)
    const bool uprior = h->probs_uniform && !L.sel && !L.llr0_rows && h->probs[0] > 0.0 && h->probs[0] < 0.5;
    // Small calls are latency-bound (a max_iter straggler runs ~2000 dependent iterations, a lone syndrome ~60): one check
    // per thread (16 waves per syndrome) iterates 25-30 % faster per syndrome, two checks per thread (4 workgroups per
    // CU) have the higher throughput.  Measured crossover on the [[1922,50]] code: 32768 syndromes per call (2048: 2.5
    // against 3.3 ms, 8192: 4.1 / 5.1, 32768: 9.6 / 10.0, 131072: 31.0 / 28.2).  A chunked host call counts as a whole.
    if (small_call) return uprior ? launch_bp_local_t<1, 1024, 8, false, true>(h, call, L) : launch_bp_local_t<1, 1024, 8, false>(h, call, L);
    if (pair) return launch_bp_local_pair_any(h, call, L, uprior ? kBplPair1024x8U : kBplPair1024x6);
    if ((h->bp_variant == 22 || h->bp_variant == 0) && uprior) return launch_bp_local_t<2, 1024, 8, false, true>(h, call, L);  // <= 64 VGPRs: 4 workgroups per CU
    if (h->bp_variant == 23 && uprior) return launch_bp_local_t<2, 1024, 6, true, true>(h, call, L);
    if (h->bp_variant == 24 && uprior) return launch_bp_local_t<2, 1024, 6, false, true>(h, call, L);
    if (h->bp_variant == 25 && uprior) return launch_bp_local_t<2, 1024, 8, true, true>(h, call, L);   // 22 with early check-pass loads
    if (h->bp_variant == 26 && uprior) return launch_bp_local_t<1, 1024, 8, false, true>(h, call, L);  // 18 with the scalar prior
    return launch_bp_local_t<2, 1024, 6, false>(h, call, L);                            // 512 threads, <= 80 VGPRs: 3 workgroups per CU
}
}  // namespace bposd_host
