// launch_bp_relay.hip -- bp_relay_kernel (relay mode: min-sum legs with a memory term per bit): launch
// One translation unit of libbposd_mi355x.so: the kernel's two instances are instantiated here and nowhere else.
#include "internal.h"

#include "bp_relay_kernel.hip.h"

using namespace bposd;
using namespace bposd_host;

namespace bposd_host {

int launch_bp_relay(bposd_handle* h, const DecodeCall& call, const BpParams& P) {
    Lane& L = *call.lane;
    BpRelayParams A{};
    copy_shot_fields(A.io, P);
    A.g = csr_graph(h);
    A.legs = h->relay_legs; A.stop_after = h->relay_stop; A.leg_init = h->relay_init;
    A.gammas = h->d_relay_gammas; A.leg_iters = h->d_relay_iters;
    int rc;
    for (int l = 0; l < h->nlanes; ++l)  // a block that grows loses what it held
        if (h->lanes[l].relay_wt.bytes < sizeof(long long) * (size_t)P.B) h->lanes[l].relay_B = -1;
    if ((rc = ensure_lanes(h, &Lane::relay_sol, sizeof(int) * (size_t)P.B))) return rc;
    if ((rc = ensure_lanes(h, &Lane::relay_leg, sizeof(int) * (size_t)P.B))) return rc;
    if ((rc = ensure_lanes(h, &Lane::relay_wt, sizeof(long long) * (size_t)P.B))) return rc;
    A.out_solutions = (int*)L.relay_sol.p;
    A.out_best_leg = (int*)L.relay_leg.p;
    A.out_weight = (long long*)L.relay_wt.p;

    // instance 1 where everything fits one CU's LDS: a workgroup size that keeps at least 16 waves on the CU
    const size_t lds_all = bp_relay_lds_bytes(h->m, h->n, h->E);
    const bool in_lds = lds_all <= h->lds_per_cu;
    const size_t lds = in_lds ? lds_all : bp_relay_byte_part(h->m, h->n);
    // (instance 2 keeps 2 n + m bytes in LDS: at most 82 KB for the largest code a handle is created for, n <= 32767, m <= 16384)
    if (lds > h->lds_per_cu)
        return fail(h, BPOSD_ERR_UNSUPPORTED, "relay mode: the decision rows of n = %d bits and m = %d checks need %zu bytes of LDS, the CU has %zu",
                    h->n, h->m, lds, h->lds_per_cu);
    int wg_per_cu = (int)std::max<size_t>(1, std::min<size_t>(8, h->lds_per_cu / std::max<size_t>(lds, 1)));
    int nt = 256;
    if (in_lds) nt = wg_per_cu >= 4 ? 256 : (wg_per_cu >= 2 ? 512 : 1024);
    else wg_per_cu = std::min(wg_per_cu, 4);  // (the workspace is per workgroup)
    const long long grid = std::max<long long>(1, std::min<long long>(P.B, (long long)h->num_cu * wg_per_cu));
    if (!in_lds) {
        if ((rc = ensure_lanes(h, &Lane::bpl_msg, sizeof(double) * (size_t)grid * bp_relay_doubles(h->n, h->E)))) return rc;
        A.ws = (double*)L.bpl_msg.p;
    }
    note_instance(h->last_bp_inst, BPOSD_BP_KERNEL_RELAY, in_lds ? 1 : 2, nt, 0, 0, P.packed_io != 0);
    if (in_lds) {
        if ((rc = set_max_lds(h, (const void*)bp_relay_kernel<true>, lds))) return rc;
        hipLaunchKernelGGL(bp_relay_kernel<true>, dim3((unsigned)grid), dim3(nt), lds, L.stream, A);
    } else {
        if ((rc = set_max_lds(h, (const void*)bp_relay_kernel<false>, lds))) return rc;
        hipLaunchKernelGGL(bp_relay_kernel<false>, dim3((unsigned)grid), dim3(nt), lds, L.stream, A);
    }
    HIP_TRY(h, hipGetLastError());
    L.relay_B = P.B;
    h->relay_lane = (int)(call.lane - h->lanes);
    return 0;
}

}  // namespace bposd_host
