// launch_bp_local_pair.inc.h -- body of launch_bp_local_pair_k<KEY>.hip: the bp_local_kernel instances with PAIRKEY =
// BPL_PAIRKEY (launch_bp_local.h).  Included once per unit, after BPL_PAIRKEY is defined.
#include "launch_bp_local.h"

namespace bposd_host {
template <>
int launch_bp_local_pair<BPL_PAIRKEY>(bposd_handle* h, const DecodeCall& call, const bposd::BpLocalParams& L, int shape) {
    constexpr int K = BPL_PAIRKEY;
    static_assert(bposd_local_keys::pair_key(K) >= 0, "a uniform key of local_keys.h");
    switch (shape) {
        case kBplPair1024x8U:
            return L.packed_io ? launch_bp_local_tp<2, 1024, 8, false, true, true, K>(h, call, L) : launch_bp_local_tp<2, 1024, 8, false, true, false, K>(h, call, L);
        case kBplPair1024x6:
            return L.packed_io ? launch_bp_local_tp<2, 1024, 6, false, false, true, K>(h, call, L) : launch_bp_local_tp<2, 1024, 6, false, false, false, K>(h, call, L);
        case kBplPair2048x4:
            return L.packed_io ? launch_bp_local_tp<2, 2048, 4, false, false, true, K>(h, call, L) : launch_bp_local_tp<2, 2048, 4, false, false, false, K>(h, call, L);
    }
    return fail(h, BPOSD_ERR_UNSUPPORTED, "no bp_local_kernel instance with a pair body for shape %d", shape);
}
}  // namespace bposd_host
