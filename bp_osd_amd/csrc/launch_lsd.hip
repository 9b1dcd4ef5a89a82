// launch_lsd.hip -- lsd_kernel (LSD mode: clusters around the unsatisfied checks of the shots BP left open): launch
// One translation unit of libbposd_mi355x.so: both instances of the kernel -- <false> LSD-0, <true> the higher orders and
// growth for free bits -- are instantiated here and nowhere else.
#include "internal.h"

#include "lsd_kernel.hip.h"

using namespace bposd;
using namespace bposd_host;

namespace bposd_host {

int lsd_max_bits() { return LSD_MAXB; }
int lsd_max_checks() { return LSD_MAXC; }
size_t lsd_lds_need(int m, int n, bool higher_order) { return lsd_lds_bytes(m, n, higher_order); }
bool lsd_higher_order(const bposd_handle* h) { return h->lsd_method != 0 || h->lsd_min_free > 0; }

// The LSD stage of one call, on the call's OSD stream behind BP's event.  `osd_follows`: an OSD kernel comes behind it.
// Q enters with the BP stage's list and leaves naming what that OSD kernel reads instead: the second list, its counters and
// its LLR rows -- and no compact rows, which lsd_compact (below) fills by the first list's slots once OSD has run.
int launch_lsd(bposd_handle* h, const DecodeCall& call, OsdParams& Q, long long B, bool osd_follows) {
    Lane& L = *call.lane;
    hipStream_t st = call.osd_stream;
    int rc;
    // The lane blocks below grow here, inside the call, like llr_ws and osd_list in decode_device_impl: a block that has to
    // grow is freed with hipFree, which waits for the device to go idle, so no kernel of another lane still reads it; this
    // call's own kernels that use these blocks are enqueued only further down.  Blocks sized once for a batch size never
    // grow again, so a stream of equal calls allocates nothing.
    const bool ho = lsd_higher_order(h);
    const int words = ho ? 6 : 4;  // status | rounds | clusters | max_bits, and for the second instance max_free | improved
    for (int l = 0; l < h->nlanes; ++l)  // a block that grows loses what it held
        if (h->lanes[l].lsd_stat.bytes < words * sizeof(int) * (size_t)B) h->lanes[l].lsd_B = -1;
    if ((rc = ensure_lanes(h, &Lane::lsd_stat, words * sizeof(int) * (size_t)B))) return rc;
    if (osd_follows) {
        if ((rc = ensure_lanes(h, &Lane::lsd_list2, sizeof(int) * (size_t)B))) return rc;
        if ((rc = ensure_lanes(h, &Lane::lsd_llr2, sizeof(double) * (size_t)B * h->n))) return rc;
    }
    if (!L.d_lsd_counters) HIP_TRY(h, L.d_lsd_counters.alloc(8 * sizeof(int)));
    const size_t lds = lsd_lds_bytes(h->m, h->n, ho);
    const int wg_per_cu = (int)std::max<size_t>(1, std::min<size_t>(8, h->lds_per_cu / lds));
    const long long grid = std::max<long long>(1, std::min<long long>(B, (long long)h->num_cu * wg_per_cu));
    if ((rc = ensure_lanes(h, &Lane::lsd_ws, sizeof(int) * (size_t)grid * lsd_ws_ints(h->m, h->n, ho)))) return rc;

    int* const stat = (int*)L.lsd_stat.p;
    HIP_TRY(h, hipMemsetAsync(L.d_lsd_counters, 0, 8 * sizeof(int), st));
    HIP_TRY(h, hipMemsetAsync(stat, 0xFF, sizeof(int) * (size_t)B, st));  // status -1: BP converged, the shot was not listed
    HIP_TRY(h, hipMemsetAsync(stat + B, 0, (words - 1) * sizeof(int) * (size_t)B, st));

    LsdParams A{};
    A.m = h->m; A.n = h->n; A.packed_io = Q.packed_io; A.tie_policy = Q.tie_policy;
    A.max_bits = h->lsd_max_bits; A.max_checks = h->lsd_max_checks; A.osd_follows = osd_follows ? 1 : 0;
    A.synd = Q.synd; A.rp = h->d_rp; A.ci = h->d_ci; A.cp = h->d_lsd_cp; A.cr = h->d_lsd_cr;
    A.llr_ws = Q.llr_ws; A.osd_list = Q.osd_list; A.counters = Q.counters;
    A.lsd_counters = L.d_lsd_counters; A.list2 = (int*)L.lsd_list2.p; A.llr_ws2 = (double*)L.lsd_llr2.p;
    A.out_osd0 = Q.out_osd0; A.out_osdw = Q.out_osdw; A.cmp_osd0 = Q.cmp_osd0; A.cmp_osdw = Q.cmp_osdw;
    A.st_status = stat; A.st_rounds = stat + B; A.st_clusters = stat + 2 * B; A.st_maxbits = stat + 3 * B;
    A.ws = (int*)L.lsd_ws.p;
    if (ho) {
        A.method = h->lsd_method; A.order = h->lsd_order; A.min_free = h->lsd_min_free; A.grow_limit = h->lsd_grow_limit;
        A.e_msb_first = Q.e_msb_first;
        A.cost = Q.cost; A.sel = Q.sel; A.cost_alt = Q.cost_alt; A.cost_rows = Q.cost_rows;  // the OSD stage's weights of this call
        A.st_maxfree = stat + 4 * B; A.st_improved = stat + 5 * B;
        if ((rc = set_max_lds(h, (const void*)lsd_kernel<true>, lds))) return rc;
        hipLaunchKernelGGL(lsd_kernel<true>, dim3((unsigned)grid), dim3(LSD_NT), lds, st, A);
    } else {
        if ((rc = set_max_lds(h, (const void*)lsd_kernel<false>, lds))) return rc;
        hipLaunchKernelGGL(lsd_kernel<false>, dim3((unsigned)grid), dim3(LSD_NT), lds, st, A);
    }
    HIP_TRY(h, hipGetLastError());
    L.lsd_B = B;
    L.lsd_words = words;
    h->lsd_launches[ho ? 1 : 0]++;
    h->lsd_lane = (int)(call.lane - h->lanes);
    if (osd_follows) {
        Q.osd_list = A.list2;
        Q.llr_ws = A.llr_ws2;
        Q.counters = L.d_lsd_counters;
        Q.cmp_osd0 = Q.cmp_osdw = nullptr;
    }
    return 0;
}

// Behind the OSD kernel of a call with compact rows: the rows OSD wrote, at the slots of the BP stage's list
int launch_lsd_compact(bposd_handle* h, const DecodeCall& call, const OsdParams& Q, const int* bp_list, const int* bp_counters,
                       uint8_t* cmp_osd0, uint8_t* cmp_osdw, long long B) {
    if (!cmp_osd0 && !cmp_osdw) return 0;
    Lane& L = *call.lane;
    const long long grid = std::max<long long>(1, std::min<long long>(B, (long long)h->num_cu * 2));
    hipLaunchKernelGGL(lsd_compact_kernel, dim3((unsigned)grid), dim3(256), 0, call.osd_stream, bp_list, bp_counters,
                       (const int*)L.lsd_stat.p, row_bytes(h->n, Q.packed_io != 0), Q.out_osdw, Q.out_osd0, cmp_osdw, cmp_osd0);
    HIP_TRY(h, hipGetLastError());
    return 0;
}

}  // namespace bposd_host
