// launch_bp_misc.hip -- bp_large_kernel (messages in HBM), bp_serial_kernel (schedule = serial), bp_anydeg_kernel (any degree): launch
// One translation unit of libbposd_mi355x.so: the kernels of this family are instantiated here and nowhere else.
#include "internal.h"

#include "bp_large_kernel.hip.h"
#include "bp_serial_kernel.hip.h"
#include "bp_anydeg_kernel.hip.h"

using namespace bposd;
using namespace bposd_host;

namespace bposd_host {
template <int DC, int DV, int METHOD>
static int launch_bp_large_tm(bposd_handle* h, const DecodeCall& call, BpLargeParams& P) {
    h->large_form = METHOD;
    const size_t lds = bp_large_lds_bytes(h->m, h->n, METHOD == 2, DC);
    auto k = bp_large_kernel<DC, DV, METHOD>;
    // persistent workgroups: what registers and LDS admit per CU (the message workspace is per workgroup)
    int wg_per_cu = 1;
    { int rc_lds = set_max_lds(h, (const void*)k, lds); if (rc_lds) return rc_lds; }
    { int rc_occ = cached_occupancy(h, (const void*)k, bp_large_threads(METHOD), lds, &wg_per_cu); if (rc_occ) return rc_occ; }
    const int occ = std::max(1, std::min(wg_per_cu, 4));
    // The check records of the min-sum form are gathered ~11 times each in a bit pass; with one workgroup per CU the 256 record
    // arrays (465 KB each on 14520 x 29524) stay in the memory-side cache between uses: 72-74 -> 61-62 ms per 1024 syndromes.
    wg_per_cu = METHOD >= 1 ? 1 : occ;
    if (const char* e = getenv("BPOSD_LARGE_WG_CAP")) wg_per_cu = std::max(1, std::min(occ, atoi(e)));
    long long grid = std::max<long long>(1, std::min<long long>(P.B, (long long)h->num_cu * wg_per_cu));
    if (const char* e = getenv("BPOSD_LARGE_BP_GRID")) grid = std::max<long long>(1, std::min<long long>(grid, atoll(e)));  // (probe: a bandwidth-bound kernel on fewer CUs)
    constexpr int SLOTS = METHOD == 1 ? DC + 4 : (METHOD == 2 ? DC + 1 : DC);  // message planes (+ the check records of the min-sum form)
    int rc;
    if ((rc = ensure_lanes(h, &Lane::bpl_msg, sizeof(double) * (size_t)grid * SLOTS * P.mp))) return rc;
    if ((rc = ensure_lanes(h, &Lane::bpl_llr, sizeof(double) * (size_t)grid * h->n))) return rc;
    P.msg_ws = (double*)call.lane->bpl_msg.p;
    P.llr_tmp = (double*)call.lane->bpl_llr.p;
    note_instance(h->last_bp_inst, BPOSD_BP_KERNEL_LARGE, DC, DV, METHOD, 0, P.packed_io != 0);
    hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(bp_large_threads(METHOD)), lds, call.lane->stream, P);
    HIP_TRY(h, hipGetLastError());
    return 0;
}

template <int DC, int DV>
static int launch_bp_large_t(bposd_handle* h, const DecodeCall& call, BpLargeParams& P) {
    if (h->cfg.bp_method != BPOSD_BP_MIN_SUM) return launch_bp_large_tm<DC, DV, 0>(h, call, P);
    // min-sum: a1 and the flags of every check in LDS where they fit (bp_variant 63 forces the form with whole records in the workspace)
    const bool a1_in_lds = bp_large_lds_bytes(h->m, h->n, true, DC) <= h->lds_per_cu && h->bp_variant != 63;
    return a1_in_lds ? launch_bp_large_tm<DC, DV, 2>(h, call, P) : launch_bp_large_tm<DC, DV, 1>(h, call, P);
}

int launch_bp_large(bposd_handle* h, const DecodeCall& call, const BpParams& G) {
    BpLargeParams P{};
    copy_shot_fields(P, G);
    P.ps_form = h->cfg.ps_math_form; P.mp = h->tab_mp;
    P.chk_deg = h->d_chk_deg; P.var_deg = h->d_var_deg; P.var_pos = h->d_var_pos; P.var_ck = h->d_var_ck;
    if (h->dc_max <= 12 && h->dv_max <= 6) return launch_bp_large_t<12, 6>(h, call, P);
    if (h->dc_max <= 16 && h->dv_max <= 8) return launch_bp_large_t<16, 8>(h, call, P);
    return fail(h, BPOSD_ERR_UNSUPPORTED, "check degree %d / bit degree %d exceed the built kernels (16 / 8)", h->dc_max, h->dv_max);
}

// ------------------------------------------------------------------ the CSR-edge kernels with their messages in HBM (bp_csr.hip.h)
// Launch of one of them.  One persistent workgroup per shot with `lds` bytes of LDS and `msg_doubles` doubles of message
// workspace: workgroups per CU (what LDS admits, at most 8), the grid, and the lane's message and LLR workspaces sized for it.
template <class Params>
static int launch_csr(bposd_handle* h, const DecodeCall& call, void (*kernel)(Params), Params& K, int nt, size_t lds, size_t msg_doubles, int family) {
    const int wg_per_cu = std::max<int>(1, std::min<size_t>(8, h->lds_per_cu / std::max<size_t>(lds, 1)));
    const long long grid = std::max<long long>(1, std::min<long long>(K.io.B, (long long)h->num_cu * wg_per_cu));
    int rc;
    if ((rc = ensure_lanes(h, &Lane::bpl_msg, sizeof(double) * (size_t)grid * msg_doubles))) return rc;
    if ((rc = ensure_lanes(h, &Lane::bpl_llr, sizeof(double) * (size_t)grid * h->n))) return rc;
    K.msg_ws = (double*)call.lane->bpl_msg.p;
    K.llr_tmp = (double*)call.lane->bpl_llr.p;
    if ((rc = set_max_lds(h, (const void*)kernel, lds))) return rc;
    note_instance(h->last_bp_inst, family, 0, 0, 0, 0, false);
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(nt), lds, call.lane->stream, K);
    HIP_TRY(h, hipGetLastError());
    return 0;
}

int launch_bp_serial(bposd_handle* h, const DecodeCall& call, const BpParams& P) {
    BpSerialParams S{};
    copy_shot_fields(S.io, P);
    S.io.tail_flag = nullptr;  // the serial-schedule kernel does not report its tail (decode_host.hip gates no chunk on it)
    S.g = csr_graph(h);
    S.bp_method = h->cfg.bp_method; S.ps_form = h->cfg.ps_math_form; S.nlevels = h->nlevels;
    S.erow = h->d_erow; S.lvl_ptr = h->d_lvl_ptr; S.lvl_bits = h->d_lvl_bits;
    return launch_csr(h, call, bp_serial_kernel, S, BPS_NT, bp_serial_lds_bytes(h->n), h->E, BPOSD_BP_KERNEL_SERIAL);
}

// any-degree BP (check degree > 16 or bit degree > 8)
int launch_bp_any(bposd_handle* h, const DecodeCall& call, const BpParams& P) {
    BpAnyParams A{};
    copy_shot_fields(A.io, P);
    A.g = csr_graph(h);
    A.bp_method = h->cfg.bp_method; A.ps_form = h->cfg.ps_math_form;
    return launch_csr(h, call, bp_anydeg_kernel, A, BPA_NT, bp_anydeg_lds_bytes(h->n), 3 * (size_t)h->E, BPOSD_BP_KERNEL_ANYDEG);
}

int bp_serial_max_dv() { return BPS_MAXDV; }
size_t bp_large_lds_need(int m, int n) { return bp_large_lds_bytes(m, n); }

}  // namespace bposd_host

// ------------------------------------------------------------------ portable_math.h on the device (diagnostic)
// One thread per element; the routines are the ones the product-sum kernels of this library inline.
__global__ void __launch_bounds__(256) portable_math_kernel(int which, const double* __restrict__ a, const double* __restrict__ b,
                                                            double* __restrict__ y, long long count) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const double x = a[i];
    double r;
    switch (which) {
        case 0: r = pm_tanh(x); break;
        case 1: r = pm_log(x); break;
        case 2: r = pm_expm1(x); break;
        case 3: r = pm_tanh_half(x); break;
        case 4: r = pm_log_quot(x, b[i]); break;
        case 5: r = pm_ps_tanh_half(x, 0); break;
        case 6: r = pm_ps_tanh_half(x, 1); break;
        case 7: r = pm_ps_log_ratio(x, 0); break;
        default: r = pm_ps_log_ratio(x, 1); break;
    }
    y[i] = r;
}

extern "C" int bposd_debug_portable_math(int32_t which, const double* a, const double* b, double* y, int64_t count) {
    if (which < 0 || which > 8 || count < 0 || (count > 0 && (!a || !y || (which == 4 && !b)))) return BPOSD_ERR_INVALID;
    if (count > (int64_t)1 << 28) return BPOSD_ERR_UNSUPPORTED;  // 2 GiB per array: a diagnostic, not a bulk interface
    if (count == 0) return BPOSD_OK;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return BPOSD_ERR_NO_DEVICE;
    const size_t bytes = sizeof(double) * (size_t)count;
    DevArray<double> d_a, d_b, d_y;
    hipError_t e = d_a.alloc(bytes);
    if (e == hipSuccess) e = d_y.alloc(bytes);
    if (e == hipSuccess && which == 4) e = d_b.alloc(bytes);
    if (e == hipSuccess) e = hipMemcpy(d_a, a, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess && which == 4) e = hipMemcpy(d_b, b, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        const unsigned grid = (unsigned)((count + 255) / 256);  // <= 2^20 blocks
        hipLaunchKernelGGL(portable_math_kernel, dim3(grid), dim3(256), 0, 0, (int)which, d_a, d_b, d_y, (long long)count);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(y, d_y, bytes, hipMemcpyDeviceToHost);  // (synchronises with the kernel on the null stream)
    return e == hipSuccess ? BPOSD_OK : BPOSD_ERR_HIP;
}
