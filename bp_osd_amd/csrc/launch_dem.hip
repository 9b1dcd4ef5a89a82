// launch_dem.hip -- the detector-error-model Monte-Carlo engine of libbposd_mi355x.so: bposd_dem_* of include/bposd_mi355x.h.
// One translation unit: both instances of dem_sample_kernel and dem_score_kernel (dem_kernels.hip.h) are instantiated here and
// nowhere else.
//
// A batch is sample faults -> detectors and true observables -> one decode straight to observables -> compare -> five
// integers.  The engine owns every buffer of it and a stream of its own; the decode goes through the decoder's
// device-pointer observables call on the decoder's next lane.  The engine's stream and that lane are ordered against each
// other by events; the host waits once per batch, for the counters (the pattern of launch_mc.hip).
#include "internal.h"

#include <cmath>
#include <cstdarg>
#include <cstring>
#include <memory>

#include "dem_engine.h"
#include "dem_kernels.hip.h"

using namespace bposd_dem_dev;

namespace {

int dem_fail(bposd_dem* dem, int code, const char* fmt, ...) __attribute__((format(printf, 3, 4)));
int dem_fail(bposd_dem* dem, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (dem) dem->err = buf;
    else bposd_host::fail(nullptr, code, "%s", buf);  // read back through bposd_last_error(NULL), like a failed bposd_create
    return code;
}

#define DEM_TRY(dem, expr)                                                                                             \
    do {                                                                                                               \
        hipError_t _e = (expr);                                                                                        \
        if (_e != hipSuccess)                                                                                          \
            return dem_fail(dem, BPOSD_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)

template <class T>
int dem_alloc(bposd_dem* dem, DevArray<T>& p, size_t count) {
    const size_t bytes = std::max<size_t>(count * sizeof(T), 256);
    DEM_TRY(dem, p.alloc(bytes));
    dem->device_bytes += bytes;
    return 0;
}

template <class T>
int dem_upload(bposd_dem* dem, DevArray<T>& p, const T* src, size_t count) {
    int rc = dem_alloc(dem, p, count);
    if (rc) return rc;
    if (count) DEM_TRY(dem, hipMemcpy(p, src, count * sizeof(T), hipMemcpyHostToDevice));
    return 0;
}

// One CSR operand of bposd_dem_tables: the reason for a refusal in `why`, or 0.
int check_dem_csr(const char* name, const int32_t* rp, const int32_t* ci, int rows, int N, std::string* why) {
    char buf[200];
    auto refuse = [&](const char* fmt, int a, int b, int c) {
        snprintf(buf, sizeof(buf), fmt, name, a, b, c);
        *why = buf;
        return BPOSD_ERR_INVALID;
    };
    if (!rp) return refuse("bposd_dem_tables: %s: null indptr", 0, 0, 0);
    if (rp[0] != 0) return refuse("bposd_dem_tables: %s: indptr[0] must be 0", 0, 0, 0);
    for (int r = 0; r < rows; ++r) {
        if (rp[r + 1] < rp[r]) return refuse("bposd_dem_tables: %s: indptr not monotone at row %d", r, 0, 0);
        if (rp[r + 1] > rp[r] && !ci) return refuse("bposd_dem_tables: %s: null indices", 0, 0, 0);
        for (int e = rp[r]; e < rp[r + 1]; ++e) {
            if (ci[e] < 0 || ci[e] >= N) return refuse("bposd_dem_tables: %s: row %d holds column %d, outside [0, %d)", r, ci[e], N);
            if (e > rp[r] && ci[e] <= ci[e - 1])
                return refuse("bposd_dem_tables: %s: the columns of row %d are not strictly ascending (at column %d)", r, ci[e], 0);
        }
    }
    return 0;
}

// CSR of H (M x N) and of L (k x N) -> CSC of H stacked on L in the accumulator's bit space: detector r is bit r,
// observable j is bit 64 * ceil(M / 64) + j.  Rows are visited in ascending order, so every column ascends.
int dem_tables(const int32_t* h_rp, const int32_t* h_ci, int M, const int32_t* l_rp, const int32_t* l_ci, int k, int N, int32_t* col_ptr,
               int32_t* col_bits, std::string* why) {
    char buf[160];
    auto refuse = [&](const char* fmt, int a, int b) {
        snprintf(buf, sizeof(buf), fmt, a, b);
        *why = buf;
        return BPOSD_ERR_INVALID;
    };
    if (!col_ptr) return refuse("bposd_dem_tables: null argument", 0, 0);
    if (M < 1 || N < 1) return refuse("bposd_dem_tables: bad shape: M %d, N %d", M, N);
    if (k < 1 || k > bposd_host::obs_max_k()) return refuse("bposd_dem_tables: k = %d is outside 1 .. %d", k, bposd_host::obs_max_k());
    if (const int rc = check_dem_csr("H", h_rp, h_ci, M, N, why)) return rc;
    if (const int rc = check_dem_csr("L", l_rp, l_ci, k, N, why)) return rc;
    const long long nnz = (long long)h_rp[M] + l_rp[k];
    if (nnz > 0x7fffffffLL) return refuse("bposd_dem_tables: too many entries", 0, 0);
    if (nnz > 0 && !col_bits) return refuse("bposd_dem_tables: null argument", 0, 0);
    std::vector<int32_t> fill((size_t)N + 1, 0);
    for (int e = 0; e < h_rp[M]; ++e) ++fill[(size_t)h_ci[e] + 1];
    for (int e = 0; e < l_rp[k]; ++e) ++fill[(size_t)l_ci[e] + 1];
    for (int i = 0; i < N; ++i) fill[(size_t)i + 1] += fill[i];
    std::copy(fill.begin(), fill.end(), col_ptr);
    for (int r = 0; r < M; ++r)
        for (int e = h_rp[r]; e < h_rp[r + 1]; ++e) col_bits[fill[h_ci[e]]++] = r;
    const int base = 64 * ((M + 63) / 64);
    for (int j = 0; j < k; ++j)
        for (int e = l_rp[j]; e < l_rp[j + 1]; ++e) col_bits[fill[l_ci[e]]++] = base + j;
    return BPOSD_OK;
}

int create_impl(bposd_dem* dem, const std::vector<int32_t>& col_ptr, const std::vector<int32_t>& col_bits, const double* priors) {
    int rc;
    if ((rc = dem_upload(dem, dem->d_priors, priors, (size_t)dem->N))) return rc;
    if ((rc = dem_upload(dem, dem->d_col_ptr, col_ptr.data(), col_ptr.size()))) return rc;
    if ((rc = dem_upload(dem, dem->d_col_bits, col_bits.data(), col_bits.size()))) return rc;
    const size_t C = (size_t)dem->capacity;
    if ((rc = dem_alloc(dem, dem->d_faults, C * dem->fw))) return rc;
    if ((rc = dem_alloc(dem, dem->d_detectors, C * dem->dw))) return rc;
    if ((rc = dem_alloc(dem, dem->d_observables, C * dem->ow))) return rc;
    if (dem->dec) {
        if ((rc = dem_alloc(dem, dem->d_obs_bp, C * dem->ow))) return rc;
        if ((rc = dem_alloc(dem, dem->d_obs_osd0, C * dem->ow))) return rc;
        if ((rc = dem_alloc(dem, dem->d_obs_osdw, C * dem->ow))) return rc;
        if ((rc = dem_alloc(dem, dem->d_flags, C))) return rc;
        if ((rc = dem_alloc(dem, dem->d_conv, C))) return rc;
        if ((rc = dem_alloc(dem, dem->d_iters, C))) return rc;
        if ((rc = dem_alloc(dem, dem->d_counters, 8))) return rc;
        if ((rc = dem_alloc(dem, dem->d_obs_fail, (size_t)dem->k))) return rc;
        DEM_TRY(dem, dem->h_counters.alloc((8 + (size_t)dem->k) * sizeof(int), hipHostMallocDefault));
    }
    if (dem->num_cu <= 0) {
        hipDeviceProp_t prop;
        DEM_TRY(dem, hipGetDeviceProperties(&prop, dem->cfg.device));
        dem->num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    }
    DEM_TRY(dem, hipStreamCreateWithFlags(&dem->stream.raw, hipStreamNonBlocking));
    for (Event* e : {&dem->ev_sampled, &dem->ev_decoded}) DEM_TRY(dem, hipEventCreateWithFlags(&e->raw, hipEventDisableTiming));
    for (Event& e : dem->ev_t) DEM_TRY(dem, hipEventCreate(&e.raw));
    return 0;
}

// two accumulator rows, and behind each the log-weight word of the weighted instance
size_t sample_lds_bytes(const bposd_dem* dem, bool weighted) {
    return 2 * sizeof(unsigned long long) * (size_t)(dem->dw + dem->ow + (weighted ? 1 : 0));
}

// dem_sample_kernel for rows [0, B) on the engine's stream, between ev_t[0] and ev_t[1]
int enqueue_sample(bposd_dem* dem, uint64_t first_shot, long long B) {
    DemSampleParams S{};
    S.B = B;
    S.first_shot = first_shot;
    S.key0 = (uint32_t)dem->cfg.seed;
    S.key1 = (uint32_t)(dem->cfg.seed >> 32);
    S.N = dem->N;
    S.fw = dem->fw;
    S.dw = dem->dw;
    S.ow = dem->ow;
    S.priors = dem->weighted ? dem->d_sample_priors : dem->d_priors;
    S.col_ptr = dem->d_col_ptr;
    S.col_bits = dem->d_col_bits;
    S.faults = dem->d_faults;
    S.detectors = dem->d_detectors;
    S.observables = dem->d_observables;
    S.incr = dem->d_incr;  // (NULL until the first bposd_dem_set_sampling; the plain instance reads neither)
    S.logw = dem->d_logw;
    const unsigned grid = (unsigned)std::min<long long>(B, (long long)dem->num_cu * 8);
    dem->logw_B = 0;
    DEM_TRY(dem, hipEventRecord(dem->ev_t[0], dem->stream));
    if (dem->weighted)
        hipLaunchKernelGGL(dem_sample_kernel<true>, dim3(grid), dim3(DEM_THREADS), sample_lds_bytes(dem, true), dem->stream, S);
    else
        hipLaunchKernelGGL(dem_sample_kernel<false>, dim3(grid), dim3(DEM_THREADS), sample_lds_bytes(dem, false), dem->stream, S);
    DEM_TRY(dem, hipGetLastError());
    DEM_TRY(dem, hipEventRecord(dem->ev_t[1], dem->stream));
    if (dem->weighted) dem->logw_B = B;
    return 0;
}

}  // namespace

int bposd_host::dem_sample_async(bposd_dem* dem, uint64_t first_shot, int64_t B, hipStream_t waiter) {
    if (B < 1 || B > dem->capacity) return dem_fail(dem, BPOSD_ERR_INVALID, "batch size %lld outside [1, capacity %lld]", (long long)B, dem->capacity);
    DeviceGuard guard(dem->cfg.device);
    DEM_TRY(dem, guard.err);
    dem->sampled_B = dem->scored_B = 0;
    if (const int rc = enqueue_sample(dem, first_shot, B)) return rc;
    DEM_TRY(dem, hipEventRecord(dem->ev_sampled, dem->stream));
    DEM_TRY(dem, hipStreamWaitEvent(waiter, dem->ev_sampled, 0));
    dem->sampled_B = B;
    return BPOSD_OK;
}

extern "C" {

const char* bposd_dem_last_error(bposd_dem* dem) { return dem ? dem->err.c_str() : bposd_last_error(nullptr); }

void bposd_dem_destroy(bposd_dem* dem) {
    if (!dem) return;
    DeviceGuard guard(dem->cfg.device);  // (outlives the delete)
    if (dem->stream) (void)hipStreamSynchronize(dem->stream);
    delete dem;
}

int bposd_dem_tables(const int32_t* h_indptr, const int32_t* h_indices, int32_t M, const int32_t* l_indptr, const int32_t* l_indices,
                     int32_t k, int32_t N, int32_t* col_ptr, int32_t* col_bits) {
    std::string why;
    if (const int rc = dem_tables(h_indptr, h_indices, M, l_indptr, l_indices, k, N, col_ptr, col_bits, &why))
        return dem_fail(nullptr, rc, "%s", why.c_str());
    return BPOSD_OK;
}

int bposd_dem_create(const bposd_dem_config* cfg, bposd_handle* dec, const int32_t* h_indptr, const int32_t* h_indices, int32_t M,
                     const int32_t* l_indptr, const int32_t* l_indices, int32_t k, int32_t N, const double* priors, bposd_dem** out) {
    if (!out) return dem_fail(nullptr, BPOSD_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!cfg) return dem_fail(nullptr, BPOSD_ERR_INVALID, "config is required");
    if (cfg->capacity < 1 || cfg->capacity > 0x7fffffffLL) return dem_fail(nullptr, BPOSD_ERR_INVALID, "capacity %lld out of range", (long long)cfg->capacity);
    if (M < 1 || N < 1 || !h_indptr || !l_indptr) return dem_fail(nullptr, BPOSD_ERR_INVALID, "bad shape or missing matrix: M %d, N %d", M, N);
    if (!priors) return dem_fail(nullptr, BPOSD_ERR_INVALID, "priors are required");
    for (int i = 0; i < N; ++i)
        if (!(priors[i] >= 0.0 && priors[i] <= 1.0))  // (a NaN fails both comparisons)
            return dem_fail(nullptr, BPOSD_ERR_INVALID, "the prior of fault %d (%g) is not a probability", i, priors[i]);
    if (dec && dec->device != cfg->device)
        return dem_fail(nullptr, BPOSD_ERR_INVALID, "the decoder lives on device %d, the engine on device %d", dec->device, cfg->device);
    if (dec && (dec->m != M || dec->n != N))
        return dem_fail(nullptr, BPOSD_ERR_INVALID, "decoder shape %d x %d does not match the model's %d detectors x %d faults", dec->m, dec->n, M, N);
    // validates H, L and k; sized from the row pointers once those are known to be usable
    std::string why;
    std::vector<int32_t> col_ptr((size_t)N + 1), col_bits;
    if (k >= 1 && k <= bposd_host::obs_max_k() && h_indptr[0] == 0 && l_indptr[0] == 0 && h_indptr[M] >= 0 && l_indptr[k] >= 0)
        col_bits.resize((size_t)h_indptr[M] + (size_t)l_indptr[k]);
    if (const int rc = dem_tables(h_indptr, h_indices, M, l_indptr, l_indices, k, N, col_ptr.data(), col_bits.data(), &why))
        return dem_fail(nullptr, rc, "%s", why.c_str());

    std::unique_ptr<bposd_dem, decltype(&bposd_dem_destroy)> owner(new bposd_dem(), bposd_dem_destroy);
    bposd_dem* const dem = owner.get();
    dem->cfg = *cfg;
    dem->dec = dec;
    dem->N = N;
    dem->M = M;
    dem->k = k;
    dem->fw = (N + 63) / 64;
    dem->dw = (M + 63) / 64;
    dem->ow = (k + 63) / 64;
    dem->capacity = cfg->capacity;
    dem->num_cu = dec ? dec->num_cu : 0;
    if (sample_lds_bytes(dem, false) > 64 * 1024)
        return dem_fail(nullptr, BPOSD_ERR_UNSUPPORTED, "%d detectors and %d observables need %zu bytes of LDS per workgroup, more than 65536", M, k,
                        sample_lds_bytes(dem, false));
    int rc = 0;
    std::vector<uint64_t> table;
    if (dec) {  // (validated before anything is allocated)
        table.resize((size_t)dem->fw * k);
        if ((rc = bposd_host::observable_table(l_indptr, l_indices, k, N, table.data(), &why))) return dem_fail(nullptr, rc, "%s", why.c_str());
    }
    {
        DeviceGuard guard(cfg->device);
        rc = guard.err != hipSuccess ? dem_fail(dem, BPOSD_ERR_HIP, "hipSetDevice(%d) failed", cfg->device) : create_impl(dem, col_ptr, col_bits, priors);
    }
    if (rc) return dem_fail(nullptr, rc, "%s", dem->err.c_str());
    // Last, once nothing of the engine's own can fail any more: the L that scores is the L the decoder multiplies by.  A
    // create that fails leaves the caller's decoder as it was.
    if (dec && (rc = bposd_set_observables(dec, table.data(), k))) return dem_fail(nullptr, rc, "bposd_set_observables: %s", bposd_last_error(dec));
    *out = owner.release();
    return BPOSD_OK;
}

int bposd_dem_set_sampling(bposd_dem* dem, const double* sample_priors, const int64_t* incr) {
    if (!dem) return BPOSD_ERR_INVALID;
    if ((sample_priors == nullptr) != (incr == nullptr))
        return dem_fail(dem, BPOSD_ERR_INVALID, "sample_priors and incr go together: give both, or NULL for both to sample plainly");
    if (!sample_priors) {  // back to the model's own priors; the tables stay allocated for the next switch
        dem->weighted = false;
        dem->logw_B = 0;
        return BPOSD_OK;
    }
    // everything is validated before anything changes: a refusal leaves the engine in the mode it was in
    unsigned long long total = 0;  // sum of |incr|: every term and the running sum stay below 2^63
    for (int i = 0; i < dem->N; ++i) {
        if (!(sample_priors[i] >= 0.0 && sample_priors[i] <= 1.0))  // (a NaN fails both comparisons)
            return dem_fail(dem, BPOSD_ERR_INVALID, "the sampling probability of fault %d (%g) is not a probability", i, sample_priors[i]);
        const unsigned long long a = incr[i] < 0 ? 0ull - (unsigned long long)incr[i] : (unsigned long long)incr[i];
        if (a >= (1ull << 62) || (total += a) >= (1ull << 62))
            return dem_fail(dem, BPOSD_ERR_INVALID, "the increments up to fault %d sum to 2^62 or more in magnitude: a shot's log-weight could overflow", i);
    }
    if (sample_lds_bytes(dem, true) > 64 * 1024)
        return dem_fail(dem, BPOSD_ERR_UNSUPPORTED, "weighted sampling needs %zu bytes of LDS per workgroup, more than 65536", sample_lds_bytes(dem, true));
    DeviceGuard guard(dem->cfg.device);
    DEM_TRY(dem, guard.err);
    DEM_TRY(dem, hipStreamSynchronize(dem->stream));  // no sampler is reading the tables
    int rc;
    if (!dem->d_sample_priors.p && (rc = dem_alloc(dem, dem->d_sample_priors, (size_t)dem->N))) return rc;
    if (!dem->d_incr.p && (rc = dem_alloc(dem, dem->d_incr, (size_t)dem->N))) return rc;
    if (!dem->d_logw.p && (rc = dem_alloc(dem, dem->d_logw, (size_t)dem->capacity))) return rc;
    dem->weighted = false;  // (until both tables are the new ones)
    dem->logw_B = 0;        // what item 10 held was summed from the table that goes
    DEM_TRY(dem, hipMemcpy(dem->d_sample_priors, sample_priors, sizeof(double) * (size_t)dem->N, hipMemcpyHostToDevice));
    DEM_TRY(dem, hipMemcpy(dem->d_incr, incr, sizeof(int64_t) * (size_t)dem->N, hipMemcpyHostToDevice));
    dem->weighted = true;
    return BPOSD_OK;
}

int bposd_dem_sample(bposd_dem* dem, uint64_t first_shot, int64_t B) {
    if (!dem) return BPOSD_ERR_INVALID;
    if (B < 1 || B > dem->capacity) return dem_fail(dem, BPOSD_ERR_INVALID, "batch size %lld outside [1, capacity %lld]", (long long)B, dem->capacity);
    DeviceGuard guard(dem->cfg.device);
    DEM_TRY(dem, guard.err);
    dem->sampled_B = dem->scored_B = 0;
    if (const int rc = enqueue_sample(dem, first_shot, B)) return rc;
    DEM_TRY(dem, hipStreamSynchronize(dem->stream));
    dem->sampled_B = B;
    return BPOSD_OK;
}

int bposd_dem_run(bposd_dem* dem, uint64_t first_shot, int64_t B, int64_t counters[5]) {
    if (!dem) return BPOSD_ERR_INVALID;
    if (!dem->dec) return dem_fail(dem, BPOSD_ERR_INVALID, "this engine was created without a decoder: it samples only (bposd_dem_sample)");
    if (!counters) return dem_fail(dem, BPOSD_ERR_INVALID, "counters is NULL");
    if (B < 1 || B > dem->capacity) return dem_fail(dem, BPOSD_ERR_INVALID, "batch size %lld outside [1, capacity %lld]", (long long)B, dem->capacity);
    bposd_handle* const dec = dem->dec;
    if (dec->obs_k != dem->k)
        return dem_fail(dem, BPOSD_ERR_INVALID, "the decoder's observable table (k = %d) is no longer the one this engine set (k = %d)", dec->obs_k, dem->k);
    DeviceGuard guard(dem->cfg.device);
    DEM_TRY(dem, guard.err);
    dem->sampled_B = dem->scored_B = 0;

    int rc;
    if ((rc = enqueue_sample(dem, first_shot, B))) return rc;
    DEM_TRY(dem, hipEventRecord(dem->ev_sampled, dem->stream));
    DEM_TRY(dem, hipMemsetAsync(dem->d_counters, 0, 8 * sizeof(int), dem->stream));
    DEM_TRY(dem, hipMemsetAsync(dem->d_obs_fail, 0, sizeof(int) * (size_t)dem->k, dem->stream));

    // the decode on the decoder's next lane, ordered behind the sampler; ev_decoded is recorded on that lane behind the call
    DEM_TRY(dem, hipStreamWaitEvent(dec->lanes[dec->next_lane].stream, dem->ev_sampled, 0));
    rc = bposd_decode_batch_observables_device(dec, dem->d_detectors, /*syndromes_packed=*/1, B, (uint64_t*)dem->d_obs_osdw.p, (uint64_t*)dem->d_obs_osd0.p,
                                               (uint64_t*)dem->d_obs_bp.p, dem->d_conv, dem->d_iters);
    if (rc) {
        (void)hipStreamSynchronize(dem->stream);  // the sampler and the memsets are queued: leave nothing running behind the error
        return dem_fail(dem, rc, "decode failed: %s", bposd_last_error(dec));
    }
    DEM_TRY(dem, hipEventRecord(dem->ev_decoded, dec->lanes[dec->last_lane].stream));
    DEM_TRY(dem, hipStreamWaitEvent(dem->stream, dem->ev_decoded, 0));

    DemScoreParams Q{};
    Q.B = B;
    Q.k = dem->k;
    Q.ow = dem->ow;
    Q.dw = dem->dw;
    Q.detectors = dem->d_detectors;
    Q.truth = dem->d_observables;
    Q.bp = dem->d_obs_bp;
    Q.osd0 = dem->d_obs_osd0;
    Q.osdw = dem->d_obs_osdw;
    Q.conv = dem->d_conv;
    Q.flags = dem->d_flags;
    Q.counters = dem->d_counters;
    Q.obs_fail = dem->d_obs_fail;
    const unsigned grid = (unsigned)std::min<long long>((B + DEM_SCORE_THREADS - 1) / DEM_SCORE_THREADS, (long long)dem->num_cu * 8);
    DEM_TRY(dem, hipEventRecord(dem->ev_t[2], dem->stream));
    hipLaunchKernelGGL(dem_score_kernel, dim3(grid), dim3(DEM_SCORE_THREADS), 0, dem->stream, Q);
    DEM_TRY(dem, hipGetLastError());
    DEM_TRY(dem, hipEventRecord(dem->ev_t[3], dem->stream));
    DEM_TRY(dem, hipMemcpyAsync(dem->h_counters.p, dem->d_counters, 5 * sizeof(int), hipMemcpyDeviceToHost, dem->stream));
    DEM_TRY(dem, hipMemcpyAsync(dem->h_counters.as<int>() + 8, dem->d_obs_fail, sizeof(int) * (size_t)dem->k, hipMemcpyDeviceToHost, dem->stream));
    DEM_TRY(dem, hipStreamSynchronize(dem->stream));  // the batch's one host wait
    for (int i = 0; i < 5; ++i) counters[i] = dem->h_counters.as<int>()[i];
    dem->sampled_B = dem->scored_B = B;
    return BPOSD_OK;
}

int bposd_dem_fetch(bposd_dem* dem, int32_t what, void* host_dst, size_t bytes) {
    if (!dem) return BPOSD_ERR_INVALID;
    if (!host_dst) return dem_fail(dem, BPOSD_ERR_INVALID, "destination is NULL");
    if (what < BPOSD_DEM_FAULTS || what > BPOSD_DEM_LOGW)
        return dem_fail(dem, BPOSD_ERR_INVALID, "what = %d is not one of BPOSD_DEM_FAULTS .. BPOSD_DEM_LOGW", what);
    if (what == BPOSD_DEM_LOGW && !dem->weighted)
        return dem_fail(dem, BPOSD_ERR_INVALID, "item %d needs weighted sampling (bposd_dem_set_sampling): this engine samples plainly", what);
    if (dem->sampled_B == 0) return dem_fail(dem, BPOSD_ERR_INVALID, "no batch has run yet");
    if (what == BPOSD_DEM_LOGW && dem->logw_B != dem->sampled_B)
        return dem_fail(dem, BPOSD_ERR_INVALID, "item %d needs a batch sampled since bposd_dem_set_sampling", what);
    if (what >= BPOSD_DEM_OBS_BP && what <= BPOSD_DEM_OBS_FAIL && dem->scored_B == 0)
        return dem_fail(dem, BPOSD_ERR_INVALID, "item %d needs bposd_dem_run: the last batch was sampled only", what);
    const void* src = nullptr;
    size_t row = 0, rows = (size_t)dem->sampled_B;
    switch (what) {
    case BPOSD_DEM_FAULTS: src = dem->d_faults; row = 8 * (size_t)dem->fw; break;
    case BPOSD_DEM_DETECTORS: src = dem->d_detectors; row = 8 * (size_t)dem->dw; break;
    case BPOSD_DEM_OBSERVABLES: src = dem->d_observables; row = 8 * (size_t)dem->ow; break;
    case BPOSD_DEM_OBS_BP: src = dem->d_obs_bp; row = 8 * (size_t)dem->ow; break;
    case BPOSD_DEM_OBS_OSD0: src = dem->d_obs_osd0; row = 8 * (size_t)dem->ow; break;
    case BPOSD_DEM_OBS_OSDW: src = dem->d_obs_osdw; row = 8 * (size_t)dem->ow; break;
    case BPOSD_DEM_FLAGS: src = dem->d_flags; row = 1; break;
    case BPOSD_DEM_CONVERGED: src = dem->d_conv; row = 1; break;
    case BPOSD_DEM_ITERS: src = dem->d_iters; row = sizeof(int32_t); break;
    case BPOSD_DEM_LOGW: src = dem->d_logw; row = sizeof(int64_t); break;
    default: src = dem->d_obs_fail; row = sizeof(int32_t) * (size_t)dem->k; rows = 1; break;  // BPOSD_DEM_OBS_FAIL: one row per batch
    }
    const size_t want = row * rows;
    if (bytes != want) return dem_fail(dem, BPOSD_ERR_INVALID, "the last batch holds %zu bytes of item %d, not %zu", want, what, bytes);
    if (what == BPOSD_DEM_OBS_FAIL) {  // came down with the counters: no device call
        memcpy(host_dst, dem->h_counters.as<int>() + 8, want);
        return BPOSD_OK;
    }
    DeviceGuard guard(dem->cfg.device);
    DEM_TRY(dem, guard.err);
    DEM_TRY(dem, hipMemcpy(host_dst, src, want, hipMemcpyDeviceToHost));  // bposd_dem_sample / bposd_dem_run have waited for the batch
    return BPOSD_OK;
}

int64_t bposd_dem_device_bytes(bposd_dem* dem) { return dem ? (int64_t)dem->device_bytes : BPOSD_ERR_INVALID; }

int bposd_debug_dem_timing(bposd_dem* dem, double* sample_ms, double* score_ms) {
    if (!dem) return BPOSD_ERR_INVALID;
    if (dem->sampled_B == 0) return dem_fail(dem, BPOSD_ERR_INVALID, "no batch has run yet");
    DeviceGuard guard(dem->cfg.device);
    DEM_TRY(dem, guard.err);
    float ms = 0.f;
    if (sample_ms) {
        DEM_TRY(dem, hipEventElapsedTime(&ms, dem->ev_t[0], dem->ev_t[1]));
        *sample_ms = ms;
    }
    if (score_ms) {
        *score_ms = 0.0;
        if (dem->scored_B) {
            DEM_TRY(dem, hipEventElapsedTime(&ms, dem->ev_t[2], dem->ev_t[3]));
            *score_ms = ms;
        }
    }
    return BPOSD_OK;
}

}  // extern "C"
