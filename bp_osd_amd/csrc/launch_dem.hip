// launch_dem.hip -- the detector-error-model Monte-Carlo engine of libbposd_mi355x.so: bposd_dem_* of include/bposd_mi355x.h.
// One translation unit: both instances of dem_sample_kernel and dem_score_kernel (dem_kernels.hip.h) and dem_subset_kernel
// (dem_subset_kernel.hip.h) are instantiated here and nowhere else.  The harvest's kernels and fault_sums_kernel have units
// of their own (harvest.h).
//
// A batch is sample faults -> detectors and true observables -> one decode straight to observables -> compare -> five
// integers.  The engine owns every buffer of it and a stream of its own; the decode goes through the decoder's
// device-pointer observables call on the decoder's next lane.  The engine's stream and that lane are ordered against each
// other by events; the host waits once per batch, for the counters.  What it shares with the other engines is engine_common.h.
#include "dem_engine.h"
#include "dem_kernels.hip.h"
#include "dem_subset_kernel.hip.h"

using namespace bposd_dem_dev;

namespace {

int create_impl(bposd_dem* dem, const std::vector<int32_t>& col_ptr, const std::vector<int32_t>& col_bits, const double* priors) {
    int rc;
    if ((rc = engine_upload(dem, dem->d_priors, priors, (size_t)dem->N))) return rc;
    if ((rc = engine_upload(dem, dem->d_col_ptr, col_ptr.data(), col_ptr.size()))) return rc;
    if ((rc = engine_upload(dem, dem->d_col_bits, col_bits.data(), col_bits.size()))) return rc;
    const size_t C = (size_t)dem->capacity;
    if ((rc = engine_alloc(dem, dem->d_faults, C * dem->fw))) return rc;
    if ((rc = engine_alloc(dem, dem->d_detectors, C * dem->dw))) return rc;
    if ((rc = engine_alloc(dem, dem->d_observables, C * dem->ow))) return rc;
    if (dem->dec) {
        if ((rc = engine_alloc(dem, dem->d_obs_bp, C * dem->ow))) return rc;
        if ((rc = engine_alloc(dem, dem->d_obs_osd0, C * dem->ow))) return rc;
        if ((rc = engine_alloc(dem, dem->d_obs_osdw, C * dem->ow))) return rc;
        if ((rc = engine_alloc(dem, dem->d_flags, C))) return rc;
        if ((rc = engine_alloc(dem, dem->d_conv, C))) return rc;
        if ((rc = engine_alloc(dem, dem->d_iters, C))) return rc;
        if ((rc = dem->counters.alloc(dem, dem->k))) return rc;
    }
    if (dem->num_cu <= 0) {
        hipDeviceProp_t prop;
        ENGINE_TRY(dem, hipGetDeviceProperties(&prop, dem->device));
        dem->num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    }
    ENGINE_TRY(dem, hipStreamCreateWithFlags(&dem->stream.raw, hipStreamNonBlocking));
    for (Event* e : {&dem->ev_sampled, &dem->ev_decoded}) ENGINE_TRY(dem, hipEventCreateWithFlags(&e->raw, hipEventDisableTiming));
    for (Event& e : dem->ev_t) ENGINE_TRY(dem, hipEventCreate(&e.raw));
    return 0;
}

// two accumulator rows, and behind each the log-weight word of the weighted instance
size_t sample_lds_bytes(const bposd_dem* dem, bool weighted) {
    return 2 * sizeof(unsigned long long) * (size_t)(dem->dw + dem->ow + (weighted ? 1 : 0));
}

// every wave of a workgroup has a row of its own: accumulator words, then the fault words
size_t subset_lds_bytes(const bposd_dem* dem) { return DEM_WAVES * sizeof(unsigned long long) * (size_t)(dem->dw + dem->ow + dem->fw); }

// binom[(j - 1) * (n + 1) + c] = C(c, j) for j = 1 .. w and c = 0 .. n by Pascal's rule; an addition that overflows, and
// every sum it enters, is 2^64 - 1.  Returns C(n, w) (saturated likewise).
unsigned long long binomial_table(int n, int w, std::vector<unsigned long long>* out) {
    const unsigned long long SAT = ~0ull;
    const size_t cols = (size_t)n + 1;
    out->assign((size_t)w * cols, 0);
    for (int j = 1; j <= w; ++j) {
        unsigned long long* row = out->data() + (size_t)(j - 1) * cols;
        const unsigned long long* up = j > 1 ? row - cols : nullptr;  // C(., j - 1); row 0 is all ones
        for (int c = 1; c <= n; ++c) {
            const unsigned long long a = row[c - 1], b = up ? up[c - 1] : 1ull;
            unsigned long long sum;
            row[c] = (a == SAT || b == SAT || __builtin_add_overflow(a, b, &sum)) ? SAT : sum;
        }
    }
    return w == 0 ? 1ull : (*out)[(size_t)(w - 1) * cols + (size_t)n];
}

// dem_subset_kernel for rows [0, B) on the engine's stream, between ev_t[0] and ev_t[1]
int enqueue_subset(bposd_dem* dem, uint64_t first_shot, long long B) {
    if (dem->subset_mode == DEM_SUBSET_ENUMERATE && (first_shot > dem->subset_count || (unsigned long long)B > dem->subset_count - first_shot))
        return engine_fail(dem, BPOSD_ERR_INVALID, "ranks %llu .. %llu: there are only %llu sets of weight %d on %d faults", (unsigned long long)first_shot,
                           (unsigned long long)first_shot + (unsigned long long)B - 1, dem->subset_count, dem->subset_w, dem->subset_n);
    DemSubsetParams S{};
    S.B = B;
    S.first_shot = first_shot;
    S.key0 = (uint32_t)dem->cfg.seed;
    S.key1 = (uint32_t)(dem->cfg.seed >> 32);
    S.mode = dem->subset_mode;
    S.w = dem->subset_w;
    S.n = dem->subset_n;
    S.N = dem->N;
    S.fw = dem->fw;
    S.dw = dem->dw;
    S.ow = dem->ow;
    S.support = dem->d_support;
    S.binom = dem->d_binom;
    S.col_ptr = dem->d_col_ptr;
    S.col_bits = dem->d_col_bits;
    S.faults = dem->d_faults;
    S.detectors = dem->d_detectors;
    S.observables = dem->d_observables;
    S.incr = dem->subset_incr ? dem->d_subset_incr : nullptr;
    S.logw = dem->d_logw;
    const unsigned grid = (unsigned)std::min<long long>((B + DEM_WAVES - 1) / DEM_WAVES, (long long)dem->num_cu * 8);
    dem->logw_B = 0;
    ENGINE_TRY(dem, hipEventRecord(dem->ev_t[0], dem->stream));
    hipLaunchKernelGGL(dem_subset_kernel, dim3(grid), dim3(DEM_THREADS), subset_lds_bytes(dem), dem->stream, S);
    ENGINE_TRY(dem, hipGetLastError());
    ENGINE_TRY(dem, hipEventRecord(dem->ev_t[1], dem->stream));
    if (dem->subset_incr) dem->logw_B = B;
    return 0;
}

// the batch's sampler for rows [0, B) on the engine's stream, between ev_t[0] and ev_t[1]: dem_subset_kernel while a subset
// mode is on, else the dem_sample_kernel instance of the engine's mode
int enqueue_sample(bposd_dem* dem, uint64_t first_shot, long long B) {
    if (dem->subset_mode) return enqueue_subset(dem, first_shot, B);
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
    ENGINE_TRY(dem, hipEventRecord(dem->ev_t[0], dem->stream));
    if (dem->weighted)
        hipLaunchKernelGGL(dem_sample_kernel<true>, dim3(grid), dim3(DEM_THREADS), sample_lds_bytes(dem, true), dem->stream, S);
    else
        hipLaunchKernelGGL(dem_sample_kernel<false>, dim3(grid), dim3(DEM_THREADS), sample_lds_bytes(dem, false), dem->stream, S);
    ENGINE_TRY(dem, hipGetLastError());
    ENGINE_TRY(dem, hipEventRecord(dem->ev_t[1], dem->stream));
    if (dem->weighted) dem->logw_B = B;
    return 0;
}

// bposd_dem_fault_sums and its debug twin behind their checks: the multipliers go up, the kernel runs on the rows the job
// names, the host waits and the arrays come down -- 4 n_mult bytes up, 8 N or 16 N down.
int fault_sums_run(bposd_dem* dem, FaultSumsJob job, const uint32_t* mult, uint64_t* counts, uint64_t* sums) {
    int rc;
    if ((rc = bposd_host::fault_sums_ensure(dem, dem->fs, dem->N))) return rc;
    hipStream_t st = dem->stream;
    job.N = dem->N;
    job.fw = dem->fw;
    job.faults = dem->d_faults;
    job.weighted = mult != nullptr;
    if (mult && job.rows) ENGINE_TRY(dem, hipMemcpyAsync(dem->fs.d_mult, mult, sizeof(uint32_t) * (size_t)job.rows, hipMemcpyHostToDevice, st));
    if ((rc = bposd_host::fault_sums_enqueue(dem, dem->fs, job))) {
        (void)hipStreamSynchronize(st);
        return rc;
    }
    ENGINE_TRY(dem, hipMemcpyAsync(counts, dem->fs.d_counts, 8 * (size_t)dem->N, hipMemcpyDeviceToHost, st));
    if (sums) ENGINE_TRY(dem, hipMemcpyAsync(sums, dem->fs.d_sums, 8 * (size_t)dem->N, hipMemcpyDeviceToHost, st));
    ENGINE_TRY(dem, hipStreamSynchronize(st));
    return BPOSD_OK;
}

}  // namespace

int bposd_host::dem_sample_async(bposd_dem* dem, uint64_t first_shot, int64_t B, hipStream_t waiter) {
    if (const int rc = engine_check_batch(dem, B)) return rc;
    DeviceGuard guard(dem->device);
    ENGINE_TRY(dem, guard.err);
    dem->sampled_B = dem->scored_B = 0;
    dem->hv.last_on = false;
    if (const int rc = enqueue_sample(dem, first_shot, B)) return rc;
    ENGINE_TRY(dem, hipEventRecord(dem->ev_sampled, dem->stream));
    ENGINE_TRY(dem, hipStreamWaitEvent(waiter, dem->ev_sampled, 0));
    dem->sampled_B = B;
    return BPOSD_OK;
}

extern "C" {

const char* bposd_dem_last_error(bposd_dem* dem) { return dem ? dem->err.c_str() : bposd_last_error(nullptr); }

void bposd_dem_destroy(bposd_dem* dem) { engine_destroy(dem); }

int bposd_dem_tables(const int32_t* h_indptr, const int32_t* h_indices, int32_t M, const int32_t* l_indptr, const int32_t* l_indices,
                     int32_t k, int32_t N, int32_t* col_ptr, int32_t* col_bits) {
    std::string why;
    if (const int rc = bposd_host::dem_tables(h_indptr, h_indices, M, l_indptr, l_indices, k, N, col_ptr, col_bits, &why))
        return engine_fail(nullptr, rc, "%s", why.c_str());
    return BPOSD_OK;
}

int bposd_dem_create(const bposd_dem_config* cfg, bposd_handle* dec, const int32_t* h_indptr, const int32_t* h_indices, int32_t M,
                     const int32_t* l_indptr, const int32_t* l_indices, int32_t k, int32_t N, const double* priors, bposd_dem** out) {
    if (!out) return engine_fail(nullptr, BPOSD_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!cfg) return engine_fail(nullptr, BPOSD_ERR_INVALID, "config is required");
    if (cfg->capacity < 1 || cfg->capacity > 0x7fffffffLL) return engine_fail(nullptr, BPOSD_ERR_INVALID, "capacity %lld out of range", (long long)cfg->capacity);
    std::string why;
    std::vector<int32_t> col_ptr, col_bits;  // (validates H, L and k)
    if (const int rc = bposd_host::stacked_csc(h_indptr, h_indices, M, l_indptr, l_indices, k, N, &col_ptr, &col_bits, &why))
        return engine_fail(nullptr, rc, "%s", why.c_str());
    if (!priors) return engine_fail(nullptr, BPOSD_ERR_INVALID, "priors are required");
    if (const int64_t bad = bposd_host::first_bad_prob(priors, N))
        return engine_fail(nullptr, BPOSD_ERR_INVALID, "the prior of fault %d (%g) is not a probability", (int)bad - 1, priors[bad - 1]);
    if (dec && dec->device != cfg->device)
        return engine_fail(nullptr, BPOSD_ERR_INVALID, "the decoder lives on device %d, the engine on device %d", dec->device, cfg->device);
    if (dec && (dec->m != M || dec->n != N))
        return engine_fail(nullptr, BPOSD_ERR_INVALID, "decoder shape %d x %d does not match the model's %d detectors x %d faults", dec->m, dec->n, M, N);

    std::unique_ptr<bposd_dem, decltype(&bposd_dem_destroy)> owner(new bposd_dem(), bposd_dem_destroy);
    bposd_dem* const dem = owner.get();
    dem->cfg = *cfg;
    dem->device = cfg->device;
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
        return engine_fail(nullptr, BPOSD_ERR_UNSUPPORTED, "%d detectors and %d observables need %zu bytes of LDS per workgroup, more than 65536", M, k,
                        sample_lds_bytes(dem, false));
    int rc = 0;
    std::vector<uint64_t> table;
    if (dec) {  // (validated before anything is allocated)
        table.resize((size_t)dem->fw * k);
        if ((rc = bposd_host::observable_table(l_indptr, l_indices, k, N, table.data(), &why))) return engine_fail(nullptr, rc, "%s", why.c_str());
    }
    if ((rc = engine_create_on_device(dem, [&] { return create_impl(dem, col_ptr, col_bits, priors); }))) return rc;
    // Last, once nothing of the engine's own can fail any more: the L that scores is the L the decoder multiplies by.  A
    // create that fails leaves the caller's decoder as it was.
    if (dec && (rc = bposd_set_observables(dec, table.data(), k))) return engine_fail(nullptr, rc, "bposd_set_observables: %s", bposd_last_error(dec));
    *out = owner.release();
    return BPOSD_OK;
}

int bposd_dem_set_sampling(bposd_dem* dem, const double* sample_priors, const int64_t* incr) {
    if (!dem) return BPOSD_ERR_INVALID;
    if ((sample_priors == nullptr) != (incr == nullptr))
        return engine_fail(dem, BPOSD_ERR_INVALID, "sample_priors and incr go together: give both, or NULL for both to sample plainly");
    if (!sample_priors) {  // back to the model's own priors; the tables stay allocated for the next switch
        dem->weighted = false;
        if (!dem->subset_mode) dem->logw_B = 0;
        return BPOSD_OK;
    }
    if (dem->subset_mode)
        return engine_fail(dem, BPOSD_ERR_INVALID, "the engine draws fault sets of a fixed weight (bposd_dem_set_subset): switch that off before weighted sampling");
    // everything is validated before anything changes: a refusal leaves the engine in the mode it was in
    if (const int64_t bad = bposd_host::first_bad_prob(sample_priors, dem->N))
        return engine_fail(dem, BPOSD_ERR_INVALID, "the sampling probability of fault %d (%g) is not a probability", (int)bad - 1, sample_priors[bad - 1]);
    unsigned long long total = 0;  // sum of |incr|: every term and the running sum stay below 2^63
    for (int i = 0; i < dem->N; ++i) {
        const unsigned long long a = incr[i] < 0 ? 0ull - (unsigned long long)incr[i] : (unsigned long long)incr[i];
        if (a >= (1ull << 62) || (total += a) >= (1ull << 62))
            return engine_fail(dem, BPOSD_ERR_INVALID, "the increments up to fault %d sum to 2^62 or more in magnitude: a shot's log-weight could overflow", i);
    }
    if (sample_lds_bytes(dem, true) > 64 * 1024)
        return engine_fail(dem, BPOSD_ERR_UNSUPPORTED, "weighted sampling needs %zu bytes of LDS per workgroup, more than 65536", sample_lds_bytes(dem, true));
    DeviceGuard guard(dem->device);
    ENGINE_TRY(dem, guard.err);
    ENGINE_TRY(dem, hipStreamSynchronize(dem->stream));  // no sampler is reading the tables
    int rc;
    if (!dem->d_sample_priors.p && (rc = engine_alloc(dem, dem->d_sample_priors, (size_t)dem->N))) return rc;
    if (!dem->d_incr.p && (rc = engine_alloc(dem, dem->d_incr, (size_t)dem->N))) return rc;
    if (!dem->d_logw.p && (rc = engine_alloc(dem, dem->d_logw, (size_t)dem->capacity))) return rc;
    dem->weighted = false;  // (until both tables are the new ones)
    dem->logw_B = 0;        // what item 10 held was summed from the table that goes
    ENGINE_TRY(dem, hipMemcpy(dem->d_sample_priors, sample_priors, sizeof(double) * (size_t)dem->N, hipMemcpyHostToDevice));
    ENGINE_TRY(dem, hipMemcpy(dem->d_incr, incr, sizeof(int64_t) * (size_t)dem->N, hipMemcpyHostToDevice));
    dem->weighted = true;
    return BPOSD_OK;
}

int bposd_dem_set_subset(bposd_dem* dem, int32_t mode, int32_t weight, const int32_t* support, int32_t n_support, const int64_t* incr) {
    if (!dem) return BPOSD_ERR_INVALID;
    if (mode == BPOSD_DEM_SUBSET_OFF) {  // back to Bernoulli rows; the tables stay until the next switch replaces them
        if (dem->subset_mode) dem->logw_B = 0;
        dem->subset_mode = 0;
        return BPOSD_OK;
    }
    // everything is validated before anything changes: a refusal leaves the engine in the mode it was in
    if (mode != BPOSD_DEM_SUBSET_ENUMERATE && mode != BPOSD_DEM_SUBSET_RANDOM)
        return engine_fail(dem, BPOSD_ERR_INVALID, "mode = %d is not BPOSD_DEM_SUBSET_OFF, _ENUMERATE or _RANDOM", mode);
    if (dem->weighted)
        return engine_fail(dem, BPOSD_ERR_INVALID, "weighted sampling is on (bposd_dem_set_sampling): switch that off before drawing fault sets of a fixed weight");
    const int n = support ? n_support : dem->N;
    if (n < 0 || n > dem->N) return engine_fail(dem, BPOSD_ERR_INVALID, "n_support = %d is outside [0, %d]", n, dem->N);
    for (int c = 0; support && c < n; ++c) {
        if (support[c] < 0 || support[c] >= dem->N)
            return engine_fail(dem, BPOSD_ERR_INVALID, "support[%d] = %d is outside [0, %d)", c, support[c], dem->N);
        if (c && support[c] <= support[c - 1])
            return engine_fail(dem, BPOSD_ERR_INVALID, "support[%d] = %d does not ascend strictly (support[%d] = %d)", c, support[c], c - 1, support[c - 1]);
    }
    if (weight < 0 || weight > std::min(n, DEM_SUBSET_MAX_WEIGHT))
        return engine_fail(dem, BPOSD_ERR_INVALID, "weight = %d is outside [0, min(n = %d, %d)]", weight, n, DEM_SUBSET_MAX_WEIGHT);
    std::vector<unsigned long long> binom;
    unsigned long long count = 0;
    if (mode == BPOSD_DEM_SUBSET_ENUMERATE) {
        count = binomial_table(n, weight, &binom);
        if (count >= (1ull << 63))
            return engine_fail(dem, BPOSD_ERR_INVALID, "C(%d, %d) is 2^63 or more: the sets of weight %d cannot be enumerated by a 63-bit rank", n, weight, weight);
    }
    if (incr)
        for (int c = 0; c < n; ++c) {
            const int i = support ? support[c] : c;
            const unsigned long long a = incr[i] < 0 ? 0ull - (unsigned long long)incr[i] : (unsigned long long)incr[i];
            if (weight && a >= ((1ull << 62) + weight - 1) / weight)  // weight * a >= 2^62
                return engine_fail(dem, BPOSD_ERR_INVALID, "%d times the increment of fault %d is 2^62 or more in magnitude: a shot's log-weight could overflow", weight, i);
        }
    if (subset_lds_bytes(dem) > 64 * 1024)
        return engine_fail(dem, BPOSD_ERR_UNSUPPORTED, "fault sets of a fixed weight need %zu bytes of LDS per workgroup, more than 65536", subset_lds_bytes(dem));
    DeviceGuard guard(dem->device);
    ENGINE_TRY(dem, guard.err);
    ENGINE_TRY(dem, hipStreamSynchronize(dem->stream));  // no sampler is reading the tables
    // the new block is whole before the engine changes: binomials, increments, support, each from a 256-byte boundary
    auto pad = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t b_binom = pad(8 * binom.size()), b_incr = pad(incr ? 8 * (size_t)dem->N : 0), b_supp = pad(4 * (size_t)n);
    std::vector<int32_t> ident;
    if (!support) {
        ident.resize((size_t)n);
        for (int c = 0; c < n; ++c) ident[c] = c;
        support = ident.data();
    }
    DevBuf fresh;
    ENGINE_TRY(dem, fresh.alloc(std::max<size_t>(b_binom + b_incr + b_supp, 256)));
    char* const base = (char*)fresh.p;
    if (!binom.empty()) ENGINE_TRY(dem, hipMemcpy(base, binom.data(), 8 * binom.size(), hipMemcpyHostToDevice));
    if (incr) ENGINE_TRY(dem, hipMemcpy(base + b_binom, incr, 8 * (size_t)dem->N, hipMemcpyHostToDevice));
    if (n) ENGINE_TRY(dem, hipMemcpy(base + b_binom + b_incr, support, 4 * (size_t)n, hipMemcpyHostToDevice));
    int rc;
    if (incr && !dem->d_logw.p && (rc = engine_alloc(dem, dem->d_logw, (size_t)dem->capacity))) return rc;
    dem->device_bytes -= dem->subset_block.bytes;
    dem->device_bytes += fresh.bytes;
    dem->subset_block = std::move(fresh);  // (what the engine held goes with `fresh`)
    dem->d_binom = (const unsigned long long*)base;
    dem->d_subset_incr = (const long long*)(base + b_binom);
    dem->d_support = (const int*)(base + b_binom + b_incr);
    dem->subset_mode = mode;
    dem->subset_w = weight;
    dem->subset_n = n;
    dem->subset_count = count;
    dem->subset_incr = incr != nullptr;
    dem->logw_B = 0;  // what item 10 held was summed from a table that went
    return BPOSD_OK;
}

int bposd_dem_sample(bposd_dem* dem, uint64_t first_shot, int64_t B) {
    if (!dem) return BPOSD_ERR_INVALID;
    if (const int rc = engine_check_batch(dem, B)) return rc;
    DeviceGuard guard(dem->device);
    ENGINE_TRY(dem, guard.err);
    dem->sampled_B = dem->scored_B = 0;
    dem->hv.last_on = false;
    if (const int rc = enqueue_sample(dem, first_shot, B)) return rc;
    ENGINE_TRY(dem, hipStreamSynchronize(dem->stream));
    dem->sampled_B = B;
    return BPOSD_OK;
}

int bposd_dem_set_harvest(bposd_dem* dem, int64_t max_rows) {
    if (!dem) return BPOSD_ERR_INVALID;
    if (!dem->dec) return engine_fail(dem, BPOSD_ERR_INVALID, "this engine was created without a decoder: it has no failing shots to harvest");
    return bposd_host::harvest_set(dem, dem->hv, max_rows, dem->fw);
}

int bposd_dem_harvest_info(bposd_dem* dem, int64_t out[3]) {
    if (!dem) return BPOSD_ERR_INVALID;
    if (!out) return engine_fail(dem, BPOSD_ERR_INVALID, "out is NULL");
    if (!dem->hv.last_on) return engine_fail(dem, BPOSD_ERR_INVALID, "the last batch ran with the harvest off (bposd_dem_set_harvest)");
    std::copy(dem->hv.info, dem->hv.info + 3, out);
    return BPOSD_OK;
}

int bposd_dem_run(bposd_dem* dem, uint64_t first_shot, int64_t B, int64_t counters[5]) {
    if (!dem) return BPOSD_ERR_INVALID;
    if (!dem->dec) return engine_fail(dem, BPOSD_ERR_INVALID, "this engine was created without a decoder: it samples only (bposd_dem_sample)");
    if (!counters) return engine_fail(dem, BPOSD_ERR_INVALID, "counters is NULL");
    if (const int rc = engine_check_batch(dem, B)) return rc;
    bposd_handle* const dec = dem->dec;
    if (dec->obs_k != dem->k)
        return engine_fail(dem, BPOSD_ERR_INVALID, "the decoder's observable table (k = %d) is no longer the one this engine set (k = %d)", dec->obs_k, dem->k);
    DeviceGuard guard(dem->device);
    ENGINE_TRY(dem, guard.err);
    dem->sampled_B = dem->scored_B = 0;
    dem->hv.last_on = false;

    int rc;
    if ((rc = enqueue_sample(dem, first_shot, B))) return rc;
    ENGINE_TRY(dem, hipEventRecord(dem->ev_sampled, dem->stream));
    ENGINE_TRY(dem, dem->counters.reset(dem->stream));

    // the decode on the decoder's next lane, ordered behind the sampler; ev_decoded is recorded on that lane behind the call
    rc = decode_behind(dem, dec, dem->ev_sampled, dem->ev_decoded, [&] {
        return bposd_decode_batch_observables_device(dec, dem->d_detectors, /*syndromes_packed=*/1, B, (uint64_t*)dem->d_obs_osdw.p, (uint64_t*)dem->d_obs_osd0.p,
                                                     (uint64_t*)dem->d_obs_bp.p, dem->d_conv, dem->d_iters);
    });
    if (rc) return rc;
    ENGINE_TRY(dem, hipStreamWaitEvent(dem->stream, dem->ev_decoded, 0));

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
    Q.counters = dem->counters.d_counters;
    Q.obs_fail = dem->counters.d_obs_fail;
    const unsigned grid = (unsigned)std::min<long long>((B + DEM_SCORE_THREADS - 1) / DEM_SCORE_THREADS, (long long)dem->num_cu * 8);
    ENGINE_TRY(dem, hipEventRecord(dem->ev_t[2], dem->stream));
    hipLaunchKernelGGL(dem_score_kernel, dim3(grid), dim3(DEM_SCORE_THREADS), 0, dem->stream, Q);
    ENGINE_TRY(dem, hipGetLastError());
    ENGINE_TRY(dem, hipEventRecord(dem->ev_t[3], dem->stream));
    const bool harvest = dem->hv.on();
    if (harvest) {
        // The osdw rows are the ones the decode left in its lane's buffers.  The engine's stream is behind ev_decoded, so
        // they are final, and they stay: this call ends in its host wait before anything else can be queued on that lane.
        const bposd_host::ObsRows rows = bposd_host::last_obs_rows(dec);
        const HarvestJob job{B, dem->N, dem->fw, /*flag_mask=*/4, /*flag_want=*/4, dem->d_flags, dem->d_faults, rows.osdw, rows.packed};
        if ((rc = bposd_host::harvest_enqueue(dem, dem->hv, job, dem->counters.d_counters))) {
            (void)hipStreamSynchronize(dem->stream);
            return rc;
        }
    }
    ENGINE_TRY(dem, dem->counters.download(dem->stream, harvest ? 8 : 5));
    ENGINE_TRY(dem, hipStreamSynchronize(dem->stream));  // the batch's one host wait
    dem->counters.read(counters, 5);
    if (harvest) bposd_host::harvest_read(dem->hv, dem->counters.h_counters.as<int>());
    dem->sampled_B = dem->scored_B = B;
    return BPOSD_OK;
}

int bposd_dem_fetch(bposd_dem* dem, int32_t what, void* host_dst, size_t bytes) {
    if (!dem) return BPOSD_ERR_INVALID;
    // the engine's own preconditions (for a batch that has run: engine_fetch refuses where none has)
    if (what == BPOSD_DEM_LOGW && dem->subset_mode && !dem->subset_incr)
        return engine_fail(dem, BPOSD_ERR_INVALID, "item %d needs an increment table: bposd_dem_set_subset was given none", what);
    if (what == BPOSD_DEM_LOGW && !dem->weighted && !dem->subset_mode)
        return engine_fail(dem, BPOSD_ERR_INVALID, "item %d needs weighted sampling (bposd_dem_set_sampling): this engine samples plainly", what);
    if (what == BPOSD_DEM_LOGW && dem->logw_B != dem->sampled_B)
        return engine_fail(dem, BPOSD_ERR_INVALID, "item %d needs a batch sampled since bposd_dem_set_sampling / bposd_dem_set_subset", what);
    if (what >= BPOSD_DEM_OBS_BP && what <= BPOSD_DEM_OBS_FAIL && dem->sampled_B && dem->scored_B == 0)
        return engine_fail(dem, BPOSD_ERR_INVALID, "item %d needs bposd_dem_run: the last batch was sampled only", what);
    if (what >= BPOSD_DEM_FAIL_ROWS && what <= BPOSD_DEM_MIN_RESIDUAL && !dem->hv.last_on)
        return engine_fail(dem, BPOSD_ERR_INVALID, "item %d needs a batch that ran with the harvest on (bposd_dem_set_harvest)", what);
    const size_t fw = 8 * (size_t)dem->fw, dw = 8 * (size_t)dem->dw, ow = 8 * (size_t)dem->ow;
    FetchItem items[16] = {{dem->d_faults, fw, false},   {dem->d_detectors, dw, false}, {dem->d_observables, ow, false},
                               {dem->d_obs_bp, ow, false},   {dem->d_obs_osd0, ow, false},  {dem->d_obs_osdw, ow, false},
                               {dem->d_flags, 1, false},     {dem->d_conv, 1, false},       {dem->d_iters, sizeof(int32_t), false},
                               {nullptr, sizeof(int32_t) * (size_t)dem->k, true},           {dem->d_logw, sizeof(int64_t), false}};
    bposd_host::harvest_items(dem->hv, dem->fw, items + 11);
    return engine_fetch(dem, items, 16, BPOSD_DEM_FAULTS, "BPOSD_DEM_FAULTS .. BPOSD_DEM_MIN_RESIDUAL", what, dem->sampled_B, dem->counters.obs_fail(),
                        host_dst, bytes);
}

int bposd_dem_fault_sums(bposd_dem* dem, int32_t select, const uint32_t* mult, int64_t n_mult, uint64_t* counts, uint64_t* sums) {
    if (!dem) return BPOSD_ERR_INVALID;
    // everything is validated before anything is allocated or queued: a refusal leaves the engine as it was
    if (select != BPOSD_DEM_SELECT_ALL && select != BPOSD_DEM_SELECT_FAILING)
        return engine_fail(dem, BPOSD_ERR_INVALID, "select = %d is not BPOSD_DEM_SELECT_ALL or BPOSD_DEM_SELECT_FAILING", select);
    if (dem->sampled_B == 0) return engine_fail(dem, BPOSD_ERR_INVALID, "no batch has run yet");
    if (select == BPOSD_DEM_SELECT_FAILING && !dem->hv.last_on)
        return engine_fail(dem, BPOSD_ERR_INVALID, "BPOSD_DEM_SELECT_FAILING needs a batch that ran with the harvest on (bposd_dem_set_harvest)");
    if (!counts) return engine_fail(dem, BPOSD_ERR_INVALID, "counts is NULL");
    if ((mult == nullptr) != (sums == nullptr))
        return engine_fail(dem, BPOSD_ERR_INVALID, "mult and sums go together: give both, or NULL for both to count only");
    const long long rows = select == BPOSD_DEM_SELECT_ALL ? dem->sampled_B : (long long)dem->hv.info[0];
    if (mult && n_mult != rows)
        return engine_fail(dem, BPOSD_ERR_INVALID, "n_mult = %lld, but the last batch has %lld %s", (long long)n_mult, rows,
                           select == BPOSD_DEM_SELECT_ALL ? "shots" : "failing shots");
    DeviceGuard guard(dem->device);
    ENGINE_TRY(dem, guard.err);
    FaultSumsJob job{};
    job.rows = rows;
    if (select == BPOSD_DEM_SELECT_FAILING) {  // the list harvest_list_kernel left, and its count: nothing is listed again
        job.list = dem->hv.d_list;
        job.count = bposd_host::harvest_count(dem->hv);
    }
    return fault_sums_run(dem, job, mult, counts, sums);
}

int64_t bposd_dem_device_bytes(bposd_dem* dem) { return dem ? (int64_t)dem->device_bytes : BPOSD_ERR_INVALID; }

int bposd_debug_dem_timing(bposd_dem* dem, double* sample_ms, double* score_ms) {
    if (!dem) return BPOSD_ERR_INVALID;
    if (dem->sampled_B == 0) return engine_fail(dem, BPOSD_ERR_INVALID, "no batch has run yet");
    DeviceGuard guard(dem->device);
    ENGINE_TRY(dem, guard.err);
    float ms = 0.f;
    if (sample_ms) {
        ENGINE_TRY(dem, hipEventElapsedTime(&ms, dem->ev_t[0], dem->ev_t[1]));
        *sample_ms = ms;
    }
    if (score_ms) {
        *score_ms = 0.0;
        if (dem->scored_B) {
            ENGINE_TRY(dem, hipEventElapsedTime(&ms, dem->ev_t[2], dem->ev_t[3]));
            *score_ms = ms;
        }
    }
    return BPOSD_OK;
}

int bposd_debug_dem_harvest(bposd_dem* dem, const uint64_t* fault_words, const void* corrections, int32_t packed, const uint8_t* select, int64_t B) {
    if (!dem) return BPOSD_ERR_INVALID;
    if (!dem->hv.on()) return engine_fail(dem, BPOSD_ERR_INVALID, "the harvest is off (bposd_dem_set_harvest)");
    if (!fault_words || !corrections || !select) return engine_fail(dem, BPOSD_ERR_INVALID, "fault rows, corrections and select are required");
    if (const int rc = engine_check_batch(dem, B)) return rc;
    DeviceGuard guard(dem->device);
    ENGINE_TRY(dem, guard.err);
    dem->sampled_B = dem->scored_B = dem->logw_B = 0;
    dem->hv.last_on = false;
    const size_t rows = (size_t)B;
    const size_t corr_bytes = packed ? 8 * rows * dem->fw : rows * (size_t)dem->N;
    std::vector<uint8_t> flags(rows);
    for (size_t b = 0; b < rows; ++b) flags[b] = select[b] ? 4 : 0;  // what dem_score_kernel leaves for an osdw failure
    DevBuf d_corr;  // (the engine has no correction rows of its own: a batch reads the decoder's)
    int rc;
    if ((rc = engine_alloc_bytes(nullptr, d_corr, corr_bytes))) return engine_fail(dem, rc, "%s", bposd_last_error(nullptr));
    ENGINE_TRY(dem, hipStreamSynchronize(dem->stream));
    ENGINE_TRY(dem, hipMemcpy(dem->d_faults, fault_words, 8 * rows * dem->fw, hipMemcpyHostToDevice));
    ENGINE_TRY(dem, hipMemcpy(dem->d_flags, flags.data(), rows, hipMemcpyHostToDevice));
    ENGINE_TRY(dem, hipMemcpy(d_corr.p, corrections, corr_bytes, hipMemcpyHostToDevice));
    ENGINE_TRY(dem, dem->counters.reset(dem->stream));
    const HarvestJob job{B, dem->N, dem->fw, 4, 4, dem->d_flags, dem->d_faults, d_corr.p, packed != 0};
    rc = bposd_host::harvest_enqueue(dem, dem->hv, job, dem->counters.d_counters);
    if (!rc) {
        const hipError_t err = dem->counters.download(dem->stream, 8);
        if (err != hipSuccess) rc = engine_fail(dem, BPOSD_ERR_HIP, "the counters' download failed: %s", hipGetErrorString(err));
    }
    const hipError_t waited = hipStreamSynchronize(dem->stream);  // (before d_corr goes)
    if (rc) return rc;
    ENGINE_TRY(dem, waited);
    bposd_host::harvest_read(dem->hv, dem->counters.h_counters.as<int>());
    // Items 0 and 11 .. 15 hold this call's rows.  scored_B stays 0 on purpose: the call has overwritten the engine's flag
    // bytes with the stand-in for `select` and decoded nothing, so bposd_dem_fetch must go on refusing the flags and every
    // other decoded item (3 .. 9) until a batch has run.
    dem->sampled_B = B;
    return BPOSD_OK;
}

int bposd_debug_dem_harvest_timing(bposd_dem* dem, double* harvest_ms) {
    if (!dem) return BPOSD_ERR_INVALID;
    if (!harvest_ms) return engine_fail(dem, BPOSD_ERR_INVALID, "harvest_ms is NULL");
    if (!dem->hv.last_on) return engine_fail(dem, BPOSD_ERR_INVALID, "the last batch ran with the harvest off (bposd_dem_set_harvest)");
    DeviceGuard guard(dem->device);
    ENGINE_TRY(dem, guard.err);
    float ms = 0.f;
    ENGINE_TRY(dem, hipEventElapsedTime(&ms, dem->hv.ev_t[0], dem->hv.ev_t[1]));
    *harvest_ms = ms;
    return BPOSD_OK;
}

int bposd_debug_dem_fault_sums(bposd_dem* dem, const uint64_t* fault_words, const uint8_t* select_bytes, const uint32_t* mult, int64_t B,
                               uint64_t* counts, uint64_t* sums) {
    if (!dem) return BPOSD_ERR_INVALID;
    if (!fault_words || !counts) return engine_fail(dem, BPOSD_ERR_INVALID, "fault rows and counts are required");
    if ((mult == nullptr) != (sums == nullptr))
        return engine_fail(dem, BPOSD_ERR_INVALID, "mult and sums go together: give both, or NULL for both to count only");
    if (select_bytes && !dem->hv.on()) return engine_fail(dem, BPOSD_ERR_INVALID, "select bytes need the harvest's list: the harvest is off (bposd_dem_set_harvest)");
    if (const int rc = engine_check_batch(dem, B)) return rc;
    DeviceGuard guard(dem->device);
    ENGINE_TRY(dem, guard.err);
    dem->sampled_B = dem->scored_B = dem->logw_B = 0;
    dem->hv.last_on = false;
    const size_t rows = (size_t)B;
    FaultSumsJob job{};
    job.rows = B;
    ENGINE_TRY(dem, hipStreamSynchronize(dem->stream));
    ENGINE_TRY(dem, hipMemcpy(dem->d_faults, fault_words, 8 * rows * dem->fw, hipMemcpyHostToDevice));
    if (select_bytes) {
        std::vector<uint8_t> flags(rows);
        long long listed = 0;
        for (size_t b = 0; b < rows; ++b) listed += (flags[b] = select_bytes[b] ? 4 : 0) != 0;  // what dem_score_kernel leaves for an osdw failure
        ENGINE_TRY(dem, hipMemcpy(dem->d_flags, flags.data(), rows, hipMemcpyHostToDevice));
        const HarvestJob list{B, dem->N, dem->fw, 4, 4, dem->d_flags, dem->d_faults, nullptr, true};
        if (const int rc = bposd_host::harvest_list_enqueue(dem, dem->hv, list)) {
            (void)hipStreamSynchronize(dem->stream);
            return rc;
        }
        job.rows = listed;
        job.list = dem->hv.d_list;
        job.count = bposd_host::harvest_count(dem->hv);
    }
    if (const int rc = fault_sums_run(dem, job, mult, counts, sums)) return rc;
    dem->sampled_B = B;  // item 0 holds this call's rows; nothing was decoded (scored_B stays 0, as after bposd_debug_dem_harvest)
    return BPOSD_OK;
}

int bposd_debug_dem_fault_sums_timing(bposd_dem* dem, double* sums_ms) {
    if (!dem) return BPOSD_ERR_INVALID;
    if (!sums_ms) return engine_fail(dem, BPOSD_ERR_INVALID, "sums_ms is NULL");
    if (!dem->fs.timed) return engine_fail(dem, BPOSD_ERR_INVALID, "no fault_sums_kernel has run since the engine's last batch selected a row");
    DeviceGuard guard(dem->device);
    ENGINE_TRY(dem, guard.err);
    float ms = 0.f;
    ENGINE_TRY(dem, hipEventElapsedTime(&ms, dem->fs.ev_t[0], dem->fs.ev_t[1]));
    *sums_ms = ms;
    return BPOSD_OK;
}

}  // extern "C"
