// launch_window.hip -- the sliding-window engine of libbposd_mi355x.so: bposd_window_* of include/bposd_mi355x.h.
// One translation unit: window_step_kernel and window_score_kernel (window_kernels.hip.h) are instantiated here and nowhere else.
//
// A batch is nwin + 1 step kernels with a decode between every two of them: step w commits window w - 1 and gathers the
// syndrome of window w, window w's decoder takes that syndrome through its plain device-pointer call on its next lane, and
// the engine's stream and that lane are ordered against each other by events (decode_behind of engine_common.h).  The engine
// owns the tables of every step and the rows of a batch; the decoders stay the caller's.  The host waits once per
// Monte-Carlo batch, for the counters.
#include "dem_engine.h"
#include "window_kernels.hip.h"

using namespace bposd_window_dev;
using bposd_host::native_packed;

namespace {

// One step on the host: the commit list of the previous window, the gather list of the next, and what follows from them.
struct StepPlan {
    std::vector<int> pos, fault, slot, corr_words, gather;
    int w_lo = 0, w_hi = 0;
    int decoded_cols = 0;  // columns of the decoded row the commit list indexes
    // the word range the committed columns touch or the gather reads, and the correction words of the commit list (faults ascend)
    void finish(const std::vector<int32_t>& col_ptr, const std::vector<int32_t>& col_bits, int dw) {
        int lo = dw, hi = 0;
        for (const int f : fault)
            for (int e = col_ptr[f]; e < col_ptr[f + 1]; ++e)
                if (col_bits[e] < 64 * dw) {
                    lo = std::min(lo, col_bits[e] >> 6);
                    hi = std::max(hi, (col_bits[e] >> 6) + 1);
                }
        for (const int d : gather) {
            lo = std::min(lo, d >> 6);
            hi = std::max(hi, (d >> 6) + 1);
        }
        w_lo = hi > lo ? lo : 0;
        w_hi = hi > lo ? hi : 0;
        slot.clear();
        corr_words.clear();
        for (const int f : fault) {
            if (corr_words.empty() || corr_words.back() != (f >> 6)) corr_words.push_back(f >> 6);
            slot.push_back((int)corr_words.size() - 1);
        }
    }
};

struct StepDev {  // where a step's lists start in the engine's device tables
    size_t commit = 0, corr = 0, gather = 0;
};

}  // namespace

struct bposd_window : EngineBase {
    bposd_window_config cfg{};
    int M = 0, N = 0, k = 0, dw = 0, ow = 0, fw = 0, nwin = 0;
    long long run_B = 0;      // rows of the last bposd_window_run that bposd_window_fetch holds
    bool timed_steps = false, timed_score = false;
    std::vector<bposd_handle*> decs;  // [nwin], the caller's
    std::vector<int> n_det, n_fault;  // [nwin]
    std::vector<char> packed;         // [nwin]: the decoder's kernels took packed rows when the engine was made (the row buffers are sized for that form)
    std::vector<StepPlan> steps;      // [nwin + 1] (lists are kept for the launch parameters' counts)
    std::vector<StepDev> at;          // [nwin + 1]
    std::vector<Event> ev_step, ev_decoded;  // [nwin]: the syndrome of window w is gathered / its rows are decoded
    std::vector<Event> ev_t;                 // 2 (nwin + 1) around the step kernels, 2 around the scorer (bposd_debug_window_timing)
    // device tables
    DevArray<int> d_col_ptr, d_col_bits;
    DevArray<int> d_commit_pos, d_commit_fault, d_commit_slot, d_corr_words, d_gather;
    // per-batch buffers (capacity rows)
    DevArray<unsigned long long> d_running, d_obs, d_truth, d_corr;
    DevBuf d_synd, d_dec;  // the current window's syndrome and decoded rows, in its decoder's form
    DevArray<uint8_t> d_conv_all, d_wconv, d_flags;
    DevArray<int> d_iters, d_witers;
    CounterBlock counters;  // 4 counters; with the harvest on, ints 5 .. 7 hold its triple
    Harvest hv;             // bposd_window_set_harvest (harvest.h)
};

namespace {

int upload(EngineBase* e, DevArray<int>& p, const std::vector<int>& v) { return engine_upload(e, p, v.data(), v.size()); }

size_t row_bytes(int cols, bool packed) { return packed ? 8 * (size_t)((cols + 63) / 64) : (size_t)cols; }

size_t step_lds(const StepPlan& s, int ow) { return window_step_lds_bytes(s.w_lo, s.w_hi, ow, (int)s.corr_words.size()); }

unsigned step_grid(long long B, int num_cu) { return (unsigned)std::min<long long>(B, (long long)num_cu * 8); }

struct Rows {  // the rows a chain of windows works on (device)
    unsigned long long *running, *obs, *corr;  // corr null: not wanted
    uint8_t* conv;
    int* iters;
};

struct StepTables {  // the model's stacked CSC and one step's lists (device)
    const int *col_ptr, *col_bits, *commit_pos, *commit_fault, *commit_slot, *corr_words, *gather;
};

// A step's launch parameters but for the two decodes around it (decoded / prev_* and syndrome), which the caller adds.
WindowStepParams step_params(const StepPlan& sp, long long B, int dw, int ow, int fw, const StepTables& t, const Rows& r) {
    WindowStepParams P{};
    P.B = B;
    P.dw = dw;
    P.ow = ow;
    P.fw = fw;
    P.w_lo = sp.w_lo;
    P.w_hi = sp.w_hi;
    P.col_ptr = t.col_ptr;
    P.col_bits = t.col_bits;
    P.n_commit = (int)sp.fault.size();
    P.n_corr = (int)sp.corr_words.size();
    P.commit_pos = t.commit_pos;
    P.commit_fault = t.commit_fault;
    P.commit_slot = t.commit_slot;
    P.corr_words = t.corr_words;
    P.decoded_cols = sp.decoded_cols;
    P.n_gather = (int)sp.gather.size();
    P.gather_det = t.gather;
    P.running = r.running;
    P.observables = r.obs;
    P.correction = r.corr;
    P.conv_all = r.conv;
    P.iters = r.iters;
    return P;
}

// Step s of the engine: its lists in the engine's tables, the decode of window s - 1 behind it and of window s ahead.
WindowStepParams step_params(const bposd_window* win, int s, long long B, const Rows& r) {
    const StepDev& a = win->at[s];
    const StepTables t{win->d_col_ptr, win->d_col_bits, win->d_commit_pos + a.commit, win->d_commit_fault + a.commit, win->d_commit_slot + a.commit,
                       win->d_corr_words + a.corr, win->d_gather + a.gather};
    WindowStepParams P = step_params(win->steps[s], B, win->dw, win->ow, win->fw, t, r);
    if (s > 0) {
        P.decoded = win->d_dec.p;
        P.decoded_packed = win->packed[s - 1];
        P.prev_conv = win->d_wconv;
        P.prev_iters = win->d_witers;
    }
    if (s < win->nwin) {
        P.syndrome = win->d_synd.p;
        P.syndrome_packed = win->packed[s];
    }
    return P;
}

// Every window of a batch, enqueued: the rows of `r` hold the detector rows in r.running on entry (in stream order) and the
// outputs on exit.  Nothing waits.
int enqueue_windows(bposd_window* win, long long B, const Rows& r) {
    hipStream_t st = win->stream;
    for (int w = 0; w < win->nwin; ++w)
        if ((native_packed(win->decs[w]) ? 1 : 0) != win->packed[w])
            return engine_fail(win, BPOSD_ERR_INVALID, "window %d: the decoder's kernel variant was changed after the engine was made (its rows are %s now)", w,
                            win->packed[w] ? "bytes" : "packed");
    ENGINE_TRY(win, hipMemsetAsync(r.obs, 0, sizeof(unsigned long long) * (size_t)B * win->ow, st));
    if (r.corr) ENGINE_TRY(win, hipMemsetAsync(r.corr, 0, sizeof(unsigned long long) * (size_t)B * win->fw, st));
    ENGINE_TRY(win, hipMemsetAsync(r.conv, 1, (size_t)B, st));
    ENGINE_TRY(win, hipMemsetAsync(r.iters, 0, sizeof(int) * (size_t)B, st));
    win->timed_steps = win->timed_score = false;
    for (int s = 0; s <= win->nwin; ++s) {
        const WindowStepParams P = step_params(win, s, B, r);
        ENGINE_TRY(win, hipEventRecord(win->ev_t[2 * s], st));
        hipLaunchKernelGGL(window_step_kernel, dim3(step_grid(B, win->num_cu)), dim3(WIN_THREADS), step_lds(win->steps[s], win->ow), st, P);
        ENGINE_TRY(win, hipGetLastError());
        ENGINE_TRY(win, hipEventRecord(win->ev_t[2 * s + 1], st));
        if (s == win->nwin) break;
        // window s on its decoder's next lane, ordered behind the gather; ev_decoded is recorded on that lane behind the call
        bposd_handle* const dec = win->decs[s];
        ENGINE_TRY(win, hipEventRecord(win->ev_step[s], st));
        const int rc = decode_behind(win, dec, win->ev_step[s], win->ev_decoded[s], [&] {
            return win->packed[s]
                       ? bposd_decode_batch_device_packed(dec, (const uint64_t*)win->d_synd.p, B, (uint64_t*)win->d_dec.p, nullptr, nullptr, win->d_wconv, win->d_witers)
                       : bposd_decode_batch_device(dec, (const uint8_t*)win->d_synd.p, B, (uint8_t*)win->d_dec.p, nullptr, nullptr, win->d_wconv, win->d_witers, nullptr);
        });
        if (rc) return engine_fail(win, rc, "window %d: %s", s, win->err.c_str());
        ENGINE_TRY(win, hipStreamWaitEvent(st, win->ev_decoded[s], 0));
    }
    win->timed_steps = true;
    return 0;
}

int create_device(bposd_window* win, const std::vector<int32_t>& col_ptr, const std::vector<int32_t>& col_bits) {
    int rc;
    if ((rc = upload(win, win->d_col_ptr, col_ptr))) return rc;
    if ((rc = upload(win, win->d_col_bits, col_bits))) return rc;
    std::vector<int> pos, fault, slot, corr, gather;
    size_t synd = 0, dec = 0;
    for (int s = 0; s <= win->nwin; ++s) {
        const StepPlan& sp = win->steps[s];
        win->at[s] = StepDev{pos.size(), corr.size(), gather.size()};
        pos.insert(pos.end(), sp.pos.begin(), sp.pos.end());
        fault.insert(fault.end(), sp.fault.begin(), sp.fault.end());
        slot.insert(slot.end(), sp.slot.begin(), sp.slot.end());
        corr.insert(corr.end(), sp.corr_words.begin(), sp.corr_words.end());
        gather.insert(gather.end(), sp.gather.begin(), sp.gather.end());
        if (s < win->nwin) {
            const bool packed = win->packed[s] != 0;
            synd = std::max(synd, row_bytes(win->n_det[s], packed));
            dec = std::max(dec, row_bytes(win->n_fault[s], packed));
        }
    }
    if ((rc = upload(win, win->d_commit_pos, pos))) return rc;
    if ((rc = upload(win, win->d_commit_fault, fault))) return rc;
    if ((rc = upload(win, win->d_commit_slot, slot))) return rc;
    if ((rc = upload(win, win->d_corr_words, corr))) return rc;
    if ((rc = upload(win, win->d_gather, gather))) return rc;
    const size_t C = (size_t)win->capacity;
    if ((rc = engine_alloc(win, win->d_running, C * win->dw))) return rc;
    if ((rc = engine_alloc(win, win->d_obs, C * win->ow))) return rc;
    if ((rc = engine_alloc(win, win->d_truth, C * win->ow))) return rc;
    if ((rc = engine_alloc(win, win->d_corr, C * win->fw))) return rc;
    if ((rc = engine_alloc_bytes(win, win->d_synd, C * synd))) return rc;
    if ((rc = engine_alloc_bytes(win, win->d_dec, C * dec))) return rc;
    if ((rc = engine_alloc(win, win->d_conv_all, C))) return rc;
    if ((rc = engine_alloc(win, win->d_iters, C))) return rc;
    if ((rc = engine_alloc(win, win->d_wconv, C))) return rc;
    if ((rc = engine_alloc(win, win->d_witers, C))) return rc;
    if ((rc = engine_alloc(win, win->d_flags, C))) return rc;
    if ((rc = win->counters.alloc(win, win->k))) return rc;
    ENGINE_TRY(win, hipStreamCreateWithFlags(&win->stream.raw, hipStreamNonBlocking));
    win->ev_step.resize(win->nwin);
    win->ev_decoded.resize(win->nwin);
    win->ev_t.resize(2 * ((size_t)win->nwin + 1) + 2);
    for (auto* v : {&win->ev_step, &win->ev_decoded})
        for (Event& e : *v) ENGINE_TRY(win, hipEventCreateWithFlags(&e.raw, hipEventDisableTiming));
    for (Event& e : win->ev_t) ENGINE_TRY(win, hipEventCreate(&e.raw));
    return 0;
}

}  // namespace

extern "C" {

const char* bposd_window_last_error(bposd_window* win) { return win ? win->err.c_str() : bposd_last_error(nullptr); }

void bposd_window_destroy(bposd_window* win) { engine_destroy(win); }

int bposd_window_create(const bposd_window_config* cfg, int32_t M, int32_t N, int32_t k, const int32_t* h_indptr, const int32_t* h_indices,
                        const int32_t* l_indptr, const int32_t* l_indices, int32_t nwin, bposd_handle* const* decs, const int32_t* win_det_ptr,
                        const int32_t* win_det, const int32_t* win_fault_ptr, const int32_t* win_fault, const uint8_t* win_commit,
                        bposd_window** out) {
    if (!out) return engine_fail(nullptr, BPOSD_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!cfg) return engine_fail(nullptr, BPOSD_ERR_INVALID, "config is required");
    if (cfg->capacity < 1 || cfg->capacity > 0x7fffffffLL) return engine_fail(nullptr, BPOSD_ERR_INVALID, "capacity %lld out of range", (long long)cfg->capacity);
    if (nwin < 1 || !decs || !win_det_ptr || !win_det || !win_fault_ptr || !win_fault || !win_commit)
        return engine_fail(nullptr, BPOSD_ERR_INVALID, "at least one window and every window list are required (nwin %d)", nwin);
    std::string why;
    std::vector<int32_t> col_ptr, col_bits;
    if (const int rc = bposd_host::stacked_csc(h_indptr, h_indices, M, l_indptr, l_indices, k, N, &col_ptr, &col_bits, &why))
        return engine_fail(nullptr, rc, "%s", why.c_str());
    // the window lists are two more CSR operands: row w holds window w's detectors / faults
    if (bposd_host::check_csr("win_det", win_det_ptr, win_det, nwin, M, true, &why) || bposd_host::check_csr("win_fault", win_fault_ptr, win_fault, nwin, N, true, &why))
        return engine_fail(nullptr, BPOSD_ERR_INVALID, "%s", why.c_str());

    std::unique_ptr<bposd_window, decltype(&bposd_window_destroy)> owner(new bposd_window(), bposd_window_destroy);
    bposd_window* const win = owner.get();
    win->cfg = *cfg;
    win->device = cfg->device;
    win->M = M;
    win->N = N;
    win->k = k;
    win->dw = (M + 63) / 64;
    win->ow = (k + 63) / 64;
    win->fw = (N + 63) / 64;
    win->nwin = nwin;
    win->capacity = cfg->capacity;
    win->decs.assign(decs, decs + nwin);
    win->n_det.resize(nwin);
    win->n_fault.resize(nwin);
    win->packed.assign(nwin, 0);
    win->steps.resize((size_t)nwin + 1);
    win->at.resize((size_t)nwin + 1);

    std::vector<int> committed_by((size_t)N, -1), pos_of((size_t)N, -1), row;
    for (int w = 0; w < nwin; ++w) {
        const int d0 = win_det_ptr[w], d1 = win_det_ptr[w + 1], f0 = win_fault_ptr[w], f1 = win_fault_ptr[w + 1];
        if (d1 <= d0 || f1 <= f0) return engine_fail(nullptr, BPOSD_ERR_INVALID, "window %d: %d detectors and %d faults: a window needs both", w, d1 - d0, f1 - f0);
        const int nd = d1 - d0, nf = f1 - f0;
        win->n_det[w] = nd;
        win->n_fault[w] = nf;
        for (int e = f0; e < f1; ++e)
            if (win_commit[e] > 1) return engine_fail(nullptr, BPOSD_ERR_INVALID, "window %d: the commit flag of fault %d is %d, not 0 or 1", w, win_fault[e], win_commit[e]);
        StepPlan& commit = win->steps[(size_t)w + 1];
        commit.decoded_cols = nf;
        for (int e = f0; e < f1; ++e) {
            if (!win_commit[e]) continue;
            const int f = win_fault[e];
            if (committed_by[f] >= 0) return engine_fail(nullptr, BPOSD_ERR_INVALID, "window %d: fault %d was committed by window %d already", w, f, committed_by[f]);
            committed_by[f] = w;
            commit.pos.push_back(e - f0);
            commit.fault.push_back(f);
        }
        win->steps[w].gather.assign(win_det + d0, win_det + d1);

        const bposd_handle* const dec = decs[w];
        if (!dec) return engine_fail(nullptr, BPOSD_ERR_INVALID, "window %d: the decoder is NULL", w);
        if (dec->device != cfg->device)
            return engine_fail(nullptr, BPOSD_ERR_INVALID, "window %d: the decoder lives on device %d, the engine on device %d", w, dec->device, cfg->device);
        win->packed[w] = native_packed(dec) ? 1 : 0;
        if (dec->m != nd || dec->n != nf)
            return engine_fail(nullptr, BPOSD_ERR_INVALID, "window %d: decoder shape %d x %d does not match the window's %d detectors x %d faults", w, dec->m, dec->n, nd, nf);
        // the decoder's matrix must be H[D_w][:, F_w]: rows and lists ascend, so the positions of a row ascend too
        for (int e = f0; e < f1; ++e) pos_of[win_fault[e]] = e - f0;
        bool same = true;
        for (int i = 0; i < nd && same; ++i) {
            const int d = win_det[d0 + i];
            row.clear();
            for (int e = h_indptr[d]; e < h_indptr[d + 1]; ++e)
                if (pos_of[h_indices[e]] >= 0) row.push_back(pos_of[h_indices[e]]);
            same = (int)row.size() == dec->rp[i + 1] - dec->rp[i] && std::equal(row.begin(), row.end(), dec->ci.begin() + dec->rp[i]);
            if (!same) engine_fail(nullptr, BPOSD_ERR_INVALID, "window %d: row %d of the decoder's matrix is not detector %d of H restricted to the window's faults", w, i, d);
        }
        for (int e = f0; e < f1; ++e) pos_of[win_fault[e]] = -1;
        if (!same) return BPOSD_ERR_INVALID;
    }
    for (int s = 0; s <= nwin; ++s) {
        StepPlan& sp = win->steps[s];
        sp.finish(col_ptr, col_bits, win->dw);
        if (step_lds(sp, win->ow) > 64 * 1024)
            return engine_fail(nullptr, BPOSD_ERR_UNSUPPORTED, "step %d (commit of window %d, gather of window %d) stages %d detector words, %d observable words and %zu correction "
                            "words: %zu bytes of LDS per workgroup, more than 65536", s, s - 1, s, sp.w_hi - sp.w_lo, win->ow, sp.corr_words.size(), step_lds(sp, win->ow));
    }
    win->num_cu = decs[0]->num_cu > 0 ? decs[0]->num_cu : 256;
    if (const int rc = engine_create_on_device(win, [&] { return create_device(win, col_ptr, col_bits); })) return rc;
    *out = owner.release();
    return BPOSD_OK;
}

int bposd_window_decode_device(bposd_window* win, const uint64_t* d_detector_words, int64_t B, uint64_t* d_obs_words, uint64_t* d_correction_words,
                               uint64_t* d_residual_words, uint8_t* d_conv, int32_t* d_iters) {
    if (!win) return BPOSD_ERR_INVALID;
    if (!d_detector_words || !d_obs_words) return engine_fail(win, BPOSD_ERR_INVALID, "detector and observable buffers are required");
    if (const int rc = engine_check_batch(win, B)) return rc;
    DeviceGuard guard(win->device);
    ENGINE_TRY(win, guard.err);
    win->run_B = 0;
    win->hv.last_on = false;
    Rows r{};
    r.running = d_residual_words ? (unsigned long long*)d_residual_words : (unsigned long long*)win->d_running;
    r.obs = (unsigned long long*)d_obs_words;
    r.corr = (unsigned long long*)d_correction_words;
    r.conv = d_conv ? d_conv : (uint8_t*)win->d_conv_all;
    r.iters = d_iters ? d_iters : (int*)win->d_iters;
    ENGINE_TRY(win, hipMemcpyAsync(r.running, d_detector_words, 8 * (size_t)B * win->dw, hipMemcpyDeviceToDevice, win->stream));
    return enqueue_windows(win, B, r);
}

int bposd_window_synchronize(bposd_window* win) {
    if (!win) return BPOSD_ERR_INVALID;
    DeviceGuard guard(win->device);
    ENGINE_TRY(win, guard.err);
    ENGINE_TRY(win, hipStreamSynchronize(win->stream));
    return BPOSD_OK;
}

int bposd_window_decode(bposd_window* win, const uint64_t* detector_words, int64_t B, uint64_t* obs_words, uint64_t* correction_words,
                        uint64_t* residual_words, uint8_t* conv, int32_t* iters) {
    if (!win) return BPOSD_ERR_INVALID;
    if (B < 0 || B > 0x7fffffffLL) return engine_fail(win, BPOSD_ERR_INVALID, "batch size %lld out of range", (long long)B);
    if (B > 0 && (!detector_words || !obs_words)) return engine_fail(win, BPOSD_ERR_INVALID, "detector and observable buffers are required");
    DeviceGuard guard(win->device);
    ENGINE_TRY(win, guard.err);
    win->run_B = 0;
    win->hv.last_on = false;
    hipStream_t st = win->stream;
    const size_t dw = win->dw, ow = win->ow, fw = win->fw;
    for (int64_t lo = 0; lo < B; lo += win->capacity) {
        const size_t cnt = (size_t)std::min<int64_t>(win->capacity, B - lo);
        Rows r{win->d_running, win->d_obs, correction_words ? (unsigned long long*)win->d_corr : nullptr, win->d_conv_all, win->d_iters};
        ENGINE_TRY(win, hipMemcpyAsync(r.running, detector_words + (size_t)lo * dw, 8 * cnt * dw, hipMemcpyHostToDevice, st));
        if (const int rc = enqueue_windows(win, (long long)cnt, r)) return rc;
        ENGINE_TRY(win, hipMemcpyAsync(obs_words + (size_t)lo * ow, r.obs, 8 * cnt * ow, hipMemcpyDeviceToHost, st));
        if (correction_words) ENGINE_TRY(win, hipMemcpyAsync(correction_words + (size_t)lo * fw, r.corr, 8 * cnt * fw, hipMemcpyDeviceToHost, st));
        if (residual_words) ENGINE_TRY(win, hipMemcpyAsync(residual_words + (size_t)lo * dw, r.running, 8 * cnt * dw, hipMemcpyDeviceToHost, st));
        if (conv) ENGINE_TRY(win, hipMemcpyAsync(conv + lo, r.conv, cnt, hipMemcpyDeviceToHost, st));
        if (iters) ENGINE_TRY(win, hipMemcpyAsync(iters + lo, r.iters, sizeof(int) * cnt, hipMemcpyDeviceToHost, st));
        ENGINE_TRY(win, hipStreamSynchronize(st));  // the next chunk reuses the engine's rows
    }
    return BPOSD_OK;
}

int bposd_window_run(bposd_window* win, bposd_dem* sampler, uint64_t first_shot, int64_t B, int64_t counters[4]) {
    if (!win) return BPOSD_ERR_INVALID;
    if (!sampler || !counters) return engine_fail(win, BPOSD_ERR_INVALID, "sampler and counters are required");
    if (sampler->dec) return engine_fail(win, BPOSD_ERR_INVALID, "the sampler must be a sample-only engine (created without a decoder)");
    if (sampler->M != win->M || sampler->N != win->N || sampler->k != win->k || sampler->device != win->device)
        return engine_fail(win, BPOSD_ERR_INVALID, "the sampler's model (%d x %d, k = %d, device %d) is not the engine's (%d x %d, k = %d, device %d)", sampler->M,
                        sampler->N, sampler->k, sampler->device, win->M, win->N, win->k, win->device);
    if (const int rc = engine_check_batch(win, B)) return rc;
    DeviceGuard guard(win->device);
    ENGINE_TRY(win, guard.err);
    win->run_B = 0;
    win->hv.last_on = false;
    hipStream_t st = win->stream;
    if (const int rc = bposd_host::dem_sample_async(sampler, first_shot, B, st)) return engine_fail(win, rc, "sampler: %s", bposd_dem_last_error(sampler));
    Rows r{win->d_running, win->d_obs, win->d_corr, win->d_conv_all, win->d_iters};
    ENGINE_TRY(win, hipMemcpyAsync(r.running, sampler->d_detectors, 8 * (size_t)B * win->dw, hipMemcpyDeviceToDevice, st));
    ENGINE_TRY(win, hipMemcpyAsync(win->d_truth, sampler->d_observables, 8 * (size_t)B * win->ow, hipMemcpyDeviceToDevice, st));
    ENGINE_TRY(win, win->counters.reset(st));
    int rc = enqueue_windows(win, B, r);
    if (rc) {
        (void)hipStreamSynchronize(st);
        return rc;
    }
    WindowScoreParams Q{};
    Q.B = B;
    Q.k = win->k;
    Q.ow = win->ow;
    Q.dw = win->dw;
    Q.detectors = sampler->d_detectors;
    Q.residual = r.running;
    Q.truth = win->d_truth;
    Q.decoded = r.obs;
    Q.conv_all = r.conv;
    Q.flags = win->d_flags;
    Q.counters = win->counters.d_counters;
    Q.obs_fail = win->counters.d_obs_fail;
    const unsigned grid = (unsigned)std::min<long long>((B + WIN_SCORE_THREADS - 1) / WIN_SCORE_THREADS, (long long)win->num_cu * 8);
    Event* const ev = &win->ev_t[2 * ((size_t)win->nwin + 1)];
    ENGINE_TRY(win, hipEventRecord(ev[0], st));
    hipLaunchKernelGGL(window_score_kernel, dim3(grid), dim3(WIN_SCORE_THREADS), 0, st, Q);
    ENGINE_TRY(win, hipGetLastError());
    ENGINE_TRY(win, hipEventRecord(ev[1], st));
    const bool harvest = win->hv.on();
    if (harvest) {
        // observables wrong (bit 0) on a residual of zero (bit 1 clear); the corrections are the engine's own packed rows, the
        // fault rows the sampler's, which the engine's stream is ordered behind
        const HarvestJob job{B, win->N, win->fw, /*flag_mask=*/3, /*flag_want=*/1, win->d_flags, sampler->d_faults, r.corr, true};
        if ((rc = bposd_host::harvest_enqueue(win, win->hv, job, win->counters.d_counters))) {
            (void)hipStreamSynchronize(st);
            return rc;
        }
    }
    ENGINE_TRY(win, win->counters.download(st, harvest ? 8 : 4));
    ENGINE_TRY(win, hipStreamSynchronize(st));  // the batch's one host wait
    win->counters.read(counters, 4);
    if (harvest) bposd_host::harvest_read(win->hv, win->counters.h_counters.as<int>());
    win->timed_score = true;
    win->run_B = B;
    return BPOSD_OK;
}

int bposd_window_fetch(bposd_window* win, int32_t what, void* host_dst, size_t bytes) {
    if (!win) return BPOSD_ERR_INVALID;
    if (win->run_B == 0) return engine_fail(win, BPOSD_ERR_INVALID, "no bposd_window_run has completed since the last decode call");
    if (what >= BPOSD_WINDOW_FAIL_ROWS && what <= BPOSD_WINDOW_MIN_RESIDUAL && !win->hv.last_on)
        return engine_fail(win, BPOSD_ERR_INVALID, "item %d needs a batch that ran with the harvest on (bposd_window_set_harvest)", what);
    const size_t ow = 8 * (size_t)win->ow;
    FetchItem items[13] = {{win->d_obs, ow, false},   {win->d_truth, ow, false},    {win->d_corr, 8 * (size_t)win->fw, false},
                               {win->d_running, 8 * (size_t)win->dw, false},            {win->d_flags, 1, false},
                               {win->d_conv_all, 1, false}, {win->d_iters, sizeof(int32_t), false},
                               {nullptr, sizeof(int32_t) * (size_t)win->k, true}};
    bposd_host::harvest_items(win->hv, win->fw, items + 8);
    return engine_fetch(win, items, 13, BPOSD_WINDOW_OBS, "BPOSD_WINDOW_OBS .. BPOSD_WINDOW_MIN_RESIDUAL", what, win->run_B, win->counters.obs_fail(),
                        host_dst, bytes);
}

int bposd_window_set_harvest(bposd_window* win, int64_t max_rows) {
    if (!win) return BPOSD_ERR_INVALID;
    return bposd_host::harvest_set(win, win->hv, max_rows, win->fw);
}

int bposd_window_harvest_info(bposd_window* win, int64_t out[3]) {
    if (!win) return BPOSD_ERR_INVALID;
    if (!out) return engine_fail(win, BPOSD_ERR_INVALID, "out is NULL");
    if (!win->hv.last_on) return engine_fail(win, BPOSD_ERR_INVALID, "the last batch ran with the harvest off (bposd_window_set_harvest)");
    std::copy(win->hv.info, win->hv.info + 3, out);
    return BPOSD_OK;
}

int64_t bposd_window_device_bytes(bposd_window* win) { return win ? (int64_t)win->device_bytes : BPOSD_ERR_INVALID; }

int bposd_debug_window_timing(bposd_window* win, double* step_ms, double* score_ms) {
    if (!win) return BPOSD_ERR_INVALID;
    if (!win->timed_steps) return engine_fail(win, BPOSD_ERR_INVALID, "no batch has run yet");
    DeviceGuard guard(win->device);
    ENGINE_TRY(win, guard.err);
    ENGINE_TRY(win, hipStreamSynchronize(win->stream));
    float ms = 0.f;
    if (step_ms) {
        *step_ms = 0.0;
        for (int s = 0; s <= win->nwin; ++s) {
            ENGINE_TRY(win, hipEventElapsedTime(&ms, win->ev_t[2 * s], win->ev_t[2 * s + 1]));
            *step_ms += ms;
        }
    }
    if (score_ms) {
        *score_ms = 0.0;
        if (win->timed_score) {
            Event* const ev = &win->ev_t[2 * ((size_t)win->nwin + 1)];
            ENGINE_TRY(win, hipEventElapsedTime(&ms, ev[0], ev[1]));
            *score_ms = ms;
        }
    }
    return BPOSD_OK;
}

int bposd_debug_window_step(bposd_window_step_args* a) {
    if (!a) return engine_fail(nullptr, BPOSD_ERR_INVALID, "args is NULL");
    const int M = a->M, N = a->N, k = a->k;
    if (a->B < 1 || a->B > 0x7fffffffLL) return engine_fail(nullptr, BPOSD_ERR_INVALID, "batch size %lld out of range", (long long)a->B);
    if (a->n_commit < 0 || a->n_gather < 0 || a->decoded_cols < 0) return engine_fail(nullptr, BPOSD_ERR_INVALID, "negative count");
    if (!a->running || !a->observables || !a->conv_all || !a->iters) return engine_fail(nullptr, BPOSD_ERR_INVALID, "running, observables, conv_all and iters are required");
    if (a->n_commit > 0 && (!a->commit_pos || !a->commit_fault || !a->decoded)) return engine_fail(nullptr, BPOSD_ERR_INVALID, "a commit needs its lists and the decoded rows");
    if (a->n_gather > 0 && (!a->gather_det || !a->syndrome)) return engine_fail(nullptr, BPOSD_ERR_INVALID, "a gather needs its list and the syndrome rows");
    std::string why;
    std::vector<int32_t> col_ptr, col_bits;
    if (const int rc = bposd_host::stacked_csc(a->h_indptr, a->h_indices, M, a->l_indptr, a->l_indices, k, N, &col_ptr, &col_bits, &why))
        return engine_fail(nullptr, rc, "%s", why.c_str());
    StepPlan sp;
    sp.decoded_cols = a->decoded_cols;
    for (int c = 0; c < a->n_commit; ++c) {
        const int j = a->commit_pos[c], f = a->commit_fault[c];
        if (j < 0 || j >= a->decoded_cols || f < 0 || f >= N || (c > 0 && (j <= a->commit_pos[c - 1] || f <= a->commit_fault[c - 1])))
            return engine_fail(nullptr, BPOSD_ERR_INVALID, "commit entry %d (position %d, fault %d) is out of range or does not ascend", c, j, f);
        sp.pos.push_back(j);
        sp.fault.push_back(f);
    }
    for (int r = 0; r < a->n_gather; ++r) {
        const int d = a->gather_det[r];
        if (d < 0 || d >= M || (r > 0 && d <= a->gather_det[r - 1])) return engine_fail(nullptr, BPOSD_ERR_INVALID, "gather entry %d (detector %d) is out of range or does not ascend", r, d);
        sp.gather.push_back(d);
    }
    const int dw = (M + 63) / 64, ow = (k + 63) / 64, fw = (N + 63) / 64;
    sp.finish(col_ptr, col_bits, dw);
    a->word_range[0] = sp.w_lo;
    a->word_range[1] = sp.w_hi;
    if (step_lds(sp, ow) > 64 * 1024) return engine_fail(nullptr, BPOSD_ERR_UNSUPPORTED, "the step needs %zu bytes of LDS per workgroup, more than 65536", step_lds(sp, ow));

    EngineBase* const none = nullptr;
    DeviceGuard guard(a->device);
    ENGINE_TRY(none, guard.err);
    hipDeviceProp_t prop;
    ENGINE_TRY(none, hipGetDeviceProperties(&prop, a->device));
    const int num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    const size_t B = (size_t)a->B;
    DevArray<int> d_col_ptr, d_col_bits, d_pos, d_fault, d_slot, d_corr_words, d_gather, d_iters, d_piters;
    DevArray<unsigned long long> d_running, d_obs, d_corr;
    DevArray<uint8_t> d_conv, d_pconv;
    DevBuf d_dec, d_synd;
    int rc;
    if ((rc = upload(nullptr, d_col_ptr, col_ptr)) || (rc = upload(nullptr, d_col_bits, col_bits)) || (rc = upload(nullptr, d_pos, sp.pos)) ||
        (rc = upload(nullptr, d_fault, sp.fault)) || (rc = upload(nullptr, d_slot, sp.slot)) || (rc = upload(nullptr, d_corr_words, sp.corr_words)) ||
        (rc = upload(nullptr, d_gather, sp.gather)))
        return rc;
    const size_t dec_bytes = B * row_bytes(a->decoded_cols, a->decoded_packed != 0), synd_bytes = B * row_bytes(a->n_gather, a->syndrome_packed != 0);
    struct Io { DevBuf* dev; void* host; size_t bytes; bool up, down; };
    const Io io[] = {{&d_running, a->running, 8 * B * dw, true, true},   {&d_obs, a->observables, 8 * B * ow, true, true},
                     {&d_corr, a->correction, 8 * B * fw, true, true},   {&d_conv, a->conv_all, B, true, true},
                     {&d_iters, a->iters, 4 * B, true, true},            {&d_pconv, (void*)a->prev_converged, B, true, false},
                     {&d_piters, (void*)a->prev_iters, 4 * B, true, false}, {&d_dec, (void*)a->decoded, dec_bytes, true, false},
                     {&d_synd, a->syndrome, synd_bytes, false, true}};
    for (const Io& x : io) {
        if (!x.host || !x.bytes) continue;
        if ((rc = engine_alloc_bytes(none, *x.dev, x.bytes))) return rc;
        if (x.up) ENGINE_TRY(none, hipMemcpy(x.dev->p, x.host, x.bytes, hipMemcpyHostToDevice));
    }
    const StepTables t{d_col_ptr, d_col_bits, d_pos, d_fault, d_slot, d_corr_words, d_gather};
    WindowStepParams P = step_params(sp, a->B, dw, ow, fw, t, Rows{d_running, d_obs, d_corr, d_conv, d_iters});
    P.decoded = d_dec.p;
    P.decoded_packed = a->decoded_packed != 0;
    P.prev_conv = d_pconv;
    P.prev_iters = d_piters;
    P.syndrome = d_synd.p;
    P.syndrome_packed = a->syndrome_packed != 0;
    hipLaunchKernelGGL(window_step_kernel, dim3(step_grid(a->B, num_cu)), dim3(WIN_THREADS), step_lds(sp, ow), nullptr, P);
    ENGINE_TRY(none, hipGetLastError());
    ENGINE_TRY(none, hipDeviceSynchronize());
    for (const Io& x : io)
        if (x.host && x.bytes && x.down) ENGINE_TRY(none, hipMemcpy(x.host, x.dev->p, x.bytes, hipMemcpyDeviceToHost));
    return BPOSD_OK;
}

}  // extern "C"
