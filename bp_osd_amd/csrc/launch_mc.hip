// launch_mc.hip -- the Monte-Carlo engine of libbposd_mi355x.so: bposd_mc_* of include/bposd_mi355x.h.
// One translation unit: mc_sample_kernel and mc_score_kernel (mc_kernels.hip.h) are instantiated here and nowhere else.
//
// A batch is sample -> syndromes -> two decodes -> logical checks -> seven integers.  The engine owns every buffer of it
// and a stream of its own; the decodes go through the decoders' device-pointer entry points on the decoders' own lanes.
// The engine's stream and those lanes are ordered against each other by events; the host waits once per batch, for the
// counters.
#include "engine_common.h"

#include <climits>

#include "mc_kernels.hip.h"

using namespace bposd_mc_dev;

struct bposd_mc : EngineBase {
    bposd_mc_config cfg{};
    bposd_handle *dec_x = nullptr, *dec_z = nullptr;
    int n = 0, mx = 0, mz = 0, k = 0, words = 0, swx = 0, swz = 0;
    long long last_B = 0;
    Event ev_sampled, ev_x, ev_z;
    std::vector<double> alt;  // second decoder's probabilities where the first one's osdw bit is 1 (channel_update != none)
    // device tables
    DevArray<double> d_thr;
    DevArray<int> d_hx_rp, d_hx_ci, d_hz_rp, d_hz_ci;
    DevArray<unsigned long long> d_lxT, d_lzT;
    // per-batch buffers (capacity rows)
    DevArray<unsigned long long> d_err_x, d_err_z, d_psynd_x, d_psynd_z;
    DevArray<uint8_t> d_synd_x, d_synd_z, d_flags;
    DevArray<uint8_t> d_out[6];  // bp x, bp z, osd0 x, osd0 z, osdw x, osdw z
    DevArray<uint8_t> d_conv_x, d_conv_z;
    DevArray<int> d_counters;
    PinnedBuf h_counters;  // 16 ints: [0..6] results, [8..14] the initial values
};

namespace {

// [k][words] -> [words][k]: the threads of the score kernel that share a residual row read consecutive words
std::vector<unsigned long long> transpose_words(const uint64_t* src, int k, int words) {
    std::vector<unsigned long long> t((size_t)k * words);
    for (int r = 0; r < k; ++r)
        for (int w = 0; w < words; ++w) t[(size_t)w * k + r] = src[(size_t)r * words + w];
    return t;
}

int create_impl(bposd_mc* mc, const int32_t* hx_rp, const int32_t* hx_ci, const int32_t* hz_rp, const int32_t* hz_ci,
                const uint64_t* lx, const uint64_t* lz, const double* px, const double* py, const double* pz) {
    int rc;
    const int n = mc->n;
    // thresholds in the reference's operation order (css_decode_sim.py:476-490): pz, pz + px, px + py + pz
    std::vector<double> thr(3 * (size_t)n);
    for (int i = 0; i < n; ++i) {
        if (!(px[i] >= 0 && py[i] >= 0 && pz[i] >= 0 && px[i] + py[i] + pz[i] <= 1))
            return engine_fail(mc, BPOSD_ERR_INVALID, "probabilities of qubit %d (%g, %g, %g) are not a channel", i, px[i], py[i], pz[i]);
        thr[i] = pz[i];
        thr[(size_t)n + i] = pz[i] + px[i];
        thr[2 * (size_t)n + i] = px[i] + py[i] + pz[i];
    }
    if ((rc = engine_upload(mc, mc->d_thr, thr.data(), thr.size()))) return rc;
    if ((rc = engine_upload(mc, mc->d_hx_rp, hx_rp, (size_t)mc->mx + 1))) return rc;
    if ((rc = engine_upload(mc, mc->d_hx_ci, hx_ci, (size_t)hx_rp[mc->mx]))) return rc;
    if ((rc = engine_upload(mc, mc->d_hz_rp, hz_rp, (size_t)mc->mz + 1))) return rc;
    if ((rc = engine_upload(mc, mc->d_hz_ci, hz_ci, (size_t)hz_rp[mc->mz]))) return rc;
    const auto lxT = transpose_words(lx, mc->k, mc->words), lzT = transpose_words(lz, mc->k, mc->words);
    if ((rc = engine_upload(mc, mc->d_lxT, lxT.data(), lxT.size()))) return rc;
    if ((rc = engine_upload(mc, mc->d_lzT, lzT.data(), lzT.size()))) return rc;
    const size_t C = (size_t)mc->capacity;
    if ((rc = engine_alloc(mc, mc->d_err_x, C * mc->words))) return rc;
    if ((rc = engine_alloc(mc, mc->d_err_z, C * mc->words))) return rc;
    if ((rc = engine_alloc(mc, mc->d_psynd_x, C * mc->swx))) return rc;
    if ((rc = engine_alloc(mc, mc->d_psynd_z, C * mc->swz))) return rc;
    if ((rc = engine_alloc(mc, mc->d_synd_x, C * mc->mz))) return rc;
    if ((rc = engine_alloc(mc, mc->d_synd_z, C * mc->mx))) return rc;
    if ((rc = engine_alloc(mc, mc->d_flags, C))) return rc;
    for (auto& p : mc->d_out)
        if ((rc = engine_alloc(mc, p, C * n))) return rc;
    if ((rc = engine_alloc(mc, mc->d_conv_x, C))) return rc;
    if ((rc = engine_alloc(mc, mc->d_conv_z, C))) return rc;
    if ((rc = engine_alloc(mc, mc->d_counters, 8))) return rc;
    ENGINE_TRY(mc, mc->h_counters.alloc(16 * sizeof(int), hipHostMallocDefault));
    int* const hc = mc->h_counters.as<int>();
    for (int i = 0; i < 16; ++i) hc[i] = 0;
    hc[8 + 5] = hc[8 + 6] = INT_MAX;
    ENGINE_TRY(mc, hipStreamCreateWithFlags(&mc->stream.raw, hipStreamNonBlocking));
    for (Event* e : {&mc->ev_sampled, &mc->ev_x, &mc->ev_z}) ENGINE_TRY(mc, hipEventCreateWithFlags(&e->raw, hipEventDisableTiming));
    return 0;
}

// One decode of the batch on the decoder's next lane, ordered behind `after` (an event of another stream); `done` is
// recorded on that lane behind the call.  select != nullptr: the per-shot two-valued channel.
int enqueue_decode(bposd_mc* mc, bposd_handle* dec, hipEvent_t after, hipEvent_t done, const uint8_t* synd, long long B,
                   const uint8_t* select, uint8_t* osdw, uint8_t* osd0, uint8_t* bp, uint8_t* conv) {
    return decode_behind(mc, dec, after, done, [&] {
        return select ? bposd_decode_batch_select_device(dec, synd, B, select, mc->alt.data(), osdw, osd0, bp, conv, nullptr, nullptr)
                      : bposd_decode_batch_device(dec, synd, B, osdw, osd0, bp, conv, nullptr, nullptr);
    });
}

}  // namespace

extern "C" {

const char* bposd_mc_last_error(bposd_mc* mc) { return mc ? mc->err.c_str() : bposd_last_error(nullptr); }

void bposd_mc_destroy(bposd_mc* mc) { engine_destroy(mc); }

int bposd_mc_create(const bposd_mc_config* cfg, bposd_handle* dec_x, bposd_handle* dec_z, const int32_t* hx_indptr,
                    const int32_t* hx_indices, int32_t mx, const int32_t* hz_indptr, const int32_t* hz_indices, int32_t mz, int32_t n,
                    const uint64_t* lx_words, const uint64_t* lz_words, int32_t k, const double* probs_x, const double* probs_y,
                    const double* probs_z, const double* alt_probs, bposd_mc** out) {
    if (!out) return engine_fail(nullptr, BPOSD_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!cfg || !dec_x || !dec_z) return engine_fail(nullptr, BPOSD_ERR_INVALID, "config and both decoders are required");
    if (cfg->channel_update < BPOSD_MC_UPDATE_NONE || cfg->channel_update > BPOSD_MC_UPDATE_Z_TO_X)
        return engine_fail(nullptr, BPOSD_ERR_INVALID, "channel_update %d is not one of BPOSD_MC_UPDATE_*", cfg->channel_update);
    if (cfg->capacity < 1 || cfg->capacity > 0x7fffffffLL) return engine_fail(nullptr, BPOSD_ERR_INVALID, "capacity %lld out of range", (long long)cfg->capacity);
    if (n < 1 || mx < 0 || mz < 0 || k < 0) return engine_fail(nullptr, BPOSD_ERR_INVALID, "bad shape: n %d, mx %d, mz %d, k %d", n, mx, mz, k);
    if (dec_x == dec_z) return engine_fail(nullptr, BPOSD_ERR_INVALID, "the two sectors need a decoder each");
    if (dec_x->device != cfg->device || dec_z->device != cfg->device)
        return engine_fail(nullptr, BPOSD_ERR_INVALID, "decoders live on devices %d and %d, the engine on device %d", dec_x->device, dec_z->device, cfg->device);
    // dec_x decodes hz . error_x, dec_z decodes hx . error_z
    if (dec_x->n != n || dec_z->n != n || dec_x->m != mz || dec_z->m != mx)
        return engine_fail(nullptr, BPOSD_ERR_INVALID, "decoder shapes (x: %d x %d, z: %d x %d) do not match hz %d x %d / hx %d x %d", dec_x->m,
                       dec_x->n, dec_z->m, dec_z->n, mz, n, mx, n);
    if (!probs_x || !probs_y || !probs_z) return engine_fail(nullptr, BPOSD_ERR_INVALID, "the three probability arrays are required");
    if (k > 0 && (!lx_words || !lz_words)) return engine_fail(nullptr, BPOSD_ERR_INVALID, "logical operators missing");
    if (cfg->channel_update != BPOSD_MC_UPDATE_NONE && !alt_probs)
        return engine_fail(nullptr, BPOSD_ERR_INVALID, "a channel update needs the second decoder's alternative probabilities");
    std::string why;  // (rows need not be sorted: the sampler XORs a row's entries in any order)
    if (bposd_host::check_csr("hx", hx_indptr, hx_indices, mx, n, false, &why) || bposd_host::check_csr("hz", hz_indptr, hz_indices, mz, n, false, &why))
        return engine_fail(nullptr, BPOSD_ERR_INVALID, "%s", why.c_str());

    std::unique_ptr<bposd_mc, decltype(&bposd_mc_destroy)> owner(new bposd_mc(), bposd_mc_destroy);
    bposd_mc* const mc = owner.get();
    mc->cfg = *cfg;
    mc->device = cfg->device;
    mc->dec_x = dec_x;
    mc->dec_z = dec_z;
    mc->n = n;
    mc->mx = mx;
    mc->mz = mz;
    mc->k = k;
    mc->words = (n + 63) / 64;
    mc->swx = (mz + 63) / 64;
    mc->swz = (mx + 63) / 64;
    mc->capacity = cfg->capacity;
    mc->num_cu = dec_x->num_cu > 0 ? dec_x->num_cu : 256;
    if (alt_probs) mc->alt.assign(alt_probs, alt_probs + n);
    if (const int rc = engine_create_on_device(mc, [&] { return create_impl(mc, hx_indptr, hx_indices, hz_indptr, hz_indices, lx_words, lz_words, probs_x, probs_y, probs_z); }))
        return rc;
    *out = owner.release();
    return BPOSD_OK;
}

int bposd_mc_run(bposd_mc* mc, uint64_t first_shot, int64_t B, int64_t counters[7]) {
    if (!mc) return BPOSD_ERR_INVALID;
    if (!counters) return engine_fail(mc, BPOSD_ERR_INVALID, "counters is NULL");
    if (const int rc = engine_check_batch(mc, B)) return rc;
    DeviceGuard guard(mc->device);
    ENGINE_TRY(mc, guard.err);
    mc->last_B = 0;
    const unsigned grid = (unsigned)std::min<long long>(B, (long long)mc->num_cu * 8);

    McSampleParams S{};
    S.B = B;
    S.first_shot = first_shot;
    S.key0 = (uint32_t)mc->cfg.seed;
    S.key1 = (uint32_t)(mc->cfg.seed >> 32);
    S.n = mc->n;
    S.words = mc->words;
    S.thr = mc->d_thr;
    S.mx = mc->mx;
    S.mz = mc->mz;
    S.swx = mc->swx;
    S.swz = mc->swz;
    S.hx_rp = mc->d_hx_rp;
    S.hx_ci = mc->d_hx_ci;
    S.hz_rp = mc->d_hz_rp;
    S.hz_ci = mc->d_hz_ci;
    S.err_x = mc->d_err_x;
    S.err_z = mc->d_err_z;
    S.synd_x = mc->d_synd_x;
    S.synd_z = mc->d_synd_z;
    S.psynd_x = mc->d_psynd_x;
    S.psynd_z = mc->d_psynd_z;
    hipLaunchKernelGGL(mc_sample_kernel, dim3(grid), dim3(MC_THREADS), 2 * sizeof(unsigned long long) * (size_t)mc->words, mc->stream, S);
    ENGINE_TRY(mc, hipGetLastError());
    ENGINE_TRY(mc, hipEventRecord(mc->ev_sampled, mc->stream));
    ENGINE_TRY(mc, hipMemcpyAsync(mc->d_counters, mc->h_counters.as<int>() + 8, 7 * sizeof(int), hipMemcpyHostToDevice, mc->stream));

    uint8_t *bp_x = mc->d_out[0], *bp_z = mc->d_out[1], *osd0_x = mc->d_out[2], *osd0_z = mc->d_out[3], *osdw_x = mc->d_out[4], *osdw_z = mc->d_out[5];
    int rc;
    switch (mc->cfg.channel_update) {
    case BPOSD_MC_UPDATE_NONE:  // both at once, each on a lane of its own handle
        if ((rc = enqueue_decode(mc, mc->dec_z, mc->ev_sampled, mc->ev_z, mc->d_synd_z, B, nullptr, osdw_z, osd0_z, bp_z, mc->d_conv_z))) return rc;
        if ((rc = enqueue_decode(mc, mc->dec_x, mc->ev_sampled, mc->ev_x, mc->d_synd_x, B, nullptr, osdw_x, osd0_x, bp_x, mc->d_conv_x))) return rc;
        break;
    case BPOSD_MC_UPDATE_X_TO_Z:  // the second decode reads the first one's osdw rows as its per-shot channel selector
        if ((rc = enqueue_decode(mc, mc->dec_x, mc->ev_sampled, mc->ev_x, mc->d_synd_x, B, nullptr, osdw_x, osd0_x, bp_x, mc->d_conv_x))) return rc;
        if ((rc = enqueue_decode(mc, mc->dec_z, mc->ev_x, mc->ev_z, mc->d_synd_z, B, osdw_x, osdw_z, osd0_z, bp_z, mc->d_conv_z))) return rc;
        break;
    default:
        if ((rc = enqueue_decode(mc, mc->dec_z, mc->ev_sampled, mc->ev_z, mc->d_synd_z, B, nullptr, osdw_z, osd0_z, bp_z, mc->d_conv_z))) return rc;
        if ((rc = enqueue_decode(mc, mc->dec_x, mc->ev_z, mc->ev_x, mc->d_synd_x, B, osdw_z, osdw_x, osd0_x, bp_x, mc->d_conv_x))) return rc;
        break;
    }
    ENGINE_TRY(mc, hipStreamWaitEvent(mc->stream, mc->ev_x, 0));
    ENGINE_TRY(mc, hipStreamWaitEvent(mc->stream, mc->ev_z, 0));

    McScoreParams Q{};
    Q.B = B;
    Q.n = mc->n;
    Q.words = mc->words;
    Q.k = mc->k;
    Q.err_x = mc->d_err_x;
    Q.err_z = mc->d_err_z;
    for (int i = 0; i < 6; ++i) Q.dec[i] = mc->d_out[i];
    Q.conv_x = mc->d_conv_x;
    Q.conv_z = mc->d_conv_z;
    Q.lzT = mc->d_lzT;
    Q.lxT = mc->d_lxT;
    Q.flags = mc->d_flags;
    Q.counters = mc->d_counters;
    hipLaunchKernelGGL(mc_score_kernel, dim3(grid), dim3(MC_THREADS), 6 * sizeof(unsigned long long) * (size_t)mc->words + 8 * sizeof(int), mc->stream, Q);
    ENGINE_TRY(mc, hipGetLastError());
    ENGINE_TRY(mc, hipMemcpyAsync(mc->h_counters.p, mc->d_counters, 7 * sizeof(int), hipMemcpyDeviceToHost, mc->stream));
    ENGINE_TRY(mc, hipStreamSynchronize(mc->stream));  // the batch's one host wait
    for (int i = 0; i < 7; ++i) counters[i] = mc->h_counters.as<int>()[i];
    mc->last_B = B;
    return BPOSD_OK;
}

int bposd_mc_fetch(bposd_mc* mc, int32_t what, void* host_dst, size_t bytes) {
    if (!mc) return BPOSD_ERR_INVALID;
    const size_t words = 8 * (size_t)mc->words;
    const FetchItem items[] = {{mc->d_err_x, words, false},        {mc->d_err_z, words, false},
                               {mc->d_synd_x, (size_t)mc->mz, false}, {mc->d_synd_z, (size_t)mc->mx, false},
                               {mc->d_flags, 1, false},            {mc->d_psynd_x, 8 * (size_t)mc->swx, false},
                               {mc->d_psynd_z, 8 * (size_t)mc->swz, false}};
    return engine_fetch(mc, items, 7, BPOSD_MC_ERROR_X, "BPOSD_MC_ERROR_X .. BPOSD_MC_SYNDROME_Z_PACKED", what, mc->last_B, nullptr, host_dst, bytes);
}

int64_t bposd_mc_device_bytes(bposd_mc* mc) { return mc ? (int64_t)mc->device_bytes : BPOSD_ERR_INVALID; }

}  // extern "C"
