// launch_frame.hip -- Pauli-frame propagation of a circuit's elementary faults: bposd_frame_* of include/bposd_mi355x.h.
// The one translation unit that instantiates frame_propagate_kernel, frame_propagate_layered_kernel, frame_count_kernel and
// frame_fill_kernel (frame_kernels.hip.h).
//
// bposd_frame_columns cuts the faults into chunks of whole words under the workspace budget.  A chunk is: zero the block,
// propagate, count, bring the counts down, prefix sum on the host, fill, bring the indices down.  The frames of a chunk are
// gone when the next one starts, so the host waits twice per chunk; a chunk is a gigabyte of frames by default, and the
// waits do not show.  The columns stay in the handle until bposd_frame_fetch copies them out.
#include "engine_common.h"
#include "frame_kernels.hip.h"

using namespace bposd_frame_dev;

struct bposd_frame : EngineBase {
    int T = 0, Q = 0, M = 0, k = 0, n_meas = 0;
    long long max_words = 0;  // words of a chunk
    bool layered = true;      // frame_propagate_layered_kernel on the groups of the call's faults
    std::vector<int> ops;     // [T][3], for the groups
    // device tables
    DevArray<int> d_ops, d_meas_before, d_md_ptr, d_md_idx, d_mo_ptr, d_mo_idx;
    // per-call blocks: they grow, and are counted in device_bytes at their current size
    DevArray<int> d_pos, d_qa, d_qb, d_cnt, d_off, d_idx, d_grp;
    DevArray<uint8_t> d_pauli;
    DevArray<u64> d_work;
    Event ev[5];  // around propagate, count and fill
    // the last bposd_frame_columns
    bool have = false;
    long long F = 0;
    std::vector<int64_t> h_ptr, l_ptr;
    std::vector<int32_t> h_idx, l_idx;
    double ms[3] = {0, 0, 0};
    long long chunks = 0, launches = 0;
};

namespace {

// a per-call block of at least `count` elements; device_bytes follows its size
template <class T>
int ensure(bposd_frame* fr, DevArray<T>& p, size_t count) {
    const size_t before = p.bytes;
    ENGINE_TRY(fr, p.ensure(count * sizeof(T)));
    fr->device_bytes += p.bytes - before;
    return 0;
}

int create_device(bposd_frame* fr, const std::vector<int>& ops, const std::vector<int>& meas_before, const int32_t* md_ptr, const int32_t* md_idx,
                  const int32_t* mo_ptr, const int32_t* mo_idx) {
    hipDeviceProp_t prop;
    ENGINE_TRY(fr, hipGetDeviceProperties(&prop, fr->device));
    fr->num_cu = prop.multiProcessorCount;
    ENGINE_TRY(fr, hipStreamCreateWithFlags(&fr->stream.raw, hipStreamNonBlocking));
    for (Event& e : fr->ev) ENGINE_TRY(fr, hipEventCreate(&e.raw));
    if (const int rc = engine_upload(fr, fr->d_ops, ops.data(), ops.size())) return rc;
    if (const int rc = engine_upload(fr, fr->d_meas_before, meas_before.data(), meas_before.size())) return rc;
    if (const int rc = engine_upload(fr, fr->d_md_ptr, md_ptr, (size_t)fr->n_meas + 1)) return rc;
    if (const int rc = engine_upload(fr, fr->d_md_idx, md_idx, (size_t)md_ptr[fr->n_meas])) return rc;
    if (const int rc = engine_upload(fr, fr->d_mo_ptr, mo_ptr, (size_t)fr->n_meas + 1)) return rc;
    if (const int rc = engine_upload(fr, fr->d_mo_idx, mo_idx, (size_t)mo_ptr[fr->n_meas])) return rc;
    return 0;
}

// the faults of one call: BPOSD_ERR_INVALID with the first offender named, before anything is uploaded or launched
int check_faults(bposd_frame* fr, const int32_t* pos, const int32_t* qa, const int32_t* qb, const uint8_t* pauli, long long F) {
    for (long long i = 0; i < F; ++i) {
        if (pos[i] < 0 || pos[i] > fr->T) return engine_fail(fr, BPOSD_ERR_INVALID, "fault %lld: pos %d is outside 0 .. T = %d", i, pos[i], fr->T);
        if (i > 0 && pos[i] < pos[i - 1]) return engine_fail(fr, BPOSD_ERR_INVALID, "fault %lld: the faults are not sorted by pos (%d behind %d)", i, pos[i], pos[i - 1]);
        if (qa[i] < 0 || qa[i] >= fr->Q) return engine_fail(fr, BPOSD_ERR_INVALID, "fault %lld: qubit qa = %d is outside [0, %d)", i, qa[i], fr->Q);
        const int pa = pauli[i] & 3, pb = (pauli[i] >> 2) & 3;
        if (pauli[i] > 15) return engine_fail(fr, BPOSD_ERR_INVALID, "fault %lld: Pauli byte %d is not pa | pb << 2", i, pauli[i]);
        if (pa == 0) return engine_fail(fr, BPOSD_ERR_INVALID, "fault %lld: Pauli code 0 on qa (a one-qubit fault of the other qubit goes on qa)", i);
        if (qb == nullptr || qb[i] == -1) {
            if (pb != 0) return engine_fail(fr, BPOSD_ERR_INVALID, "fault %lld: Pauli code %d on qb = -1", i, pb);
            continue;
        }
        if (qb[i] < 0 || qb[i] >= fr->Q) return engine_fail(fr, BPOSD_ERR_INVALID, "fault %lld: qubit qb = %d is outside [0, %d) and not -1", i, qb[i], fr->Q);
        if (qb[i] == qa[i]) return engine_fail(fr, BPOSD_ERR_INVALID, "fault %lld: qa == qb == %d", i, qa[i]);
        if (pb == 0) return engine_fail(fr, BPOSD_ERR_INVALID, "fault %lld: Pauli code 0 on qb = %d (a one-qubit fault has qb = -1)", i, qb[i]);
    }
    return 0;
}

// grp[t]: how many ops from t on frame_propagate_layered_kernel takes as one group (frame_kernels.hip.h).  Op u joins the
// group that starts at t when it is no measurement, shares no qubit with the ops t .. u - 1, and shares none with a fault at
// a position in (t, u]: those faults are injected behind the group, which is the same frame only if no op of the group from
// their position on touches their qubits.
std::vector<int> op_groups(const bposd_frame* fr, const int32_t* pos, const int32_t* qa, const int32_t* qb, long long F) {
    const int T = fr->T;
    std::vector<int> grp((size_t)T, 1);
    std::vector<long long> first((size_t)T + 2, F);  // faults at position t: [first[t], first[t + 1])
    for (long long i = F - 1; i >= 0; --i) first[pos[i]] = i;
    for (int t = T; t >= 0; --t) first[t] = std::min(first[t], first[(size_t)t + 1]);
    std::vector<int> in_op((size_t)fr->Q, -1), in_fault((size_t)fr->Q, -1);
    auto is_meas = [&](int t) { return fr->ops[3 * (size_t)t] >= OP_M && fr->ops[3 * (size_t)t] <= OP_MRX; };
    auto two = [&](int t) { return fr->ops[3 * (size_t)t] == OP_CX || fr->ops[3 * (size_t)t] == OP_CZ; };
    for (int t = 0; t < T; ++t) {
        if (is_meas(t)) continue;
        in_op[fr->ops[3 * (size_t)t + 1]] = t;
        if (two(t)) in_op[fr->ops[3 * (size_t)t + 2]] = t;
        int n = 1;
        for (; n < FRAME_GROUP && t + n < T; ++n) {
            const int u = t + n;
            if (is_meas(u)) break;
            for (long long i = first[u]; i < first[(size_t)u + 1]; ++i) {
                in_fault[qa[i]] = t;
                if (qb && qb[i] >= 0) in_fault[qb[i]] = t;
            }
            const int a = fr->ops[3 * (size_t)u + 1], b = two(u) ? fr->ops[3 * (size_t)u + 2] : a;
            if (in_op[a] == t || in_op[b] == t || in_fault[a] == t || in_fault[b] == t) break;
            in_op[a] = in_op[b] = t;
        }
        grp[t] = n;
    }
    return grp;
}

// chunk [word0, word0 + nw): its columns are appended to the handle's
int run_chunk(bposd_frame* fr, long long word0, int nw, std::vector<int>& cnt, std::vector<int>& off) {
    hipStream_t st = fr->stream;
    const size_t ld = (size_t)nw;
    u64* const x = fr->d_work;
    u64* const z = x + (size_t)fr->Q * ld;
    u64* const D = z + (size_t)fr->Q * ld;
    u64* const O = D + (size_t)fr->M * ld;
    const size_t slots = 64 * ld;  // fault slots of the chunk: [0, slots) of H, [slots, 2 slots) of L
    ENGINE_TRY(fr, hipMemsetAsync(x, 0, 8 * ld * (2 * (size_t)fr->Q + fr->M + fr->k), st));
    ENGINE_TRY(fr, hipMemsetAsync(fr->d_cnt, 0, 2 * slots * sizeof(int), st));

    FramePropagateParams P{};
    P.ops = fr->d_ops;
    P.meas_before = fr->d_meas_before;
    P.T = fr->T;
    P.md_ptr = fr->d_md_ptr;
    P.md_idx = fr->d_md_idx;
    P.mo_ptr = fr->d_mo_ptr;
    P.mo_idx = fr->d_mo_idx;
    P.grp = fr->d_grp;
    P.f_pos = fr->d_pos;
    P.f_qa = fr->d_qa;
    P.f_qb = fr->d_qb;
    P.f_pauli = fr->d_pauli;
    P.F = fr->F;
    P.word0 = word0;
    P.nw = nw;
    P.x = x;
    P.z = z;
    P.D = D;
    P.O = O;
    FrameRowsParams R{};
    R.D = D;
    R.O = O;
    R.M = fr->M;
    R.k = fr->k;
    R.nw = nw;
    R.fault0 = 64 * word0;
    R.F = fr->F;
    R.cnt_h = fr->d_cnt;
    R.cnt_l = fr->d_cnt + slots;

    ENGINE_TRY(fr, hipEventRecord(fr->ev[0], st));
    const dim3 grid((unsigned)((nw + FRAME_THREADS - 1) / FRAME_THREADS));
    if (fr->layered) hipLaunchKernelGGL(frame_propagate_layered_kernel, grid, dim3(FRAME_THREADS), 0, st, P);
    else hipLaunchKernelGGL(frame_propagate_kernel, grid, dim3(FRAME_THREADS), 0, st, P);
    ENGINE_TRY(fr, hipGetLastError());
    ++fr->launches;
    ENGINE_TRY(fr, hipEventRecord(fr->ev[1], st));
    hipLaunchKernelGGL(frame_count_kernel, dim3((unsigned)nw), dim3(64), 0, st, R);
    ENGINE_TRY(fr, hipGetLastError());
    ++fr->launches;
    ENGINE_TRY(fr, hipEventRecord(fr->ev[2], st));
    cnt.resize(2 * slots);
    ENGINE_TRY(fr, hipMemcpyAsync(cnt.data(), fr->d_cnt, 2 * slots * sizeof(int), hipMemcpyDeviceToHost, st));
    ENGINE_TRY(fr, hipStreamSynchronize(st));

    // prefix sums: H's and L's indices of the chunk go into one block, L's behind H's
    off.resize(2 * slots);
    long long nh = 0, nl = 0;
    for (size_t i = 0; i < slots; ++i) nh += cnt[i];
    for (size_t i = 0; i < slots; ++i) nl += cnt[slots + i];
    if (nh + nl > 0x7fffffffLL) return engine_fail(fr, BPOSD_ERR_UNSUPPORTED, "a chunk of %d words holds %lld column entries, more than 2^31 - 1: lower max_words", nw, nh + nl);
    long long run_h = 0, run_l = nh;
    const long long live = std::min<long long>((long long)slots, fr->F - 64 * word0);
    for (long long i = 0; i < live; ++i) {
        off[i] = (int)run_h;
        off[slots + i] = (int)run_l;
        run_h += cnt[i];
        run_l += cnt[slots + i];
        fr->h_ptr.push_back(fr->h_ptr.back() + cnt[i]);
        fr->l_ptr.push_back(fr->l_ptr.back() + cnt[slots + i]);
    }
    for (size_t i = (size_t)live; i < slots; ++i) off[i] = off[slots + i] = 0;
    float t01 = 0, t12 = 0, t34 = 0;
    ENGINE_TRY(fr, hipEventElapsedTime(&t01, fr->ev[0], fr->ev[1]));
    ENGINE_TRY(fr, hipEventElapsedTime(&t12, fr->ev[1], fr->ev[2]));
    fr->ms[0] += t01;
    fr->ms[1] += t12;
    ++fr->chunks;
    if (nh + nl == 0) return 0;

    if (const int rc = ensure(fr, fr->d_idx, (size_t)(nh + nl))) return rc;
    ENGINE_TRY(fr, hipMemcpyAsync(fr->d_off, off.data(), 2 * slots * sizeof(int), hipMemcpyHostToDevice, st));
    R.off_h = fr->d_off;
    R.off_l = fr->d_off + slots;
    R.idx_h = fr->d_idx;
    R.idx_l = fr->d_idx;  // (off_l starts behind H's entries)
    ENGINE_TRY(fr, hipEventRecord(fr->ev[3], st));
    hipLaunchKernelGGL(frame_fill_kernel, dim3((unsigned)nw), dim3(64), 0, st, R);
    ENGINE_TRY(fr, hipGetLastError());
    ++fr->launches;
    ENGINE_TRY(fr, hipEventRecord(fr->ev[4], st));
    const size_t h0 = fr->h_idx.size(), l0 = fr->l_idx.size();
    fr->h_idx.resize(h0 + (size_t)nh);
    fr->l_idx.resize(l0 + (size_t)nl);
    if (nh) ENGINE_TRY(fr, hipMemcpyAsync(fr->h_idx.data() + h0, fr->d_idx, (size_t)nh * sizeof(int), hipMemcpyDeviceToHost, st));
    if (nl) ENGINE_TRY(fr, hipMemcpyAsync(fr->l_idx.data() + l0, fr->d_idx + nh, (size_t)nl * sizeof(int), hipMemcpyDeviceToHost, st));
    ENGINE_TRY(fr, hipStreamSynchronize(st));
    ENGINE_TRY(fr, hipEventElapsedTime(&t34, fr->ev[3], fr->ev[4]));
    fr->ms[2] += t34;
    return 0;
}

}  // namespace

extern "C" {

const char* bposd_frame_last_error(bposd_frame* fr) { return fr ? fr->err.c_str() : bposd_last_error(nullptr); }

void bposd_frame_destroy(bposd_frame* fr) { engine_destroy(fr); }

int64_t bposd_frame_device_bytes(bposd_frame* fr) { return fr ? (int64_t)fr->device_bytes : BPOSD_ERR_INVALID; }

int bposd_frame_create(const bposd_frame_config* cfg, const int32_t* ops, int32_t T, int32_t Q, int32_t n_meas, const int32_t* md_indptr,
                       const int32_t* md_indices, const int32_t* mo_indptr, const int32_t* mo_indices, int32_t M, int32_t k, bposd_frame** out) {
    if (!out) return engine_fail(nullptr, BPOSD_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!cfg) return engine_fail(nullptr, BPOSD_ERR_INVALID, "config is required");
    if (T < 0 || Q < 1 || M < 0 || k < 0 || n_meas < 0 || (T > 0 && !ops))
        return engine_fail(nullptr, BPOSD_ERR_INVALID, "bad shape or missing op table: T %d, Q %d, M %d, k %d, measurements %d", T, Q, M, k, n_meas);
    if (cfg->layered < 0 || cfg->layered > 2) return engine_fail(nullptr, BPOSD_ERR_INVALID, "layered = %d is not 0 (default), 1 (op by op) or 2 (groups)", cfg->layered);
    if (cfg->max_words < 0 || cfg->workspace_bytes < 0)
        return engine_fail(nullptr, BPOSD_ERR_INVALID, "max_words %lld and workspace_bytes %lld must not be negative", (long long)cfg->max_words, (long long)cfg->workspace_bytes);
    std::vector<int> meas_before((size_t)T + 1, 0);
    int seen = 0;
    for (int t = 0; t < T; ++t) {
        const int op = ops[3 * (size_t)t], a = ops[3 * (size_t)t + 1], b = ops[3 * (size_t)t + 2];
        meas_before[t] = seen;
        if (op < 0 || op >= OP_COUNT) return engine_fail(nullptr, BPOSD_ERR_INVALID, "op %d: opcode %d is not one of 0 .. %d", t, op, OP_COUNT - 1);
        if (a < 0 || a >= Q) return engine_fail(nullptr, BPOSD_ERR_INVALID, "op %d: qubit a = %d is outside [0, %d)", t, a, Q);
        if (op == OP_CX || op == OP_CZ) {
            if (b < 0 || b >= Q) return engine_fail(nullptr, BPOSD_ERR_INVALID, "op %d: qubit b = %d is outside [0, %d)", t, b, Q);
            if (a == b) return engine_fail(nullptr, BPOSD_ERR_INVALID, "op %d: a two-qubit op with a == b == %d", t, a);
        }
        if (op >= OP_M && op <= OP_MRX) ++seen;
    }
    meas_before[T] = seen;
    if (seen != n_meas)
        return engine_fail(nullptr, BPOSD_ERR_INVALID, "the op table holds %d measurements, the measurement tables have %d rows: a measurement index is out of range", seen, n_meas);
    std::string why;
    if (bposd_host::check_csr("measurement -> detector", md_indptr, md_indices, n_meas, M, true, &why) ||
        bposd_host::check_csr("measurement -> observable", mo_indptr, mo_indices, n_meas, k, true, &why))
        return engine_fail(nullptr, BPOSD_ERR_INVALID, "%s", why.c_str());

    std::unique_ptr<bposd_frame, decltype(&bposd_frame_destroy)> owner(new bposd_frame(), bposd_frame_destroy);
    bposd_frame* const fr = owner.get();
    fr->device = cfg->device;
    fr->T = T;
    fr->Q = Q;
    fr->M = M;
    fr->k = k;
    fr->n_meas = n_meas;
    fr->layered = cfg->layered != BPOSD_FRAME_OP_BY_OP;
    // words of a chunk: what the byte budget admits (1 GiB unless the caller says otherwise), capped by max_words when that is given
    const long long budget = cfg->workspace_bytes > 0 ? cfg->workspace_bytes : (1LL << 30);
    const long long per_word = 8 * (2 * (long long)Q + M + k) + 2 * 2 * 64 * (long long)sizeof(int);  // frames and rows, counts and offsets
    long long words = std::max<long long>(1, budget / per_word);
    if (cfg->max_words > 0) words = std::min<long long>(words, cfg->max_words);
    fr->max_words = std::min<long long>(words, 1LL << 24);  // (64 nw fault slots stay far inside an int)
    fr->capacity = fr->max_words;
    fr->ops.assign(ops, ops + 3 * (size_t)T);
    if (const int rc = engine_create_on_device(fr, [&] { return create_device(fr, fr->ops, meas_before, md_indptr, md_indices, mo_indptr, mo_indices); })) return rc;
    *out = owner.release();
    return BPOSD_OK;
}

int bposd_frame_columns(bposd_frame* fr, const int32_t* pos, const int32_t* qa, const int32_t* qb, const uint8_t* pauli, int64_t F, int64_t counts_out[2]) {
    if (!fr) return BPOSD_ERR_INVALID;
    fr->have = false;
    if (F < 0 || (F > 0 && (!pos || !qa || !pauli))) return engine_fail(fr, BPOSD_ERR_INVALID, "F = %lld faults need pos, qa and pauli", (long long)F);
    if (const int rc = check_faults(fr, pos, qa, qb, pauli, F)) return rc;
    DeviceGuard guard(fr->device);
    ENGINE_TRY(fr, guard.err);
    fr->F = F;
    fr->h_ptr.assign(1, 0);
    fr->l_ptr.assign(1, 0);
    fr->h_idx.clear();
    fr->l_idx.clear();
    fr->ms[0] = fr->ms[1] = fr->ms[2] = 0;
    fr->chunks = 0;
    const long long W = (F + 63) / 64;
    if (W > 0) {
        const long long wc = std::min<long long>(W, fr->max_words);
        std::vector<int32_t> qb_v;
        if (!qb) qb_v.assign((size_t)F, -1);
        if (const int rc = ensure(fr, fr->d_pos, (size_t)F)) return rc;
        if (const int rc = ensure(fr, fr->d_qa, (size_t)F)) return rc;
        if (const int rc = ensure(fr, fr->d_qb, (size_t)F)) return rc;
        if (const int rc = ensure(fr, fr->d_pauli, (size_t)F)) return rc;
        if (const int rc = ensure(fr, fr->d_work, (size_t)wc * (2 * (size_t)fr->Q + fr->M + fr->k))) return rc;
        if (const int rc = ensure(fr, fr->d_cnt, 2 * 64 * (size_t)wc)) return rc;
        if (const int rc = ensure(fr, fr->d_off, 2 * 64 * (size_t)wc)) return rc;
        ENGINE_TRY(fr, hipMemcpy(fr->d_pos, pos, (size_t)F * sizeof(int), hipMemcpyHostToDevice));
        ENGINE_TRY(fr, hipMemcpy(fr->d_qa, qa, (size_t)F * sizeof(int), hipMemcpyHostToDevice));
        ENGINE_TRY(fr, hipMemcpy(fr->d_qb, qb ? qb : qb_v.data(), (size_t)F * sizeof(int), hipMemcpyHostToDevice));
        ENGINE_TRY(fr, hipMemcpy(fr->d_pauli, pauli, (size_t)F, hipMemcpyHostToDevice));
        if (fr->layered && fr->T > 0) {
            const std::vector<int> grp = op_groups(fr, pos, qa, qb, F);
            if (const int rc = ensure(fr, fr->d_grp, grp.size())) return rc;
            ENGINE_TRY(fr, hipMemcpy(fr->d_grp, grp.data(), grp.size() * sizeof(int), hipMemcpyHostToDevice));
        }
        std::vector<int> cnt, off;
        for (long long w0 = 0; w0 < W; w0 += wc)
            if (const int rc = run_chunk(fr, w0, (int)std::min<long long>(wc, W - w0), cnt, off)) return rc;
    }
    fr->have = true;
    if (counts_out) {
        counts_out[0] = fr->h_ptr.back();
        counts_out[1] = fr->l_ptr.back();
    }
    return BPOSD_OK;
}

int bposd_frame_fetch(bposd_frame* fr, int64_t* h_indptr, int32_t* h_indices, int64_t* l_indptr, int32_t* l_indices) {
    if (!fr) return BPOSD_ERR_INVALID;
    if (!fr->have) return engine_fail(fr, BPOSD_ERR_INVALID, "no bposd_frame_columns call has succeeded yet");
    if (!h_indptr || !l_indptr || (!h_indices && !fr->h_idx.empty()) || (!l_indices && !fr->l_idx.empty()))
        return engine_fail(fr, BPOSD_ERR_INVALID, "a destination is NULL");
    std::copy(fr->h_ptr.begin(), fr->h_ptr.end(), h_indptr);
    std::copy(fr->l_ptr.begin(), fr->l_ptr.end(), l_indptr);
    std::copy(fr->h_idx.begin(), fr->h_idx.end(), h_indices);
    std::copy(fr->l_idx.begin(), fr->l_idx.end(), l_indices);
    return BPOSD_OK;
}

int bposd_debug_frame_timing(bposd_frame* fr, double ms[3], int64_t info[2]) {
    if (!fr) return BPOSD_ERR_INVALID;
    if (ms) {
        if (!fr->have) return engine_fail(fr, BPOSD_ERR_INVALID, "no bposd_frame_columns call has succeeded yet");
        std::copy(fr->ms, fr->ms + 3, ms);
    }
    if (info) {
        info[0] = fr->chunks;
        info[1] = fr->launches;
    }
    return BPOSD_OK;
}

}  // extern "C"
