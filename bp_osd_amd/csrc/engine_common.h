// engine_common.h -- what the three Monte-Carlo engines of libbposd_mi355x.so (launch_mc.hip, launch_dem.hip,
// launch_window.hip) share on the host: the state every engine carries, errors and allocation, the validators of their
// matrix operands, the ordering of a decode against the decoder's lanes, the counter readback and the fetch of a batch's
// rows.  Host only: no kernel and no launch parameter lives here.  An engine keeps its own config, tables, kernels and the
// preconditions and wording of its own calls.
#pragma once
#include "internal.h"

#include <cstdarg>
#include <cstring>
#include <memory>

// First in every engine struct.  `stream` is the engine's own; the decoders' lanes are ordered against it by events.
struct EngineBase {
    int device = 0;
    long long capacity = 0;  // rows the per-batch buffers hold
    int num_cu = 0;
    size_t device_bytes = 0;  // what engine_alloc has handed out
    Stream stream;
    std::string err;
};

inline int engine_fail(EngineBase* e, int code, const char* fmt, ...) __attribute__((format(printf, 3, 4)));
inline int engine_fail(EngineBase* e, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);  // (before e->err is written: an argument may be e->err itself)
    va_end(ap);
    if (e) e->err = buf;
    else bposd_host::fail(nullptr, code, "%s", buf);  // read back through bposd_last_error(NULL), like a failed bposd_create
    return code;
}

#define ENGINE_TRY(e, expr)                                                                                              \
    do {                                                                                                                 \
        hipError_t _e = (expr);                                                                                          \
        if (_e != hipSuccess)                                                                                            \
            return engine_fail(e, BPOSD_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)

// A block of at least 256 bytes, counted in the engine's device_bytes (e null: a block of the caller's own).
inline int engine_alloc_bytes(EngineBase* e, DevBuf& p, size_t bytes) {
    bytes = std::max<size_t>(bytes, 256);
    ENGINE_TRY(e, p.alloc(bytes));
    if (e) e->device_bytes += bytes;
    return 0;
}

template <class T>
int engine_alloc(EngineBase* e, DevArray<T>& p, size_t count) {
    return engine_alloc_bytes(e, p, count * sizeof(T));
}

template <class T>
int engine_upload(EngineBase* e, DevArray<T>& p, const T* src, size_t count) {
    if (const int rc = engine_alloc(e, p, count)) return rc;
    if (count) ENGINE_TRY(e, hipMemcpy(p, src, count * sizeof(T), hipMemcpyHostToDevice));
    return 0;
}

inline int engine_check_batch(EngineBase* e, long long B) {
    if (B < 1 || B > e->capacity) return engine_fail(e, BPOSD_ERR_INVALID, "batch size %lld outside [1, capacity %lld]", B, e->capacity);
    return 0;
}

// bposd_*_destroy: the engine's stream is drained on the engine's device before its resources go.
template <class E>
void engine_destroy(E* e) {
    if (!e) return;
    DeviceGuard guard(e->device);  // (outlives the delete)
    if (e->stream) (void)hipStreamSynchronize(e->stream);
    delete e;
}

// The device half of a create: `impl` runs with the engine's device current; what it leaves in e->err becomes the creation
// error (the engine is about to go, and bposd_*_last_error(NULL) is what the caller can still read).
template <class F>
int engine_create_on_device(EngineBase* e, F impl) {
    int rc;
    {
        DeviceGuard guard(e->device);
        rc = guard.err != hipSuccess ? engine_fail(e, BPOSD_ERR_HIP, "hipSetDevice(%d) failed", e->device) : impl();
    }
    return rc ? engine_fail(nullptr, rc, "%s", e->err.c_str()) : 0;
}

namespace bposd_host {

// One CSR operand (rows x cols): 0, or BPOSD_ERR_INVALID with the reason behind `name` in `why`.  The row pointers are
// checked as a whole before any index is read.
inline int check_csr(const char* name, const int32_t* rp, const int32_t* ci, int rows, int cols, bool strictly_ascending, std::string* why) {
    char buf[200];
    auto refuse = [&](const char* fmt, int a, int b, int c) {
        snprintf(buf, sizeof(buf), fmt, name, a, b, c);
        *why = buf;
        return BPOSD_ERR_INVALID;
    };
    if (!rp) return refuse("%s: null indptr", 0, 0, 0);
    if (rp[0] != 0) return refuse("%s: indptr[0] must be 0", 0, 0, 0);
    for (int r = 0; r < rows; ++r)
        if (rp[r + 1] < rp[r]) return refuse("%s: indptr not monotone at row %d", r, 0, 0);
    if (rp[rows] > 0 && !ci) return refuse("%s: null indices", 0, 0, 0);
    for (int r = 0; r < rows; ++r)
        for (int e = rp[r]; e < rp[r + 1]; ++e) {
            if (ci[e] < 0 || ci[e] >= cols) return refuse("%s: row %d holds column %d, outside [0, %d)", r, ci[e], cols);
            if (strictly_ascending && e > rp[r] && ci[e] <= ci[e - 1])
                return refuse("%s: the columns of row %d are not strictly ascending (at column %d)", r, ci[e], 0);
        }
    return 0;
}

// bposd_dem_tables: CSR of H (M x N) and of L (k x N) -> CSC of H stacked on L in the accumulator's bit space: detector r
// is bit r, observable j is bit 64 * ceil(M / 64) + j.  Rows are visited in ascending order, so every column ascends.
inline int dem_tables(const int32_t* h_rp, const int32_t* h_ci, int M, const int32_t* l_rp, const int32_t* l_ci, int k, int N, int32_t* col_ptr,
                      int32_t* col_bits, std::string* why) {
    char buf[160];
    auto refuse = [&](const char* fmt, int a, int b) {
        snprintf(buf, sizeof(buf), fmt, a, b);
        *why = buf;
        return BPOSD_ERR_INVALID;
    };
    if (!col_ptr) return refuse("bposd_dem_tables: null argument", 0, 0);
    if (M < 1 || N < 1) return refuse("bposd_dem_tables: bad shape: M %d, N %d", M, N);
    if (k < 1 || k > obs_max_k()) return refuse("bposd_dem_tables: k = %d is outside 1 .. %d", k, obs_max_k());
    if (check_csr("H", h_rp, h_ci, M, N, true, why) || check_csr("L", l_rp, l_ci, k, N, true, why)) {
        why->insert(0, "bposd_dem_tables: ");
        return BPOSD_ERR_INVALID;
    }
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

// dem_tables into vectors of the caller's: col_bits is sized from the row pointers once those are known to be usable (where
// they are not, dem_tables refuses before it writes).
inline int stacked_csc(const int32_t* h_rp, const int32_t* h_ci, int M, const int32_t* l_rp, const int32_t* l_ci, int k, int N,
                       std::vector<int32_t>* col_ptr, std::vector<int32_t>* col_bits, std::string* why) {
    if (M < 1 || N < 1 || !h_rp || !l_rp) {
        char buf[96];
        snprintf(buf, sizeof(buf), "bad shape or missing matrix: M %d, N %d", M, N);
        *why = buf;
        return BPOSD_ERR_INVALID;
    }
    col_ptr->assign((size_t)N + 1, 0);
    col_bits->clear();
    if (k >= 1 && k <= obs_max_k() && h_rp[0] == 0 && l_rp[0] == 0 && h_rp[M] >= 0 && l_rp[k] >= 0)
        col_bits->resize((size_t)h_rp[M] + (size_t)l_rp[k]);
    return dem_tables(h_rp, h_ci, M, l_rp, l_ci, k, N, col_ptr->data(), col_bits->data(), why);
}

}  // namespace bposd_host

// One decode on the decoder's next lane, ordered behind `after` (an event of the engine's stream or of another lane);
// `done` is recorded on the lane the call took, behind the call.  A decode that fails leaves nothing of the engine's running.
template <class F>
int decode_behind(EngineBase* e, bposd_handle* dec, hipEvent_t after, hipEvent_t done, F call) {
    ENGINE_TRY(e, hipStreamWaitEvent(dec->lanes[dec->next_lane].stream, after, 0));
    if (const int rc = call()) {
        (void)hipStreamSynchronize(e->stream);
        return engine_fail(e, rc, "decode failed: %s", bposd_last_error(dec));
    }
    ENGINE_TRY(e, hipEventRecord(done, dec->lanes[dec->last_lane].stream));
    return 0;
}

// The counters of a scored batch and its failures per observable: zeroed in front of the scorer, and both brought down
// into one page-locked block in front of the batch's one host wait.
struct CounterBlock {
    DevArray<int> d_counters, d_obs_fail;
    PinnedBuf h_counters;  // 8 ints for the counters, and behind them the k ints of obs_fail
    int k = 0;
    int alloc(EngineBase* e, int k_) {
        k = k_;
        if (const int rc = engine_alloc(e, d_counters, 8)) return rc;
        if (const int rc = engine_alloc(e, d_obs_fail, (size_t)k)) return rc;
        ENGINE_TRY(e, h_counters.alloc((8 + (size_t)k) * sizeof(int), hipHostMallocDefault));
        return 0;
    }
    hipError_t reset(hipStream_t st) {
        const hipError_t err = hipMemsetAsync(d_counters, 0, 8 * sizeof(int), st);
        return err != hipSuccess ? err : hipMemsetAsync(d_obs_fail, 0, sizeof(int) * (size_t)k, st);
    }
    hipError_t download(hipStream_t st, int n_counters) {
        const hipError_t err = hipMemcpyAsync(h_counters.p, d_counters, n_counters * sizeof(int), hipMemcpyDeviceToHost, st);
        return err != hipSuccess ? err : hipMemcpyAsync(h_counters.as<int>() + 8, d_obs_fail, sizeof(int) * (size_t)k, hipMemcpyDeviceToHost, st);
    }
    void read(int64_t* out, int n) const {  // (after the host has waited for download's stream)
        for (int i = 0; i < n; ++i) out[i] = h_counters.as<int>()[i];
    }
    const int* obs_fail() const { return h_counters.as<int>() + 8; }
};

// One item of bposd_*_fetch: device rows of row_bytes each, one per shot of the batch or (per_batch) one for the batch; an
// item with a row count of its own (the harvest's: as many rows as the batch had failures) says so in `rows`.
struct FetchItem {
    const void* src;
    size_t row_bytes;
    bool per_batch;
    long long rows = -1;  // >= 0: the item's own row count in the last batch, whatever the batch's
};

// bposd_*_fetch behind the engine's own preconditions: item `what` of items[first_id .. first_id + n_items), `rows` shots
// in the last batch (0: none yet).  The engine's run call has waited for the batch.  The per-batch item is the obs_fail row
// that came down with the counters (pinned_obs_fail): no device call.
inline int engine_fetch(EngineBase* e, const FetchItem* items, int n_items, int first_id, const char* names, int what, long long rows,
                        const int* pinned_obs_fail, void* host_dst, size_t bytes) {
    if (!host_dst) return engine_fail(e, BPOSD_ERR_INVALID, "destination is NULL");
    if (what < first_id || what >= first_id + n_items) return engine_fail(e, BPOSD_ERR_INVALID, "what = %d is not one of %s", what, names);
    if (rows == 0) return engine_fail(e, BPOSD_ERR_INVALID, "no batch has run yet");
    const FetchItem& it = items[what - first_id];
    const size_t want = it.row_bytes * (it.per_batch ? 1 : it.rows >= 0 ? (size_t)it.rows : (size_t)rows);
    if (bytes != want) return engine_fail(e, BPOSD_ERR_INVALID, "the last batch holds %zu bytes of item %d, not %zu", want, what, bytes);
    if (want == 0) return BPOSD_OK;
    if (it.per_batch) {
        memcpy(host_dst, pinned_obs_fail, want);
        return BPOSD_OK;
    }
    DeviceGuard guard(e->device);
    ENGINE_TRY(e, guard.err);
    ENGINE_TRY(e, hipMemcpy(host_dst, it.src, want, hipMemcpyDeviceToHost));
    return BPOSD_OK;
}
