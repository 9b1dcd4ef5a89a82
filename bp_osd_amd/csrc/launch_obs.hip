// launch_obs.hip -- logical observables: the one translation unit that instantiates obs_kernel (obs_kernel.hip.h), its launch
// and the host-side construction of the transposed, packed table it reads.
#include "internal.h"
#include "obs_kernel.hip.h"

using namespace bposd_obs_dev;

namespace bposd_host {

int obs_max_k() { return OBS_MAX_K; }

// L as CSR (k rows, n columns) -> table [ceil(n/64)][k]: bit (c & 63) of table[(c >> 6) * k + j] = L[j][c].  Returns 0, or
// the reason for a refusal in `why` (nothing is written then).
int observable_table(const int32_t* indptr, const int32_t* indices, int k, int n, uint64_t* table, std::string* why) {
    char buf[160];
    auto refuse = [&](const char* fmt, int a, int b, int c) {
        snprintf(buf, sizeof(buf), fmt, a, b, c);
        *why = buf;
        return BPOSD_ERR_INVALID;
    };
    if (!indptr || !table) return refuse("bposd_observable_table: null argument", 0, 0, 0);
    if (k < 1 || k > OBS_MAX_K) return refuse("bposd_observable_table: k = %d is outside 1 .. %d", k, OBS_MAX_K, 0);
    if (n < 1 || n > OBS_MAX_N) return refuse("bposd_observable_table: n = %d is outside 1 .. %d", n, OBS_MAX_N, 0);
    if (indptr[0] != 0) return refuse("bposd_observable_table: indptr[0] must be 0", 0, 0, 0);
    for (int j = 0; j < k; ++j) {
        if (indptr[j + 1] < indptr[j]) return refuse("bposd_observable_table: indptr not monotone at row %d", j, 0, 0);
        if (indptr[j + 1] > indptr[j] && !indices) return refuse("bposd_observable_table: null argument", 0, 0, 0);
        for (int e = indptr[j]; e < indptr[j + 1]; ++e) {
            if (indices[e] < 0 || indices[e] >= n)
                return refuse("bposd_observable_table: row %d holds column %d, outside [0, %d)", j, indices[e], n);
            if (e > indptr[j] && indices[e] <= indices[e - 1])
                return refuse("bposd_observable_table: the columns of row %d are not strictly ascending (at column %d)", j, indices[e], 0);
        }
    }
    const int words = (n + 63) / 64;
    std::fill(table, table + (size_t)words * k, (uint64_t)0);
    for (int j = 0; j < k; ++j)
        for (int e = indptr[j]; e < indptr[j + 1]; ++e) {
            const int c = indices[e];
            table[(size_t)(c >> 6) * k + j] |= (uint64_t)1 << (c & 63);
        }
    return BPOSD_OK;
}

// obs_kernel on `st`: the present row sets of B shots (rows of h->n bits, packed words or bytes) against the handle's table.
int launch_obs(bposd_handle* h, hipStream_t st, const void* const rows[3], bool packed, long long B, uint64_t* const out[3]) {
    if (B <= 0) return 0;
    ObsParams P{};
    P.B = B;
    P.n = h->n;
    P.words = (h->n + 63) / 64;
    P.k = h->obs_k;
    P.kw = (h->obs_k + 63) / 64;
    P.packed = packed ? 1 : 0;
    P.table_in_lds = obs_table_fits_lds(P.words, P.k) ? 1 : 0;
    P.table = h->d_obs_table;
    for (int s = 0; s < OBS_SETS; ++s) {
        P.rows[s] = rows[s];
        P.out[s] = (unsigned long long*)out[s];
    }
    const size_t lds = obs_lds_bytes(P.words, P.k);
    if (lds > 64 * 1024) {
        if (const int rc = set_max_lds(h, (const void*)obs_kernel, lds)) return rc;
    }
    // As many workgroups as are resident at once (by LDS: 2 per CU with the largest table and rows, 8 -- every wave slot -- with
    // the 13 KB of [[1922,50]]), each taking its shots in turn: the kernel is bound by the latency of a shot's two barriers,
    // so resident waves are what hides it, and a workgroup loads its table once.  BPOSD_OBS_WG_PER_CU overrides, for probes.
    int per_cu = 2;
    if (const int rc = cached_occupancy(h, (const void*)obs_kernel, OBS_THREADS, lds, &per_cu)) return rc;
    if (const char* e = getenv("BPOSD_OBS_WG_PER_CU")) per_cu = std::max(1, atoi(e));
    const unsigned grid = (unsigned)std::min<long long>(B, (long long)h->num_cu * per_cu);
    hipLaunchKernelGGL(obs_kernel, dim3(grid), dim3(OBS_THREADS), lds, st, P);
    HIP_TRY(h, hipGetLastError());
    return 0;
}

}  // namespace bposd_host
