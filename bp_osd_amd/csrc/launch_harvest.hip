// launch_harvest.hip -- the failing-shot harvest of the detector-error-model engines (harvest.h): the one translation unit
// that instantiates harvest_list_kernel, harvest_rows_kernel and harvest_min_kernel (harvest_kernels.hip.h).
#include "harvest.h"
#include "harvest_kernels.hip.h"

using namespace bposd_harvest_dev;

static_assert(sizeof(HarvestState) <= 256, "the state has 256 bytes of the block");

int bposd_host::harvest_set(EngineBase* e, Harvest& hv, long long K, int fw) {
    if (K < 0) return engine_fail(e, BPOSD_ERR_INVALID, "max_rows = %lld is negative", K);
    if (K > 0x7fffffffLL) return engine_fail(e, BPOSD_ERR_INVALID, "max_rows = %lld is out of range", K);
    if (K > hv.alloc_rows) {
        DeviceGuard guard(e->device);
        ENGINE_TRY(e, guard.err);
        ENGINE_TRY(e, hipStreamSynchronize(e->stream));  // no harvest is writing the block that goes
        // everything that can fail comes first: the events, then the new block; only then does the engine change
        for (Event& ev : hv.ev_t)
            if (!ev) ENGINE_TRY(e, hipEventCreate(&ev.raw));
        const size_t bytes = harvest_bytes(e->capacity, K, fw);
        DevBuf fresh;
        ENGINE_TRY(e, fresh.alloc(bytes));
        if (hv.alloc_rows) e->device_bytes -= harvest_bytes(e->capacity, hv.alloc_rows, fw);
        e->device_bytes += bytes;
        hv.block = std::move(fresh);  // (what the engine held goes with `fresh`)
        hv.alloc_rows = K;
        const size_t row = (size_t)fw, C = (size_t)e->capacity;
        hv.d_residual = (unsigned long long*)hv.block.p;
        hv.d_faults = hv.d_residual + (size_t)K * row;
        hv.d_min_residual = hv.d_faults + (size_t)K * row;
        hv.d_state = hv.d_min_residual + row;
        hv.d_list = (int*)((char*)hv.d_state + 256);
        hv.d_weight = hv.d_list + C;
        hv.last_on = false;  // the last batch's items went with the old block
    }
    hv.max_rows = K;
    return BPOSD_OK;
}

int bposd_host::harvest_enqueue(EngineBase* e, Harvest& hv, const HarvestJob& job, int* d_counters) {
    HarvestParams P{};
    P.B = job.B;
    P.N = job.N;
    P.fw = job.fw;
    P.flag_mask = job.flag_mask;
    P.flag_want = job.flag_want;
    P.max_rows = hv.max_rows;
    P.flags = job.flags;
    P.faults = job.faults;
    P.corr = job.corr;
    P.corr_packed = job.corr_packed ? 1 : 0;
    P.state = (HarvestState*)hv.d_state;
    P.list = hv.d_list;
    P.weight = hv.d_weight;
    P.residual_out = hv.d_residual;
    P.faults_out = hv.d_faults;
    P.min_residual = hv.d_min_residual;
    P.triple = d_counters + HARVEST_TRIPLE_AT;
    hipStream_t st = e->stream;
    hv.last_on = false;
    const int num_cu = e->num_cu > 0 ? e->num_cu : 256;
    const unsigned grid = (unsigned)std::min<long long>((job.B + ROWS_WAVES - 1) / ROWS_WAVES, (long long)num_cu * 8);
    ENGINE_TRY(e, hipEventRecord(hv.ev_t[0], st));
    hipLaunchKernelGGL(harvest_list_kernel, dim3(1), dim3(LIST_THREADS), 0, st, P);
    ENGINE_TRY(e, hipGetLastError());
    hipLaunchKernelGGL(harvest_rows_kernel, dim3(grid), dim3(ROWS_THREADS), 0, st, P);
    ENGINE_TRY(e, hipGetLastError());
    hipLaunchKernelGGL(harvest_min_kernel, dim3(1), dim3(MIN_THREADS), 0, st, P);
    ENGINE_TRY(e, hipGetLastError());
    ENGINE_TRY(e, hipEventRecord(hv.ev_t[1], st));
    return 0;
}

int bposd_host::harvest_list_enqueue(EngineBase* e, Harvest& hv, const HarvestJob& job) {
    HarvestParams P{};
    P.B = job.B;
    P.flag_mask = job.flag_mask;
    P.flag_want = job.flag_want;
    P.flags = job.flags;
    P.state = (HarvestState*)hv.d_state;
    P.list = hv.d_list;
    hv.last_on = false;
    hipLaunchKernelGGL(harvest_list_kernel, dim3(1), dim3(LIST_THREADS), 0, e->stream, P);
    ENGINE_TRY(e, hipGetLastError());
    return 0;
}

const int* bposd_host::harvest_count(const Harvest& hv) { return &((const HarvestState*)hv.d_state)->count; }

void bposd_host::harvest_read(Harvest& hv, const int* h_counters) {
    for (int i = 0; i < 3; ++i) hv.info[i] = h_counters[HARVEST_TRIPLE_AT + i];
    hv.last_rows = std::min<long long>(hv.info[0], hv.max_rows);
    hv.last_on = true;
}

void bposd_host::harvest_items(const Harvest& hv, int fw, FetchItem out[5]) {
    const size_t row = 8 * (size_t)fw;
    const long long count = hv.info[0];
    out[0] = FetchItem{hv.d_list, sizeof(int32_t), false, count};
    out[1] = FetchItem{hv.d_weight, sizeof(int32_t), false, count};
    out[2] = FetchItem{hv.d_residual, row, false, hv.last_rows};
    out[3] = FetchItem{hv.d_faults, row, false, hv.last_rows};
    out[4] = FetchItem{hv.d_min_residual, row, false, 1};
}
