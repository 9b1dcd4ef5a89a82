// launch_fault_sums.hip -- the per-fault sums over selected rows of a detector-error-model batch (harvest.h): the one
// translation unit that instantiates fault_sums_kernel (fault_sums_kernel.hip.h).
#include "harvest.h"
#include "fault_sums_kernel.hip.h"

using namespace bposd_fault_sums_dev;

int bposd_host::fault_sums_ensure(EngineBase* e, FaultSums& fs, int N) {
    if (fs.block.p) return 0;
    // everything that can fail comes first: the events, then the block; only then does the engine change
    for (Event& ev : fs.ev_t)
        if (!ev) ENGINE_TRY(e, hipEventCreate(&ev.raw));
    const size_t bytes = fault_sums_bytes(e->capacity, N);
    DevBuf fresh;
    ENGINE_TRY(e, fresh.alloc(bytes));
    e->device_bytes += bytes;
    fs.block = std::move(fresh);
    fs.d_counts = (unsigned long long*)fs.block.p;
    fs.d_sums = fs.d_counts + N;
    fs.d_mult = (uint32_t*)(fs.d_sums + N);
    fs.timed = false;
    return 0;
}

int bposd_host::fault_sums_enqueue(EngineBase* e, FaultSums& fs, const FaultSumsJob& job) {
    hipStream_t st = e->stream;
    fs.timed = false;
    ENGINE_TRY(e, hipMemsetAsync(fs.d_counts, 0, (job.weighted ? 16 : 8) * (size_t)job.N, st));
    if (job.rows < 1) return 0;
    FaultSumsParams P{};
    P.rows = job.rows;
    P.count = job.count;
    P.list = job.list;
    P.N = job.N;
    P.fw = job.fw;
    P.faults = job.faults;
    P.mult = fs.d_mult;
    P.counts = fs.d_counts;
    P.sums = fs.d_sums;
    // A chunk of the list per workgroup: at least 16 rows a wave, so that a workgroup's flush (up to 4096 global atomics an
    // array) is paid for by rows walked, and no more workgroups than two per CU share the columns of a tile.
    const int num_cu = e->num_cu > 0 ? e->num_cu : 256;
    const long long tiles = (job.fw + FS_TILE_WORDS - 1) / FS_TILE_WORDS;
    const long long by_rows = (job.rows + 16 * FS_WAVES - 1) / (16 * FS_WAVES);
    const long long chunks = std::max<long long>(1, std::min<long long>(by_rows, std::max<long long>(1, 2 * (long long)num_cu / tiles)));
    const dim3 grid((unsigned)tiles, (unsigned)chunks);
    ENGINE_TRY(e, hipEventRecord(fs.ev_t[0], st));
    if (job.weighted) hipLaunchKernelGGL(fault_sums_kernel<true>, grid, dim3(FS_THREADS), 0, st, P);
    else hipLaunchKernelGGL(fault_sums_kernel<false>, grid, dim3(FS_THREADS), 0, st, P);
    ENGINE_TRY(e, hipGetLastError());
    ENGINE_TRY(e, hipEventRecord(fs.ev_t[1], st));
    fs.timed = true;
    return 0;
}
