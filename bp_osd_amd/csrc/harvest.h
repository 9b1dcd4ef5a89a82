// harvest.h -- the host side of the failing-shot harvest (harvest_kernels.hip.h) that the detector-error-model engine and
// the sliding-window engine share: its state in an engine, switching it, and the three launches behind a scorer.  The
// kernels are instantiated in launch_harvest.hip and nowhere else.  Behind it: the per-fault sums over the rows a harvest
// listed, or over all rows of a batch (fault_sums_kernel.hip.h, instantiated in launch_fault_sums.hip and nowhere else).
//
// Off (max_rows == 0, the default) it is nothing: no launch, no allocation, and the counters' download stays as short as it
// was.  On, an engine's batch gains three launches on the engine's stream between its scorer and the counters' download, so
// a batch keeps its single host wait; the triple (count, min weight, min row) rides in ints 5 .. 7 of the engine's counter
// block (CounterBlock of engine_common.h; neither engine counts beyond int 4) and comes down with the counters.
#pragma once
#include "engine_common.h"

struct Harvest {
    long long max_rows = 0;    // K of bposd_*_set_harvest; 0: off
    long long alloc_rows = 0;  // K the block was carved for (0: no block yet)
    bool last_on = false;      // the engine's last batch ran the harvest: info and the items below are that batch's
    long long last_rows = 0;   // min(count, K) of that batch
    int64_t info[3] = {0, -1, -1};  // count, min weight, min row
    // one device block, carved in this order: residual rows [K][fw], fault rows [K][fw], the lightest residual [fw] (64-bit
    // words), 256 bytes of kernel state, the list [capacity] and the weights [capacity] (ints)
    DevBuf block;
    unsigned long long *d_residual = nullptr, *d_faults = nullptr, *d_min_residual = nullptr;
    void* d_state = nullptr;
    int *d_list = nullptr, *d_weight = nullptr;
    Event ev_t[2];  // around the three launches of the last harvest (bposd_debug_dem_harvest_timing)
    bool on() const { return max_rows > 0; }
};

// What one harvest reads: the batch's flag bytes and which of them select a row, the fault rows, and the corrections in the
// decoder's form (packed words [B][fw], or bytes [B][N]).
struct HarvestJob {
    long long B;
    int N, fw;
    int flag_mask, flag_want;  // row b is selected when (flags[b] & flag_mask) == flag_want
    const uint8_t* flags;
    const unsigned long long* faults;
    const void* corr;
    bool corr_packed;
};

constexpr int HARVEST_TRIPLE_AT = 5;  // ints 5 .. 7 of CounterBlock::d_counters / h_counters

namespace bposd_host {

// Bytes bposd_*_set_harvest adds to an engine's device_bytes: 8 per shot of capacity for list and weights, 2 K rows of
// 8 ceil(N / 64) bytes, one more such row for the lightest residual, and 256 of kernel state.  (The feature was specified
// with 8 capacity + 2 K 8 ceil(N / 64); the lightest residual has to live on the device whether or not its row is among the
// first K, and the running minimum and the count have to live there between the launches, so the block is that much larger
// and the account says so rather than hiding the two in another allocation's slack.)
inline size_t harvest_bytes(long long capacity, long long K, int fw) {
    return 8 * (size_t)capacity + (2 * (size_t)K + 1) * 8 * (size_t)fw + 256;
}

// bposd_*_set_harvest behind the engine's own preconditions.  K < 0 is refused; K == 0 switches off and keeps the block; a K
// beyond what the block was carved for replaces it (the engine's stream is drained first).  A refusal or a failed
// allocation leaves the engine as it was.
int harvest_set(EngineBase* e, Harvest& hv, long long K, int fw);

// The three launches on the engine's stream, between hv.ev_t[0] and hv.ev_t[1]; the triple goes to d_counters[5 .. 7].
// Nothing waits.  The caller downloads 8 counters and, after its host wait, calls harvest_read.
int harvest_enqueue(EngineBase* e, Harvest& hv, const HarvestJob& job, int* d_counters);
void harvest_read(Harvest& hv, const int* h_counters);

// The five fetch items of a harvest in the order of the headers' enums (FAIL_ROWS, FAIL_WEIGHT, FAIL_RESIDUAL, FAIL_FAULTS,
// MIN_RESIDUAL), with the row counts of the last batch.
void harvest_items(const Harvest& hv, int fw, FetchItem out[5]);

// harvest_list_kernel alone on the engine's stream: the rows whose flag byte passes the job's test go to hv.d_list in
// ascending order and their count to the harvest's device state (harvest_count).  Nothing of the job but B and the flags is
// read; the items of a harvest are not formed, so hv.last_on stays false.
int harvest_list_enqueue(EngineBase* e, Harvest& hv, const HarvestJob& job);
// where the device keeps the number of rows the last harvest_list_kernel listed
const int* harvest_count(const Harvest& hv);

}  // namespace bposd_host

// Per-fault sums over selected rows of a batch.  One device block, made by the first call that needs it:
// counts [N] and sums [N] (64-bit words), then the multipliers [capacity] (32-bit).
struct FaultSums {
    DevBuf block;
    unsigned long long *d_counts = nullptr, *d_sums = nullptr;
    uint32_t* d_mult = nullptr;
    Event ev_t[2];       // around the last launch (bposd_debug_dem_fault_sums_timing)
    bool timed = false;  // ... if there was one
};

// What one launch reads: `rows` selected rows of the fault rows [.][fw] -- the rows list[0 .. rows), whose number the device
// also holds in *count (the harvest's list and count), or, list == NULL, the rows 0 .. rows - 1.  The multipliers, if any,
// are in fs.d_mult.
struct FaultSumsJob {
    long long rows;
    int N, fw;
    const unsigned long long* faults;
    const int* list;
    const int* count;
    bool weighted;
};

namespace bposd_host {

inline size_t fault_sums_bytes(long long capacity, int N) { return 16 * (size_t)N + 4 * (size_t)capacity; }

// The block and the events, once; counted in the engine's device_bytes.  A failure leaves the engine as it was.
int fault_sums_ensure(EngineBase* e, FaultSums& fs, int N);
// Clears counts (and sums) and launches the kernel behind it on the engine's stream, between fs.ev_t[0] and fs.ev_t[1];
// with no row selected the arrays are cleared and nothing is launched.  Nothing waits.
int fault_sums_enqueue(EngineBase* e, FaultSums& fs, const FaultSumsJob& job);

}  // namespace bposd_host
