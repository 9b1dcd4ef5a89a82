// dem_engine.h -- the state of a detector-error-model engine (bposd_dem of include/bposd_mi355x.h), shared by launch_dem.hip,
// which owns it, and launch_window.hip, whose Monte-Carlo run samples on a sample-only engine and reads its rows.
#pragma once
#include "harvest.h"

struct bposd_dem : EngineBase {
    bposd_dem_config cfg{};
    bposd_handle* dec = nullptr;  // NULL: a sample-only engine
    int N = 0, M = 0, k = 0, fw = 0, dw = 0, ow = 0;
    long long sampled_B = 0, scored_B = 0;  // rows of the last batch that items 0-2 / items 3-9 hold
    long long logw_B = 0;                   // rows of the last batch that item 10 holds: sampled_B if it was drawn weighted, else 0
    bool weighted = false;                  // bposd_dem_set_sampling: draw against d_sample_priors and sum d_incr per shot
    // bposd_dem_set_subset: shots are fault sets of a fixed weight (dem_subset_kernel).  One block holds the tables of the
    // mode that is on: binomials (enumerate), increments (if given), support; a switch replaces it.
    int subset_mode = 0, subset_w = 0, subset_n = 0;
    unsigned long long subset_count = 0;  // enumerate: C(n, w), the ranks there are
    bool subset_incr = false;             // an increment table was given: item 10 is valid
    DevBuf subset_block;
    const unsigned long long* d_binom = nullptr;
    const long long* d_subset_incr = nullptr;
    const int* d_support = nullptr;
    Event ev_sampled, ev_decoded;
    Event ev_t[4];  // around the two kernels of the last batch (bposd_debug_dem_timing)
    // device tables
    DevArray<double> d_priors;
    DevArray<int> d_col_ptr, d_col_bits;
    DevArray<double> d_sample_priors;  // importance sampling (allocated by the first bposd_dem_set_sampling)
    DevArray<long long> d_incr;
    // per-batch buffers (capacity rows)
    DevArray<unsigned long long> d_faults, d_detectors, d_observables;
    DevArray<unsigned long long> d_obs_bp, d_obs_osd0, d_obs_osdw;
    DevArray<uint8_t> d_flags, d_conv;
    DevArray<int> d_iters;
    DevArray<long long> d_logw;
    CounterBlock counters;  // 5 counters; with the harvest on, ints 5 .. 7 hold its triple
    Harvest hv;             // bposd_dem_set_harvest (harvest.h)
    FaultSums fs;           // bposd_dem_fault_sums (harvest.h): nothing until the first call
};

namespace bposd_host {

// bposd_dem_sample without the host wait, for another engine's batch: the sampler for rows [0, B) on the engine's stream,
// and `waiter` ordered behind it by the engine's ev_sampled.  Items 0-2 of bposd_dem_fetch hold the batch once the caller
// has waited for `waiter`.  Errors are left in dem->err.
int dem_sample_async(bposd_dem* dem, uint64_t first_shot, int64_t B, hipStream_t waiter);

}  // namespace bposd_host
