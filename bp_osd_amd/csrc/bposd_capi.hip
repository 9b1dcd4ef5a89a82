// bposd_capi.hip -- host side of libbposd_mi355x.so: the C-ABI declared in
// include/bposd_mi355x.h -- creation, the one BP + OSD launch pair every decode call ends in (decode_device_impl: lanes,
// streams, events, kernel dispatch), the device-pointer calls, workspace and HIP-event timing.  The host-pointer calls are in
// decode_host.hip, table construction in host_tables.hip.  gfx950 only; there is no CPU fallback anywhere in this file:
// without a HIP device every entry point fails with BPOSD_ERR_NO_DEVICE.
//
// Reference interface replaced: the `bposd_decoder` / `BpOsdDecoder` object of the
// third-party `ldpc` package as used at /root/reference/README.md:178-202 and
// /root/reference/src/bposd/css_decode_sim.py:444-463,174-202.
#include "../../include/bposd_mi355x.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <climits>
#include <cstring>
#include <string>
#include <tuple>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <vector>

#include "internal.h"
#include <array>

using namespace bposd;
using namespace bposd_host;

namespace {

thread_local std::string g_create_error;

}  // namespace

namespace bposd_host {

int fail(bposd_handle* h, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (h) h->err = buf;
    else g_create_error = buf;
    return code;
}
int sync_all_lanes(bposd_handle* h) {
    for (auto& l : h->lanes) {
        if (l.stream) HIP_TRY(h, hipStreamSynchronize(l.stream));
        if (l.osd_stream) HIP_TRY(h, hipStreamSynchronize(l.osd_stream));
        if (l.copy_stream) HIP_TRY(h, hipStreamSynchronize(l.copy_stream));
    }
    h->async_pending = false;
    return 0;
}

// hipFuncAttributeMaxDynamicSharedMemorySize is a property of the kernel on a device, shared by every handle: it is
// only ever raised (a handle that needs less launches fine under a larger limit), and the API is called only when it
// has to be -- it costs microseconds on the one-syndrome path.
int set_max_lds(bposd_handle* h, const void* kernel, size_t lds) {
    static std::mutex mu;
    static std::map<std::pair<int, const void*>, size_t> limit;
    std::lock_guard<std::mutex> lock(mu);
    size_t& cur = limit[{h->device, kernel}];
    if (lds <= cur) return 0;
    HIP_TRY(h, hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    cur = lds;
    return 0;
}

// Resident workgroups per CU of a kernel at a workgroup size and dynamic-LDS size: asked of the runtime once per process,
// device and configuration (the query costs microseconds on the one-syndrome path).
int cached_occupancy(bposd_handle* h, const void* kernel, int nt, size_t lds, int* out) {
    static std::mutex mu;
    static std::map<std::tuple<int, const void*, int, size_t>, int> memo;
    std::lock_guard<std::mutex> lock(mu);
    auto key = std::make_tuple(h->device, kernel, nt, lds);
    auto it = memo.find(key);
    if (it == memo.end()) {
        int v = 1;
        HIP_TRY(h, hipOccupancyMaxActiveBlocksPerMultiprocessor(&v, kernel, nt, lds));
        it = memo.emplace(key, std::max(v, 1)).first;
    }
    *out = it->second;
    return 0;
}

int ensure(bposd_handle* h, DevBuf& b, size_t bytes) {
    HIP_TRY(h, b.ensure(bytes));
    return 0;
}

// The page-locked counterpart, for a block made with `flags`: nothing happens when it is large enough, else it is freed
// and allocated anew (contents are not kept).
int ensure_pinned(bposd_handle* h, PinnedBuf& b, size_t bytes, unsigned flags) {
    if (bytes <= b.bytes) return 0;
    HIP_TRY(h, b.alloc(bytes, flags));
    return 0;
}

// Workspaces are per lane; when one has to grow, the same buffer of every lane this handle cycles through grows with it,
// so that the allocation (and the page mapping behind it) is paid by the first call of a size class, not by the first
// call that happens to land on each lane.
int ensure_lanes(bposd_handle* h, DevBuf Lane::*member, size_t bytes) {
    for (int l = 0; l < h->nlanes; ++l) {
        int rc = ensure(h, h->lanes[l].*member, bytes);
        if (rc) return rc;
    }
    return 0;
}

// The same buffer of every lane holds at least `bytes`; where one has to grow, the calls in flight are drained first (once
// per entry point: `drained`) -- they may still use the old buffers.  No allocation inside a later call of the same size.
int grow_lanes(bposd_handle* h, DevBuf Lane::*member, size_t bytes, bool* drained) {
    bool have = true;
    for (int l = 0; l < h->nlanes; ++l) have = have && (h->lanes[l].*member).p && (h->lanes[l].*member).bytes >= bytes;
    if (have) return 0;
    if (!*drained && h->async_pending) { int rcs = sync_all_lanes(h); if (rcs) return rcs; }
    *drained = true;
    return ensure_lanes(h, member, bytes);
}
}  // namespace bposd_host

__global__ void pack_rows_kernel(const uint8_t* __restrict__ in, long long B, int n, int wpr,
                                 unsigned long long* __restrict__ out) {
    // one wave per 64-bit output word: lane l supplies bit l (ballot); grid-stride over words
    const long long nwords = B * wpr;
    const int lane = threadIdx.x & 63;
    const long long wave0 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const long long nwave = ((long long)gridDim.x * blockDim.x) >> 6;
    for (long long w = wave0; w < nwords; w += nwave) {
        const long long b = w / wpr;
        const int i = (int)(w - b * wpr) * 64 + lane;
        const bool bit = (i < n) && (in[b * n + i] & 1);
        const unsigned long long v = __ballot(bit);
        if (lane == 0) out[w] = v;
    }
}

// the inverse: B rows of wpr little-endian 64-bit words -> B rows of n 0/1 bytes (the form the decode kernels read)
__global__ void unpack_rows_kernel(const unsigned long long* __restrict__ in, long long B, int n, int wpr, uint8_t* __restrict__ out) {
    const long long total = B * (long long)n;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
        const long long b = e / n;
        const int i = (int)(e - b * n);
        out[e] = (uint8_t)((in[b * wpr + (i >> 6)] >> (i & 63)) & 1ull);
    }
}

namespace bposd_host {

// wg_per_cu caps the grid: 2 inside the decode paths (few, fat workgroups: see launch_unpack), 16 for a stand-alone pack
int launch_pack(bposd_handle* h, hipStream_t st, const uint8_t* d_bytes, long long B, int n, unsigned long long* d_words, int wg_per_cu) {
    if (B <= 0) return 0;
    const int wpr = (n + 63) / 64, threads = 256;
    const long long want = ((long long)B * wpr * 64 + threads - 1) / threads;
    const unsigned grid = (unsigned)std::min<long long>(want, (long long)h->num_cu * wg_per_cu);
    hipLaunchKernelGGL(pack_rows_kernel, dim3(grid), dim3(threads), 0, st, d_bytes, B, n, wpr, d_words);
    HIP_TRY(h, hipGetLastError());
    return 0;
}

int launch_unpack(bposd_handle* h, hipStream_t st, const unsigned long long* d_words, long long B, int n, uint8_t* d_bytes) {
    if (B <= 0) return 0;
    const int wpr = (n + 63) / 64, threads = 256;
    const long long want = ((long long)B * n + threads - 1) / threads;
    // few, fat workgroups: next to a persistent BP grid that takes every slot that frees up, a grid of thousands of short
    // workgroups is starved after its first placements (traced: 6 ms per pack kernel instead of 0.4 ms)
    const unsigned grid = (unsigned)std::min<long long>(want, (long long)h->num_cu * 2);
    hipLaunchKernelGGL(unpack_rows_kernel, dim3(grid), dim3(threads), 0, st, d_words, B, n, wpr, d_bytes);
    HIP_TRY(h, hipGetLastError());
    return 0;
}

// ---- what the decode entry points of this file and of decode_host.hip share (declared in internal.h)
// Does a stage behind BP -- the OSD stage, or the sweep of LSD mode inside the clusters -- rank candidates by the channel's
// weights (else per-shot weight rows are never read)?
bool stage_weighs_candidates(const bposd_handle* h) {
    if (h->cfg.weight_fn != 0) return false;
    if (h->lsd_on && h->lsd_method != BPOSD_LSD_0) return true;  // the sweep inside the clusters weighs like the OSD stage
    return h->cfg.osd_method >= BPOSD_OSD_E && h->cfg.osd_order > 0;
}

// What every decode entry point checks before anything is enqueued (B == 0 is a valid call that does nothing).
int check_batch(bposd_handle* h, int64_t B, const void* synd, const void* osdw) {
    if (!h) return BPOSD_ERR_INVALID;
    if (B < 0 || B > 0x7fffffffLL) return fail(h, BPOSD_ERR_INVALID, "batch size %lld out of range", (long long)B);
    if (B > 0 && (!synd || !osdw)) return fail(h, BPOSD_ERR_INVALID, "syndromes and osdw buffers are required");
    return BPOSD_OK;
}

// A stand-alone device-pointer call takes the handle's next lane and is record 0 of a new "last call".  The entry point
// takes the lane once, stages what the call needs on it and hands it to decode_device_impl.
DecodeCall take_next_lane(bposd_handle* h) {
    const int lane = h->next_lane;
    h->next_lane = (lane + 1) % h->nlanes;
    h->last_lane = lane;
    h->nrec = 0;
    h->async_pending = true;
    Lane& L = h->lanes[lane];
    DecodeCall call{&L, &h->lane_rec[lane], L.osd_stream};  // stream order on the lane: its previous call has filled the record by now
    call.device_ptr = true;
    return call;
}

static int report_osd_debug(bposd_handle* h, const DecodeCall& call);

// One BP launch + one OSD launch on the call's lane, `io` in device memory.
int decode_device_impl(bposd_handle* h, const DecodeCall& call, const IoPtrs& io, int64_t B) {
    // lean (the small host-pointer call): everything on the lane's own stream in program order -- no events, no second
    // stream -- so that the call costs a memset, two launches, one 32-byte copy and one synchronisation
    DeviceGuard dev_guard(h->device);
    HIP_TRY(h, dev_guard.err);
    Lane& L = *call.lane;
    CallRecord& R = *call.rec;
    const bool lean = call.lean;
    const bool osd_kernel_on = h->cfg.osd_method != BPOSD_OSD_OFF && !call.bp_only;
    const bool lsd_on = h->lsd_on && !call.bp_only;  // LSD mode: lsd_kernel consumes BP's list, with or without an OSD kernel behind it
    const bool osd_on = osd_kernel_on || lsd_on;     // BP leaves a list, and something runs over it on the OSD stream
    int rc;
    if (osd_on) {
        if ((rc = ensure_lanes(h, &Lane::llr_ws, sizeof(double) * (size_t)B * h->n))) return rc;
        if ((rc = ensure_lanes(h, &Lane::osd_list, sizeof(int) * (size_t)B))) return rc;
    }
    HIP_TRY(h, hipMemsetAsync(L.d_counters, 0, bposd_local_park::kCounterBytes, L.stream));

    BpParams P{};
    P.m = h->m;
    P.n = h->n;
    P.B = B;
    P.max_iter = h->max_iter;
    P.ms_scaling = h->cfg.ms_scaling_factor;
    P.ps_clip = h->cfg.ps_clip;
    P.osd_enabled = osd_on ? 1 : 0;
    P.synd = io.synd;
    P.llr0 = h->d_llr0;
    P.sel = io.sel;
    P.llr0_alt = call.lane_alt ? L.d_alt : h->d_llr0_alt;
    P.llr0_rows = io.llr0_rows;
    P.chk_deg = h->d_chk_deg;
    P.var_deg = h->d_var_deg;
    P.var_pos = h->d_var_pos;
    P.pos_bit = h->d_pos_bit;
    P.out_bp = io.bp;
    P.out_osd0 = io.osd0;
    P.out_osdw = io.osdw;
    P.out_conv = io.conv;
    P.out_iters = io.iters;
    P.out_llr = io.llr;
    P.llr_ws = (double*)L.llr_ws.p;
    P.osd_list = (int*)L.osd_list.p;
    P.counters = L.d_counters;
    P.iter_total = (unsigned long long*)(L.d_counters + 4);
    P.tail_flag = call.tail_gate ? L.h_tail.as<int>() : nullptr;
    P.packed_io = call.packed ? 1 : 0;

    // At most TWO calls have kernels on the device: this call's BP kernel waits for the END of the call two back (its OSD
    // kernel included).  (i) A third BP kernel that became ready meanwhile would share the slots the first one frees with the
    // second from the first workgroup on -- both then take twice as long and finish together.  (ii) The OSD kernel needs a
    // whole CU (131 KB of LDS for H1922); while ANY persistent BP grid is waiting, every slot a draining CU frees goes to a BP
    // workgroup, which fits, and the eliminations of call k starve until the pipeline runs dry (traced with three and four
    // asynchronous host calls in flight: completions came in bursts of three).  With this rule OSD(k) gets its CUs in the tail
    // of BP(k + 1), whatever the number of calls queued -- and only as fast as that tail frees whole CUs: a workgroup of the
    // persistent grid finishes the shot it holds after the queue has run dry, a max_iter straggler pins its CU for
    // milliseconds, and BP(k + 2) waits behind that ramp and the eliminations.  The local-edge kernel therefore ends its
    // first launch at the drain (park at drain, local_park.h / launch_bp_local.h: unfinished shots go into records, a second
    // launch of the kernel's small footprint finishes them next to OSD(k) and BP(k + 2)); the other BP kernels drain as before.
    // (Not where BP is HBM-resident: there both kernels need a whole CU, the OSD stream has the higher priority, and three calls in
    // flight are what fills the CUs -- see the lane count in bposd_create.  BPOSD_TWO_BACK=0/1 overrides, for probes.)
    static const char* two_back_env = getenv("BPOSD_TWO_BACK");
    const bool two_back_rule = two_back_env ? two_back_env[0] == '1' : !h->bp_hbm;
    if (!lean && !call.tail_gate && h->nlanes >= 3 && two_back_rule) {  // (the chunks of a synchronous host call are released one by one by the host: tail_gate)
        Lane& two_back = h->lanes[((int)(call.lane - h->lanes) + h->nlanes - 2) % h->nlanes];
        if (two_back.done_recorded) HIP_TRY(h, hipStreamWaitEvent(L.stream, two_back.ev_done, 0));
    }
    if (!lean) HIP_TRY(h, hipEventRecord(R.ev[0], L.stream));
    L.relay_B = -1;  // (launch_bp_relay sets it)
    L.lsd_B = -1;    // (launch_lsd sets it)
    if (h->relay_legs > 0) {
        h->last_bp_kernel = BPOSD_BP_KERNEL_RELAY;
        if ((rc = launch_bp_relay(h, call, P))) return rc;
    } else if (h->cfg.schedule == 1) {
        h->last_bp_kernel = BPOSD_BP_KERNEL_SERIAL;
        if ((rc = launch_bp_serial(h, call, P))) return rc;
    } else if (h->bp_any || h->bp_variant == 64) {
        h->last_bp_kernel = BPOSD_BP_KERNEL_ANYDEG;
        if ((rc = launch_bp_any(h, call, P))) return rc;
    } else if (h->bp_hbm) {
        h->last_bp_kernel = BPOSD_BP_KERNEL_LARGE;
        if ((rc = launch_bp_large(h, call, P))) return rc;
    } else if (h->local_ok && h->cfg.bp_method == BPOSD_BP_MIN_SUM && (h->bp_variant == 0 || (h->bp_variant >= 16 && h->bp_variant <= 26))) {
        h->last_bp_kernel = BPOSD_BP_KERNEL_LOCAL;
        if ((rc = launch_bp_local(h, call, P))) return rc;
    } else if (h->class_ok && (h->bp_variant == 32 || (h->bp_variant == 0 && class_preferred(h)))) {
        h->last_bp_kernel = BPOSD_BP_KERNEL_CLASS;
        if ((rc = launch_bp_class(h, call, P))) return rc;
    } else {
        h->last_bp_kernel = BPOSD_BP_KERNEL_LDS;
        if ((rc = launch_bp(h, call, P))) return rc;
    }
    if (!lean) HIP_TRY(h, hipEventRecord(R.ev[1], L.stream));
    R.ran_osd = false;
    R.ran_obs = false;
    if (!lean && (osd_on || call.tail_gate)) HIP_TRY(h, hipEventRecord(L.ev_bp, L.stream));  // the BP kernel has ended
    if (osd_on) {
        if (!lean) HIP_TRY(h, hipStreamWaitEvent(L.osd_stream, L.ev_bp, 0));
        OsdParams Q{};
        Q.m = h->m;
        Q.n = h->n;
        Q.rank = h->rank;
        Q.osd_method = h->cfg.osd_order == 0 ? BPOSD_OSD_0 : h->cfg.osd_method;
        Q.osd_order = h->cfg.osd_order;
        Q.tie_policy = h->cfg.sort_tie_policy;
        Q.e_msb_first = h->cfg.osd_e_bit_order;
        Q.synd = io.synd;
        Q.rp = h->d_rp;
        Q.ci = h->d_ci;
        Q.llr_ws = (const double*)L.llr_ws.p;
        Q.osd_list = (const int*)L.osd_list.p;
        Q.counters = L.d_counters;
        Q.out_osd0 = io.osd0;
        Q.out_osdw = io.osdw;
        Q.cmp_osd0 = io.osd0 ? call.cmp_osd0 : nullptr;
        Q.cmp_osdw = call.cmp_osdw;
        Q.dbg = nullptr;
        Q.packed_io = call.packed ? 1 : 0;
        Q.cost = (h->fp_weights || ((io.sel || io.cost_rows) && h->cfg.weight_fn == 0)) ? h->d_cost : nullptr;  // (non-null = the fp64 weight path)
        Q.cost_rows = h->cfg.weight_fn == 0 ? io.cost_rows : nullptr;
        Q.sel = io.sel;
        Q.cost_alt = call.lane_alt ? L.d_alt + h->n : h->d_cost_alt;
        const char* dbg_env = getenv("BPOSD_OSD_DEBUG");
        if (dbg_env && dbg_env[0] == '1') {
            if (!L.d_osd_dbg) HIP_TRY(h, L.d_osd_dbg.alloc(8192 * sizeof(long long)));
            HIP_TRY(h, hipMemsetAsync(L.d_osd_dbg, 0, 8192 * sizeof(long long), call.osd_stream));
            Q.dbg = L.d_osd_dbg;
        }
        // LSD mode: lsd_kernel first; the OSD kernel then walks the list of the shots it handed on (launch_lsd redirects Q)
        if (lsd_on && (rc = launch_lsd(h, call, Q, B, osd_kernel_on))) return rc;
        if (osd_kernel_on) {
            if (h->large) {
                h->last_osd_kernel = 3;
                if ((rc = launch_osd_large(h, call, Q, B, nullptr))) return rc;
            } else if ((rc = launch_osd(h, call, Q, B))) return rc;
            if (lsd_on && (rc = launch_lsd_compact(h, call, Q, (const int*)L.osd_list.p, L.d_counters, io.osd0 ? call.cmp_osd0 : nullptr, call.cmp_osdw, B))) return rc;
        }
        R.ran_osd = true;
        if (Q.dbg && osd_kernel_on && (rc = report_osd_debug(h, call))) return rc;
    }
    if (osd_on && !lean) {  // whatever follows on the lane's stream comes after the OSD kernel
        HIP_TRY(h, hipEventRecord(L.ev_osd, L.osd_stream));
        L.osd_recorded = true;
        HIP_TRY(h, hipStreamWaitEvent(L.stream, L.ev_osd, 0));
    }
    if (!lean) {
        HIP_TRY(h, hipEventRecord(R.ev[2], L.stream));
        HIP_TRY(h, hipEventRecord(L.ev_done, L.stream));  // both kernels of this call have ended
        L.done_recorded = true;
    }
    HIP_TRY(h, hipMemcpyAsync(R.counters(), L.d_counters, 32, hipMemcpyDeviceToHost, L.stream));
    R.recorded = true;
    R.timed = !lean;
    h->have_timing = true;
    return BPOSD_OK;
}

// BPOSD_OSD_DEBUG=1: waits for the call's OSD kernel and prints the phase timestamps it left in the lane's d_osd_dbg
static int report_osd_debug(bposd_handle* h, const DecodeCall& call) {
    std::vector<long long> all(h->large ? 8192 : 2048);
    const long long* st = all.data();
    HIP_TRY(h, hipStreamSynchronize(call.osd_stream));
    HIP_TRY(h, hipMemcpy(all.data(), call.lane->d_osd_dbg, sizeof(long long) * all.size(), hipMemcpyDeviceToHost));
    if (!h->large) {
        if (const char* dump = getenv("BPOSD_OSD_DUMP")) {
            if (FILE* f = fopen(dump, "wb")) { fwrite(st, sizeof(long long), 2048, f); fclose(f); }
        }
        fprintf(stderr, "[bposd osd phases, s_memtime ticks] sort %lld  rowbuild %lld  eliminate %lld  osd0 %lld  sweep %lld  write %lld\n",
                st[1] - st[0], st[2] - st[1], st[3] - st[2], st[4] - st[3], st[5] - st[4], st[6] - st[5]);
        fprintf(stderr, "[bposd osd elimination] panel phase %lld (claims + barrier %lld, solve + tables %lld of which the six steps %lld, absorb %lld)  trailing phase %lld (publish %lld, tables %lld)  pivots %lld\n", st[1190], st[1195], st[1196], st[1189], st[1197], st[1191], st[1193], st[1194], st[1192]);
        return 0;
    }
    fprintf(stderr, "[bposd large osd, sparse apply passes %lld: %lld ticks, %lld listed rows, %lld mask bits; word of the last search column %lld]\n", st[12], st[24], st[25], st[26], st[27]);
    fprintf(stderr, "[bposd large osd, s_memtime ticks, list slot 0] sort %lld  build %lld  E1 %lld  E2 %lld  E3 %lld  apply %lld  "
            "sweep %lld (back-substitution %lld, column vectors %lld, candidates %lld, write-out %lld) | words %lld groups %lld applies %lld | apply look-ups/thread %lld row-words/thread %lld | apply pass: row walks %lld, wait for the slowest walker %lld, own table build %lld, wait for the builders %lld, list builds %lld\n", st[0], st[1], st[2], st[3], st[4], st[5] + st[17] + st[18] + st[19] + st[20], st[6], st[13], st[14], st[15], st[16], st[7], st[8], st[9], st[10], st[11], st[5], st[19], st[17], st[18], st[20]);
    // every elimination of the launch (osd_large_kernel writes 16 numbers per list slot behind the first 32)
    std::vector<std::array<long long, 16>> v;
    for (int i = 0; i < 500; ++i)
        if (all[32 + i * 16] > 0) {
            std::array<long long, 16> a;
            for (int k = 0; k < 16; ++k) a[k] = all[32 + i * 16 + k];
            v.push_back(a);
        }
    if (v.size() <= 1) return 0;
    std::sort(v.begin(), v.end());
    fprintf(stderr, "[bposd large osd, all %zu eliminations of the launch, sorted by ticks] M ticks: total | sort build E2 E3 row-walks sweep | words groups applies | own-table-build E1c E2c-one-wave sparse-apply-passes | wave 0's pivot search alone (E2 column = the rest of the panel phase; E2c-one-wave = the wait for the other waves' share of E3 after it)\n", v.size());
    for (size_t i = 0; i < v.size(); i += (i + 8 < v.size() ? v.size() / 8 : 1)) {
        const auto& a = v[i];
        fprintf(stderr, "  [%3zu] %.0f | %.1f %.1f %.1f %.1f %.1f %.1f | %lld %lld %lld | %.1f %.1f %.1f %.1f | %.1f\n", i, a[0] * 1e-6, a[1] * 1e-6, a[2] * 1e-6, a[4] * 1e-6, a[5] * 1e-6,
                a[6] * 1e-6, a[7] * 1e-6, a[8], a[9], a[10], a[12] * 1e-6, a[13] * 1e-6, a[14] * 1e-6, a[15] * 1e-6, a[3] * 1e-6);
    }
    return 0;
}

// the alternative channel of the two-valued per-shot form: validated first, then its prior LLRs and OSD-W weights
int check_alt_channel(bposd_handle* h, const double* alt) {
    if (!alt) return fail(h, BPOSD_ERR_INVALID, "channel_probs_alt is required");
    if (const int64_t bad = first_bad_prob(alt, h->n))
        return fail(h, BPOSD_ERR_INVALID, "channel_probs_alt[%d] = %g is not a probability", (int)(bad - 1), alt[bad - 1]);
    return 0;
}

static void alt_channel_tables(int n, const double* alt, double* l0, double* cost) { (void)channel_tables(alt, n, l0, cost); }

int upload_alt_channel(bposd_handle* h, const double* alt) {
    { int rca = check_alt_channel(h, alt); if (rca) return rca; }
    std::vector<double> l0(h->n), cost(h->n);
    alt_channel_tables(h->n, alt, l0.data(), cost.data());
    DeviceGuard dev_guard(h->device);
    HIP_TRY(h, dev_guard.err);
    { int rcs = sync_all_lanes(h); if (rcs) return rcs; }  // earlier calls may still read the old tables
    HIP_TRY(h, hipMemcpy(h->d_llr0_alt, l0.data(), sizeof(double) * h->n, hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(h->d_cost_alt, cost.data(), sizeof(double) * h->n, hipMemcpyHostToDevice));
    return 0;
}

int check_observables(bposd_handle* h) {
    if (!h) return BPOSD_ERR_INVALID;
    if (h->obs_k <= 0) return fail(h, BPOSD_ERR_INVALID, "no observables are set on this handle (bposd_set_observables)");
    return BPOSD_OK;
}

// Lane buffers of an observables decode of up to `cap` syndromes: the rows the kernels write (packed where the kernels are,
// bytes otherwise), the syndromes in the kernels' form where the caller's are in the other one, and for a host-pointer
// call the syndromes as uploaded and the outputs to download.
int obs_reserve(bposd_handle* h, size_t cap, const ObsOut& out, bool host, bool synd_packed) {
    const bool native = native_packed(h);
    const size_t rs = row_bytes(h->n, native), ob = sizeof(uint64_t) * (size_t)((h->obs_k + 63) / 64);
    bool drained = false;
    int rc;
    if ((rc = grow_lanes(h, native ? &Lane::io_posdw : &Lane::io_osdw, cap * rs, &drained))) return rc;
    if (out.osd0 && (rc = grow_lanes(h, native ? &Lane::io_posd0 : &Lane::io_osd0, cap * rs, &drained))) return rc;
    if (out.bp && (rc = grow_lanes(h, native ? &Lane::io_pbp : &Lane::io_bp, cap * rs, &drained))) return rc;
    if ((host || native != synd_packed) && (rc = grow_lanes(h, native ? &Lane::io_psynd : &Lane::io_synd, cap * row_bytes(h->m, native), &drained))) return rc;
    if (!host) return 0;
    if (native != synd_packed && (rc = grow_lanes(h, synd_packed ? &Lane::io_psynd : &Lane::io_synd, cap * row_bytes(h->m, synd_packed), &drained))) return rc;
    if ((rc = grow_lanes(h, &Lane::io_obsw, cap * ob, &drained))) return rc;
    if (out.osd0 && (rc = grow_lanes(h, &Lane::io_obs0, cap * ob, &drained))) return rc;
    if (out.bp && (rc = grow_lanes(h, &Lane::io_obsbp, cap * ob, &drained))) return rc;
    if ((rc = grow_lanes(h, &Lane::io_conv, cap, &drained))) return rc;
    return grow_lanes(h, &Lane::io_iters, sizeof(int) * cap, &drained);
}

// One decode into the lane's own row buffers with obs_kernel behind it, everything on the call's lane: `d_synd` (bytes or
// packed words) is brought into the kernels' form first where it is in the other one; `out` is device memory.
int decode_obs_impl(bposd_handle* h, DecodeCall call, const void* d_synd, bool synd_packed, int64_t B, const ObsOut& out) {
    Lane& L = *call.lane;
    // the lane's io buffers are also read by its copy stream in the host-pointer decode path
    if (L.copy_pending) { HIP_TRY(h, hipStreamSynchronize(L.copy_stream)); L.copy_pending = false; }
    const bool native = native_packed(h);
    int rc;
    if (native && !synd_packed) {
        if ((rc = launch_pack(h, L.stream, (const uint8_t*)d_synd, B, h->m, (unsigned long long*)L.io_psynd.p))) return rc;
        d_synd = L.io_psynd.p;
    } else if (!native && synd_packed) {
        if ((rc = launch_unpack(h, L.stream, (const unsigned long long*)d_synd, B, h->m, (uint8_t*)L.io_synd.p))) return rc;
        d_synd = L.io_synd.p;
    }
    call.packed = native;
    IoPtrs want;  // (which of the lane's row buffers the call writes: the ones whose observables are asked for)
    want.osd0 = (uint8_t*)out.osd0;
    want.bp = (uint8_t*)out.bp;
    IoPtrs dev = lane_ptrs(L, native, want);
    dev.synd = (const uint8_t*)d_synd;
    dev.conv = out.conv;
    dev.iters = out.iters;
    if ((rc = decode_device_impl(h, call, dev, B))) return rc;
    // (decode_device_impl has made the lane's stream wait for the OSD kernel: the rows are final)
    const void* const rows[3] = {dev.osdw, dev.osd0, dev.bp};
    uint64_t* const outs[3] = {out.osdw, out.osd0, out.bp};
    CallRecord& R = *call.rec;  // (bposd_last_timing's events end in front of obs_kernel: it has a pair of its own)
    for (auto& e : R.ev_obs)
        if (!e) HIP_TRY(h, hipEventCreate(&e.raw));
    HIP_TRY(h, hipEventRecord(R.ev_obs[0], L.stream));
    if ((rc = launch_obs(h, L.stream, rows, native, B, outs))) return rc;
    HIP_TRY(h, hipEventRecord(R.ev_obs[1], L.stream));
    R.ran_obs = true;
    return 0;
}

}  // namespace bposd_host

// ================================================================================ C-ABI
extern "C" {

int bposd_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char* bposd_version(void) { return "bposd_mi355x 0.1 (gfx950)"; }

const char* bposd_last_error(bposd_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

void bposd_destroy(bposd_handle* h) {
    if (!h) return;
    DeviceGuard dev_guard(h->device);  // (outlives the delete: the members free themselves on the handle's device)
    for (auto& l : h->lanes) {
        if (l.stream) (void)hipStreamSynchronize(l.stream);
        if (l.osd_stream) (void)hipStreamSynchronize(l.osd_stream);
    }
    delete h;
}

int bposd_create(const bposd_config* cfg, const int32_t* indptr, const int32_t* indices, int32_t m,
                 int32_t n, const double* channel_probs, bposd_handle** out) {
    if (out) *out = nullptr;
    if (!cfg || !indptr || !indices || !channel_probs || !out)
        return fail(nullptr, BPOSD_ERR_INVALID, "null argument");
    if (m <= 0 || n <= 0) return fail(nullptr, BPOSD_ERR_INVALID, "empty parity-check matrix (%d x %d)", m, n);
    if (cfg->bp_method != BPOSD_BP_PRODUCT_SUM && cfg->bp_method != BPOSD_BP_MIN_SUM)
        return fail(nullptr, BPOSD_ERR_INVALID, "bp_method must be 0 (product-sum) or 1 (min-sum)");
    if (cfg->osd_method < BPOSD_OSD_OFF || cfg->osd_method > BPOSD_OSD_CS)
        return fail(nullptr, BPOSD_ERR_INVALID, "osd_method out of range");
    if (cfg->max_iter < 0 || cfg->osd_order < 0) return fail(nullptr, BPOSD_ERR_INVALID, "negative max_iter / osd_order");
    if (cfg->sort_tie_policy < 0 || cfg->sort_tie_policy > 1 || cfg->weight_fn < 0 || cfg->weight_fn > 1)
        return fail(nullptr, BPOSD_ERR_INVALID, "sort_tie_policy / weight_fn out of range");
    if (cfg->osd_e_bit_order < 0 || cfg->osd_e_bit_order > 1)
        return fail(nullptr, BPOSD_ERR_INVALID, "osd_e_bit_order must be 0 (LSB first) or 1 (MSB first)");
    if (cfg->ps_math_form < 0 || cfg->ps_math_form > 1)
        return fail(nullptr, BPOSD_ERR_INVALID, "ps_math_form must be 0 (the reference's operation order) or 1 (two divisions per edge)");
    if (cfg->schedule != 0 && cfg->schedule != 1) return fail(nullptr, BPOSD_ERR_INVALID, "schedule must be 0 (parallel) or 1 (serial)");
    if (!(cfg->ps_clip >= 0.0) || std::isinf(cfg->ps_clip)) return fail(nullptr, BPOSD_ERR_INVALID, "ps_clip must be 0 (off) or a finite positive bound");
    if (indptr[0] != 0) return fail(nullptr, BPOSD_ERR_INVALID, "csr_indptr[0] must be 0");
    for (int c = 0; c < m; ++c) {
        if (indptr[c + 1] < indptr[c]) return fail(nullptr, BPOSD_ERR_INVALID, "csr_indptr not monotone");
        for (int e = indptr[c]; e < indptr[c + 1]; ++e) {
            if (indices[e] < 0 || indices[e] >= n) return fail(nullptr, BPOSD_ERR_INVALID, "column index out of range");
            if (e > indptr[c] && indices[e] <= indices[e - 1])
                return fail(nullptr, BPOSD_ERR_INVALID, "column indices must be strictly ascending within a row");
        }
    }
    if (const int64_t bad = first_bad_prob(channel_probs, n))
        return fail(nullptr, BPOSD_ERR_INVALID, "channel_probs[%d] = %g is not a probability", (int)(bad - 1), channel_probs[bad - 1]);

    int ndev = bposd_device_count();
    if (ndev <= 0) return fail(nullptr, BPOSD_ERR_NO_DEVICE, "no HIP device visible: the MI355X decoder has no CPU path");
    if (cfg->device < 0 || cfg->device >= ndev)
        return fail(nullptr, BPOSD_ERR_INVALID, "device %d out of range (%d visible)", cfg->device, ndev);

    // Whatever the handle holds by the time a check below fails goes back with it: every failure is a plain return.
    std::unique_ptr<bposd_handle, decltype(&bposd_destroy)> owner(new bposd_handle(), bposd_destroy);
    bposd_handle* const h = owner.get();
    h->cfg = *cfg;
    h->device = cfg->device;
    h->m = m;
    h->n = n;
    h->E = indptr[m];
    h->rp.assign(indptr, indptr + m + 1);
    h->ci.assign(indices, indices + h->E);
    h->probs.assign(channel_probs, channel_probs + n);
    h->max_iter = cfg->max_iter > 0 ? cfg->max_iter : n;  // A.1: 0 => block length

    // a HIP call of the creation: a failure names it in the creation error
#define CREATE_HIP(expr)                                                                        \
    do {                                                                                        \
        hipError_t _e = (expr);                                                                 \
        if (_e != hipSuccess) return fail(nullptr, BPOSD_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(_e)); \
    } while (0)
    auto failed = [h](int rc) { g_create_error = h->err; return rc; };  // a step that left its message in the handle
    int rc;

    DeviceGuard dev_guard(h->device);
    CREATE_HIP(dev_guard.err);
    hipDeviceProp_t prop;
    CREATE_HIP(hipGetDeviceProperties(&prop, h->device));
    h->num_cu = prop.multiProcessorCount;
    if (prop.maxSharedMemoryPerMultiProcessor > 0) h->lds_per_cu = prop.maxSharedMemoryPerMultiProcessor;
    int prio_least = 0, prio_greatest = 0;
    CREATE_HIP(hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest));
    for (auto& l : h->lanes) {
        CREATE_HIP(hipStreamCreateWithFlags(&l.stream.raw, hipStreamNonBlocking));
        CREATE_HIP(hipStreamCreateWithPriority(&l.osd_stream.raw, hipStreamNonBlocking, prio_greatest));
        for (Event* e : {&l.ev_bp, &l.ev_osd, &l.ev_park, &l.ev_done, &l.ev_up, &l.ev_copy}) CREATE_HIP(hipEventCreateWithFlags(&e->raw, hipEventDisableTiming));
        CREATE_HIP(hipStreamCreateWithFlags(&l.copy_stream.raw, hipStreamNonBlocking));
        CREATE_HIP(l.d_counters.alloc(bposd_local_park::kCounterBytes));  // 4 counters + the 64-bit iteration total (one copy) + the park words: one memset
        CREATE_HIP(hipMemset(l.d_counters, 0, bposd_local_park::kCounterBytes));  // (bposd_debug_last_parked of a lane no call has run on reads 0, not what the allocation held)
        CREATE_HIP(l.h_tail.alloc(64, hipHostMallocMapped));
        *l.h_tail.as<int>() = 0;
    }
    for (CallRecord* rs : {h->rec, h->lane_rec})
        for (int k = 0; k < (rs == h->rec ? BPOSD_MAX_CHUNKS : BPOSD_LANES); ++k) {
            for (auto& e : rs[k].ev) CREATE_HIP(hipEventCreate(&e.raw));
            CREATE_HIP(rs[k].h_counters.alloc(32, hipHostMallocDefault));
            rs[k].counters()[0] = rs[k].counters()[1] = 0;
            *rs[k].iter_total() = 0;
        }

    // degrees
    std::vector<int> vdeg(n, 0);
    int dc_min = 1 << 30, dv_min = 1 << 30;
    for (int c = 0; c < m; ++c) {
        const int d = indptr[c + 1] - indptr[c];
        h->dc_max = std::max(h->dc_max, d);
        dc_min = std::min(dc_min, d);
        for (int e = indptr[c]; e < indptr[c + 1]; ++e) vdeg[indices[e]]++;
    }
    for (int i = 0; i < n; ++i) {
        h->dv_max = std::max(h->dv_max, vdeg[i]);
        dv_min = std::min(dv_min, vdeg[i]);
    }
    h->regular = (dc_min == h->dc_max) && (dv_min == h->dv_max);

    DegPair pair{16, 8};
    if (is_reg63(h)) pair = {6, 3};
    else if (!pick_pair(h->dc_max, h->dv_max, &pair)) h->bp_any = true;  // beyond the compiled degrees: run-time degree loops
    // small path: messages in LDS, OSD rows in registers.  Anything beyond goes to the HBM-resident kernels.
    // BP in LDS whenever a workgroup shape holds the messages (up to 2048 checks); OSD in registers up to m = 1024 /
    // n = 2047.  Anything beyond goes to the HBM-resident kernels, BP and OSD independently.
    const int shp = h->bp_any ? 0 : pick_shape(h);
    h->bp_hbm = !h->bp_any && (!shp || bp_lds_bytes(pair.dc, shape_threads(h, shp) * shape_cpt(shp)) > h->lds_per_cu);
    h->large = (m > 1024) || (osd_words(n) == 0) || h->bp_hbm;
    if (const char* e = getenv("BPOSD_FORCE_LARGE_OSD")) h->large = h->large || e[0] == '1';  // (probe: the HBM-resident OSD kernel on a small code)
    if (h->large) {
        // Two lanes, three where BP is HBM-resident too: its workgroups take a whole CU like the eliminations', a call is a
        // 35-50 ms BP launch followed by an OSD launch that lasts as long as its slowest elimination (87 ms on L29k, twice the
        // median), and with two calls in flight the CUs the fast eliminations free stay idle until the next call's BP kernel is
        // launched (l29k_ms_e15: 88 ms per step with two lanes, 82-83 with three or four -- the sum of the kernels' CU time).
        h->nlanes = h->bp_hbm ? 3 : 2;
        if (const char* e = getenv("BPOSD_LARGE_LANES")) h->nlanes = std::max(1, std::min(BPOSD_LANES, atoi(e)));
        if (n > 32767 || m > 16384 || (h->bp_hbm && bp_large_lds_need(m, n) > h->lds_per_cu))
            return fail(nullptr, BPOSD_ERR_UNSUPPORTED, "code too large even for the HBM-resident kernels (m=%d n=%d; limits 16384 / 32767)", m, n);
        const int span_cap = osd_large_maxspan(cfg->osd_method == BPOSD_OSD_CS);
        if (cfg->osd_method >= BPOSD_OSD_E && cfg->osd_order > span_cap)
            return fail(nullptr, BPOSD_ERR_UNSUPPORTED,
                        "osd order %d > %d is not supported by the HBM-resident OSD kernel (m=%d n=%d)", cfg->osd_order,
                        span_cap, m, n);
    }

    h->rank = h->large ? std::min(m, n) : gf2_rank_host(m, n, h->rp, h->ci);  // large: probed on the device below
    h->kprime = n - h->rank;
    if (cfg->osd_method != BPOSD_OSD_OFF && !h->large) {
        if (m > 1024 || osd_words(n) == 0)
            return fail(nullptr, BPOSD_ERR_UNSUPPORTED,
                        "code too large for the register-resident OSD kernel (m=%d > 1024 or n=%d > 2047): large-code path not built yet",
                        m, n);
        if (cfg->osd_method >= BPOSD_OSD_E && cfg->osd_order > h->kprime)
            return fail(nullptr, BPOSD_ERR_INVALID, "osd_order %d exceeds the number of non-pivot columns n - rank = %d",
                        cfg->osd_order, h->kprime);
        if (cfg->osd_method == BPOSD_OSD_E && cfg->osd_order > 20)
            return fail(nullptr, BPOSD_ERR_UNSUPPORTED, "osd_e order %d > 20 not supported", cfg->osd_order);
        if (cfg->osd_method == BPOSD_OSD_CS && cfg->osd_order > 64)
            return fail(nullptr, BPOSD_ERR_UNSUPPORTED, "osd_cs order %d > 64 not supported", cfg->osd_order);
    }
    h->ncand = num_candidates(h);

    if ((rc = upload_ints(h, h->d_rp, h->rp))) return failed(rc);
    if ((rc = upload_ints(h, h->d_ci, h->ci))) return failed(rc);
    for (DevArray<double>* t : {&h->d_llr0, &h->d_cost, &h->d_llr0_alt, &h->d_cost_alt}) CREATE_HIP(t->alloc(sizeof(double) * n));
    if (h->bp_any) rc = build_tables_serial(h);  // (its CSC edge map is what the any-degree kernel walks)
    else if (h->bp_hbm) rc = build_tables_large(h, h->dv_max <= 6 ? 6 : 8, (m + 63) / 64 * 64);
    else rc = build_tables(h, pair.dc, pair.dv, shape_threads(h, shp) * shape_cpt(shp), shape_threads(h, shp), 2 * shape_cpt(shp));
    if (rc) return failed(rc);
    if (!h->bp_any && !h->bp_hbm && cfg->bp_method == BPOSD_BP_MIN_SUM && (rc = build_tables_local(h))) return failed(rc);
    if (!h->bp_any && !h->bp_hbm && (!(h->local_ok && cfg->bp_method == BPOSD_BP_MIN_SUM) || getenv("BPOSD_CLASS_ALWAYS")) && (rc = build_tables_class(h)))
        return failed(rc);
    if (cfg->schedule == 1) {
        if (h->dv_max > bp_serial_max_dv())
            return failed(fail(h, BPOSD_ERR_UNSUPPORTED, "serial schedule: bit degree %d exceeds %d", h->dv_max, bp_serial_max_dv()));
        if (!h->bp_any && (rc = build_tables_serial(h))) return failed(rc);
    }
    if ((rc = upload_priors(h))) return failed(rc);
    if (h->large) {
        DecodeCall probe;
        probe.lane = &h->lanes[0];
        probe.osd_stream = probe.lane->osd_stream;
        if ((rc = probe_rank_large(h, probe, &h->rank))) return failed(rc);
        h->kprime = n - h->rank;
        if (cfg->osd_method >= BPOSD_OSD_E && cfg->osd_order > h->kprime)
            return failed(fail(h, BPOSD_ERR_INVALID, "osd_order %d exceeds the number of non-pivot columns n - rank = %d",
                               cfg->osd_order, h->kprime));
        h->ncand = num_candidates(h);
    }
    *out = owner.release();
    return BPOSD_OK;
#undef CREATE_HIP
}

int bposd_update_channel_probs(bposd_handle* h, const double* channel_probs) {
    if (!h || !channel_probs) return fail(h, BPOSD_ERR_INVALID, "null argument");
    if (const int64_t bad = first_bad_prob(channel_probs, h->n))
        return fail(h, BPOSD_ERR_INVALID, "channel_probs[%d] = %g is not a probability", (int)(bad - 1), channel_probs[bad - 1]);
    DeviceGuard dev_guard(h->device);
    HIP_TRY(h, dev_guard.err);
    { int rcs = sync_all_lanes(h); if (rcs) return rcs; }
    h->probs.assign(channel_probs, channel_probs + h->n);
    return upload_priors(h);
}

int bposd_set_bp_variant(bposd_handle* h, int32_t variant) {
    if (!h) return BPOSD_ERR_INVALID;
    if (variant != 0 && variant != 1 && variant != 2 && variant != 4 && !(variant >= 16 && variant <= 26) && variant != 32 && variant != 63 && variant != 64)
        return fail(h, BPOSD_ERR_INVALID, "bp variant must be 0 (auto), 1, 2, 4 (LDS kernel shapes), 16 .. 26 (local-edge kernel), 32 (class kernel), 63 (HBM-resident min-sum with whole check records in the workspace) or 64 (any-degree kernel)");
    if (variant == 64) {  // the any-degree kernel as a second implementation for cross-checks: its CSC edge map
        const int rc_any = ensure_csc_tables(h);
        if (rc_any) return rc_any;
    }
    if (variant == 32 && !h->class_ok)
        return fail(h, BPOSD_ERR_UNSUPPORTED, "the class BP kernel needs one check degree and bit degrees of a compiled range");
    if (variant >= 16 && variant <= 26 && !(h->local_ok && h->cfg.bp_method == BPOSD_BP_MIN_SUM))
        return fail(h, BPOSD_ERR_UNSUPPORTED, "the local-edge BP kernel needs a (3,6)-regular code with n = 2m and min-sum");
    h->bp_variant = variant;
    return BPOSD_OK;
}

int bposd_set_relay(bposd_handle* h, int32_t legs, const double* gammas, const int32_t* leg_iters, int32_t stop_after, int32_t leg_init) {
    if (!h) return BPOSD_ERR_INVALID;
    if (legs == 0) {  // off: the tables stay where they are
        h->relay_legs = 0;
        return BPOSD_OK;
    }
    if (legs < 0) return fail(h, BPOSD_ERR_INVALID, "relay: legs = %d is negative", legs);
    if (h->lsd_on) return fail(h, BPOSD_ERR_UNSUPPORTED, "relay mode cannot be combined with LSD mode (switch LSD mode off first)");
    if (h->cfg.bp_method != BPOSD_BP_MIN_SUM) return fail(h, BPOSD_ERR_UNSUPPORTED, "relay mode needs min-sum (bp_method is product-sum)");
    if (h->cfg.schedule != 0) return fail(h, BPOSD_ERR_UNSUPPORTED, "relay mode needs the flooding schedule (schedule is serial)");
    if (!gammas || !leg_iters) return fail(h, BPOSD_ERR_INVALID, "relay: %s is NULL with legs = %d", !gammas ? "gammas" : "leg_iters", legs);
    if (stop_after < 1) return fail(h, BPOSD_ERR_INVALID, "relay: stop_after = %d must be at least 1", stop_after);
    if (leg_init != 0 && leg_init != 1) return fail(h, BPOSD_ERR_INVALID, "relay: leg_init = %d must be 0 (reset the messages) or 1 (keep them)", leg_init);
    for (int r = 0; r < legs; ++r)
        if (leg_iters[r] < 1) return fail(h, BPOSD_ERR_INVALID, "relay: leg_iters[%d] = %d must be at least 1", r, leg_iters[r]);
    const size_t count = (size_t)legs * h->n;
    for (size_t k = 0; k < count; ++k)
        if (!std::isfinite(gammas[k]))
            return fail(h, BPOSD_ERR_INVALID, "relay: gammas[%d][%d] = %g is not finite", (int)(k / h->n), (int)(k % h->n), gammas[k]);
    DeviceGuard dev_guard(h->device);
    HIP_TRY(h, dev_guard.err);
    { int rcs = sync_all_lanes(h); if (rcs) return rcs; }  // earlier calls may still read the old tables
    // (ensure_csc_tables guards and drains again where it builds: bposd_set_bp_variant calls it bare; the sync above is for the uploads below)
    { int rct = ensure_csc_tables(h); if (rct) return rct; }
    h->relay_legs = 0;  // (a failed upload leaves the mode off: the tables may be half written)
    HIP_TRY(h, h->d_relay_gammas.ensure(sizeof(double) * count));
    HIP_TRY(h, h->d_relay_iters.ensure(sizeof(int) * (size_t)legs));
    HIP_TRY(h, hipMemcpy(h->d_relay_gammas, gammas, sizeof(double) * count, hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(h->d_relay_iters, leg_iters, sizeof(int) * (size_t)legs, hipMemcpyHostToDevice));
    h->relay_legs = legs;
    h->relay_stop = stop_after;
    h->relay_init = leg_init;
    return BPOSD_OK;
}

int bposd_relay_stats(bposd_handle* h, int32_t lane, int32_t* solutions, int32_t* best_leg, int64_t* weight, int64_t B) {
    if (!h) return BPOSD_ERR_INVALID;
    if (lane == -1) lane = h->relay_lane;
    if (lane < 0 || lane >= h->nlanes) return fail(h, BPOSD_ERR_INVALID, "lane %d out of range", lane);
    Lane& L = h->lanes[lane];
    if (L.relay_B < 0) return fail(h, BPOSD_ERR_INVALID, "the last call on lane %d did not run in relay mode", lane);
    // no arrays: the batch size of that call (check_batch admits no batch above 2^31 - 1, so the value fits the return code)
    if (!solutions && !best_leg && !weight) return (int)std::min<long long>(L.relay_B, INT_MAX);
    if (B != L.relay_B) return fail(h, BPOSD_ERR_INVALID, "the last call on lane %d decoded %lld syndromes, not %lld", lane, L.relay_B, (long long)B);
    DeviceGuard dev_guard(h->device);
    HIP_TRY(h, dev_guard.err);
    HIP_TRY(h, hipStreamSynchronize(L.stream));
    if (solutions) HIP_TRY(h, hipMemcpy(solutions, L.relay_sol.p, sizeof(int) * (size_t)B, hipMemcpyDeviceToHost));
    if (best_leg) HIP_TRY(h, hipMemcpy(best_leg, L.relay_leg.p, sizeof(int) * (size_t)B, hipMemcpyDeviceToHost));
    if (weight) HIP_TRY(h, hipMemcpy(weight, L.relay_wt.p, sizeof(long long) * (size_t)B, hipMemcpyDeviceToHost));
    return BPOSD_OK;
}

int bposd_set_lsd(bposd_handle* h, int32_t on, int32_t max_cluster_bits, int32_t max_cluster_checks) {
    if (!h) return BPOSD_ERR_INVALID;
    if (!on) {  // off: the tables stay where they are
        h->lsd_on = false;
        return BPOSD_OK;
    }
    if (h->relay_legs > 0) return fail(h, BPOSD_ERR_UNSUPPORTED, "LSD mode cannot be combined with relay mode (switch relay mode off first)");
    if (max_cluster_bits < 1 || max_cluster_bits > lsd_max_bits())
        return fail(h, BPOSD_ERR_INVALID, "lsd: max_cluster_bits = %d must be in [1, %d] (the ceiling of lsd_kernel)", max_cluster_bits, lsd_max_bits());
    if (max_cluster_checks < 1 || max_cluster_checks > lsd_max_checks())
        return fail(h, BPOSD_ERR_INVALID, "lsd: max_cluster_checks = %d must be in [1, %d] (the ceiling of lsd_kernel)", max_cluster_checks, lsd_max_checks());
    // 16 bits per check, and the sparse set tells a lane's tag (0x8000 | lane) from a list index only while every index -- a
    // check or a slot of a list of checks -- is below 0x8000 (a handle is created for m <= 16384)
    if (h->m > 0x8000)
        return fail(h, BPOSD_ERR_UNSUPPORTED, "LSD mode: m = %d checks do not fit lsd_kernel's 15-bit check indices", h->m);
    if (lsd_lds_need(h->m, h->n, lsd_higher_order(h)) > h->lds_per_cu)
        return fail(h, BPOSD_ERR_UNSUPPORTED, "LSD mode: the cluster state of m = %d checks and n = %d bits needs %zu bytes of LDS, the CU has %zu",
                    h->m, h->n, lsd_lds_need(h->m, h->n, lsd_higher_order(h)), h->lds_per_cu);
    DeviceGuard dev_guard(h->device);
    HIP_TRY(h, dev_guard.err);
    { int rcs = sync_all_lanes(h); if (rcs) return rcs; }  // earlier calls run without the mode
    if (!h->d_lsd_cp) {
        const int rct = build_tables_lsd(h);
        if (rct) return rct;
    }
    h->lsd_max_bits = max_cluster_bits;
    h->lsd_max_checks = max_cluster_checks;
    h->lsd_on = true;
    return BPOSD_OK;
}

int bposd_set_lsd_order(bposd_handle* h, int32_t method, int32_t order, int32_t min_free_bits, int32_t grow_bits_limit) {
    if (!h) return BPOSD_ERR_INVALID;
    if (method != BPOSD_LSD_0 && method != BPOSD_LSD_CS && method != BPOSD_LSD_E)
        return fail(h, BPOSD_ERR_INVALID, "lsd: method = %d must be BPOSD_LSD_0, BPOSD_LSD_CS or BPOSD_LSD_E", method);
    const int lo = method == BPOSD_LSD_0 ? 0 : 1, hi = method == BPOSD_LSD_0 ? 0 : method == BPOSD_LSD_CS ? 64 : 10;
    if (order < lo || order > hi)
        return fail(h, BPOSD_ERR_INVALID, "lsd: order = %d must be in [%d, %d] with method %s", order, lo, hi,
                    method == BPOSD_LSD_0 ? "lsd_0" : method == BPOSD_LSD_CS ? "lsd_cs" : "lsd_e");
    if (min_free_bits < 0 || min_free_bits > 64) return fail(h, BPOSD_ERR_INVALID, "lsd: min_free_bits = %d must be in [0, 64]", min_free_bits);
    if (grow_bits_limit < 1 || grow_bits_limit > lsd_max_bits())
        return fail(h, BPOSD_ERR_INVALID, "lsd: grow_bits_limit = %d must be in [1, %d] (the ceiling of lsd_kernel)", grow_bits_limit, lsd_max_bits());
    const bool ho = method != BPOSD_LSD_0 || min_free_bits > 0;
    if (h->lsd_on && lsd_lds_need(h->m, h->n, ho) > h->lds_per_cu)
        return fail(h, BPOSD_ERR_UNSUPPORTED, "LSD mode: the cluster state of m = %d checks and n = %d bits with a sweep needs %zu bytes of LDS, the CU has %zu",
                    h->m, h->n, lsd_lds_need(h->m, h->n, ho), h->lds_per_cu);
    // (read on the host when a call is enqueued: the calls in flight keep what they were launched with)
    h->lsd_method = method;
    h->lsd_order = order;
    h->lsd_min_free = min_free_bits;
    h->lsd_grow_limit = grow_bits_limit;
    return BPOSD_OK;
}

int bposd_lsd_order_stats(bposd_handle* h, int32_t lane, int32_t* max_free, int32_t* improved, int64_t B) {
    if (!h) return BPOSD_ERR_INVALID;
    if (lane == -1) lane = h->lsd_lane;
    if (lane < 0 || lane >= h->nlanes) return fail(h, BPOSD_ERR_INVALID, "lane %d out of range", lane);
    Lane& L = h->lanes[lane];
    if (L.lsd_B < 0) return fail(h, BPOSD_ERR_INVALID, "the last call on lane %d did not run in LSD mode", lane);
    if (!max_free && !improved) return (int)std::min<long long>(L.lsd_B, INT_MAX);
    if (B != L.lsd_B) return fail(h, BPOSD_ERR_INVALID, "the last call on lane %d decoded %lld syndromes, not %lld", lane, L.lsd_B, (long long)B);
    int32_t* const dst[2] = {max_free, improved};
    if (L.lsd_words < 6) {  // the LSD-0 instance keeps four words: no free columns counted, no sweep
        for (int k = 0; k < 2; ++k)
            if (dst[k]) std::fill(dst[k], dst[k] + B, 0);
        return BPOSD_OK;
    }
    DeviceGuard dev_guard(h->device);
    HIP_TRY(h, dev_guard.err);
    HIP_TRY(h, hipStreamSynchronize(L.stream));
    for (int k = 0; k < 2; ++k)
        if (dst[k]) HIP_TRY(h, hipMemcpy(dst[k], (const int*)L.lsd_stat.p + (size_t)(4 + k) * B, sizeof(int) * (size_t)B, hipMemcpyDeviceToHost));
    return BPOSD_OK;
}

int bposd_debug_lsd_launches(bposd_handle* h, int64_t launches[2]) {
    if (!h || !launches) return BPOSD_ERR_INVALID;
    launches[0] = h->lsd_launches[0];
    launches[1] = h->lsd_launches[1];
    return BPOSD_OK;
}

int bposd_lsd_stats(bposd_handle* h, int32_t lane, int32_t* status, int32_t* rounds, int32_t* clusters, int32_t* max_bits, int64_t B) {
    if (!h) return BPOSD_ERR_INVALID;
    if (lane == -1) lane = h->lsd_lane;
    if (lane < 0 || lane >= h->nlanes) return fail(h, BPOSD_ERR_INVALID, "lane %d out of range", lane);
    Lane& L = h->lanes[lane];
    if (L.lsd_B < 0) return fail(h, BPOSD_ERR_INVALID, "the last call on lane %d did not run in LSD mode", lane);
    // no arrays: the batch size of that call (as bposd_relay_stats)
    if (!status && !rounds && !clusters && !max_bits) return (int)std::min<long long>(L.lsd_B, INT_MAX);
    if (B != L.lsd_B) return fail(h, BPOSD_ERR_INVALID, "the last call on lane %d decoded %lld syndromes, not %lld", lane, L.lsd_B, (long long)B);
    DeviceGuard dev_guard(h->device);
    HIP_TRY(h, dev_guard.err);
    HIP_TRY(h, hipStreamSynchronize(L.stream));
    int32_t* const dst[4] = {status, rounds, clusters, max_bits};
    for (int k = 0; k < 4; ++k)
        if (dst[k]) HIP_TRY(h, hipMemcpy(dst[k], (const int*)L.lsd_stat.p + (size_t)k * B, sizeof(int) * (size_t)B, hipMemcpyDeviceToHost));
    return BPOSD_OK;
}

int bposd_info(bposd_handle* h, int32_t* rank, int32_t* ncand, int32_t* max_iter, int32_t* nnz) {
    if (!h) return BPOSD_ERR_INVALID;
    if (rank) *rank = h->rank;
    if (ncand) *ncand = h->ncand;
    if (max_iter) *max_iter = h->max_iter;
    if (nnz) *nnz = h->E;
    return BPOSD_OK;
}

int bposd_pack_rows_device(bposd_handle* h, const uint8_t* d_bytes, int64_t B, int32_t n, uint64_t* d_words) {
    if (!h) return BPOSD_ERR_INVALID;
    return bposd_pack_rows_device_lane(h, h->last_lane, d_bytes, B, n, d_words);
}

int bposd_pack_rows_device_lane(bposd_handle* h, int32_t lane, const uint8_t* d_bytes, int64_t B, int32_t n, uint64_t* d_words) {
    if (!h) return BPOSD_ERR_INVALID;
    if (lane < 0 || lane >= h->nlanes) return fail(h, BPOSD_ERR_INVALID, "lane %d out of range", lane);
    if (B < 0 || n <= 0 || (B > 0 && (!d_bytes || !d_words))) return fail(h, BPOSD_ERR_INVALID, "bad pack arguments");
    if (B == 0) return BPOSD_OK;
    DeviceGuard dev_guard(h->device);
    HIP_TRY(h, dev_guard.err);
    // queued behind the device-pointer decode that ran on this lane (stream order)
    return launch_pack(h, h->lanes[lane].stream, d_bytes, B, n, (unsigned long long*)d_words, /*wg_per_cu=*/16);
}

int bposd_layout_info(bposd_handle* h, int64_t* natural, int64_t* chosen, int64_t* ideal) {
    if (!h) return BPOSD_ERR_INVALID;
    if (natural) *natural = h->layout_cost_natural;
    if (chosen) *chosen = h->layout_cost;
    if (ideal) *ideal = h->layout_cost_ideal;
    return BPOSD_OK;
}

int bposd_set_osd_variant(bposd_handle* h, int32_t variant) {
    if (!h) return BPOSD_ERR_INVALID;
    if (variant < 0 || variant > 2) return fail(h, BPOSD_ERR_INVALID, "osd variant must be 0 (auto), 1 (workgroup kernel) or 2 (wave kernel where it applies)");
    h->osd_variant = variant;
    return BPOSD_OK;
}

int bposd_last_osd_kernel(bposd_handle* h) { return h ? h->last_osd_kernel : BPOSD_ERR_INVALID; }

int bposd_bp_kernel_info(bposd_handle* h, int32_t* kernel, int64_t* lds_model) {
    if (!h) return BPOSD_ERR_INVALID;
    if (kernel) *kernel = h->last_bp_kernel;
    if (lds_model) {
        for (int k = 0; k < 4; ++k) lds_model[k] = 0;
        if (h->last_bp_kernel == BPOSD_BP_KERNEL_LOCAL) {
            lds_model[0] = h->local_passes; lds_model[1] = 4 * (h->local_mp / 32);
            lds_model[2] = h->local_wcycles; lds_model[3] = 6 * 4 * (h->local_mp / 64);
        } else if (h->last_bp_kernel == BPOSD_BP_KERNEL_CLASS) {
            lds_model[0] = h->class_read_cycles; lds_model[1] = h->class_read_floor;
            lds_model[2] = h->class_write_cycles; lds_model[3] = h->class_write_floor;
        } else if (h->last_bp_kernel == BPOSD_BP_KERNEL_LARGE) {
            lds_model[0] = h->large_form;  // (no bank model: which form of the kernel ran -- bp_large_kernel.hip.h)
        }
    }
    return BPOSD_OK;
}

int bposd_debug_last_instance(bposd_handle* h, int32_t bp[6], int32_t osd[6]) {
    if (!h) return BPOSD_ERR_INVALID;
    if (bp) std::copy(h->last_bp_inst, h->last_bp_inst + 6, bp);
    if (osd) std::copy(h->last_osd_inst, h->last_osd_inst + 6, osd);
    return BPOSD_OK;
}

int bposd_debug_set_park(bposd_handle* h, int32_t mode) {
    if (!h) return BPOSD_ERR_INVALID;
    if (mode < bposd_local_park::kAuto || mode > bposd_local_park::kAlways) return fail(h, BPOSD_ERR_INVALID, "bposd_debug_set_park: mode must be 0 (auto), 1 (never) or 2 (force)");
    h->park_mode = mode;
    return BPOSD_OK;
}

int bposd_debug_last_parked(bposd_handle* h, int32_t lane, int32_t* parked) {
    if (!h || !parked) return BPOSD_ERR_INVALID;
    if (lane < 0 || lane >= h->nlanes) return fail(h, BPOSD_ERR_INVALID, "lane %d out of range (%d lanes)", lane, h->nlanes);
    DeviceGuard dev_guard(h->device);
    HIP_TRY(h, dev_guard.err);
    // the lane's counter block keeps the word until the lane's next call clears it
    HIP_TRY(h, hipStreamSynchronize(h->lanes[lane].stream));
    int v = 0;
    HIP_TRY(h, hipMemcpy(&v, h->lanes[lane].d_counters + bposd_local_park::kParkCount, sizeof(int), hipMemcpyDeviceToHost));
    *parked = v;
    return BPOSD_OK;
}

int bposd_debug_last_pair_key(bposd_handle* h, int32_t* pair_key) {
    if (!h || !pair_key) return BPOSD_ERR_INVALID;
    *pair_key = h->last_bp_inst[0] == BPOSD_BP_KERNEL_LOCAL ? h->last_bp_pair_key : -1;
    return BPOSD_OK;
}

int bposd_synchronize(bposd_handle* h) {
    if (!h) return BPOSD_ERR_INVALID;
    DeviceGuard dev_guard(h->device);
    HIP_TRY(h, dev_guard.err);
    return sync_all_lanes(h);
}

int bposd_decode_batch_device(bposd_handle* h, const uint8_t* d_synd, int64_t B, uint8_t* d_osdw,
                              uint8_t* d_osd0, uint8_t* d_bp, uint8_t* d_conv, int32_t* d_iters,
                              double* d_llr) {
    if (const int rc = check_batch(h, B, d_synd, d_osdw); rc || B == 0) return rc;
    return decode_device_impl(h, take_next_lane(h), IoPtrs{d_synd, nullptr, d_osdw, d_osd0, d_bp, d_conv, d_iters, d_llr}, B);
}

int bposd_decode_batch_device_packed(bposd_handle* h, const uint64_t* d_synd_words, int64_t B, uint64_t* d_osdw_words,
                                     uint64_t* d_osd0_words, uint64_t* d_bp_words, uint8_t* d_conv, int32_t* d_iters) {
    if (!h) return BPOSD_ERR_INVALID;
    if (!native_packed(h))
        return fail(h, BPOSD_ERR_UNSUPPORTED, "this code's kernels take byte rows (any-degree or serial-schedule kernel): "
                    "use bposd_decode_batch_device and bposd_pack_rows_device");
    if (const int rc = check_batch(h, B, d_synd_words, d_osdw_words); rc || B == 0) return rc;
    DecodeCall call = take_next_lane(h);
    call.packed = true;
    return decode_device_impl(h, call, IoPtrs{(const uint8_t*)d_synd_words, nullptr, (uint8_t*)d_osdw_words, (uint8_t*)d_osd0_words,
                                              (uint8_t*)d_bp_words, d_conv, d_iters, nullptr}, B);
}

int bposd_decode_batch_select_device(bposd_handle* h, const uint8_t* d_synd, int64_t B, const uint8_t* d_sel,
                                     const double* alt, uint8_t* d_osdw, uint8_t* d_osd0, uint8_t* d_bp,
                                     uint8_t* d_conv, int32_t* d_iters, double* d_llr) {
    if (!h) return BPOSD_ERR_INVALID;
    if (!d_sel) return fail(h, BPOSD_ERR_INVALID, "select is required");
    if (const int rc = check_alt_channel(h, alt)) return rc;
    if (const int rc = check_batch(h, B, d_synd, d_osdw); rc || B == 0) return rc;
    // asynchronous like the plain device-pointer call: the alternative channel goes to the buffers of the lane this call
    // runs on, through that lane's stream
    DeviceGuard dev_guard(h->device);
    HIP_TRY(h, dev_guard.err);
    DecodeCall call = take_next_lane(h);
    call.lane_alt = true;
    Lane& L = *call.lane;
    const size_t bytes = sizeof(double) * 2 * (size_t)h->n;
    if (!L.d_alt) HIP_TRY(h, L.d_alt.alloc(bytes));
    if (const int rc = ensure_pinned(h, L.h_alt, bytes, hipHostMallocDefault)) return rc;
    if (!L.ev_alt) HIP_TRY(h, hipEventCreateWithFlags(&L.ev_alt.raw, hipEventDisableTiming));
    if (L.alt_busy) HIP_TRY(h, hipEventSynchronize(L.ev_alt));  // the copy of this lane's previous select call has read the staging block
    alt_channel_tables(h->n, alt, L.h_alt.as<double>(), L.h_alt.as<double>() + h->n);
    HIP_TRY(h, hipMemcpyAsync(L.d_alt, L.h_alt.p, bytes, hipMemcpyHostToDevice, L.stream));
    HIP_TRY(h, hipEventRecord(L.ev_alt, L.stream));
    L.alt_busy = true;
    return decode_device_impl(h, call, IoPtrs{d_synd, d_sel, d_osdw, d_osd0, d_bp, d_conv, d_iters, d_llr}, B);
}

int bposd_channel_tables(const double* probs, int64_t count, double* prior_llr, double* cost) {
    if (count < 0 || (count > 0 && !probs)) return fail(nullptr, BPOSD_ERR_INVALID, "bposd_channel_tables: probs and a count >= 0 are required");
    if (const int64_t bad = channel_tables(probs, count, prior_llr, cost))
        return fail(nullptr, BPOSD_ERR_INVALID, "probs[%lld] = %g is not a probability", (long long)(bad - 1), probs[bad - 1]);
    return BPOSD_OK;
}

/* A channel of its own for every syndrome, device-pointer form: the rows replace the handle's channel for this call only. */
int bposd_decode_batch_rows_device(bposd_handle* h, const uint8_t* d_synd, int64_t B, const double* d_prior_llr_rows,
                                   const double* d_cost_rows, uint8_t* d_osdw, uint8_t* d_osd0, uint8_t* d_bp,
                                   uint8_t* d_conv, int32_t* d_iters, double* d_llr) {
    if (!h) return BPOSD_ERR_INVALID;
    if (!d_prior_llr_rows) return fail(h, BPOSD_ERR_INVALID, "prior_llr_rows is required");
    const bool weighs = stage_weighs_candidates(h);
    if (weighs && !d_cost_rows) return fail(h, BPOSD_ERR_INVALID, "cost_rows is required: this handle's %s weighs its candidates with the channel",
                                                  h->lsd_on && h->lsd_method != BPOSD_LSD_0 ? "LSD sweep" : "OSD stage");
    if (const int rc = check_batch(h, B, d_synd, d_osdw); rc || B == 0) return rc;
    IoPtrs io{d_synd, nullptr, d_osdw, d_osd0, d_bp, d_conv, d_iters, d_llr};
    io.llr0_rows = d_prior_llr_rows;
    io.cost_rows = weighs ? d_cost_rows : nullptr;
    return decode_device_impl(h, take_next_lane(h), io, B);
}

// ================================================================================ logical observables
// What a caller asks of a correction is which logical observables it flips: obs_kernel (obs_kernel.hip.h) computes L . row for
// the rows a decode left on its lane, and ceil(k / 64) words per shot and output leave the device instead of ceil(n / 64).

int bposd_observable_table(const int32_t* indptr, const int32_t* indices, int32_t k, int32_t n, uint64_t* table) {
    std::string why;
    if (const int rc = observable_table(indptr, indices, k, n, table, &why)) return fail(nullptr, rc, "%s", why.c_str());
    return BPOSD_OK;
}

int bposd_set_observables(bposd_handle* h, const uint64_t* table, int32_t k) {
    if (!h) return BPOSD_ERR_INVALID;
    if (k < 0 || k > obs_max_k()) return fail(h, BPOSD_ERR_INVALID, "bposd_set_observables: k = %d is outside 0 .. %d", k, obs_max_k());
    if (k > 0 && !table) return fail(h, BPOSD_ERR_INVALID, "bposd_set_observables: the table is required");
    DeviceGuard dev_guard(h->device);
    HIP_TRY(h, dev_guard.err);
    { int rcs = sync_all_lanes(h); if (rcs) return rcs; }  // earlier calls may still read the old table
    h->obs_k = 0;
    if (k == 0) {
        HIP_TRY(h, h->d_obs_table.release());
        return BPOSD_OK;
    }
    const size_t bytes = sizeof(uint64_t) * (size_t)((h->n + 63) / 64) * (size_t)k;
    HIP_TRY(h, h->d_obs_table.alloc(bytes));
    HIP_TRY(h, hipMemcpy(h->d_obs_table, table, bytes, hipMemcpyHostToDevice));
    h->obs_k = k;
    return BPOSD_OK;
}

int bposd_observables_device_lane(bposd_handle* h, int32_t lane, const void* d_rows, int32_t packed, int64_t B, uint64_t* d_obs_words) {
    if (const int rc = check_observables(h)) return rc;
    if (lane < 0 || lane >= h->nlanes) return fail(h, BPOSD_ERR_INVALID, "lane %d out of range", lane);
    if (B < 0 || B > 0x7fffffffLL || (B > 0 && (!d_rows || !d_obs_words))) return fail(h, BPOSD_ERR_INVALID, "bad observables arguments");
    if (B == 0) return BPOSD_OK;
    DeviceGuard dev_guard(h->device);
    HIP_TRY(h, dev_guard.err);
    // queued behind the device-pointer decode that ran on this lane (stream order)
    const void* const rows[3] = {d_rows, nullptr, nullptr};
    uint64_t* const outs[3] = {d_obs_words, nullptr, nullptr};
    return launch_obs(h, h->lanes[lane].stream, rows, packed != 0, B, outs);
}

int bposd_decode_batch_observables_device(bposd_handle* h, const void* d_synd, int32_t synd_packed, int64_t B, uint64_t* d_obs_osdw,
                                          uint64_t* d_obs_osd0, uint64_t* d_obs_bp, uint8_t* d_conv, int32_t* d_iters) {
    if (const int rc = check_observables(h)) return rc;
    if (const int rc = check_batch(h, B, d_synd, d_obs_osdw); rc || B == 0) return rc;
    DeviceGuard dev_guard(h->device);
    HIP_TRY(h, dev_guard.err);
    const ObsOut out{d_obs_osdw, d_obs_osd0, d_obs_bp, d_conv, d_iters};
    if (const int rc = obs_reserve(h, (size_t)B, out, /*host=*/false, synd_packed != 0)) return rc;
    return decode_obs_impl(h, take_next_lane(h), d_synd, synd_packed != 0, B, out);
}

int bposd_debug_obs_timing(bposd_handle* h, int32_t lane, double* obs_ms) {
    if (!h || !obs_ms) return BPOSD_ERR_INVALID;
    if (lane < -1 || lane >= BPOSD_LANES) return fail(h, BPOSD_ERR_INVALID, "lane %d out of range", lane);
    DeviceGuard dev_guard(h->device);
    HIP_TRY(h, dev_guard.err);
    CallRecord* recs = lane < 0 ? h->rec : &h->lane_rec[lane];
    const int count = lane < 0 ? h->nrec : 1;
    if (lane < 0) { int rcs = sync_all_lanes(h); if (rcs) return rcs; }
    else HIP_TRY(h, hipStreamSynchronize(h->lanes[lane].stream));
    double sum = 0.0;
    bool any = false;
    for (int r = 0; r < count; ++r) {
        if (!recs[r].ran_obs) continue;
        float ms = 0.f;
        HIP_TRY(h, hipEventElapsedTime(&ms, recs[r].ev_obs[0], recs[r].ev_obs[1]));
        sum += ms;
        any = true;
    }
    if (!any) return fail(h, BPOSD_ERR_INVALID, "no observables call has run there");
    *obs_ms = sum;
    return BPOSD_OK;
}

static int record_timing(bposd_handle* h, CallRecord* recs, int count, double* bp_ms, double* osd_ms,
                         int64_t* bp_iterations, int64_t* osd_invocations) {
    double a_sum = 0.0, b_sum = 0.0;
    int64_t it_sum = 0, osd_sum = 0;
    for (int r = 0; r < count; ++r) {
        CallRecord& R = recs[r];
        if (!R.recorded) continue;
        float a = 0.f, b = 0.f;
        if (R.timed) {  // (the lean small-call path records counters only: its times read 0)
            HIP_TRY(h, hipEventElapsedTime(&a, R.ev[0], R.ev[1]));
            HIP_TRY(h, hipEventElapsedTime(&b, R.ev[1], R.ev[2]));
        }
        a_sum += a;
        if (R.ran_osd) b_sum += b;
        it_sum += (int64_t)*R.iter_total();
        osd_sum += R.counters()[1];
    }
    if (bp_ms) *bp_ms = a_sum;
    if (osd_ms) *osd_ms = b_sum;
    if (bp_iterations) *bp_iterations = it_sum;
    if (osd_invocations) *osd_invocations = osd_sum;
    return BPOSD_OK;
}

int bposd_last_timing(bposd_handle* h, double* bp_ms, double* osd_ms, int64_t* bp_iterations,
                      int64_t* osd_invocations) {
    if (!h) return BPOSD_ERR_INVALID;
    if (!h->have_timing) return fail(h, BPOSD_ERR_INVALID, "no decode call has been made on this handle");
    DeviceGuard dev_guard(h->device);
    HIP_TRY(h, dev_guard.err);
    if (h->nrec > 0) {
        // a host-pointer call is several kernel pairs (one per chunk); their durations are summed (chunks overlap on
        // the device, so the sum can exceed the call's wall time), the counters add up to the batch's totals
        int rcs = sync_all_lanes(h);
        if (rcs) return rcs;
        return record_timing(h, h->rec, h->nrec, bp_ms, osd_ms, bp_iterations, osd_invocations);
    }
    HIP_TRY(h, hipStreamSynchronize(h->lanes[h->last_lane].stream));
    return record_timing(h, &h->lane_rec[h->last_lane], 1, bp_ms, osd_ms, bp_iterations, osd_invocations);
}

int bposd_num_lanes(bposd_handle* h) { return h ? h->nlanes : BPOSD_LANES; }

int bposd_last_lane(bposd_handle* h) { return h ? h->last_lane : BPOSD_ERR_INVALID; }

int bposd_synchronize_lane(bposd_handle* h, int32_t lane) {
    if (!h) return BPOSD_ERR_INVALID;
    if (lane < 0 || lane >= BPOSD_LANES) return fail(h, BPOSD_ERR_INVALID, "lane %d out of range", lane);
    DeviceGuard dev_guard(h->device);
    HIP_TRY(h, dev_guard.err);
    HIP_TRY(h, hipStreamSynchronize(h->lanes[lane].stream));
    return BPOSD_OK;
}

int bposd_lane_timing(bposd_handle* h, int32_t lane, double* bp_ms, double* osd_ms, int64_t* bp_iterations,
                      int64_t* osd_invocations) {
    if (!h) return BPOSD_ERR_INVALID;
    if (lane < 0 || lane >= BPOSD_LANES) return fail(h, BPOSD_ERR_INVALID, "lane %d out of range", lane);
    if (!h->have_timing) return fail(h, BPOSD_ERR_INVALID, "no decode call has been made on this handle");
    DeviceGuard dev_guard(h->device);
    HIP_TRY(h, dev_guard.err);
    HIP_TRY(h, hipStreamSynchronize(h->lanes[lane].stream));
    return record_timing(h, &h->lane_rec[lane], 1, bp_ms, osd_ms, bp_iterations, osd_invocations);
}

void* bposd_host_alloc(size_t bytes) {
    void* p = nullptr;
    if (bytes == 0 || hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) return nullptr;
    return p;
}

void bposd_host_free(void* p) {
    (void)free_pinned(p);
}

}  // extern "C"
