// decode_host.hip -- host side of libbposd_mi355x.so: the host-pointer decode calls of include/bposd_mi355x.h (numpy in,
// numpy out).  The synchronous call cuts its batch into chunks (host_chunk_plan) that alternate between the handle's lanes and
// runs every chunk through named stages; the asynchronous call is one lane in stream order; the observables forms follow
// the same two shapes.  Every one of them ends in decode_device_impl / decode_obs_impl (bposd_capi.hip): this unit holds no
// kernel and launches none itself.  The declarations shared with bposd_capi.hip are in internal.h.
#include "internal.h"

#include <chrono>
#include <cstring>
#include <mutex>
#include <thread>

using namespace bposd;
using namespace bposd_host;

namespace bposd_host {

size_t row_bytes(int bits, bool packed) { return packed ? ((size_t)bits + 63) / 64 * 8 : (size_t)bits; }

// A lane's staging buffers for a host-pointer call that wants the outputs named in `host`: rows of words or of bytes.
// The kernels get lane_ptrs(L, native, ...), uploads and downloads use lane_ptrs(L, packed, ...); the two differ for packed
// rows around kernels that take bytes (an unpack kernel in front of them, pack kernels behind).
IoPtrs lane_ptrs(const Lane& L, bool words, const IoPtrs& host) {
    IoPtrs d;
    d.synd = (const uint8_t*)(words ? L.io_psynd.p : L.io_synd.p);
    d.sel = host.sel ? (const uint8_t*)L.io_sel.p : nullptr;
    d.osdw = (uint8_t*)(words ? L.io_posdw.p : L.io_osdw.p);
    d.osd0 = host.osd0 ? (uint8_t*)(words ? L.io_posd0.p : L.io_osd0.p) : nullptr;
    d.bp = host.bp ? (uint8_t*)(words ? L.io_pbp.p : L.io_bp.p) : nullptr;
    d.conv = host.conv ? (uint8_t*)L.io_conv.p : nullptr;
    d.iters = host.iters ? (int32_t*)L.io_iters.p : nullptr;
    d.llr = host.llr ? (double*)L.io_llr.p : nullptr;
    return d;
}

// Chunks of ~32768 syndromes (measured on the headline workload, 131072 syndromes: 4 chunks on the 4 lanes 31.9 ms,
// 8 chunks 35.6 ms -- a lane's next chunk waits for the previous one's OSD kernel and download, and every chunk pays
// its own straggler tail -- 2 chunks 33.0 ms), at most BPOSD_MAX_CHUNKS; BPOSD_HOST_CHUNK overrides the target size (read on
// every call).  An HBM-resident code (`large`) keeps at least four workgroups per CU in a chunk.  Pure: no handle, no device.
HostChunkPlan host_chunk_plan(long long B, int n, bool per_shot_rows, int nlanes, int num_cu, bool large, bool taper) {
    long long target = 32768;
    // (a channel row per shot is 16 n bytes next to the syndrome's m: chunks of ~64 MB of rows bound what a lane stages)
    if (per_shot_rows) target = std::min<long long>(target, std::max<long long>(1024, ((long long)64 << 20) / (16LL * n)));
    if (const char* e = getenv("BPOSD_HOST_CHUNK")) target = std::max(1LL, atoll(e));
    HostChunkPlan plan;
    plan.count = (int)std::min<long long>(BPOSD_MAX_CHUNKS, std::max<long long>(1, (B + target / 2) / target));
    if (large) plan.count = (int)std::min<long long>(plan.count, std::max<long long>(1, B / (4LL * num_cu)));
    plan.capacity = (B + plan.count - 1) / plan.count;
    plan.count = (int)((B + plan.capacity - 1) / plan.capacity);
    // chunk boundaries: equal sizes, except that a four-chunk call (one chunk per lane) tapers 7 : 7 : 6 : 4 -- what
    // stays exposed at the end of the call is the LAST chunk's download and straggler tail
    for (int c = 0; c <= plan.count; ++c) plan.lo[c] = std::min<long long>(B, (long long)c * plan.capacity);
    if (taper && plan.count == 4 && nlanes >= 4 && B >= 4096) {
        const long long w[4] = {7, 7, 6, 4};
        long long acc = 0;
        for (int c = 0; c < 4; ++c) { plan.lo[c] = std::min<long long>(acc, B); acc += (B * w[c] / 24 + 63) / 64 * 64; }
        plan.lo[4] = B;
        plan.capacity = 0;
        for (int c = 0; c < 4; ++c) plan.capacity = std::max(plan.capacity, plan.lo[c + 1] - plan.lo[c]);
    }
    return plan;
}

}  // namespace bposd_host

namespace {

// [0, count) cut into equal slices for at most min(16, hardware threads) host threads (one below 64 K items); f(lo, hi)
template <class F>
void parallel_slices(size_t count, F f) {
    const unsigned hw = std::thread::hardware_concurrency();
    const size_t nt = std::max<size_t>(1, std::min<size_t>({(size_t)16, (size_t)(hw ? hw : 1), count / 65536 + 1}));
    if (nt == 1) { f((size_t)0, count); return; }
    std::vector<std::thread> pool;
    for (size_t t = 1; t < nt; ++t) pool.emplace_back(f, count * t / nt, count * (t + 1) / nt);
    f((size_t)0, count / nt);
    for (auto& th : pool) th.join();
}

// `count` error probabilities into prior LLRs and (cost non-null) OSD-W weights: bposd_channel_tables' routine, a few threads
void convert_rows(const double* src, size_t count, double* l0, double* cost) {
    parallel_slices(count, [&](size_t lo, size_t hi) { (void)channel_tables(src + lo, (int64_t)(hi - lo), l0 + lo, cost ? cost + lo : nullptr); });
}

// The host-pointer paths drain what they have enqueued before they return an error: downloads into the caller's buffers,
// or into a buffer local to a caller of theirs, may be in flight.  Armed from its declaration to the successful return.
struct DrainOnError {
    bposd_handle* h;
    bool armed = true;
    ~DrainOnError() {
        if (!armed) return;
        const std::string first = h->err;  // (the error being returned, not one of the drain)
        (void)sync_all_lanes(h);
        h->err = first;
    }
};

// The result rows (osdw, osd0, bp) of `cnt` syndromes from the lane to row `row0` of the caller's arrays on stream `st`,
// packed on the way where the kernels wrote bytes (dev) and the caller takes words (wire).
int download_rows(bposd_handle* h, hipStream_t st, const IoPtrs& host, size_t row0, const IoPtrs& dev, const IoPtrs& wire,
                  long long cnt, size_t rsn) {
    const struct { uint8_t* host; const uint8_t* dev; uint8_t* wire; } outs[3] = {{host.osdw, dev.osdw, wire.osdw}, {host.osd0, dev.osd0, wire.osd0}, {host.bp, dev.bp, wire.bp}};
    for (auto& o : outs) {
        if (!o.host) continue;
        // (the pack kernels wait for a free workgroup slot like any kernel: with the next chunk's persistent BP grid
        // resident that is that chunk's tail -- the rows then leave one eighth as large)
        if (o.wire != o.dev) { int rc = launch_pack(h, st, o.dev, cnt, h->n, (unsigned long long*)o.wire); if (rc) return rc; }
        HIP_TRY(h, hipMemcpyAsync(o.host + row0 * rsn, o.wire, (size_t)cnt * rsn, hipMemcpyDeviceToHost, st));
    }
    return 0;
}

// ================================================================================ the synchronous host-pointer call
// What the stages of one synchronous call read besides the handle and the caller's arrays (`IoPtrs host`).  decode_host_impl
// fills it in once and every stage takes it by const reference, like DecodeCall: nothing of it is kept in the handle.
struct HostCall {
    int64_t B = 0;
    bool packed = false;   // the caller's syndromes and result rows are little-endian 64-bit words
    bool native = false;   // ... and the kernels read and write that form themselves (else unpack / pack kernels surround them)
    bool bp_only = false;  // bposd_posterior_llr: no OSD stage, no OSD list
    bool osd_on = false;
    const double* prob_rows = nullptr;  // bposd_decode_batch_rows: [B, n] error probabilities, a channel per syndrome
    bool rows_cost = false;             // ... of which the OSD stage reads the weights too
    size_t rsn = 0, rsm = 0;            // the caller's row strides in bytes: result rows, syndromes
    HostChunkPlan plan;
    bool gate = false;  // chunk c's kernels are released by chunk c - 1's tail flag (wait_for_tail)
};

// Where a small call's arrays sit in the lane's page-locked, device-visible staging block (64-byte aligned), and their sum
struct SmallLayout {
    size_t syn, sel, osdw, osd0, bp, conv, it, llr, r0, rc, total;
};

SmallLayout small_layout(const bposd_handle* h, const IoPtrs& host, const HostCall& hc) {
    const size_t n8 = (size_t)h->n, m8 = (size_t)h->m, b8 = (size_t)hc.B;
    auto a64 = [](size_t x) { return (x + 63) & ~(size_t)63; };
    SmallLayout o;
    o.syn = 0;
    o.sel = o.syn + a64(b8 * m8);
    o.osdw = o.sel + (host.sel ? a64(b8 * n8) : 0);
    o.osd0 = o.osdw + a64(b8 * n8);
    o.bp = o.osd0 + (host.osd0 ? a64(b8 * n8) : 0);
    o.conv = o.bp + (host.bp ? a64(b8 * n8) : 0);
    o.it = o.conv + a64(b8);
    o.llr = o.it + a64(b8 * 4);
    o.r0 = o.llr + (host.llr ? a64(b8 * n8 * 8) : 0);
    o.rc = o.r0 + (hc.prob_rows ? a64(b8 * n8 * 8) : 0);
    o.total = o.rc + (hc.rows_cost ? a64(b8 * n8 * 8) : 0);
    return o;
}

// Small calls (the reference's one-syndrome `.decode()`): no copy commands at all.  The kernels read the syndromes from,
// and write every result to, a page-locked staging area that the device addresses directly; the call costs two host
// memcpys, the launches and one stream synchronisation.
int decode_host_small(bposd_handle* h, const IoPtrs& host, const HostCall& hc, const SmallLayout& o) {
    const size_t n8 = (size_t)h->n, m8 = (size_t)h->m, b8 = (size_t)hc.B;
    Lane& L = h->lanes[0];
    if (const int rcs = ensure_pinned(h, L.h_stage, std::max<size_t>(o.total, (size_t)1 << 16), hipHostMallocMapped)) return rcs;
    unsigned char* st = L.h_stage.as<unsigned char>();
    memcpy(st + o.syn, host.synd, b8 * m8);
    if (host.sel) memcpy(st + o.sel, host.sel, b8 * n8);
    if (hc.prob_rows) convert_rows(hc.prob_rows, b8 * n8, (double*)(st + o.r0), hc.rows_cost ? (double*)(st + o.rc) : nullptr);
    DecodeCall call{&L, &h->rec[0]};
    call.bp_only = hc.bp_only;
    call.lean = !getenv("BPOSD_OSD_DEBUG");
    call.osd_stream = call.lean ? L.stream : L.osd_stream;
    IoPtrs zio{st + o.syn, host.sel ? st + o.sel : nullptr, st + o.osdw, host.osd0 ? st + o.osd0 : nullptr,
               host.bp ? st + o.bp : nullptr, st + o.conv, (int32_t*)(st + o.it), host.llr ? (double*)(st + o.llr) : nullptr};
    if (hc.prob_rows) zio.llr0_rows = (const double*)(st + o.r0);
    if (hc.rows_cost) zio.cost_rows = (const double*)(st + o.rc);
    int rcz = decode_device_impl(h, call, zio, hc.B);
    if (rcz) { (void)sync_all_lanes(h); return rcz; }
    h->nrec = 1;
    if (!call.lean) { rcz = sync_all_lanes(h); if (rcz) return rcz; }
    else HIP_TRY(h, hipStreamSynchronize(L.stream));
    memcpy(host.osdw, st + o.osdw, b8 * n8);
    if (host.osd0) memcpy(host.osd0, st + o.osd0, b8 * n8);
    if (host.bp) memcpy(host.bp, st + o.bp, b8 * n8);
    if (host.conv) memcpy(host.conv, st + o.conv, b8);
    if (host.iters) memcpy(host.iters, st + o.it, b8 * 4);
    if (host.llr) memcpy(host.llr, st + o.llr, b8 * n8 * 8);
    return BPOSD_OK;
}

// Rows of chunk c that the OSD kernel rewrote: from the compact copies into the caller's arrays.  Waits for the chunk's
// lane, which is idle afterwards -- so this also comes before anything of that lane is reserved or reused.
int patch_osd_rows(bposd_handle* h, const IoPtrs& host, const HostCall& hc, int c) {
    Lane& L = h->lanes[c % h->nlanes];
    HIP_TRY(h, hipStreamSynchronize(L.stream));       // chunk c's kernels and its counter copy
    HIP_TRY(h, hipStreamSynchronize(L.copy_stream));  // its bulk downloads (the patched rows must land after them)
    L.copy_pending = false;
    if (!hc.osd_on || !h->rec[c].ran_osd) return 0;
    const long long lo = hc.plan.lo[c];
    const int count = h->rec[c].counters()[1];
    if (count <= 0) return 0;
    const size_t rsn = hc.rsn;
    std::vector<uint8_t> rows((size_t)count * rsn);
    for (int which = 0; which < 2; ++which) {
        uint8_t* dst = which ? host.osd0 : host.osdw;
        if (!dst) continue;
        const void* src = which ? L.io_cmp0.p : L.io_cmpw.p;
        if (hc.packed && !hc.native) {  // the compact rows, packed on the (idle) lane's stream
            int rcp = launch_pack(h, L.stream, (const uint8_t*)src, count, h->n, (unsigned long long*)L.io_pcmp.p);
            if (rcp) return rcp;
            HIP_TRY(h, hipMemcpyAsync(rows.data(), L.io_pcmp.p, rows.size(), hipMemcpyDeviceToHost, L.stream));
            HIP_TRY(h, hipStreamSynchronize(L.stream));
        } else {
            HIP_TRY(h, hipMemcpy(rows.data(), src, rows.size(), hipMemcpyDeviceToHost));
        }
        for (int k = 0; k < count; ++k) memcpy(dst + ((size_t)lo + (size_t)L.h_list.as<int>()[k]) * rsn, rows.data() + (size_t)k * rsn, rsn);
    }
    return 0;
}

// The lane's staging buffers for a chunk of this call, sized for the plan's capacity (the largest chunk), never for the chunk
// at hand: a buffer that has to grow is freed and allocated anew, so the lane's previous chunk must have left it.
int reserve_chunk_io(bposd_handle* h, const IoPtrs& host, const HostCall& hc, Lane& L) {
    const size_t CH = (size_t)hc.plan.capacity, n = (size_t)h->n, m = (size_t)h->m;
    int rc;
    if ((rc = ensure(h, L.io_synd, CH * m))) return rc;
    if ((rc = ensure(h, L.io_osdw, CH * n))) return rc;
    if (host.osd0 && (rc = ensure(h, L.io_osd0, CH * n))) return rc;
    if (host.bp && (rc = ensure(h, L.io_bp, CH * n))) return rc;
    if (host.conv && (rc = ensure(h, L.io_conv, CH))) return rc;
    if (host.iters && (rc = ensure(h, L.io_iters, sizeof(int) * CH))) return rc;
    if (host.llr && (rc = ensure(h, L.io_llr, sizeof(double) * CH * n))) return rc;
    if (hc.osd_on) {
        if ((rc = ensure(h, L.io_cmpw, CH * n))) return rc;
        if (host.osd0 && (rc = ensure(h, L.io_cmp0, CH * n))) return rc;
        if ((rc = ensure_pinned(h, L.h_list, sizeof(int) * CH, hipHostMallocDefault))) return rc;
    }
    if (hc.packed) {
        if ((rc = ensure(h, L.io_psynd, CH * hc.rsm))) return rc;
        if ((rc = ensure(h, L.io_posdw, CH * hc.rsn))) return rc;
        if (host.osd0 && (rc = ensure(h, L.io_posd0, CH * hc.rsn))) return rc;
        if (host.bp && (rc = ensure(h, L.io_pbp, CH * hc.rsn))) return rc;
        if (hc.osd_on && (rc = ensure(h, L.io_pcmp, CH * hc.rsn))) return rc;
    }
    if (host.sel && (rc = ensure(h, L.io_sel, CH * n))) return rc;
    if (hc.prob_rows) {  // prior rows, weight rows where OSD reads them, and the page-locked block both are converted into
        if ((rc = ensure(h, L.io_l0rows, sizeof(double) * CH * n))) return rc;
        if (hc.rows_cost && (rc = ensure(h, L.io_costrows, sizeof(double) * CH * n))) return rc;
        if ((rc = ensure_pinned(h, L.h_rows, sizeof(double) * CH * n * (hc.rows_cost ? 2 : 1), hipHostMallocDefault))) return rc;
    }
    return 0;
}

// The lane's buffers as the kernels see them (dev) and as uploads and downloads do (wire): see lane_ptrs
struct ChunkIo {
    IoPtrs dev, wire;
};

ChunkIo chunk_io(const Lane& L, const IoPtrs& host, const HostCall& hc) {
    ChunkIo io{lane_ptrs(L, hc.native, host), lane_ptrs(L, hc.packed, host)};
    if (hc.prob_rows) {
        io.dev.llr0_rows = (const double*)L.io_l0rows.p;
        io.dev.cost_rows = hc.rows_cost ? (const double*)L.io_costrows.p : nullptr;
    }
    return io;
}

// Chunk c's inputs on its lane's stream, behind the previous chunk's upload (uploads go one at a time, in chunk order):
// syndromes, sel, the per-shot channel rows (converted on the host into the lane's page-locked block first), ev_up, and the
// unpack kernel where the kernels take bytes and the caller sent words.
int upload_chunk(bposd_handle* h, const IoPtrs& host, const HostCall& hc, int c, const ChunkIo& io) {
    Lane& L = h->lanes[c % h->nlanes];
    const long long lo = hc.plan.lo[c], cnt = hc.plan.lo[c + 1] - lo;
    const size_t n = (size_t)h->n, bn = (size_t)cnt * n;
    if (c > 0) HIP_TRY(h, hipStreamWaitEvent(L.stream, h->lanes[(c - 1) % h->nlanes].ev_up, 0));
    HIP_TRY(h, hipMemcpyAsync((void*)io.wire.synd, host.synd + (size_t)lo * hc.rsm, (size_t)cnt * hc.rsm, hipMemcpyHostToDevice, L.stream));
    if (host.sel) HIP_TRY(h, hipMemcpyAsync(L.io_sel.p, host.sel + (size_t)lo * n, bn, hipMemcpyHostToDevice, L.stream));
    if (hc.prob_rows) {  // (the lane's previous chunk has been drained by patch_osd_rows: its staging block is free)
        const size_t cap = (size_t)hc.plan.capacity * n;
        double* const rows = L.h_rows.as<double>();
        convert_rows(hc.prob_rows + (size_t)lo * n, bn, rows, hc.rows_cost ? rows + cap : nullptr);
        HIP_TRY(h, hipMemcpyAsync(L.io_l0rows.p, rows, sizeof(double) * bn, hipMemcpyHostToDevice, L.stream));
        if (hc.rows_cost) HIP_TRY(h, hipMemcpyAsync(L.io_costrows.p, rows + cap, sizeof(double) * bn, hipMemcpyHostToDevice, L.stream));
    }
    HIP_TRY(h, hipEventRecord(L.ev_up, L.stream));
    if (io.wire.synd != io.dev.synd) return launch_unpack(h, L.stream, (const unsigned long long*)io.wire.synd, cnt, h->m, (uint8_t*)io.dev.synd);
    return 0;
}

// Chunk c's kernels are released when chunk c - 1's BP kernel has handed out its last syndrome (its tail begins; the
// flag is written by that kernel into page-locked memory) or has ended: the chunks then run in order, each filling
// the previous one's tail, instead of sharing the CUs from the start and all finishing at the end of the call.
int wait_for_tail(bposd_handle* h, int c) {
    Lane& Pv = h->lanes[(c - 1) % h->nlanes];
    // poll the flag (a plain load from page-locked memory); the runtime is asked only every so often and the
    // thread backs off after a short spin -- a chunk's BP kernel runs for milliseconds
    hipError_t qe = hipErrorNotReady;
    for (unsigned spins = 0; *Pv.h_tail.as<volatile int>() == 0; ++spins) {
        if ((spins & 63) == 63) {
            qe = hipEventQuery(Pv.ev_bp);
            if (qe != hipErrorNotReady) break;
        }
        if (spins < 2000) __builtin_ia32_pause();
        else std::this_thread::sleep_for(std::chrono::microseconds(20));
    }
    if (qe != hipErrorNotReady && qe != hipSuccess)
        return fail(h, BPOSD_ERR_HIP, "hipEventQuery failed while waiting for chunk %d: %s", c - 1, hipGetErrorString(qe));
    return 0;
}

// Downloads: everything the BP kernel wrote is final when it ends, except the osdw / osd0 rows of its non-converged
// syndromes -- those are patched from the compact copies once the OSD kernel has run (patch_osd_rows).  (Queued behind the
// OSD kernel on the lane's stream, as in the first version, a chunk's downloads started a whole chunk late: the OSD kernel
// needs a drained CU and the next chunk's persistent BP workgroups take every slot that frees up.)
int download_chunk(bposd_handle* h, const IoPtrs& host, const HostCall& hc, int c, const ChunkIo& io) {
    Lane& L = h->lanes[c % h->nlanes];
    const long long lo = hc.plan.lo[c], cnt = hc.plan.lo[c + 1] - lo;
    const IoPtrs& dev = io.dev;
    hipStream_t cs = L.copy_stream;
    HIP_TRY(h, hipStreamWaitEvent(cs, L.ev_bp, 0));
    if (const int rc = download_rows(h, cs, host, (size_t)lo, dev, io.wire, cnt, hc.rsn)) return rc;
    if (host.conv) HIP_TRY(h, hipMemcpyAsync(host.conv + lo, dev.conv, (size_t)cnt, hipMemcpyDeviceToHost, cs));
    if (host.iters) HIP_TRY(h, hipMemcpyAsync(host.iters + lo, dev.iters, sizeof(int) * (size_t)cnt, hipMemcpyDeviceToHost, cs));
    if (host.llr) HIP_TRY(h, hipMemcpyAsync(host.llr + (size_t)lo * h->n, dev.llr, sizeof(double) * (size_t)cnt * h->n, hipMemcpyDeviceToHost, cs));
    if (hc.osd_on) HIP_TRY(h, hipMemcpyAsync(L.h_list.p, L.osd_list.p, sizeof(int) * (size_t)cnt, hipMemcpyDeviceToHost, cs));
    L.copy_pending = true;
    return 0;
}

// Host-pointer decode: the batch is cut into chunks that alternate between the handle's lanes, so that the upload of
// chunk c + 1, the kernels of chunk c and the download of chunk c - 1 overlap, and the BP workgroups of chunk c + 1 take
// over the CUs that chunk c's stragglers and OSD kernel leave idle.  Within a lane everything is stream-ordered
// (upload, BP, OSD, downloads), so a lane's staging buffers are reused safely two chunks later.  Page-locked host
// buffers (bposd_host_alloc) make the copies asynchronous; with pageable memory the host thread blocks inside each
// copy while the other lane's kernels keep running.
// packed: synd / osdw / osd0 / bp are rows of ceil(m / 64) resp. ceil(n / 64) little-endian 64-bit words (bit i & 63 of
// word i >> 6 = entry i) -- one eighth of the bytes over PCIe; the device unpacks the syndromes in front of the BP kernel and
// packs the result rows behind it (sel and llr are not offered in this form).
// bp_only (bposd_posterior_llr): no OSD stage, no OSD list, on the small path and on every chunk alike.
// prob_rows (bposd_decode_batch_rows; validated by the caller): [B, n] error probabilities, a channel per syndrome.  Each
// chunk's rows are converted on the host into the lane's page-locked block and uploaded next to the syndromes; the weight
// rows only where the OSD stage reads them.
int decode_host_impl(bposd_handle* h, const IoPtrs& host, int64_t B, bool packed = false, bool bp_only = false,
                     const double* prob_rows = nullptr) {
    if (const int rc0 = check_batch(h, B, host.synd, host.osdw); rc0 || B == 0) return rc0;
    DeviceGuard dev_guard(h->device);
    HIP_TRY(h, dev_guard.err);
    // the records and lanes are about to be reused: earlier asynchronous calls must have drained
    if (h->async_pending) { int rcs = sync_all_lanes(h); if (rcs) return rcs; }
    HostCall hc;
    hc.B = B;
    hc.packed = packed;
    hc.native = packed && native_packed(h);
    hc.bp_only = bp_only;
    hc.osd_on = (h->cfg.osd_method != BPOSD_OSD_OFF || h->lsd_on) && !bp_only;  // (LSD mode rewrites rows behind BP like an OSD stage)
    hc.prob_rows = prob_rows;
    hc.rows_cost = prob_rows && hc.osd_on && stage_weighs_candidates(h);
    hc.rsn = row_bytes(h->n, packed);
    hc.rsm = row_bytes(h->m, packed);
    if (const SmallLayout small = small_layout(h, host, hc); !packed && small.total <= (size_t)1 << 20)
        return decode_host_small(h, host, hc, small);
    hc.plan = host_chunk_plan(B, h->n, prob_rows != nullptr, h->nlanes, h->num_cu, h->large, /*taper=*/true);
    hc.gate = hc.plan.count > 1 && h->cfg.schedule == 0;  // (the serial-schedule kernel does not report its tail)
    const int nchunks = hc.plan.count;
    int rc;
    DrainOnError drain{h};
    for (int c = 0; c < nchunks; ++c) {
        const long long cnt = hc.plan.lo[c + 1] - hc.plan.lo[c];
        if (cnt <= 0) { h->rec[c].recorded = false; h->rec[c].ran_osd = false; continue; }
        Lane& L = h->lanes[c % h->nlanes];
        if (c >= h->nlanes && (rc = patch_osd_rows(h, host, hc, c - h->nlanes))) return rc;  // the lane's previous chunk
        if ((rc = reserve_chunk_io(h, host, hc, L))) return rc;
        const ChunkIo io = chunk_io(L, host, hc);
        if ((rc = upload_chunk(h, host, hc, c, io))) return rc;
        if (c > 0 && hc.gate && (rc = wait_for_tail(h, c))) return rc;
        *L.h_tail.as<volatile int>() = 0;
        DecodeCall call{&L, &h->rec[c], L.osd_stream};
        call.batch_hint = B;  // kernel variants are chosen for the call, not for a chunk
        call.cmp_osdw = hc.osd_on ? (uint8_t*)L.io_cmpw.p : nullptr;
        call.cmp_osd0 = (hc.osd_on && host.osd0) ? (uint8_t*)L.io_cmp0.p : nullptr;
        call.bp_only = bp_only;
        call.packed = hc.native;
        call.tail_gate = true;  // (also makes the call record ev_bp, which the downloads wait for)
        if ((rc = decode_device_impl(h, call, io.dev, cnt))) return rc;
        if ((rc = download_chunk(h, host, hc, c, io))) return rc;
    }
    for (int c = std::max(0, nchunks - h->nlanes); c < nchunks; ++c)
        if ((rc = patch_osd_rows(h, host, hc, c))) return rc;
    h->nrec = nchunks;
    drain.armed = false;
    return sync_all_lanes(h);
}

// Asynchronous host-pointer decode: ONE lane, everything in stream order -- upload (packed rows: + unpack kernel), BP,
// OSD, (pack kernels,) downloads -- and the call returns once that is enqueued.  Consecutive calls take consecutive lanes,
// so call k + 1's BP workgroups fill the straggler tail of call k and call k's OSD kernel, packing and downloads run
// under call k + 1's BP kernel: the host-to-host rate of a stream of batches approaches the device-resident one (a lone
// synchronous call always pays its own upload, its 1922-iteration tail and its download).  The caller's buffers must be
// page-locked (bposd_host_alloc) for the copies to be asynchronous, and stay untouched until bposd_synchronize_lane().
int decode_host_async_impl(bposd_handle* h, const IoPtrs& host, int64_t B, bool packed) {
    if (const int rc0 = check_batch(h, B, host.synd, host.osdw); rc0 || B == 0) return rc0;
    if (packed && host.llr) return fail(h, BPOSD_ERR_INVALID, "the packed form has no LLR output");
    DeviceGuard dev_guard(h->device);
    HIP_TRY(h, dev_guard.err);
    // a synchronous host-pointer call leaves no work behind, but its per-chunk records and staging are per lane too: nothing
    // to drain here.  Buffers grow on every lane at once (no allocation inside a later call of the same size).
    const size_t n = (size_t)h->n, m = (size_t)h->m, b8 = (size_t)B;
    const size_t rsn = row_bytes(h->n, packed), rsm = row_bytes(h->m, packed);
    int rc;
    bool grew = false;
    auto need = [&](DevBuf Lane::*member, size_t bytes) -> int { return grow_lanes(h, member, bytes, &grew); };
    if ((rc = need(&Lane::io_synd, b8 * m))) return rc;
    if ((rc = need(&Lane::io_osdw, b8 * n))) return rc;
    if (host.osd0 && (rc = need(&Lane::io_osd0, b8 * n))) return rc;
    if (host.bp && (rc = need(&Lane::io_bp, b8 * n))) return rc;
    if ((rc = need(&Lane::io_conv, b8))) return rc;
    if ((rc = need(&Lane::io_iters, sizeof(int) * b8))) return rc;
    if (host.llr && (rc = need(&Lane::io_llr, sizeof(double) * b8 * n))) return rc;
    if (packed) {
        if ((rc = need(&Lane::io_psynd, b8 * rsm))) return rc;
        if ((rc = need(&Lane::io_posdw, b8 * rsn))) return rc;
        if (host.osd0 && (rc = need(&Lane::io_posd0, b8 * rsn))) return rc;
        if (host.bp && (rc = need(&Lane::io_pbp, b8 * rsn))) return rc;
    }
    DecodeCall call = take_next_lane(h);
    call.device_ptr = false;
    Lane& L = *call.lane;
    if (L.copy_pending) { HIP_TRY(h, hipStreamSynchronize(L.copy_stream)); L.copy_pending = false; }
    // The copies and the pack / unpack kernels go to the lane's HIGH-PRIORITY stream (the one its OSD kernel runs on), ordered
    // against the lane's main stream by events: when workgroup slots free up in the tail of another call's BP kernel these small
    // kernels are dispatched first instead of competing with the next persistent BP grid for every slot.
    hipStream_t hs = L.osd_stream;
    HIP_TRY(h, hipEventRecord(L.ev_copy, L.stream));   // the lane's previous call (its downloads included) has finished
    HIP_TRY(h, hipStreamWaitEvent(hs, L.ev_copy, 0));
    call.packed = packed && native_packed(h);  // the kernels read packed syndromes / write packed rows themselves
    IoPtrs dev = lane_ptrs(L, call.packed, host);
    dev.conv = (uint8_t*)L.io_conv.p;  // (written whether or not the caller takes them)
    dev.iters = (int32_t*)L.io_iters.p;
    const IoPtrs wire = lane_ptrs(L, packed, host);
    HIP_TRY(h, hipMemcpyAsync((void*)wire.synd, host.synd, b8 * rsm, hipMemcpyHostToDevice, hs));
    if (wire.synd != dev.synd && (rc = launch_unpack(h, hs, (const unsigned long long*)wire.synd, B, (int)m, (uint8_t*)dev.synd))) return rc;
    HIP_TRY(h, hipEventRecord(L.ev_up, hs));
    HIP_TRY(h, hipStreamWaitEvent(L.stream, L.ev_up, 0));
    DrainOnError drain{h};
    if ((rc = decode_device_impl(h, call, dev, B))) return rc;
    // (decode_device_impl has made L.stream wait for the OSD kernel: an event on it covers both kernels)
    HIP_TRY(h, hipEventRecord(L.ev_copy, L.stream));
    HIP_TRY(h, hipStreamWaitEvent(hs, L.ev_copy, 0));
    if (host.conv) HIP_TRY(h, hipMemcpyAsync(host.conv, dev.conv, b8, hipMemcpyDeviceToHost, hs));
    if (host.iters) HIP_TRY(h, hipMemcpyAsync(host.iters, dev.iters, sizeof(int) * b8, hipMemcpyDeviceToHost, hs));
    if ((rc = download_rows(h, hs, host, 0, dev, wire, B, rsn))) return rc;
    if (host.llr) HIP_TRY(h, hipMemcpyAsync(host.llr, dev.llr, sizeof(double) * b8 * n, hipMemcpyDeviceToHost, hs));
    HIP_TRY(h, hipEventRecord(L.ev_osd, hs));               // bposd_synchronize_lane waits on the main stream:
    HIP_TRY(h, hipStreamWaitEvent(L.stream, L.ev_osd, 0));  // make it cover the downloads
    drain.armed = false;
    return BPOSD_OK;
}

// ================================================================================ logical observables, host pointers
// Syndromes [lo, lo + cnt) of a host-pointer call on the call's lane, in stream order: upload, decode + obs_kernel on
// lane-resident rows, download of cnt x ceil(k / 64) words per requested output and of the flags and iteration counts.
// (An asynchronous call with its copies and the conversion kernel on the lane's high-priority stream, the way
// decode_host_async_impl places its own, was measured and is slower here: 23.4 against 22.8 ms per call of 131072 on
// [[1922,50]], DESIGN.md 4.10 -- these copies are 24 B per shot, not 744.)
int obs_host_step(bposd_handle* h, const DecodeCall& call, const uint8_t* synd, bool synd_packed, int64_t lo, int64_t cnt,
                  const ObsOut& host) {
    Lane& L = *call.lane;
    const size_t rsm = row_bytes(h->m, synd_packed), kw = (size_t)((h->obs_k + 63) / 64), c8 = (size_t)cnt;
    void* const wire = synd_packed ? L.io_psynd.p : L.io_synd.p;
    HIP_TRY(h, hipMemcpyAsync(wire, synd + (size_t)lo * rsm, c8 * rsm, hipMemcpyHostToDevice, L.stream));
    ObsOut dev;
    dev.osdw = (uint64_t*)L.io_obsw.p;
    dev.osd0 = host.osd0 ? (uint64_t*)L.io_obs0.p : nullptr;
    dev.bp = host.bp ? (uint64_t*)L.io_obsbp.p : nullptr;
    dev.conv = (uint8_t*)L.io_conv.p;
    dev.iters = (int32_t*)L.io_iters.p;
    if (const int rc = decode_obs_impl(h, call, wire, synd_packed, cnt, dev)) return rc;
    const struct { uint64_t* host; const uint64_t* dev; } outs[3] = {{host.osdw, dev.osdw}, {host.osd0, dev.osd0}, {host.bp, dev.bp}};
    for (auto& o : outs)
        if (o.host) HIP_TRY(h, hipMemcpyAsync(o.host + (size_t)lo * kw, o.dev, sizeof(uint64_t) * c8 * kw, hipMemcpyDeviceToHost, L.stream));
    if (host.conv) HIP_TRY(h, hipMemcpyAsync(host.conv + lo, dev.conv, c8, hipMemcpyDeviceToHost, L.stream));
    if (host.iters) HIP_TRY(h, hipMemcpyAsync(host.iters + lo, dev.iters, sizeof(int) * c8, hipMemcpyDeviceToHost, L.stream));
    return 0;
}

// Host-pointer observables decode.  Synchronous: equal chunks of ~32768 syndromes (host_chunk_plan without the taper)
// alternate between the lanes like those of bposd_decode_batch, one record per chunk.  Asynchronous: the whole call on the
// handle's next lane.  Neither needs the compact-row machinery of decode_host_impl: obs_kernel runs after OSD has rewritten
// its rows on the device.
int decode_obs_host_impl(bposd_handle* h, const void* synd, bool synd_packed, int64_t B, const ObsOut& host, bool async) {
    if (const int rc = check_observables(h)) return rc;
    if (const int rc = check_batch(h, B, synd, host.osdw); rc || B == 0) return rc;
    DeviceGuard dev_guard(h->device);
    HIP_TRY(h, dev_guard.err);
    int rc;
    if (async) {
        if ((rc = obs_reserve(h, (size_t)B, host, /*host=*/true, synd_packed))) return rc;
        DecodeCall call = take_next_lane(h);
        call.device_ptr = false;
        DrainOnError drain{h};
        if ((rc = obs_host_step(h, call, (const uint8_t*)synd, synd_packed, 0, B, host))) return rc;
        drain.armed = false;
        return BPOSD_OK;
    }
    // the records and lanes are about to be reused: earlier asynchronous calls must have drained
    if (h->async_pending) { int rcs = sync_all_lanes(h); if (rcs) return rcs; }
    const HostChunkPlan plan = host_chunk_plan(B, h->n, /*per_shot_rows=*/false, h->nlanes, h->num_cu, h->large, /*taper=*/false);
    if ((rc = obs_reserve(h, (size_t)plan.capacity, host, /*host=*/true, synd_packed))) return rc;
    DrainOnError drain{h};
    for (int c = 0; c < plan.count; ++c) {
        Lane& L = h->lanes[c % h->nlanes];
        DecodeCall call{&L, &h->rec[c], L.osd_stream};
        call.batch_hint = B;  // kernel variants are chosen for the call, not for a chunk
        if ((rc = obs_host_step(h, call, (const uint8_t*)synd, synd_packed, plan.lo[c], plan.lo[c + 1] - plan.lo[c], host))) return rc;
    }
    h->nrec = plan.count;
    drain.armed = false;
    return sync_all_lanes(h);
}

}  // namespace

// ================================================================================ C-ABI
extern "C" {

int bposd_decode_batch(bposd_handle* h, const uint8_t* synd, int64_t B, uint8_t* osdw, uint8_t* osd0,
                       uint8_t* bp, uint8_t* conv, int32_t* iters, double* llr) {
    return decode_host_impl(h, IoPtrs{synd, nullptr, osdw, osd0, bp, conv, iters, llr}, B);
}

int bposd_decode_batch_packed(bposd_handle* h, const uint64_t* synd_words, int64_t B, uint64_t* osdw_words, uint64_t* osd0_words,
                              uint64_t* bp_words, uint8_t* conv, int32_t* iters) {
    return decode_host_impl(h, IoPtrs{(const uint8_t*)synd_words, nullptr, (uint8_t*)osdw_words, (uint8_t*)osd0_words, (uint8_t*)bp_words,
                                      conv, iters, nullptr}, B, /*packed=*/true);
}

/* A channel of its own for every syndrome, host pointers: channel_probs_rows [B, n] are error probabilities, validated before
 * anything is enqueued. */
int bposd_decode_batch_rows(bposd_handle* h, const uint8_t* synd, int64_t B, const double* channel_probs_rows, uint8_t* osdw,
                            uint8_t* osd0, uint8_t* bp, uint8_t* conv, int32_t* iters, double* llr) {
    if (!h) return BPOSD_ERR_INVALID;
    if (!channel_probs_rows) return fail(h, BPOSD_ERR_INVALID, "channel_probs_rows is required");
    if (const int rc = check_batch(h, B, synd, osdw); rc || B == 0) return rc;
    const size_t total = (size_t)B * (size_t)h->n;
    std::mutex mu;
    size_t first_bad = total;
    parallel_slices(total, [&](size_t lo, size_t hi) {
        if (const int64_t bad = first_bad_prob(channel_probs_rows + lo, (int64_t)(hi - lo))) {
            std::lock_guard<std::mutex> g(mu);
            first_bad = std::min(first_bad, lo + (size_t)bad - 1);
        }
    });
    if (first_bad < total)
        return fail(h, BPOSD_ERR_INVALID, "channel_probs_rows[%lld][%d] = %g is not a probability", (long long)(first_bad / h->n),
                    (int)(first_bad % h->n), channel_probs_rows[first_bad]);
    return decode_host_impl(h, IoPtrs{synd, nullptr, osdw, osd0, bp, conv, iters, llr}, B, false, false, channel_probs_rows);
}

int bposd_posterior_llr(bposd_handle* h, const uint8_t* synd, int64_t B, double* llr, uint8_t* bp, uint8_t* conv, int32_t* iters) {
    if (!h) return BPOSD_ERR_INVALID;
    if (!llr) return fail(h, BPOSD_ERR_INVALID, "llr buffer is required");
    std::vector<uint8_t> scratch;
    if (!bp) { scratch.resize((size_t)std::max<int64_t>(B, 0) * h->n); bp = scratch.data(); }
    // the osdw slot of the call receives BP's hard decisions (what a decoder with osd_method "osd_off" returns)
    return decode_host_impl(h, IoPtrs{synd, nullptr, bp, nullptr, nullptr, conv, iters, llr}, B, /*packed=*/false, /*bp_only=*/true);
}

int bposd_decode_batch_select(bposd_handle* h, const uint8_t* synd, int64_t B, const uint8_t* sel,
                              const double* alt, uint8_t* osdw, uint8_t* osd0, uint8_t* bp, uint8_t* conv,
                              int32_t* iters, double* llr) {
    if (!h) return BPOSD_ERR_INVALID;
    if (!sel) return fail(h, BPOSD_ERR_INVALID, "select is required");
    int rc = upload_alt_channel(h, alt);
    if (rc) return rc;
    return decode_host_impl(h, IoPtrs{synd, sel, osdw, osd0, bp, conv, iters, llr}, B);
}

int bposd_decode_batch_async(bposd_handle* h, const uint8_t* synd, int64_t B, uint8_t* osdw, uint8_t* osd0, uint8_t* bp,
                             uint8_t* conv, int32_t* iters, double* llr) {
    return decode_host_async_impl(h, IoPtrs{synd, nullptr, osdw, osd0, bp, conv, iters, llr}, B, /*packed=*/false);
}

int bposd_decode_batch_packed_async(bposd_handle* h, const uint64_t* synd_words, int64_t B, uint64_t* osdw_words, uint64_t* osd0_words,
                                    uint64_t* bp_words, uint8_t* conv, int32_t* iters) {
    return decode_host_async_impl(h, IoPtrs{(const uint8_t*)synd_words, nullptr, (uint8_t*)osdw_words, (uint8_t*)osd0_words, (uint8_t*)bp_words, conv,
                                            iters, nullptr}, B, /*packed=*/true);
}

int bposd_decode_batch_observables(bposd_handle* h, const uint8_t* synd, int64_t B, uint64_t* obs_osdw, uint64_t* obs_osd0,
                                   uint64_t* obs_bp, uint8_t* conv, int32_t* iters) {
    return decode_obs_host_impl(h, synd, false, B, ObsOut{obs_osdw, obs_osd0, obs_bp, conv, iters}, /*async=*/false);
}

int bposd_decode_batch_observables_packed(bposd_handle* h, const uint64_t* synd_words, int64_t B, uint64_t* obs_osdw, uint64_t* obs_osd0,
                                          uint64_t* obs_bp, uint8_t* conv, int32_t* iters) {
    return decode_obs_host_impl(h, synd_words, true, B, ObsOut{obs_osdw, obs_osd0, obs_bp, conv, iters}, /*async=*/false);
}

int bposd_decode_batch_observables_async(bposd_handle* h, const uint8_t* synd, int64_t B, uint64_t* obs_osdw, uint64_t* obs_osd0,
                                         uint64_t* obs_bp, uint8_t* conv, int32_t* iters) {
    return decode_obs_host_impl(h, synd, false, B, ObsOut{obs_osdw, obs_osd0, obs_bp, conv, iters}, /*async=*/true);
}

int bposd_decode_batch_observables_packed_async(bposd_handle* h, const uint64_t* synd_words, int64_t B, uint64_t* obs_osdw,
                                                uint64_t* obs_osd0, uint64_t* obs_bp, uint8_t* conv, int32_t* iters) {
    return decode_obs_host_impl(h, synd_words, true, B, ObsOut{obs_osdw, obs_osd0, obs_bp, conv, iters}, /*async=*/true);
}

int bposd_debug_host_chunks(int64_t B, int32_t n, int32_t per_shot_rows, int32_t nlanes, int32_t num_cu, int32_t large, int32_t taper,
                            int64_t* bounds) {
    if (B <= 0 || B > 0x7fffffffLL || n <= 0 || nlanes <= 0 || num_cu <= 0 || !bounds)
        return fail(nullptr, BPOSD_ERR_INVALID, "bposd_debug_host_chunks: B in 1 .. 2^31 - 1, positive n, nlanes and num_cu and a bounds array are required");
    const HostChunkPlan plan = host_chunk_plan(B, n, per_shot_rows != 0, nlanes, num_cu, large != 0, taper != 0);
    std::copy(plan.lo, plan.lo + plan.count + 1, bounds);
    return plan.count;
}

}  // extern "C"
