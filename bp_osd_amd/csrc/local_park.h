// local_park.h -- bp_local_kernel's park-at-drain scheme: what the kernel and the host share, in plain C++ (no HIP), so
// that a host-only test can compile it (tests/test_local_park_cpu.py).
//
// The non-LLR iteration loops of bp_local_kernel run in chunks of kChunk iterations.  Once the call's queue has run dry,
// a workgroup that reaches a chunk boundary with an unfinished shot PARKS it: it writes the shot's whole state to a record
// in device memory and leaves the kernel, so the first launch ends when the queue ends plus at most two chunks.  A second
// launch of the same kernel (its RESUME instance), on the lane's high-priority stream and ordered behind the first by an
// event (launch_bp_local.h), takes the records from a queue of their own, restores each and iterates it to its end.  The
// record is everything the loop carries from one iteration to the next.
#pragma once
#include <stddef.h>

namespace bposd_local_park {

#ifndef BPOSD_BPL_CH
#define BPOSD_BPL_CH 32
#endif
constexpr int kChunk = BPOSD_BPL_CH;  // iterations per chunk: a shot that starts at iteration 1 meets boundaries after iteration kChunk, 2 * kChunk, ...
static_assert(kChunk >= 1, "a chunk holds at least one iteration (two barriers between a park word's write and its read)");

// The counter block of a lane (Lane::d_counters), ints: [0] queue head, [1] OSD list length, [2] OSD queue head, [3] spare,
// [4..5] the 64-bit iteration total, [6..7] spare -- these 32 bytes go into the call record -- and behind them:
constexpr int kParkCount = 8;   // records written by the first launch (claimed with atomicAdd)
constexpr int kResumeHead = 9;  // queue head of the second launch
constexpr int kCounterBytes = 48;

// park_on_dry of BpLocalParams
enum Mode { kOff = 0, kOnDry = 1, kForce = 2 };  // kForce: park at the first chunk boundary whatever the queue says (tests)

// One record, for a kernel with mp positions (any checks-per-thread: 2 * mp owned bits, at most mp threads).
struct Layout {
    size_t shot;    // long long: the shot's index in the batch
    size_t iter;    // int: the iteration the shot goes on from
    size_t msg;     // (4 * mp + 2) doubles: the message region of LDS as it is, padding slots included
    size_t loc;     // 2 * mp doubles: entry r * threads + tid is thread tid's local message r
    size_t bitmap;  // mp / 32 words: the mismatch bitmap
    size_t dec;     // mp words (threads used): entry tid is thread tid's decision mask
    size_t bytes;   // the record, a multiple of 128
};
constexpr Layout layout(int mp) {
    Layout l{};
    l.shot = 0;
    l.iter = 8;
    l.msg = 16;
    l.loc = l.msg + ((size_t)4 * mp + 2) * 8;
    l.bitmap = l.loc + (size_t)2 * mp * 8;
    l.dec = l.bitmap + (size_t)(mp / 32) * 4;
    l.bytes = (l.dec + (size_t)mp * 4 + 127) / 128 * 128;
    return l;
}

// user_mode of bposd_debug_set_park / BPOSD_PARK (0 = kNever, 1 = kAuto: the rule below still decides, it is not "on";
// force = kAlways; anything else, the empty string included, leaves the handle's mode alone)
enum UserMode { kAuto = 0, kNever = 1, kAlways = 2 };

// park_on_dry of a launch.  What the kernel needs whatever the mode: the instance is one auto-selection takes (the others
// are A/B variants), the shot's LLRs are not stored every iteration, and an OSD stage follows whose start the drain delays.
// kAuto further asks for what makes the drain matter: a device-pointer call that is neither lean nor tail-gated (those are
// released or waited for by the host), work of another lane in flight to share the machine with, and a call that is not
// small (launch_bp_local's latency-bound regime, one check per thread: there the second launch costs more than the drain --
// measured at 2048 shots per call, 1.37 -> 1.51 ms per step with the park, and 2.20 -> 2.23 at 8192).
constexpr int park_rule(int user_mode, bool device_call, bool lean, bool tail_gate, bool out_llr, bool osd_on, bool specialised, bool other_lane_busy,
                        bool small_call) {
    if (user_mode == kNever || out_llr || !osd_on || !specialised || lean || tail_gate) return kOff;
    if (user_mode == kAlways) return kForce;
    return (device_call && other_lane_busy && !small_call) ? kOnDry : kOff;
}

}  // namespace bposd_local_park
