// side_lane.h — the side lane of a frame (frame.hip): two library-owned streams beside the caller's, and the events that
// fork work onto them and join it again.
//
// Level 0 (warp + CostRegNet + depth regression) consumes only the FeatureNet's coarsest map, and its deep small layers leave
// most of the chip idle (mfma busy 0.05-0.13 on 80-640 tiles); the FeatureNet's top-down half — up2+lat1, smooth1 (level 1's
// source maps) and the fused up2+lat0+smooth0 (the render texels, the second largest kernel of the frame) — is needed later.
// So enerf_forward forks that half onto the `side` stream right after the trunk and joins it with events before its first
// consumer: the two chains overlap inside ONE frame.  The render of a non-final cascade level (render_if True,True: lego,
// training-style eval) is a leaf as well — nothing in the next level reads its rgb/depth/weights — so it is forked onto the
// `render` stream after the level's depth regression and joined at the end of the frame.
//
// The composite network's frame (enerf_forward_composite, frame.hip CompositeRun) uses the same three streams differently: its
// 1 + L cascades read nothing of each other until a rendered level's layer merge, and the foreground and background chains are
// about equally long.  The caller's stream carries feature_net_bg and the background cascade; everything foreground is forked
// behind the frame's preparation launch (`fork`): feature_net and the texel packs of src_inps on `side` (`feats` tells `render`
// they are done), then layer l's cascade and raw renders on `side` for even l, on `render` for odd l — one layer per stream at
// L = 2, and never more streams than these three (a process here has four hardware queues).  In front of each rendered level's
// enerf_composite_layers, and at the end of the call, the caller's stream waits for `sidedone` / `done`, recorded behind the
// last launch of `side` / `render`.
//
// The driver speaks two verbs only: record(event, stream) and wait(stream, event), over named streams and events.
// One lane per (device, caller stream), created on first use, never destroyed (process lifetime).  Two implementations:
//   * HIP: lowest-priority non-blocking streams and timing-free events;
//   * the CPU emulator (ENERF_EMU): fake stream handles, every record and wait appended to the launch trace of
//     tests/emu/hip_emu.h.  The emulator runs launches synchronously in enqueue order, which is a valid schedule whenever every
//     wait names an already recorded event — so the emulator takes the same driver path as the GPU, and tests/test_frame_driver.py
//     checks the fork/join discipline on the trace.
#pragma once
#include <map>
#include <mutex>

#include "common.h"

namespace enerf {
namespace {        // internal linkage: the lane is the frame driver's alone and adds nothing to the library's symbols

enum LaneStream { kLaneMain = 0, kLaneSide, kLaneRender, kLaneStreams };        // main: the caller's stream
enum LaneEvent { kEvTrunk = 0, kEvL1, kEvL2, kEvFork, kEvDone, kEvFeats, kEvSideDone, kLaneEvents };

struct SideLane {
    hipStream_t stream[kLaneStreams];
    // the events are shared by every frame enqueued on this caller stream: two host threads calling enerf_forward on the SAME
    // stream would interleave record / wait pairs (a wait could bind to the other call's record).  The enqueue is serialised
    // per lane; a frame holds the lock until it has enqueued its last join.
    std::mutex busy;
#ifndef ENERF_EMU
    hipEvent_t event[kLaneEvents];
    bool create() {
        // lowest priority: the lanes carry leaves of the frame, the caller's stream carries its critical path — when both have
        // workgroups waiting, the chain everything else depends on should get the compute units first (a GPU-filling smooth0
        // on the lane stretched a small level-0 layer on the caller's stream 10x at 1024x1024: zju 430 -> 437 frames/s)
        int least = 0, greatest = 0;
        if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) least = 0;
        // (a CU-masked lane stream — hipExtStreamCreateWithCUMask keeping 4 / 6 / 7 of every 8 CUs, so that the chain's small layers always
        // find free CUs — measured round 6: dtu 1320 -> 962 frames/s, zju 555 -> 479 whatever the mask: profiles/r06_ab_lane_cu_mask.txt)
        bool ok = true;
        for (int s = kLaneSide; s < kLaneStreams; ++s)
            ok = ok && hipStreamCreateWithPriority(&stream[s], hipStreamNonBlocking, least) == hipSuccess;
        for (int e = 0; e < kLaneEvents; ++e) ok = ok && hipEventCreateWithFlags(&event[e], hipEventDisableTiming) == hipSuccess;
        if (!ok) (void)hipGetLastError();
        return ok;
    }
    static int device() { int dev = 0; return hipGetDevice(&dev) == hipSuccess ? dev : -1; }
    void record(LaneEvent e, LaneStream on) { hipEventRecord(event[e], stream[on]); }
    void wait(LaneStream who, LaneEvent e) { hipStreamWaitEvent(stream[who], event[e], 0); }
#else
    char handle[kLaneStreams];                     // the fake stream handles are the addresses of these
    bool create() {
        for (int s = kLaneSide; s < kLaneStreams; ++s) stream[s] = &handle[s];
        return true;
    }
    static int device() { return 0; }
#ifdef ENERF_EMU_TRACE                             // (hip_emu.h has the trace; without it the verbs do nothing)
    static const char* name(LaneStream s) { static const char* n[] = {"main", "side", "render"}; return n[s]; }
    static const char* name(LaneEvent e) { static const char* n[] = {"trunk", "l1", "l2", "fork", "done", "feats", "sidedone"}; return n[e]; }
    void record(LaneEvent e, LaneStream on) { emu::trace_sync("record", name(e), name(on), stream[on]); }
    void wait(LaneStream who, LaneEvent e) { emu::trace_sync("wait", name(e), name(who), stream[who]); }
#else
    void record(LaneEvent, LaneStream) {}
    void wait(LaneStream, LaneEvent) {}
#endif
#endif
};

// the lane of the caller's stream `main` on the current device; nullptr = none (a failed creation is remembered: the frame then
// runs on one stream)
SideLane* side_lane(hipStream_t main) {
    static std::mutex mu;
    static std::map<std::pair<int, hipStream_t>, SideLane*> lanes;
    const int dev = SideLane::device();
    if (dev < 0) return nullptr;
    std::lock_guard<std::mutex> lock(mu);
    const auto key = std::make_pair(dev, main);
    auto it = lanes.find(key);
    if (it != lanes.end()) return it->second;
    SideLane* L = new SideLane();
    L->stream[kLaneMain] = main;
    if (!L->create()) { delete L; L = nullptr; }
    lanes[key] = L;
    return L;
}

}  // namespace
}  // namespace enerf
