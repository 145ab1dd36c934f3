// pt_sample_host.h -- the launch frame of the host units whose calls trace path samples: pt_gather.cpp, pt_light_probes.cpp,
// pt_radiance.cpp and pt_light_passes.cpp.  One of each: the rule that cuts a call into launches, the per-device workspace table with the
// wait for what the latest device-form call left running, the sizing of a launch's spill area and plane, and the two brackets a call's
// work is enqueued between -- host form and device form.  Internal, like pt_host.h.
#ifndef PT_SAMPLE_HOST_H
#define PT_SAMPLE_HOST_H

#include "pt_host.h"

namespace pth {

// The (item, sample) pairs of one launch where the environment variable does not say: one default per variable
const int GATHER_CHUNK_DEFAULT = 4 << 20;      // PT_GATHER_CHUNK
const int LIGHT_PROBE_CHUNK_DEFAULT = 2 << 20; // PT_LIGHT_PROBE_CHUNK
const int RADIANCE_CHUNK_DEFAULT = 2 << 20;    // PT_RADIANCE_CHUNK (pt_light_passes.cpp divides it by its passes)

// Items -- points, probes, rays or pixels -- per launch: whole ones, `env` / divisor pairs at the most, one where one alone has more.
// The variable is read per call.
inline size_t chunk_items(const char *env, int default_pairs, int32_t samples, uint32_t divisor) {
    const int pairs = std::max(env_int(env, default_pairs), 1);
    return std::max<size_t>(static_cast<size_t>(pairs) / divisor / static_cast<size_t>(samples), 1);
}

// What every per-device workspace has: the workspace of one launch -- the samples' plane and the walks' spill area -- and the order of
// the calls.  One call at a time per device (`mutex`, taken behind the scene's render lock); `last` marks the end of the latest
// device-form call, whose work may still run when the next call comes: that call waits for it (settle) before it touches a buffer.
// A unit derives its own workspace from this and adds its buffers.
struct SampleWorkspace {
    std::mutex mutex;
    DevBuf<F4> plane;
    DevBuf<uint2> spill;
    hipEvent_t last = nullptr;
    bool pending = false;
};

// The workspace of type W of a device: one table per W, so every unit keeps its own, with a mutex and buffers of its own.  Created on
// first use under the table's mutex; lives as long as the process (never freed: a static destructor would run after the HIP runtime
// has gone).
template<typename W>
W &sample_workspace(int device) {
    static std::mutex table_mutex;
    static std::vector<W *> table;
    std::lock_guard<std::mutex> lock(table_mutex);
    if(static_cast<size_t>(device) >= table.size()) {
        table.resize(static_cast<size_t>(device) + 1, nullptr);
    }
    if(table[static_cast<size_t>(device)] == nullptr) {
        table[static_cast<size_t>(device)] = new W();
    }
    return *table[static_cast<size_t>(device)];
}

// ws.mutex held: what the latest device-form call left running has ended
inline int settle(SampleWorkspace &ws) {
    if(ws.pending) {
        PT_HIP(hipEventSynchronize(ws.last));
        ws.pending = false;
    }
    return PT_OK;
}

// The launch configuration of a call whose largest launch has `lanes` lanes, with its spill area, and `cells` float4 in `plane` (null:
// the call has no plane).  render_mutex held, the device set.
inline int size_launch(pt_scene *s, DevBuf<uint2> &spill, size_t lanes, DevBuf<F4> *plane, size_t cells, PtPathConfig *cfg) {
    PT_TRY(setup_path(s));
    *cfg = s->path_cfg;
    PT_HIP(spill.ensure(((lanes + 255) / 256) * 256 * cfg->spill_depth));
    cfg->spill = spill.ptr;
    if(plane != nullptr) {
        PT_HIP(plane->ensure(cells));
    }
    return PT_OK;
}

// Host form: what `enqueue_all` puts on the scene's stream -- its uploads, its launches and its downloads; it returns a status --, then
// the wait for it.  A failure on the way waits as well: the stream may hold work of a call that must not outlive the call.
template<typename Enqueue>
int run_host(pt_scene *s, Enqueue enqueue_all) {
    StreamDrain drain{s->stream};
    PT_TRY(enqueue_all());
    PT_HIP(hipGetLastError());
    drain.armed = false;
    PT_HIP(hipStreamSynchronize(s->stream));
    return PT_OK;
}

// Device form: the same between the two halves of a StreamOrder.  `ws` (null: the call uses no workspace that outlives it -- its buffers
// are the scene's or the caller's, ordered by the scene's stream) gets the end of the work recorded for the next call's settle.  A call
// without a caller stream still waits.
template<typename Enqueue>
int run_device(pt_scene *s, SampleWorkspace *ws, void *stream, Enqueue enqueue_all) {
    StreamOrder order;
    PT_TRY(order.begin(stream, s->stream));
    PT_TRY(enqueue_all());
    PT_HIP(hipGetLastError());
    if(ws != nullptr) {
        if(ws->last == nullptr) {
            PT_HIP(hipEventCreateWithFlags(&ws->last, hipEventDisableTiming));
        }
        PT_HIP(hipEventRecord(ws->last, s->stream));
        ws->pending = true;
    }
    PT_TRY(order.end());
    if(order.caller == nullptr) {
        PT_HIP(hipStreamSynchronize(s->stream));
    }
    return PT_OK;
}

} // namespace pth

#endif
