// pt_nearest.cpp -- the entry points of include/pt_nearest.h: the nearest surface to free points, and distance grids.
// The kernel is pt_nearest_kernels.h's (in pt_nearest.hip); this unit checks the arguments, keeps the host forms' buffers on the scene
// (grown on demand) and cuts a call into launches of at most PT_NEAREST_CHUNK queries, so that the walks' spill area -- the queries' own,
// query_spill, sized from PtPathConfig::spill_depth under the render lock -- stays bounded whatever the call's size.  The records'
// instance table is pt_query.cpp's.  Nothing here changes the scene, so every call is allowed beside a live pt_frame and with or
// without a motion mark.
#include "pt_sample_host.h"

using namespace pth;

namespace {

const size_t NEAREST_MAX = 0x7fffffffULL;
const int NEAREST_CHUNK_DEFAULT = 1 << 18; // PT_NEAREST_CHUNK: queries per launch (1024 workgroups)

int check_points(pt_scene *s, const void *points, size_t n, const void *out) {
    if(s == nullptr || (n > 0 && (points == nullptr || out == nullptr))) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    if(n > NEAREST_MAX) {
        return fail(PT_ERR_INVALID, "too many queries in one call");
    }
    return PT_OK;
}

int check_grid(pt_scene *s, const pt_distance_grid *grid, const void *out_distance, size_t *cells) {
    if(s == nullptr || grid == nullptr || out_distance == nullptr) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    if(grid->count[0] == 0 || grid->count[1] == 0 || grid->count[2] == 0) {
        return fail(PT_ERR_INVALID, "a grid count is zero");
    }
    // (each factor is below 2^32 and the running product is tested before the next one is taken in: nothing overflows)
    uint64_t n = static_cast<uint64_t>(grid->count[0]) * grid->count[1];
    if(n > NEAREST_MAX || n * grid->count[2] > NEAREST_MAX) {
        return fail(PT_ERR_INVALID, "too many cells in one call");
    }
    *cells = static_cast<size_t>(n * grid->count[2]);
    return PT_OK;
}

// What a call's launches need (render_mutex held, the device set): the walks' depth, their spill area for the largest launch, and
// (tables != nullptr) the records' tables
struct Launches {
    size_t chunk = 0;
    uint2 *spill = nullptr;
    uint32_t spill_depth = 0;
};

int prepare(pt_scene *s, size_t n, Launches *l, PtQueryTables *tables) {
    PT_TRY(setup_path(s));
    l->chunk = static_cast<size_t>(std::max(env_int("PT_NEAREST_CHUNK", NEAREST_CHUNK_DEFAULT), 1));
    l->spill_depth = s->path_cfg.spill_depth;
    const size_t lanes = (std::min(n, l->chunk) + 255) / 256 * 256;
    PT_HIP(s->query_spill.ensure(lanes * l->spill_depth));
    l->spill = s->query_spill.ptr;
    if(tables != nullptr) {
        PT_TRY(query_record_tables(s, tables));
    }
    return PT_OK;
}

void enqueue_points(pt_scene *s, const Launches &l, const PtQueryTables &tables, const float *d_points, size_t n, pt_nearest *d_out, unsigned long long *counts) {
    for(size_t first = 0; first < n; first += l.chunk) {
        pt_launch_nearest_points(s->stream, s->dev, d_points, static_cast<uint32_t>(first), static_cast<uint32_t>(std::min(l.chunk, n - first)), reinterpret_cast<float4 *>(d_out),
                                 tables, l.spill, l.spill_depth, counts);
    }
}

void enqueue_grid(pt_scene *s, const Launches &l, const pt_distance_grid *grid, float max_distance, size_t n, float *d_distance, int32_t *d_object) {
    PtDistanceGrid g;
    for(int k = 0; k < 3; k++) {
        g.origin[k] = grid->origin[k];
        g.step[k] = grid->step[k];
        g.count[k] = grid->count[k];
    }
    for(size_t first = 0; first < n; first += l.chunk) {
        pt_launch_nearest_grid(s->stream, s->dev, g, max_distance, static_cast<uint32_t>(first), static_cast<uint32_t>(std::min(l.chunk, n - first)), d_distance, d_object, l.spill,
                               l.spill_depth);
    }
}

} // namespace

extern "C" {

int pt_nearest_points(pt_scene *s, const float *points, size_t n, pt_nearest *out) {
    PT_TRY(check_points(s, points, n, out));
    if(n == 0) {
        return PT_OK;
    }
    std::lock_guard<std::mutex> lock(s->render_mutex);
    PT_HIP(hipSetDevice(s->device));
    Launches l;
    PtQueryTables tables;
    PT_TRY(prepare(s, n, &l, &tables));
    PT_HIP(s->nearest_in.ensure(4 * n));
    PT_HIP(s->nearest_out.ensure(n));
    return run_host(s, [&]() -> int {
        PT_HIP(hipMemcpyAsync(s->nearest_in.ptr, points, 4 * n * sizeof(float), hipMemcpyHostToDevice, s->stream));
        enqueue_points(s, l, tables, s->nearest_in.ptr, n, s->nearest_out.ptr, nullptr);
        PT_HIP(hipGetLastError());
        PT_HIP(hipMemcpyAsync(out, s->nearest_out.ptr, n * sizeof(pt_nearest), hipMemcpyDeviceToHost, s->stream));
        return PT_OK;
    });
}

int pt_nearest_points_device(pt_scene *s, const float *d_points, size_t n, pt_nearest *d_out, void *stream) {
    PT_TRY(check_points(s, d_points, n, d_out));
    if(n == 0) {
        return PT_OK;
    }
    std::lock_guard<std::mutex> lock(s->render_mutex);
    PT_HIP(hipSetDevice(s->device));
    Launches l;
    PtQueryTables tables;
    PT_TRY(prepare(s, n, &l, &tables));
    return run_device(s, nullptr, stream, [&]() -> int {
        enqueue_points(s, l, tables, d_points, n, d_out, nullptr);
        return PT_OK;
    });
}

int pt_distance_grid_fill(pt_scene *s, const pt_distance_grid *grid, float max_distance, float *out_distance, int32_t *out_object) {
    size_t n = 0;
    PT_TRY(check_grid(s, grid, out_distance, &n));
    std::lock_guard<std::mutex> lock(s->render_mutex);
    PT_HIP(hipSetDevice(s->device));
    Launches l;
    PT_TRY(prepare(s, n, &l, nullptr));
    PT_HIP(s->nearest_distance.ensure(n));
    if(out_object != nullptr) {
        PT_HIP(s->nearest_object.ensure(n));
    }
    return run_host(s, [&]() -> int {
        enqueue_grid(s, l, grid, max_distance, n, s->nearest_distance.ptr, out_object != nullptr ? s->nearest_object.ptr : nullptr);
        PT_HIP(hipGetLastError());
        PT_HIP(hipMemcpyAsync(out_distance, s->nearest_distance.ptr, n * sizeof(float), hipMemcpyDeviceToHost, s->stream));
        if(out_object != nullptr) {
            PT_HIP(hipMemcpyAsync(out_object, s->nearest_object.ptr, n * sizeof(int32_t), hipMemcpyDeviceToHost, s->stream));
        }
        return PT_OK;
    });
}

int pt_distance_grid_fill_device(pt_scene *s, const pt_distance_grid *grid, float max_distance, float *d_out_distance, int32_t *d_out_object, void *stream) {
    size_t n = 0;
    PT_TRY(check_grid(s, grid, d_out_distance, &n));
    std::lock_guard<std::mutex> lock(s->render_mutex);
    PT_HIP(hipSetDevice(s->device));
    Launches l;
    PT_TRY(prepare(s, n, &l, nullptr));
    return run_device(s, nullptr, stream, [&]() -> int {
        enqueue_grid(s, l, grid, max_distance, n, d_out_distance, d_out_object);
        return PT_OK;
    });
}

// Diagnostic, not part of include/pt_hip.h (tools/nearest_timing.py): pt_nearest_points on host points, with the pair and leaf records
// the walks fetched in out_counts[0] and out_counts[1] and the kernels' time on the device in *out_ms.  The records stay on the device.
int pt_debug_nearest_counts(pt_scene *s, const float *points, size_t n, unsigned long long *out_counts, float *out_ms) {
    PT_TRY(check_points(s, points, n, out_counts));
    if(n == 0 || out_ms == nullptr) {
        return fail(PT_ERR_INVALID, "nothing to measure");
    }
    std::lock_guard<std::mutex> lock(s->render_mutex);
    PT_HIP(hipSetDevice(s->device));
    Launches l;
    PtQueryTables tables;
    PT_TRY(prepare(s, n, &l, &tables));
    PT_HIP(s->nearest_in.ensure(4 * n));
    PT_HIP(s->nearest_out.ensure(n));
    DevBuf<unsigned long long> counts;
    PT_HIP(counts.ensure(2));
    EventPair timer;
    return run_host(s, [&]() -> int {
        PT_HIP(hipMemcpyAsync(s->nearest_in.ptr, points, 4 * n * sizeof(float), hipMemcpyHostToDevice, s->stream));
        PT_HIP(hipMemsetAsync(counts.ptr, 0, 2 * sizeof(unsigned long long), s->stream));
        PT_HIP(timer.begin(s->stream));
        enqueue_points(s, l, tables, s->nearest_in.ptr, n, s->nearest_out.ptr, counts.ptr);
        PT_HIP(hipGetLastError());
        PT_HIP(timer.end(s->stream));
        PT_HIP(hipMemcpyAsync(out_counts, counts.ptr, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s->stream));
        PT_HIP(hipStreamSynchronize(s->stream));
        PT_HIP(timer.ms(out_ms));
        return PT_OK;
    });
}

} // extern "C"
