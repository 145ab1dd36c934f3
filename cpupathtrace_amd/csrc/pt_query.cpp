// pt_query.cpp -- the entry points of include/pt_query.h: hit records for rays, pixels and frames, and occlusion tests
// of segments.  The kernels are pt_query_kernels.h's (in pt_walks.hip); this unit checks the arguments, keeps the queries' buffers on
// the scene (grown on demand), and keeps the instance table the records are made with: the instances that have objects, by first
// object, uploaded when the scene's instance ranges are not the ones it was made from -- after creation and after every rebuild, not
// per call.  Nothing here changes the scene, so every call is allowed with a live pt_frame and with or without a motion mark.
#include "pt_host.h"

using namespace pth;

namespace {

const size_t QUERY_MAX = 0x7fffffffULL;

int check_batch(pt_scene *s, const void *in, size_t n, const void *out) {
    if(s == nullptr || (n > 0 && (in == nullptr || out == nullptr))) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    if(n > QUERY_MAX) {
        return fail(PT_ERR_INVALID, "too many queries in one call");
    }
    return PT_OK;
}

int check_frame(pt_scene *s, const pt_camera_params *camera, const pt_options *options) {
    PT_TRY(check_render_args(s, camera, options));
    if(static_cast<uint64_t>(options->image_width) * static_cast<uint64_t>(options->image_height) > QUERY_MAX) {
        return fail(PT_ERR_INVALID, "too many queries in one call");
    }
    return PT_OK;
}

// The tables a record is made with (render_mutex held, the device set).  The instance table is made again only when the scene's ranges
// differ from the ones it was made from; the upload is waited for, since it reads this function's vector.
int query_tables(pt_scene *s, PtQueryTables *out) {
    *out = PtQueryTables{nullptr, 0, s->n_desc_objects, nullptr};
    if(s->pose == nullptr) {
        return PT_OK;
    }
    const PoseKeep &keep = *s->pose;
    if(!s->query_table_made || s->query_inst_first != s->inst_first || s->query_inst_count != s->inst_count) {
        std::vector<PtQueryInstance> table;
        uint64_t face_first = 0;
        for(size_t i = 0; i < keep.instances.size(); i++) {
            const KeptMesh &mesh = *keep.meshes[keep.instances[i].mesh];
            const uint64_t first_face = face_first;
            face_first += mesh.n_faces;
            if(s->inst_count[i] == 0) { // (shares its first object with a neighbour: never looked up)
                continue;
            }
            PtQueryInstance q{};
            q.first = s->inst_first[i];
            q.count = s->inst_count[i];
            q.face_first = static_cast<uint32_t>(first_face);
            q.n_faces = mesh.n_faces;
            q.instance = static_cast<uint32_t>(i);
            table.push_back(q);
        }
        if(!table.empty()) {
            PT_HIP(s->query_instances.ensure(table.size()));
            PT_HIP(hipMemcpyAsync(s->query_instances.ptr, table.data(), table.size() * sizeof(PtQueryInstance), hipMemcpyHostToDevice, s->stream));
            PT_HIP(hipStreamSynchronize(s->stream));
        }
        s->query_n_instances = static_cast<uint32_t>(table.size());
        s->query_inst_first = s->inst_first;
        s->query_inst_count = s->inst_count;
        s->query_table_made = true;
    }
    out->inst = s->query_instances.ptr;
    out->n_inst = s->query_n_instances;
    if(keep.mark != nullptr && keep.mark->has_table) {
        out->face_of = keep.mark->face_of.ptr;
    }
    return PT_OK;
}

// The launch configuration of n walks with the queries' own spill area, and (tables != nullptr) the records' tables
int prepare(pt_scene *s, size_t n, PtPathConfig *cfg, PtQueryTables *tables) {
    PT_TRY(setup_path(s));
    *cfg = s->path_cfg;
    PT_HIP(s->query_spill.ensure(((n + 255) / 256) * 256 * cfg->spill_depth));
    cfg->spill = s->query_spill.ptr;
    if(tables != nullptr) {
        PT_TRY(query_tables(s, tables));
    }
    return PT_OK;
}

PtDevCamera pixel_camera(const pt_camera_params *camera) {
    PtDevCamera cam = derive_camera(camera);
    cam.aperture_kind = PT_APERTURE_NONE; // the rays are a pure function of camera and pixel
    return cam;
}

// What the four entry points differ in: `enqueue` launches on the scene's stream.  Host form: upload `in` (in_bytes, may be null: a
// frame has no input), enqueue, download out_bytes.  Device form: the same launch between the two halves of a StreamOrder.
template<typename Enqueue>
int run_host(pt_scene *s, const void *in, size_t in_bytes, void *d_in, void *out, size_t out_bytes, const void *d_out, Enqueue enqueue) {
    if(in != nullptr) {
        PT_HIP(hipMemcpyAsync(d_in, in, in_bytes, hipMemcpyHostToDevice, s->stream));
    }
    StreamDrain drain{s->stream};
    enqueue();
    PT_HIP(hipGetLastError());
    PT_HIP(hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, s->stream));
    drain.armed = false;
    PT_HIP(hipStreamSynchronize(s->stream));
    return PT_OK;
}

template<typename Enqueue>
int run_device(pt_scene *s, void *stream, Enqueue enqueue) {
    // order after the caller's stream, trace on the library's stream, then make the caller's stream wait for it
    StreamOrder order;
    PT_TRY(order.begin(stream, s->stream));
    enqueue();
    PT_HIP(hipGetLastError());
    PT_TRY(order.end());
    if(order.caller == nullptr) {
        PT_HIP(hipStreamSynchronize(s->stream));
    }
    return PT_OK;
}

} // namespace

int pth::query_record_tables(pt_scene *s, PtQueryTables *out) {
    return query_tables(s, out);
}

extern "C" {

int pt_query_rays(pt_scene *s, const float *rays, size_t n, pt_hit *out) {
    PT_TRY(check_batch(s, rays, n, out));
    if(n == 0) {
        return PT_OK;
    }
    std::lock_guard<std::mutex> lock(s->render_mutex);
    PT_HIP(hipSetDevice(s->device));
    PtPathConfig cfg;
    PtQueryTables tables;
    PT_TRY(prepare(s, n, &cfg, &tables));
    PT_HIP(s->query_in.ensure(6 * n));
    PT_HIP(s->query_out.ensure(n));
    return run_host(s, rays, 6 * n * sizeof(float), s->query_in.ptr, out, n * sizeof(pt_hit), s->query_out.ptr, [&] {
        pt_launch_query_rays(s->stream, s->dev, s->query_in.ptr, static_cast<uint32_t>(n), reinterpret_cast<float4 *>(s->query_out.ptr), tables, cfg);
    });
}

int pt_query_rays_device(pt_scene *s, const float *d_rays, size_t n, pt_hit *d_out, void *stream) {
    PT_TRY(check_batch(s, d_rays, n, d_out));
    if(n == 0) {
        return PT_OK;
    }
    std::lock_guard<std::mutex> lock(s->render_mutex);
    PT_HIP(hipSetDevice(s->device));
    PtPathConfig cfg;
    PtQueryTables tables;
    PT_TRY(prepare(s, n, &cfg, &tables));
    return run_device(s, stream, [&] { pt_launch_query_rays(s->stream, s->dev, d_rays, static_cast<uint32_t>(n), reinterpret_cast<float4 *>(d_out), tables, cfg); });
}

int pt_query_pixels(pt_scene *s, const pt_camera_params *camera, const pt_options *options, const int32_t *xy, size_t n, pt_hit *out) {
    PT_TRY(check_frame(s, camera, options));
    PT_TRY(check_batch(s, xy, n, out));
    for(size_t i = 0; i < n; i++) {
        if(xy[2 * i] < 0 || xy[2 * i] >= options->image_width || xy[2 * i + 1] < 0 || xy[2 * i + 1] >= options->image_height) {
            return fail(PT_ERR_INVALID, "pixel " + std::to_string(i) + " lies outside the frame");
        }
    }
    if(n == 0) {
        return PT_OK;
    }
    std::lock_guard<std::mutex> lock(s->render_mutex);
    PT_HIP(hipSetDevice(s->device));
    PtPathConfig cfg;
    PtQueryTables tables;
    PT_TRY(prepare(s, n, &cfg, &tables));
    PT_HIP(s->query_in.ensure(2 * n));
    PT_HIP(s->query_out.ensure(n));
    const PtDevCamera cam = pixel_camera(camera);
    const int32_t *d_xy = reinterpret_cast<const int32_t *>(s->query_in.ptr); // (4 bytes per entry either way)
    return run_host(s, xy, 2 * n * sizeof(int32_t), s->query_in.ptr, out, n * sizeof(pt_hit), s->query_out.ptr, [&] {
        pt_launch_query_pixels(s->stream, s->dev, cam, options->image_width, options->image_height, d_xy, static_cast<uint32_t>(n), reinterpret_cast<float4 *>(s->query_out.ptr),
                               tables, cfg);
    });
}

int pt_query_pixels_device(pt_scene *s, const pt_camera_params *camera, const pt_options *options, const int32_t *d_xy, size_t n, pt_hit *d_out, void *stream) {
    PT_TRY(check_frame(s, camera, options));
    PT_TRY(check_batch(s, d_xy, n, d_out));
    if(n == 0) {
        return PT_OK;
    }
    std::lock_guard<std::mutex> lock(s->render_mutex);
    PT_HIP(hipSetDevice(s->device));
    PtPathConfig cfg;
    PtQueryTables tables;
    PT_TRY(prepare(s, n, &cfg, &tables));
    const PtDevCamera cam = pixel_camera(camera);
    return run_device(s, stream, [&] {
        pt_launch_query_pixels(s->stream, s->dev, cam, options->image_width, options->image_height, d_xy, static_cast<uint32_t>(n), reinterpret_cast<float4 *>(d_out), tables, cfg);
    });
}

int pt_query_frame(pt_scene *s, const pt_camera_params *camera, const pt_options *options, pt_hit *out) {
    PT_TRY(check_frame(s, camera, options));
    if(out == nullptr) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    const size_t n = static_cast<size_t>(options->image_width) * static_cast<size_t>(options->image_height);
    std::lock_guard<std::mutex> lock(s->render_mutex);
    PT_HIP(hipSetDevice(s->device));
    PtPathConfig cfg;
    PtQueryTables tables;
    PT_TRY(prepare(s, n, &cfg, &tables));
    PT_HIP(s->query_out.ensure(n));
    const PtDevCamera cam = pixel_camera(camera);
    return run_host(s, nullptr, 0, nullptr, out, n * sizeof(pt_hit), s->query_out.ptr, [&] {
        pt_launch_query_pixels(s->stream, s->dev, cam, options->image_width, options->image_height, nullptr, static_cast<uint32_t>(n), reinterpret_cast<float4 *>(s->query_out.ptr),
                               tables, cfg);
    });
}

int pt_query_frame_device(pt_scene *s, const pt_camera_params *camera, const pt_options *options, pt_hit *d_out, void *stream) {
    PT_TRY(check_frame(s, camera, options));
    if(d_out == nullptr) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    const size_t n = static_cast<size_t>(options->image_width) * static_cast<size_t>(options->image_height);
    std::lock_guard<std::mutex> lock(s->render_mutex);
    PT_HIP(hipSetDevice(s->device));
    PtPathConfig cfg;
    PtQueryTables tables;
    PT_TRY(prepare(s, n, &cfg, &tables));
    const PtDevCamera cam = pixel_camera(camera);
    return run_device(s, stream, [&] {
        pt_launch_query_pixels(s->stream, s->dev, cam, options->image_width, options->image_height, nullptr, static_cast<uint32_t>(n), reinterpret_cast<float4 *>(d_out), tables, cfg);
    });
}

int pt_occluded_rays(pt_scene *s, const float *segments, size_t n, uint8_t *out) {
    PT_TRY(check_batch(s, segments, n, out));
    if(n == 0) {
        return PT_OK;
    }
    std::lock_guard<std::mutex> lock(s->render_mutex);
    PT_HIP(hipSetDevice(s->device));
    PtPathConfig cfg;
    PT_TRY(prepare(s, n, &cfg, nullptr));
    PT_HIP(s->query_in.ensure(7 * n));
    PT_HIP(s->query_flags.ensure(n));
    return run_host(s, segments, 7 * n * sizeof(float), s->query_in.ptr, out, n, s->query_flags.ptr,
                    [&] { pt_launch_occluded(s->stream, s->dev, s->query_in.ptr, static_cast<uint32_t>(n), s->query_flags.ptr, cfg); });
}

int pt_occluded_rays_device(pt_scene *s, const float *d_segments, size_t n, uint8_t *d_out, void *stream) {
    PT_TRY(check_batch(s, d_segments, n, d_out));
    if(n == 0) {
        return PT_OK;
    }
    std::lock_guard<std::mutex> lock(s->render_mutex);
    PT_HIP(hipSetDevice(s->device));
    PtPathConfig cfg;
    PT_TRY(prepare(s, n, &cfg, nullptr));
    return run_device(s, stream, [&] { pt_launch_occluded(s->stream, s->dev, d_segments, static_cast<uint32_t>(n), d_out, cfg); });
}

} // extern "C"
