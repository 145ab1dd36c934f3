// pt_motion_shapes.cpp -- the entry points of include/pt_motion_shapes.h: the mark a scene keeps of its previous
// frame -- instance matrices, and per mesh the vertices it had and its shape serial --, the table of the face every instance triangle
// came from (made behind every assembly chunk while a mark exists: assemble_batch in pt_meshes.cpp, adopted by rebuild_instances in
// pt_pose.cpp), and the feature pass that reprojects hits on deformed meshes per vertex (pt_walks.hip: pt_motion_shapes_kernel).  A call
// in which no instance is deformed is pt_render_features_motion's own route (pt_motion.cpp) with the marked matrices.
#include "pt_host.h"

using namespace pth;

namespace {

// The scene's mark, or the refusal (render_mutex held)
int marked_scene(pt_scene *s, MotionMark **out) {
    if(s->pose == nullptr) {
        return fail(PT_ERR_UNSUPPORTED, DEFORM_NO_INSTANCES);
    }
    if(s->pose->mark == nullptr) {
        return fail(PT_ERR_INVALID, "the scene has no motion mark (pt_scene_motion_mark first)");
    }
    *out = s->pose->mark.get();
    return PT_OK;
}

// The kind of instance i against the mark, and for MOVED its tables (the identity or zero otherwise)
uint8_t marked_kind(const PoseKeep &keep, const MotionMark &mark, size_t i, float back[12], float normal[9]) {
    const pt_mesh_instance &in = keep.instances[i];
    const float *p = mark.transforms.data() + 16 * i;
    uint8_t kind;
    if(keep.meshes[in.mesh]->shape_serial == mark.serial[in.mesh]) {
        kind = motion_of(in.transform, p, back, normal);
    }
    else {
        kind = PT_MOTION_DEFORMED;
        for(int k = 0; k < 16; k++) {
            if(!std::isfinite(p[k])) {
                kind = PT_MOTION_NONE;
            }
        }
    }
    if(kind != PT_MOTION_MOVED) {
        motion_identity(kind == PT_MOTION_STATIC ? PT_MOTION_STATIC : PT_MOTION_NONE, back, normal);
    }
    return kind;
}

// The device table of a marked call (render_mutex held).  *deformed: whether any instance that has objects is DEFORMED; only then is
// there a table, of *n_out entries.  No device work before the last refusal.
int shape_instances(pt_scene *s, MotionMark &mark, bool *deformed, uint32_t *n_out) {
    const PoseKeep &keep = *s->pose;
    *deformed = false;
    *n_out = 0;
    // (the pose-only route needs none of the table: the serials alone say whether a mesh with objects changed shape)
    bool any_changed = false;
    for(size_t i = 0; i < keep.instances.size(); i++) {
        const uint32_t mesh = keep.instances[i].mesh;
        any_changed = any_changed || (s->inst_count[i] != 0 && keep.meshes[mesh]->shape_serial != mark.serial[mesh]);
    }
    if(!any_changed) {
        return PT_OK;
    }
    std::vector<PtShapeMotionInstance> table;
    uint64_t face_first = 0;
    for(size_t i = 0; i < keep.instances.size(); i++) {
        const KeptMesh &mesh = *keep.meshes[keep.instances[i].mesh];
        const uint64_t first_face = face_first;
        face_first += mesh.n_faces;
        if(s->inst_count[i] == 0) { // (shares its first object with a neighbour: never looked up)
            continue;
        }
        PtShapeMotionInstance m{};
        float back[12], normal[9];
        m.kind = marked_kind(keep, mark, i, back, normal);
        *deformed = *deformed || m.kind == PT_MOTION_DEFORMED;
        m.first = s->inst_first[i];
        m.count = s->inst_count[i];
        m.face_first = static_cast<uint32_t>(first_face);
        std::copy(back, back + 12, m.back);
        for(int r = 0; r < 3; r++) {
            std::copy(normal + 3 * r, normal + 3 * r + 3, m.normal + 4 * r);
        }
        m.faces = mesh.faces.ptr;
        m.marked = mark.shape[keep.instances[i].mesh];
        std::copy(mark.transforms.begin() + 16 * i, mark.transforms.begin() + 16 * i + 16, m.m);
        table.push_back(m);
    }
    if(!*deformed) {
        return PT_OK;
    }
    if(!mark.has_table) { // cannot happen: a serial only moves in a rebuild, and every rebuild of a marked scene makes the table
        return fail(PT_ERR_HIP, "internal: a deformed instance without a face table");
    }
    PT_HIP(hipSetDevice(s->device));
    PT_HIP(mark.table.ensure(table.size()));
    PT_HIP(hipMemcpyAsync(mark.table.ptr, table.data(), table.size() * sizeof(PtShapeMotionInstance), hipMemcpyHostToDevice, s->stream));
    PT_HIP(hipStreamSynchronize(s->stream)); // the table is this function's vector
    *n_out = static_cast<uint32_t>(table.size());
    return PT_OK;
}

// Enqueues the marked pass on the scene's stream (render_mutex held): pt_motion_kernel when nothing is deformed, else pt_motion_shapes_kernel
int marked_launch(pt_scene *s, MotionMark &mark, const pt_camera_params *camera, const pt_options *options, float4 *d_features, float4 *d_motion) {
    bool deformed = false;
    uint32_t n_shape = 0;
    PT_TRY(shape_instances(s, mark, &deformed, &n_shape));
    if(!deformed) {
        uint32_t n_instances = 0;
        PT_TRY(motion_instances(s, mark.transforms.data(), &n_instances));
        return motion_launch(s, camera, options, n_instances, d_features, d_motion);
    }
    PT_TRY(setup_path(s));
    PtDevCamera cam = derive_camera(camera);
    cam.aperture_kind = PT_APERTURE_NONE; // the rays are a pure function of camera and pixel
    PtPathConfig cfg = s->path_cfg;
    const size_t n = static_cast<size_t>(options->image_width) * static_cast<size_t>(options->image_height);
    PT_HIP(s->feature_spill.ensure(((n + 255) / 256) * 256 * cfg.spill_depth));
    cfg.spill = s->feature_spill.ptr;
    pt_launch_features_motion_shapes(s->stream, s->dev, cam, options->image_width, options->image_height, d_features, d_motion, mark.table.ptr, n_shape, mark.face_of.ptr,
                                     s->n_desc_objects, cfg);
    PT_HIP(hipGetLastError());
    return PT_OK;
}

} // namespace

extern "C" {

int pt_scene_motion_mark(pt_scene *s, pt_motion_mark_info *info) {
    if(info != nullptr) {
        *info = pt_motion_mark_info{};
    }
    if(s == nullptr) {
        return fail(PT_ERR_INVALID, "null scene");
    }
    std::lock_guard<std::mutex> lock(s->render_mutex);
    if(s->pose == nullptr) {
        return fail(PT_ERR_UNSUPPORTED, DEFORM_NO_INSTANCES);
    }
    const auto t_begin = std::chrono::steady_clock::now();
    PoseKeep &keep = *s->pose;
    const size_t n_meshes = keep.meshes.size(), n_instances = keep.instances.size();
    PT_HIP(hipSetDevice(s->device));
    // Allocations come first: a refusal there leaves the old mark as it was.  The copies overwrite the `marked` buffers the old mark
    // names, so a copy or a wait that fails leaves the scene WITHOUT a mark (Unmark below) rather than with a half-written one.
    const bool first = keep.mark == nullptr;
    std::unique_ptr<MotionMark> fresh;
    if(first) {
        uint64_t faces = 0;
        for(const pt_mesh_instance &in : keep.instances) {
            faces += keep.meshes[in.mesh]->n_faces;
        }
        fresh.reset(new MotionMark());
        PT_TRY(ensure_counted(keep, fresh->face_of, static_cast<size_t>(faces)));
        PT_TRY(ensure_counted(keep, fresh->face_of_spare, static_cast<size_t>(faces)));
    }
    for(size_t m = 0; m < n_meshes; m++) {
        if(keep.meshes[m] != nullptr && keep.meshes[m]->shape != keep.meshes[m]->vertices.ptr) {
            PT_TRY(ensure_counted(keep, keep.meshes[m]->deform->marked, 3 * static_cast<size_t>(keep.meshes[m]->n_vertices)));
        }
    }
    StreamDrain drain{s->stream};
    struct Unmark {
        PoseKeep &keep;
        bool armed = true;
        ~Unmark() {
            if(armed) {
                (void)hipStreamSynchronize(keep_stream);
                keep.mark.reset();
            }
        }
        hipStream_t keep_stream;
    } unmark{keep, true, s->stream};
    uint32_t copied = 0;
    uint64_t bytes = 0;
    std::vector<const float *> shape(n_meshes, nullptr);
    std::vector<uint64_t> serial(n_meshes, 0);
    for(size_t m = 0; m < n_meshes; m++) {
        if(keep.meshes[m] == nullptr) {
            continue;
        }
        KeptMesh &mesh = *keep.meshes[m];
        serial[m] = mesh.shape_serial;
        if(mesh.shape == mesh.vertices.ptr) {
            shape[m] = mesh.vertices.ptr;
            continue;
        }
        const size_t size = 3 * static_cast<size_t>(mesh.n_vertices) * sizeof(float);
        if(size > 0) {
            PT_HIP(hipMemcpyAsync(mesh.deform->marked.ptr, mesh.shape, size, hipMemcpyDeviceToDevice, s->stream));
        }
        shape[m] = mesh.deform->marked.ptr;
        copied++;
        bytes += size;
    }
    PT_HIP(hipStreamSynchronize(s->stream));
    drain.armed = false;
    unmark.armed = false;
    if(first) {
        keep.mark = std::move(fresh);
    }
    MotionMark &mark = *keep.mark;
    mark.transforms.resize(16 * n_instances);
    for(size_t i = 0; i < n_instances; i++) {
        std::copy(keep.instances[i].transform, keep.instances[i].transform + 16, mark.transforms.begin() + 16 * i);
    }
    mark.shape = std::move(shape);
    mark.serial = std::move(serial);
    if(info != nullptr) {
        info->n_instances = static_cast<uint32_t>(n_instances);
        info->n_meshes_copied = copied;
        info->bytes_copied = bytes;
        info->allocations = static_cast<uint32_t>(keep.scratch.allocations + keep.deform_allocations);
        info->total_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    }
    return PT_OK;
}

int pt_scene_motion_unmark(pt_scene *s) {
    if(s == nullptr) {
        return fail(PT_ERR_INVALID, "null scene");
    }
    std::lock_guard<std::mutex> lock(s->render_mutex);
    if(s->pose == nullptr) {
        return fail(PT_ERR_UNSUPPORTED, DEFORM_NO_INSTANCES);
    }
    PoseKeep &keep = *s->pose;
    if(keep.mark == nullptr) {
        return PT_OK;
    }
    PT_HIP(hipSetDevice(s->device));
    PT_HIP(hipStreamSynchronize(s->stream)); // (nothing reads the mark's buffers any more)
    keep.mark.reset();
    for(const std::unique_ptr<KeptMesh> &mesh : keep.meshes) {
        if(mesh != nullptr && mesh->deform != nullptr) {
            mesh->deform->marked.release();
        }
    }
    return PT_OK;
}

int pt_scene_get_motion_mark(pt_scene *s, float *out_transforms, uint8_t *out_kind) {
    if(s == nullptr) {
        return fail(PT_ERR_INVALID, "null scene");
    }
    std::lock_guard<std::mutex> lock(s->render_mutex);
    MotionMark *mark = nullptr;
    PT_TRY(marked_scene(s, &mark));
    const PoseKeep &keep = *s->pose;
    if(out_transforms != nullptr) {
        std::copy(mark->transforms.begin(), mark->transforms.end(), out_transforms);
    }
    for(size_t i = 0; out_kind != nullptr && i < keep.instances.size(); i++) {
        float back[12], normal[9];
        out_kind[i] = marked_kind(keep, *mark, i, back, normal);
    }
    return PT_OK;
}

int pt_scene_get_triangle_faces(pt_scene *s, uint32_t *out, uint32_t *n) {
    if(s == nullptr) {
        return fail(PT_ERR_INVALID, "null scene");
    }
    std::lock_guard<std::mutex> lock(s->render_mutex);
    MotionMark *mark = nullptr;
    PT_TRY(marked_scene(s, &mark));
    if(!mark->has_table) {
        return fail(PT_ERR_INVALID, "no rebuild since the first mark: the face table is made by the next pt_scene_pose, pt_scene_deform or pt_scene_morph");
    }
    const uint32_t count = s->n_objects - s->n_desc_objects;
    if(n != nullptr) {
        *n = count;
    }
    if(out != nullptr && count > 0) {
        PT_HIP(hipSetDevice(s->device));
        PT_HIP(hipMemcpyAsync(out, mark->face_of.ptr, count * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
        PT_HIP(hipStreamSynchronize(s->stream));
    }
    return PT_OK;
}

int pt_render_features_motion_marked(pt_scene *s, const pt_camera_params *camera, const pt_options *options, float *out_features, float *out_motion) {
    PT_TRY(motion_check(s, camera, options, out_features, out_motion));
    const size_t n = static_cast<size_t>(options->image_width) * static_cast<size_t>(options->image_height);
    std::lock_guard<std::mutex> lock(s->render_mutex);
    MotionMark *mark = nullptr;
    PT_TRY(marked_scene(s, &mark));
    PT_HIP(hipSetDevice(s->device));
    PT_HIP(s->features.ensure(3 * n));
    PT_HIP(s->motion.ensure(2 * n));
    PT_TRY(marked_launch(s, *mark, camera, options, reinterpret_cast<float4 *>(s->features.ptr), reinterpret_cast<float4 *>(s->motion.ptr)));
    PT_HIP(hipMemcpyAsync(out_features, s->features.ptr, 3 * n * sizeof(F4), hipMemcpyDeviceToHost, s->stream));
    PT_HIP(hipMemcpyAsync(out_motion, s->motion.ptr, 2 * n * sizeof(F4), hipMemcpyDeviceToHost, s->stream));
    PT_HIP(hipStreamSynchronize(s->stream));
    return PT_OK;
}

int pt_render_features_motion_marked_device(pt_scene *s, const pt_camera_params *camera, const pt_options *options, float *d_out_features, float *d_out_motion, void *stream) {
    PT_TRY(motion_check(s, camera, options, d_out_features, d_out_motion));
    std::lock_guard<std::mutex> lock(s->render_mutex);
    MotionMark *mark = nullptr;
    PT_TRY(marked_scene(s, &mark));
    PT_HIP(hipSetDevice(s->device));
    // order after the caller's stream, trace on the library's stream, then make the caller's stream wait for it
    StreamOrder order;
    PT_TRY(order.begin(stream, s->stream));
    PT_TRY(marked_launch(s, *mark, camera, options, reinterpret_cast<float4 *>(d_out_features), reinterpret_cast<float4 *>(d_out_motion)));
    PT_TRY(order.end());
    if(order.caller == nullptr) {
        PT_HIP(hipStreamSynchronize(s->stream));
    }
    return PT_OK;
}

} // extern "C"
