// pt_deform.cpp -- the entry points of include/pt_deform.h: a scene's meshes under new vertices, in place.  A mesh's
// current vertices are made in its spare buffer -- uploaded, or skinned from the rest vertices by pt_skin_launch (pt_deform.hip) on the
// scene's stream --, the meshes' `shape` pointers are turned to them, and the rest is a pose: rebuild_instances (pt_pose.cpp) assembles
// all instances behind the skinning launches without a host wait between them and adopts the finished scene.  Only then do spare and
// current buffers change places; a call that fails turns the pointers back.  That back half -- adopt_shapes, with the pose arguments'
// checks and the vertex buffers beside it -- is shared with pt_scene_morph (pt_morph.cpp), which makes its vertices with another kernel.
#include "pt_host.h"

using namespace pth;

namespace pth {

const char *const DEFORM_NO_INSTANCES = "the scene has no instances: it was not made by pt_scene_create_meshes with instances";
const char *const DEFORM_LIVE_FRAME = "the scene has a live frame: its parked state belongs to the present geometry (pt_frame_destroy first)";

int used_mesh(PoseKeep &keep, uint32_t mesh, KeptMesh **out) {
    if(mesh >= keep.meshes.size()) {
        return fail(PT_ERR_INVALID, "mesh index " + std::to_string(mesh) + " out of range: the scene was created with " + std::to_string(keep.meshes.size()));
    }
    if(keep.meshes[mesh] == nullptr) {
        return fail(PT_ERR_INVALID, "mesh " + std::to_string(mesh) + " is used by no instance");
    }
    *out = keep.meshes[mesh].get();
    return PT_OK;
}

int check_pose_arguments(const PoseKeep &keep, const uint32_t *instances, uint32_t n) {
    const uint32_t n_instances = static_cast<uint32_t>(keep.instances.size());
    if(instances == nullptr && n != 0 && n != n_instances) {
        return fail(PT_ERR_INVALID, "a pose of all instances needs " + std::to_string(n_instances) + " matrices, not " + std::to_string(n));
    }
    for(uint32_t k = 0; instances != nullptr && k < n; k++) {
        if(instances[k] >= n_instances) {
            return fail(PT_ERR_INVALID, "instance index " + std::to_string(instances[k]) + " out of range: the scene has " + std::to_string(n_instances));
        }
    }
    return PT_OK;
}

std::vector<pt_mesh_instance> posed_instances(const PoseKeep &keep, const uint32_t *instances, uint32_t n, const float *transforms) {
    std::vector<pt_mesh_instance> posed = keep.instances; // (adopted with the rest, on success)
    for(uint32_t k = 0; k < n; k++) {
        const uint32_t i = instances != nullptr ? instances[k] : k;
        std::copy(transforms + 16 * static_cast<size_t>(k), transforms + 16 * static_cast<size_t>(k) + 16, posed[i].transform);
    }
    return posed;
}

int ensure_vertex_buffers(PoseKeep &keep, KeptMesh &mesh) {
    if(mesh.deform == nullptr) {
        mesh.deform.reset(new MeshDeform());
    }
    PT_TRY(ensure_counted(keep, mesh.deform->current, 3 * static_cast<size_t>(mesh.n_vertices)));
    PT_TRY(ensure_counted(keep, mesh.deform->spare, 3 * static_cast<size_t>(mesh.n_vertices)));
    return PT_OK;
}

namespace {

template<typename T>
void exchange(DevBuf<T> &a, DevBuf<T> &b) {
    std::swap(a.ptr, b.ptr);
    std::swap(a.count, b.count);
}

} // namespace

int adopt_shapes(pt_scene *s, const std::vector<const float *> &shape, const std::vector<uint8_t> &in_spare, std::vector<pt_mesh_instance> &&posed,
                 std::chrono::steady_clock::time_point t_begin, pt_pose_info *info) {
    PoseKeep &keep = *s->pose;
    const size_t n_meshes = keep.meshes.size();
    std::vector<const float *> before(n_meshes, nullptr);
    for(size_t m = 0; m < n_meshes; m++) {
        if(shape[m] != nullptr) {
            before[m] = keep.meshes[m]->shape;
            keep.meshes[m]->shape = shape[m];
        }
    }
    const int rc = rebuild_instances(s, std::move(posed), t_begin, info);
    if(rc != PT_OK) {
        for(size_t m = 0; m < n_meshes; m++) {
            if(shape[m] != nullptr) {
                keep.meshes[m]->shape = before[m];
            }
        }
        return rc;
    }
    for(size_t m = 0; m < n_meshes; m++) {
        if(shape[m] != nullptr) {
            keep.meshes[m]->shape_serial++; // (what pt_scene_motion_mark compares: pt_motion_shapes.cpp)
        }
        if(in_spare[m] != 0) {
            exchange(keep.meshes[m]->deform->current, keep.meshes[m]->deform->spare); // (shape names the buffer that is `current` now)
        }
    }
    return PT_OK;
}

} // namespace pth

extern "C" {

int pt_scene_bind_skin(pt_scene *s, const pt_skin *skin) {
    if(skin == nullptr) {
        return fail(PT_ERR_INVALID, "null skin");
    }
    const bool unbind = skin->n_bones == 0 || skin->bone == nullptr;
    if(!unbind && (skin->influences < 1 || skin->influences > PT_SKIN_MAX_INFLUENCES)) {
        return fail(PT_ERR_INVALID, "influences per vertex must be 1 .. " + std::to_string(PT_SKIN_MAX_INFLUENCES) + ", not " + std::to_string(skin->influences));
    }
    if(!unbind && skin->weight == nullptr) {
        return fail(PT_ERR_INVALID, "null weights");
    }
    if(s == nullptr) {
        return fail(PT_ERR_INVALID, "null scene");
    }
    std::lock_guard<std::mutex> lock(s->render_mutex);
    if(s->pose == nullptr) {
        return fail(PT_ERR_UNSUPPORTED, DEFORM_NO_INSTANCES);
    }
    PoseKeep &keep = *s->pose;
    KeptMesh *mesh = nullptr;
    PT_TRY(used_mesh(keep, skin->mesh, &mesh));
    const size_t n = unbind ? 0 : static_cast<size_t>(mesh->n_vertices) * skin->influences;
    for(size_t j = 0; j < n; j++) {
        if(skin->bone[j] >= skin->n_bones) {
            return fail(PT_ERR_INVALID, "bone index " + std::to_string(skin->bone[j]) + " of vertex " + std::to_string(j / skin->influences) + " out of range: the rig has " +
                                            std::to_string(skin->n_bones) + " bones");
        }
    }
    if(s->live_frames.load() != 0) {
        return fail(PT_ERR_INVALID, DEFORM_LIVE_FRAME);
    }
    if(mesh->deform == nullptr) {
        if(unbind) {
            return PT_OK;
        }
        mesh->deform.reset(new MeshDeform());
    }
    MeshDeform &md = *mesh->deform;
    md.skin_bones = md.skin_k = 0; // (no skin until the new one is complete)
    if(unbind) {
        md.skin_bone.release();
        md.skin_weight.release();
        return PT_OK;
    }
    PT_HIP(hipSetDevice(s->device));
    PT_TRY(ensure_counted(keep, md.skin_bone, n));
    PT_TRY(ensure_counted(keep, md.skin_weight, n));
    if(n > 0) {
        PT_HIP(hipMemcpy(md.skin_bone.ptr, skin->bone, n * sizeof(uint32_t), hipMemcpyHostToDevice));
        PT_HIP(hipMemcpy(md.skin_weight.ptr, skin->weight, n * sizeof(float), hipMemcpyHostToDevice));
    }
    md.skin_bones = skin->n_bones;
    md.skin_k = skin->influences;
    return PT_OK;
}

int pt_scene_deform(pt_scene *s, const pt_mesh_deform *deforms, uint32_t n_deforms, const uint32_t *instances, uint32_t n, const float *transforms, pt_deform_info *info) {
    if(info != nullptr) {
        *info = pt_deform_info{};
    }
    if(n_deforms > 0 && deforms == nullptr) {
        return fail(PT_ERR_INVALID, "null deforms");
    }
    for(uint32_t e = 0; e < n_deforms; e++) {
        if(deforms[e].kind != PT_DEFORM_VERTICES && deforms[e].kind != PT_DEFORM_BONES && deforms[e].kind != PT_DEFORM_REST) {
            return fail(PT_ERR_INVALID, "unknown kind " + std::to_string(deforms[e].kind) + " in deform " + std::to_string(e));
        }
        if(deforms[e].kind != PT_DEFORM_REST && deforms[e].data == nullptr) {
            return fail(PT_ERR_INVALID, "null data in deform " + std::to_string(e));
        }
    }
    if(n > 0 && transforms == nullptr) {
        return fail(PT_ERR_INVALID, "null transforms");
    }
    if(s == nullptr) {
        return fail(PT_ERR_INVALID, "null scene");
    }
    std::lock_guard<std::mutex> lock(s->render_mutex);
    if(s->pose == nullptr) {
        return fail(PT_ERR_UNSUPPORTED, DEFORM_NO_INSTANCES);
    }
    PoseKeep &keep = *s->pose;
    PT_TRY(check_pose_arguments(keep, instances, n));
    std::vector<int64_t> entry(keep.meshes.size(), -1); // the last deform that names each mesh
    for(uint32_t e = 0; e < n_deforms; e++) {
        const pt_mesh_deform &de = deforms[e];
        KeptMesh *mesh = nullptr;
        PT_TRY(used_mesh(keep, de.mesh, &mesh));
        if(de.kind == PT_DEFORM_VERTICES && de.count != mesh->n_vertices) {
            return fail(PT_ERR_INVALID, "deform " + std::to_string(e) + " has " + std::to_string(de.count) + " vertices, mesh " + std::to_string(de.mesh) + " has " +
                                            std::to_string(mesh->n_vertices));
        }
        if(de.kind == PT_DEFORM_BONES) {
            if(mesh->deform == nullptr || mesh->deform->skin_bones == 0) {
                return fail(PT_ERR_INVALID, "mesh " + std::to_string(de.mesh) + " has no skin (pt_scene_bind_skin first)");
            }
            if(de.count != mesh->deform->skin_bones) {
                return fail(PT_ERR_INVALID, "deform " + std::to_string(e) + " has " + std::to_string(de.count) + " bones, the skin of mesh " + std::to_string(de.mesh) + " has " +
                                                std::to_string(mesh->deform->skin_bones));
            }
        }
        entry[de.mesh] = e;
    }
    if(s->live_frames.load() != 0) {
        return fail(PT_ERR_INVALID, DEFORM_LIVE_FRAME);
    }

    using clock = std::chrono::steady_clock;
    const auto t_begin = clock::now();
    std::vector<pt_mesh_instance> posed = posed_instances(keep, instances, n, transforms);
    PT_HIP(hipSetDevice(s->device));
    PT_HIP(hipStreamSynchronize(s->stream));

    // ---- 1. the new vertices, each mesh's in its spare buffer; the shapes the assembly is to read ---------------------------------------
    const size_t n_meshes = keep.meshes.size();
    std::vector<const float *> shape(n_meshes, nullptr);
    std::vector<uint8_t> in_spare(n_meshes, 0);
    uint32_t n_deformed = 0, n_skinned_meshes = 0;
    uint64_t n_skinned = 0, total_bones = 0;
    for(size_t m = 0; m < n_meshes; m++) {
        if(entry[m] < 0) {
            continue;
        }
        KeptMesh &mesh = *keep.meshes[m];
        const pt_mesh_deform &de = deforms[entry[m]];
        n_deformed++;
        if(de.kind == PT_DEFORM_REST) {
            shape[m] = mesh.vertices.ptr;
            continue;
        }
        // (both buffers with the first deformation, so that no later one allocates: they change places after every call)
        PT_TRY(ensure_vertex_buffers(keep, mesh));
        shape[m] = mesh.deform->spare.ptr;
        in_spare[m] = 1;
        if(de.kind == PT_DEFORM_BONES) {
            total_bones += de.count;
            n_skinned_meshes++;
        }
    }
    if(total_bones > 0) {
        PT_TRY(ensure_counted(keep, keep.bone_table, 12 * static_cast<size_t>(total_bones)));
    }
    // (from here on the stream may hold work of this call: whatever happens, it is waited for before the call returns)
    StreamDrain drain{s->stream};
    const auto t_upload = clock::now();
    size_t bone_at = 0;
    std::vector<size_t> table_at(n_meshes, 0);
    for(size_t m = 0; m < n_meshes; m++) {
        if(entry[m] < 0) {
            continue;
        }
        const KeptMesh &mesh = *keep.meshes[m];
        const pt_mesh_deform &de = deforms[entry[m]];
        if(de.kind == PT_DEFORM_VERTICES && mesh.n_vertices > 0) {
            PT_HIP(hipMemcpyAsync(mesh.deform->spare.ptr, de.data, 3 * static_cast<size_t>(mesh.n_vertices) * sizeof(float), hipMemcpyHostToDevice, s->stream));
        }
        if(de.kind == PT_DEFORM_BONES) {
            table_at[m] = bone_at;
            PT_HIP(hipMemcpyAsync(keep.bone_table.ptr + bone_at, de.data, 12 * static_cast<size_t>(de.count) * sizeof(float), hipMemcpyHostToDevice, s->stream));
            bone_at += 12 * static_cast<size_t>(de.count);
        }
    }
    const float vertex_upload_ms = std::chrono::duration<float, std::milli>(clock::now() - t_upload).count();
    EventPair skin;
    if(n_skinned_meshes > 0) {
        // (the table is staged in LDS up to PT_SKIN_LDS_BONES bones; PT_SKIN_LDS_BONES in the environment lowers that, 0 = never)
        const uint32_t lds_bones = static_cast<uint32_t>(std::max(env_int("PT_SKIN_LDS_BONES", static_cast<int>(PT_SKIN_LDS_BONES)), 0));
        PT_HIP(skin.begin(s->stream));
        for(size_t m = 0; m < n_meshes; m++) {
            if(entry[m] < 0 || deforms[entry[m]].kind != PT_DEFORM_BONES) {
                continue;
            }
            const KeptMesh &mesh = *keep.meshes[m];
            const MeshDeform &md = *mesh.deform;
            const hipError_t e = pt_skin_launch(s->stream, mesh.n_vertices, mesh.vertices.ptr, md.skin_k, md.skin_bone.ptr, md.skin_weight.ptr, keep.bone_table.ptr + table_at[m],
                                                md.skin_bones, lds_bones, md.spare.ptr);
            if(e != hipSuccess) {
                return fail(PT_ERR_HIP, std::string("skinning kernel: ") + hipGetErrorString(e));
            }
            n_skinned += mesh.n_vertices;
        }
        PT_HIP(skin.end(s->stream));
    }

    // ---- 2. and 3. the pose: the assembly reads the new shapes behind the launches above; a failure turns the pointers back -------------
    pt_pose_info posed_info{};
    PT_TRY(adopt_shapes(s, shape, in_spare, std::move(posed), t_begin, &posed_info));
    drain.armed = false; // (rebuild_instances has waited)
    float skin_ms = 0.0F;
    if(n_skinned_meshes > 0) {
        PT_HIP(skin.ms(&skin_ms));
    }
    const float total_ms = std::chrono::duration<float, std::milli>(clock::now() - t_begin).count();
    if(info != nullptr) {
        info->n_instances = posed_info.n_instances;
        info->n_triangles = posed_info.n_triangles;
        info->assembly_syncs = posed_info.assembly_syncs;
        info->assembly_chunks = posed_info.assembly_chunks;
        info->upload_ms = posed_info.upload_ms;
        info->assembly_ms = posed_info.assembly_ms;
        info->tree_ms = posed_info.tree_ms;
        info->rest_ms = std::max(total_ms - posed_info.upload_ms - posed_info.assembly_ms - posed_info.tree_ms, 0.0F);
        info->total_ms = total_ms;
        info->n_meshes_deformed = n_deformed;
        info->n_vertices_skinned = static_cast<uint32_t>(std::min<uint64_t>(n_skinned, 0xffffffffULL));
        info->skin_ms = skin_ms;
        info->vertex_upload_ms = vertex_upload_ms;
        info->allocations = static_cast<uint32_t>(keep.scratch.allocations + keep.deform_allocations);
    }
    if(env_int("PT_DEBUG", 0) != 0) {
        std::fprintf(stderr, "[pt] deform: %u mesh(es), %llu vertices skinned in %.3f ms, vertex upload %.1f ms; %u triangles kept, assembly %.1f ms, tree %.1f ms, total %.1f ms\n",
                     n_deformed, static_cast<unsigned long long>(n_skinned), skin_ms, vertex_upload_ms, posed_info.n_triangles, posed_info.assembly_ms, posed_info.tree_ms, total_ms);
    }
    return PT_OK;
}

int pt_scene_get_mesh_vertices(pt_scene *s, uint32_t mesh_index, float *out, uint32_t *n_vertices) {
    if(s == nullptr) {
        return fail(PT_ERR_INVALID, "null scene");
    }
    std::lock_guard<std::mutex> lock(s->render_mutex);
    if(s->pose == nullptr) {
        return fail(PT_ERR_UNSUPPORTED, DEFORM_NO_INSTANCES);
    }
    KeptMesh *mesh = nullptr;
    PT_TRY(used_mesh(*s->pose, mesh_index, &mesh));
    if(n_vertices != nullptr) {
        *n_vertices = mesh->n_vertices;
    }
    if(out != nullptr && mesh->n_vertices > 0) {
        PT_HIP(hipSetDevice(s->device));
        PT_HIP(hipMemcpy(out, mesh->shape, 3 * static_cast<size_t>(mesh->n_vertices) * sizeof(float), hipMemcpyDeviceToHost));
    }
    return PT_OK;
}

} // extern "C"
