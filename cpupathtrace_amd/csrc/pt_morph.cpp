// pt_morph.cpp -- the entry points of include/pt_morph.h: blend shapes for a scene's meshes, in place.  Binding turns a
// set's target-major lists into vertex-major rows on the host -- a stable counting sort by vertex -- and uploads them once.  A morph
// makes a mesh's current vertices in its spare buffer with pt_morph_launch (pt_deform.hip) on the scene's stream, alone or through the
// bound rig in the same launch, and the rest is what pt_scene_deform does behind its own kernels: adopt_shapes (pt_deform.cpp).
#include "pt_host.h"
#include "pt_morph_rows.h"

using namespace pth;

namespace {

const uint64_t MAX_ENTRIES = 0x7fffffffULL;

} // namespace

extern "C" {

int pt_scene_bind_morphs(pt_scene *s, const pt_morph_set *set) {
    if(set == nullptr) {
        return fail(PT_ERR_INVALID, "null morph set");
    }
    const bool unbind = set->n_targets == 0 || set->targets == nullptr;
    for(uint32_t t = 0; !unbind && t < set->n_targets; t++) {
        const pt_morph_target &target = set->targets[t];
        if(target.n_deltas > 0 && target.delta == nullptr) {
            return fail(PT_ERR_INVALID, "null deltas in target " + std::to_string(t));
        }
        for(uint32_t j = 1; target.vertex != nullptr && j < target.n_deltas; j++) {
            if(target.vertex[j] <= target.vertex[j - 1]) {
                return fail(PT_ERR_INVALID, "vertex indices of target " + std::to_string(t) + " are not strictly ascending at entry " + std::to_string(j));
            }
        }
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
    PT_TRY(used_mesh(keep, set->mesh, &mesh));
    const uint32_t n_vertices = mesh->n_vertices;
    uint64_t n_entries = 0;
    for(uint32_t t = 0; !unbind && t < set->n_targets; t++) {
        const pt_morph_target &target = set->targets[t];
        if(target.vertex == nullptr && target.n_deltas != 0 && target.n_deltas != n_vertices) {
            return fail(PT_ERR_INVALID, "dense target " + std::to_string(t) + " has " + std::to_string(target.n_deltas) + " deltas, mesh " + std::to_string(set->mesh) + " has " +
                                            std::to_string(n_vertices) + " vertices");
        }
        // (ascending: the last index is the largest)
        if(target.vertex != nullptr && target.n_deltas > 0 && target.vertex[target.n_deltas - 1] >= n_vertices) {
            return fail(PT_ERR_INVALID, "vertex index " + std::to_string(target.vertex[target.n_deltas - 1]) + " of target " + std::to_string(t) + " out of range: mesh " +
                                            std::to_string(set->mesh) + " has " + std::to_string(n_vertices) + " vertices");
        }
        n_entries += target.n_deltas;
    }
    if(n_entries > MAX_ENTRIES) {
        return fail(PT_ERR_UNSUPPORTED, "a morph set of " + std::to_string(n_entries) + " entries: at most " + std::to_string(MAX_ENTRIES));
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
    md.morph_targets = 0; // (no set until the new one is complete)
    md.morph_entry_count = 0;
    if(unbind) {
        md.morph_row_start.release();
        md.morph_entries.release();
        return PT_OK;
    }

    std::vector<uint32_t> row_start;
    std::vector<PtMorphEntry> entries;
    pt_morph_rows(n_vertices, set->targets, set->n_targets, row_start, entries); // vertex-major, a row's entries in target order
    PT_HIP(hipSetDevice(s->device));
    PT_TRY(ensure_counted(keep, md.morph_row_start, row_start.size()));
    PT_TRY(ensure_counted(keep, md.morph_entries, entries.size()));
    PT_HIP(hipMemcpy(md.morph_row_start.ptr, row_start.data(), row_start.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    if(!entries.empty()) {
        PT_HIP(hipMemcpy(md.morph_entries.ptr, entries.data(), entries.size() * sizeof(PtMorphEntry), hipMemcpyHostToDevice));
    }
    md.morph_targets = set->n_targets;
    md.morph_entry_count = n_entries;
    return PT_OK;
}

int pt_scene_morph(pt_scene *s, const pt_mesh_morph *morphs, uint32_t n_morphs, const uint32_t *instances, uint32_t n, const float *transforms, pt_morph_info *info) {
    if(info != nullptr) {
        *info = pt_morph_info{};
    }
    if(n_morphs > 0 && morphs == nullptr) {
        return fail(PT_ERR_INVALID, "null morphs");
    }
    for(uint32_t e = 0; e < n_morphs; e++) {
        if(morphs[e].weights == nullptr) {
            return fail(PT_ERR_INVALID, "null weights in morph " + std::to_string(e));
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
    std::vector<int64_t> entry(keep.meshes.size(), -1); // the last morph that names each mesh
    for(uint32_t e = 0; e < n_morphs; e++) {
        const pt_mesh_morph &mo = morphs[e];
        KeptMesh *mesh = nullptr;
        PT_TRY(used_mesh(keep, mo.mesh, &mesh));
        if(mesh->deform == nullptr || mesh->deform->morph_targets == 0) {
            return fail(PT_ERR_INVALID, "mesh " + std::to_string(mo.mesh) + " has no morph set (pt_scene_bind_morphs first)");
        }
        if(mo.n_weights != mesh->deform->morph_targets) {
            return fail(PT_ERR_INVALID, "morph " + std::to_string(e) + " has " + std::to_string(mo.n_weights) + " weights, the set of mesh " + std::to_string(mo.mesh) + " has " +
                                            std::to_string(mesh->deform->morph_targets) + " targets");
        }
        if(mo.bones != nullptr) {
            if(mesh->deform->skin_bones == 0) {
                return fail(PT_ERR_INVALID, "mesh " + std::to_string(mo.mesh) + " has no skin (pt_scene_bind_skin first)");
            }
            if(mo.n_bones != mesh->deform->skin_bones) {
                return fail(PT_ERR_INVALID, "morph " + std::to_string(e) + " has " + std::to_string(mo.n_bones) + " bones, the skin of mesh " + std::to_string(mo.mesh) + " has " +
                                                std::to_string(mesh->deform->skin_bones));
            }
        }
        entry[mo.mesh] = e;
    }
    if(s->live_frames.load() != 0) {
        return fail(PT_ERR_INVALID, DEFORM_LIVE_FRAME);
    }

    using clock = std::chrono::steady_clock;
    const auto t_begin = clock::now();
    std::vector<pt_mesh_instance> posed = posed_instances(keep, instances, n, transforms);
    PT_HIP(hipSetDevice(s->device));
    PT_HIP(hipStreamSynchronize(s->stream));

    // ---- 1. the new vertices, each mesh's in its spare buffer -------------------------------------------------------------------------------
    const size_t n_meshes = keep.meshes.size();
    std::vector<const float *> shape(n_meshes, nullptr);
    std::vector<uint8_t> in_spare(n_meshes, 0);
    uint32_t n_morphed_meshes = 0;
    uint64_t n_morphed = 0, n_skinned = 0, n_entries = 0, total_weights = 0, total_bones = 0;
    for(size_t m = 0; m < n_meshes; m++) {
        if(entry[m] < 0) {
            continue;
        }
        KeptMesh &mesh = *keep.meshes[m];
        const pt_mesh_morph &mo = morphs[entry[m]];
        PT_TRY(ensure_vertex_buffers(keep, mesh));
        shape[m] = mesh.deform->spare.ptr;
        in_spare[m] = 1;
        n_morphed_meshes++;
        total_weights += mo.n_weights;
        total_bones += mo.bones != nullptr ? mo.n_bones : 0;
    }
    if(total_weights > 0) {
        PT_TRY(ensure_counted(keep, keep.morph_weights, static_cast<size_t>(total_weights)));
    }
    if(total_bones > 0) {
        PT_TRY(ensure_counted(keep, keep.bone_table, 12 * static_cast<size_t>(total_bones)));
    }
    // (from here on the stream may hold work of this call: whatever happens, it is waited for before the call returns)
    StreamDrain drain{s->stream};
    const auto t_upload = clock::now();
    size_t weight_at = 0, bone_at = 0;
    std::vector<size_t> weights_at(n_meshes, 0), table_at(n_meshes, 0);
    for(size_t m = 0; m < n_meshes; m++) {
        if(entry[m] < 0) {
            continue;
        }
        const pt_mesh_morph &mo = morphs[entry[m]];
        weights_at[m] = weight_at;
        PT_HIP(hipMemcpyAsync(keep.morph_weights.ptr + weight_at, mo.weights, static_cast<size_t>(mo.n_weights) * sizeof(float), hipMemcpyHostToDevice, s->stream));
        weight_at += mo.n_weights;
        if(mo.bones != nullptr) {
            table_at[m] = bone_at;
            PT_HIP(hipMemcpyAsync(keep.bone_table.ptr + bone_at, mo.bones, 12 * static_cast<size_t>(mo.n_bones) * sizeof(float), hipMemcpyHostToDevice, s->stream));
            bone_at += 12 * static_cast<size_t>(mo.n_bones);
        }
    }
    const float vertex_upload_ms = std::chrono::duration<float, std::milli>(clock::now() - t_upload).count();
    EventPair morph;
    if(n_morphed_meshes > 0) {
        // (weights and bone table are staged in LDS up to PT_MORPH_LDS_TARGETS targets and PT_SKIN_LDS_BONES bones; the variables of
        // these names in the environment lower that, 0 = never)
        const uint32_t lds_targets = static_cast<uint32_t>(std::max(env_int("PT_MORPH_LDS_TARGETS", static_cast<int>(PT_MORPH_LDS_TARGETS)), 0));
        const uint32_t lds_bones = static_cast<uint32_t>(std::max(env_int("PT_SKIN_LDS_BONES", static_cast<int>(PT_SKIN_LDS_BONES)), 0));
        PT_HIP(morph.begin(s->stream));
        for(size_t m = 0; m < n_meshes; m++) {
            if(entry[m] < 0) {
                continue;
            }
            const KeptMesh &mesh = *keep.meshes[m];
            const MeshDeform &md = *mesh.deform;
            const pt_mesh_morph &mo = morphs[entry[m]];
            const bool skinned = mo.bones != nullptr;
            const hipError_t e = pt_morph_launch(s->stream, mesh.n_vertices, mesh.vertices.ptr, md.morph_row_start.ptr, md.morph_entries.ptr,
                                                 keep.morph_weights.ptr + weights_at[m], md.morph_targets, lds_targets, skinned ? md.skin_k : 0, md.skin_bone.ptr,
                                                 md.skin_weight.ptr, skinned ? keep.bone_table.ptr + table_at[m] : nullptr, skinned ? md.skin_bones : 0, lds_bones,
                                                 md.spare.ptr);
            if(e != hipSuccess) {
                return fail(PT_ERR_HIP, std::string("morph kernel: ") + hipGetErrorString(e));
            }
            n_morphed += mesh.n_vertices;
            n_skinned += skinned ? mesh.n_vertices : 0;
            n_entries += md.morph_entry_count;
        }
        PT_HIP(morph.end(s->stream));
    }

    // ---- 2. and 3. the pose: the assembly reads the new shapes behind the launches above ------------------------------------------------------
    pt_pose_info posed_info{};
    PT_TRY(adopt_shapes(s, shape, in_spare, std::move(posed), t_begin, &posed_info));
    drain.armed = false; // (rebuild_instances has waited)
    float morph_ms = 0.0F;
    if(n_morphed_meshes > 0) {
        PT_HIP(morph.ms(&morph_ms));
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
        info->n_meshes_deformed = n_morphed_meshes;
        info->n_vertices_skinned = static_cast<uint32_t>(std::min<uint64_t>(n_skinned, 0xffffffffULL));
        info->skin_ms = 0.0F;
        info->vertex_upload_ms = vertex_upload_ms;
        info->allocations = static_cast<uint32_t>(keep.scratch.allocations + keep.deform_allocations);
        info->n_vertices_morphed = static_cast<uint32_t>(std::min<uint64_t>(n_morphed, 0xffffffffULL));
        info->morph_ms = morph_ms;
        info->n_entries_read = n_entries;
    }
    if(env_int("PT_DEBUG", 0) != 0) {
        std::fprintf(stderr, "[pt] morph: %u mesh(es), %llu vertices (%llu through bones), %llu entries in %.3f ms; %u triangles kept, assembly %.1f ms, tree %.1f ms, total %.1f ms\n",
                     n_morphed_meshes, static_cast<unsigned long long>(n_morphed), static_cast<unsigned long long>(n_skinned), static_cast<unsigned long long>(n_entries), morph_ms,
                     posed_info.n_triangles, posed_info.assembly_ms, posed_info.tree_ms, total_ms);
    }
    return PT_OK;
}

int pt_scene_get_morphs(pt_scene *s, uint32_t mesh_index, uint32_t *n_targets, uint64_t *n_entries) {
    if(s == nullptr) {
        return fail(PT_ERR_INVALID, "null scene");
    }
    std::lock_guard<std::mutex> lock(s->render_mutex);
    if(s->pose == nullptr) {
        return fail(PT_ERR_UNSUPPORTED, DEFORM_NO_INSTANCES);
    }
    KeptMesh *mesh = nullptr;
    PT_TRY(used_mesh(*s->pose, mesh_index, &mesh));
    const bool bound = mesh->deform != nullptr && mesh->deform->morph_targets != 0;
    if(n_targets != nullptr) {
        *n_targets = bound ? mesh->deform->morph_targets : 0;
    }
    if(n_entries != nullptr) {
        *n_entries = bound ? mesh->deform->morph_entry_count : 0;
    }
    return PT_OK;
}

} // extern "C"
