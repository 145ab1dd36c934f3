// pt_pose.cpp -- pt_scene_get_pose and pt_scene_pose of include/pt_pose.h: a scene's mesh instances under new matrices, in place
// (DESIGN.md 4.3.2).  The two halves of pt_scene_create_meshes do the work (pt_meshes.cpp): assemble_mesh_scene puts all instances through
// the batched assembler (pt_mesh_batch.h) into arrays of their own, finish_mesh_scene builds a scene from them aside on the unchanged
// create_scene path, and only a finished scene's content is moved into the live handle, which keeps its address, stream, lock, pinned
// words and workspace buffers.  rebuild_instances is that work; pt_scene_deform (pt_deform.cpp) ends with it as well.
#include "pt_host.h"

using namespace pth;

namespace pth {

int rebuild_instances(pt_scene *s, std::vector<pt_mesh_instance> &&posed, std::chrono::steady_clock::time_point t_begin, pt_pose_info *info) {
    using clock = std::chrono::steady_clock;
    auto ms_since = [](clock::time_point t0) { return std::chrono::duration<float, std::milli>(clock::now() - t0).count(); };
    PoseKeep &keep = *s->pose;
    const uint32_t n_instances = static_cast<uint32_t>(keep.instances.size());
    const pt_scene_desc *d = &keep.desc.d;

    // ---- the arrays the instances are expanded into, behind the description's own triangles (the meshes are there) ---------------------
    const bool with_normals = keep.any_smooth || (d->n_triangles > 0 && d->tri_nrm != nullptr);
    DevBuf<float> pos;
    take(pos, keep.spare_pos);
    // whatever happens, the arrays go back to the scene: the positions as its spare unless a new scene takes them over
    struct Return {
        DevBuf<float> &pos, &spare;
        ~Return() {
            if(pos.ptr != nullptr) {
                take(spare, pos);
            }
        }
    } give_back{pos, keep.spare_pos};
    DevBuf<float> &nrm = keep.spare_nrm;
    PT_HIP(pos.ensure(9 * static_cast<size_t>(keep.capacity)));
    if(with_normals) {
        PT_HIP(nrm.ensure(9 * static_cast<size_t>(keep.capacity)));
    }
    // (a marked scene also tracks the face of every triangle, made aside like the positions: pt_motion_shapes.cpp)
    uint32_t *face_of = keep.mark != nullptr ? keep.mark->face_of_spare.ptr : nullptr;
    MeshAssembly assembly;
    const int assembled = assemble_mesh_scene(s->stream, d, keep.meshes, posed, keep.scratch, keep.capacity, pos.ptr, with_normals ? nrm.ptr : nullptr, &assembly, face_of);
    if(assembled != PT_OK) {
        (void)hipStreamSynchronize(s->stream); // (nothing of the failed call is in flight when its buffers are used again)
        return assembled;
    }
    const float upload_ms = std::chrono::duration<float, std::milli>(assembly.front_done - t_begin).count();

    // ---- the scene of these arrays, built aside by the path every scene takes -------------------------------------------------------------
    pt_scene *built = nullptr;
    const int rc = finish_mesh_scene(s->device, d, assembly, pos, &built);
    if(rc != PT_OK) {
        (void)hipStreamSynchronize(s->stream); // (nothing of the failed pose is in flight when the arrays are used again)
        return rc;
    }
    std::unique_ptr<pt_scene> t(built);
    PT_HIP(hipStreamSynchronize(s->stream));
    float assembly_ms = 0.0F;
    PT_HIP(assembly.chain.ms(&assembly_ms));

    // ---- adoption: the content moves, the handle stays ---------------------------------------------------------------------------------------
    s->tree = std::move(t->tree);
    s->n_nodes = t->n_nodes;
    s->depth = t->depth;
    s->device_built = t->device_built;
    std::copy(t->build_ms, t->build_ms + 4, s->build_ms);
    s->tri_obj = std::move(t->tri_obj);
    s->sph_obj = std::move(t->sph_obj);
    s->n_objects = t->n_objects;
    s->n_desc_objects = t->n_desc_objects;
    s->n_desc_tris = t->n_desc_tris;
    s->inst_first = std::move(t->inst_first);
    s->inst_count = std::move(t->inst_count);
    s->desc_ref = std::move(t->desc_ref);
    take(keep.spare_pos, s->tri_pos_kept); // (the positions of the pose before: the next pose assembles into them)
    take(s->tri_pos_kept, t->tri_pos_kept);
    take(s->leaf_order, t->leaf_order); // (empty behind the host builder: the next relight uploads the new tree's order)
    s->n_emissive = t->n_emissive;
    s->emissive_obj = std::move(t->emissive_obj);
    s->emissive_cdf = std::move(t->emissive_cdf);
    take(s->recs, t->recs);
    take(s->pairs, t->pairs);
    take(s->tris, t->tris);
    take(s->tri_shade, t->tri_shade);
    take(s->spheres, t->spheres);
    take(s->materials, t->materials);
    take(s->lights, t->lights);
    take(s->emis, t->emis);
    take(s->sph_meta, t->sph_meta);
    take(s->emis_cdf, t->emis_cdf);
    s->dev = t->dev; // (its pointers name the buffers that have just moved)
    keep.instances = std::move(posed);
    if(keep.mark != nullptr) {
        std::swap(keep.mark->face_of.ptr, keep.mark->face_of_spare.ptr);
        std::swap(keep.mark->face_of.count, keep.mark->face_of_spare.count);
        keep.mark->has_table = true;
    }
    // What the render workspace was sized from has changed: the configuration derived from the tree (in_lds, wide, stack_lds, lds_bytes,
    // spill_depth) is derived again, and every entry point sizes its buffers from it per call ("the hazard")
    s->path_cfg = PtPathConfig{};
    s->path_blocks_per_cu = 0;
    s->path_slots = s->path_waves = s->path_cap = 0;
    s->host_path_args = PtPathArgs{};
    PT_TRY(setup_path(s));
    const float tree_ms = s->device_built ? s->build_ms[2] : s->build_ms[0];
    t.reset();

    const float total_ms = ms_since(t_begin);
    const uint32_t n_kept = assembly.triangles.n_triangles - d->n_triangles;
    if(info != nullptr) {
        info->n_instances = n_instances;
        info->n_triangles = n_kept;
        info->assembly_syncs = assembly.chunks; // (one wait per chunk)
        info->assembly_chunks = assembly.chunks;
        info->upload_ms = upload_ms;
        info->assembly_ms = assembly_ms;
        info->tree_ms = tree_ms;
        info->rest_ms = std::max(total_ms - upload_ms - assembly_ms - tree_ms, 0.0F);
        info->total_ms = total_ms;
    }
    return PT_OK;
}

} // namespace pth

extern "C" {

int pt_scene_get_pose(const pt_scene *scene, float *transforms) {
    if(scene == nullptr || transforms == nullptr) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    if(scene->pose == nullptr) {
        return fail(PT_ERR_UNSUPPORTED, "the scene has no instances: it was not made by pt_scene_create_meshes with instances");
    }
    std::lock_guard<std::mutex> lock(const_cast<pt_scene *>(scene)->render_mutex);
    const std::vector<pt_mesh_instance> &instances = scene->pose->instances;
    for(size_t i = 0; i < instances.size(); i++) {
        std::copy(instances[i].transform, instances[i].transform + 16, transforms + 16 * i);
    }
    return PT_OK;
}

int pt_scene_pose(pt_scene *s, const uint32_t *instances, uint32_t n, const float *transforms, pt_pose_info *info) {
    if(info != nullptr) {
        *info = pt_pose_info{};
    }
    if(s == nullptr) {
        return fail(PT_ERR_INVALID, "null scene");
    }
    if(n > 0 && transforms == nullptr) {
        return fail(PT_ERR_INVALID, "null transforms");
    }
    std::lock_guard<std::mutex> lock(s->render_mutex);
    if(s->pose == nullptr) {
        return fail(PT_ERR_UNSUPPORTED, "the scene has no instances: it was not made by pt_scene_create_meshes with instances");
    }
    PoseKeep &keep = *s->pose;
    const uint32_t n_instances = static_cast<uint32_t>(keep.instances.size());
    if(instances == nullptr && n != n_instances) {
        return fail(PT_ERR_INVALID, "a pose of all instances needs " + std::to_string(n_instances) + " matrices, not " + std::to_string(n));
    }
    for(uint32_t k = 0; instances != nullptr && k < n; k++) {
        if(instances[k] >= n_instances) {
            return fail(PT_ERR_INVALID, "instance index " + std::to_string(instances[k]) + " out of range: the scene has " + std::to_string(n_instances));
        }
    }
    if(s->live_frames.load() != 0) {
        return fail(PT_ERR_INVALID, "the scene has a live frame: its parked state belongs to the present geometry (pt_frame_destroy first)");
    }

    const auto t_begin = std::chrono::steady_clock::now();
    std::vector<pt_mesh_instance> posed = keep.instances; // (adopted with the rest, on success)
    for(uint32_t k = 0; k < n; k++) {
        const uint32_t i = instances != nullptr ? instances[k] : k;
        std::copy(transforms + 16 * static_cast<size_t>(k), transforms + 16 * static_cast<size_t>(k) + 16, posed[i].transform);
    }
    PT_HIP(hipSetDevice(s->device));
    PT_HIP(hipStreamSynchronize(s->stream));
    pt_pose_info done{};
    PT_TRY(rebuild_instances(s, std::move(posed), t_begin, &done));
    if(info != nullptr) {
        *info = done;
    }
    if(env_int("PT_DEBUG", 0) != 0) {
        std::fprintf(stderr, "[pt] pose: %u instances, %llu triangles kept, %u chunk(s); upload %.1f ms, assembly %.1f ms, tree %.1f ms, total %.1f ms; scratch allocations so far %llu\n",
                     done.n_instances, static_cast<unsigned long long>(done.n_triangles), done.assembly_chunks, done.upload_ms, done.assembly_ms, done.tree_ms, done.total_ms,
                     static_cast<unsigned long long>(keep.scratch.allocations));
    }
    return PT_OK;
}

} // extern "C"
