// pt_pose.cpp -- the entry points of include/pt_pose.h: a scene's mesh instances under new matrices, in place.  All
// instances go through the batched assembler (pt_mesh_batch.h) into arrays of their own, the unchanged create_scene path builds a scene
// from them aside (finish_mesh_scene, pt_meshes.cpp: the tail of pt_scene_create_meshes), and only a finished scene's content is moved
// into the live handle, which keeps its address, stream, lock, pinned words and workspace buffers.
#include "pt_host.h"

using namespace pth;

namespace {

struct StreamGuard {
    hipStream_t stream = nullptr;
    ~StreamGuard() {
        if(stream != nullptr) {
            (void)hipStreamDestroy(stream);
        }
    }
};

template<typename T>
void take(DevBuf<T> &to, DevBuf<T> &from) {
    to.release();
    to.ptr = from.ptr;
    to.count = from.count;
    from.ptr = nullptr;
    from.count = 0;
}

struct BatchResult {
    uint32_t chunks = 0, syncs = 0;
    uint64_t kept = 0;
};

// All instances through the batched assembler, chunk after chunk, each behind the survivors of the one before: positions and normals at
// pos / nrm (room for `room` triangles), the per-instance counts to counts[instances.size()].  The last chunk's sort and smoothing are
// only enqueued when this returns.
int assemble_batch(hipStream_t stream, PtBatchScratch &scratch, const std::vector<const KeptMesh *> &mesh_of, const pt_mesh_instance *instances, uint32_t n_instances,
                   std::vector<PtBatchInstance> &table, uint64_t room, float *pos, float *nrm, uint32_t *counts, BatchResult *result) {
    table.resize(n_instances);
    std::vector<uint32_t> nv(n_instances), nf(n_instances);
    for(uint32_t i = 0; i < n_instances; i++) {
        const KeptMesh &m = *mesh_of[i];
        PtBatchInstance &t = table[i];
        t.vertices = m.vertices.ptr;
        t.faces = m.faces.ptr;
        t.n_vertices = nv[i] = m.n_vertices;
        t.n_faces = nf[i] = m.n_faces;
        t.vertex_base = t.face_base = 0;
        t.smooth = instances[i].smooth != 0 ? 1u : 0u;
        t.pad = 0;
        std::copy(instances[i].transform, instances[i].transform + 16, t.m);
    }
    const PtBatchLimits limits;
    for(uint32_t first = 0; first < n_instances;) {
        const uint32_t end = pt_mesh_batch_chunk_end(nv.data(), nf.data(), n_instances, first, limits);
        const size_t at = 9 * static_cast<size_t>(result->kept);
        uint64_t kept = 0;
        const char *what = "";
        const hipError_t e = pt_mesh_batch_chunk(stream, scratch, table.data() + first, end - first, room - result->kept, pos + at, nrm != nullptr ? nrm + at : nullptr,
                                                 counts + first, &kept, &what);
        if(e != hipSuccess) {
            return fail(PT_ERR_HIP, std::string("batched mesh assembly (") + what + "): " + hipGetErrorString(e));
        }
        result->kept += kept;
        result->chunks++;
        result->syncs++;
        first = end;
    }
    if(result->kept > room) {
        return fail(PT_ERR_HIP, "internal: batched mesh assembly kept more triangles than there are faces");
    }
    return PT_OK;
}

} // namespace

extern "C" {

int pt_mesh_assemble_batch(int device, const pt_mesh_data *meshes, uint32_t n_meshes, const pt_mesh_instance *instances, uint32_t n_instances, uint64_t capacity,
                           float *out_pos, float *out_nrm, uint32_t *out_counts, uint64_t *n_triangles) {
    if(n_triangles == nullptr || (n_meshes > 0 && meshes == nullptr) || (n_instances > 0 && instances == nullptr) ||
       (capacity > 0 && (out_pos == nullptr || out_nrm == nullptr))) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    *n_triangles = 0;
    std::vector<uint8_t> used(n_meshes, 0);
    uint64_t faces = 0;
    for(uint32_t i = 0; i < n_instances; i++) {
        if(instances[i].mesh >= n_meshes) {
            return fail(PT_ERR_INVALID, "instance names a mesh that is not there");
        }
        used[instances[i].mesh] = 1;
        faces += meshes[instances[i].mesh].n_faces;
    }
    for(uint32_t m = 0; m < n_meshes; m++) {
        if(used[m] != 0) {
            PT_TRY(check_mesh(&meshes[m]));
        }
    }
    if(faces > PT_REF_INDEX) {
        return fail(PT_ERR_UNSUPPORTED, "too many faces");
    }
    PT_TRY(check_device(device));
    PT_HIP(hipSetDevice(device));
    if(n_instances == 0) {
        return PT_OK;
    }
    StreamGuard sg;
    PT_HIP(hipStreamCreateWithFlags(&sg.stream, hipStreamNonBlocking));
    std::vector<std::unique_ptr<KeptMesh>> uploaded(n_meshes);
    for(uint32_t m = 0; m < n_meshes; m++) {
        if(used[m] != 0) {
            uploaded[m].reset(new KeptMesh());
            PT_TRY(uploaded[m]->upload(meshes[m]));
        }
    }
    std::vector<const KeptMesh *> mesh_of(n_instances);
    for(uint32_t i = 0; i < n_instances; i++) {
        mesh_of[i] = uploaded[instances[i].mesh].get();
    }
    DevBuf<float> pos, nrm;
    PT_HIP(pos.ensure(9 * static_cast<size_t>(faces)));
    PT_HIP(nrm.ensure(9 * static_cast<size_t>(faces)));
    PtBatchScratch scratch;
    std::vector<PtBatchInstance> table;
    std::vector<uint32_t> counts(n_instances, 0);
    BatchResult result;
    PT_TRY(assemble_batch(sg.stream, scratch, mesh_of, instances, n_instances, table, faces, pos.ptr, nrm.ptr, counts.data(), &result));
    const size_t n_out = static_cast<size_t>(std::min<uint64_t>(result.kept, capacity));
    if(n_out > 0) {
        PT_HIP(hipMemcpyAsync(out_pos, pos.ptr, 9 * n_out * sizeof(float), hipMemcpyDeviceToHost, sg.stream));
        PT_HIP(hipMemcpyAsync(out_nrm, nrm.ptr, 9 * n_out * sizeof(float), hipMemcpyDeviceToHost, sg.stream));
    }
    PT_HIP(hipStreamSynchronize(sg.stream)); // (before the scratch and the arrays go)
    if(out_counts != nullptr) {
        std::copy(counts.begin(), counts.end(), out_counts);
    }
    *n_triangles = result.kept;
    return PT_OK;
}

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

    using clock = std::chrono::steady_clock;
    auto ms_since = [](clock::time_point t0) { return std::chrono::duration<float, std::milli>(clock::now() - t0).count(); };
    const auto t_begin = clock::now();
    std::vector<pt_mesh_instance> posed = keep.instances; // (adopted with the rest, on success)
    for(uint32_t k = 0; k < n; k++) {
        const uint32_t i = instances != nullptr ? instances[k] : k;
        std::copy(transforms + 16 * static_cast<size_t>(k), transforms + 16 * static_cast<size_t>(k) + 16, posed[i].transform);
    }
    const pt_scene_desc *d = &keep.desc.d;
    PT_HIP(hipSetDevice(s->device));
    PT_HIP(hipStreamSynchronize(s->stream));

    // ---- upload: the description's own triangles in front of the arrays the instances are expanded into (the meshes are there) --------
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
    if(d->n_triangles > 0) {
        PT_HIP(hipMemcpyAsync(pos.ptr, d->tri_pos, 9 * static_cast<size_t>(d->n_triangles) * sizeof(float), hipMemcpyHostToDevice, s->stream));
        if(d->tri_nrm != nullptr) {
            PT_HIP(hipMemcpyAsync(nrm.ptr, d->tri_nrm, 9 * static_cast<size_t>(d->n_triangles) * sizeof(float), hipMemcpyHostToDevice, s->stream));
        }
        else if(with_normals) {
            PT_HIP(pt_mesh_face_normals(s->stream, d->n_triangles, pos.ptr, nrm.ptr));
        }
    }
    const float upload_ms = ms_since(t_begin);

    // ---- assembly: one chain of launches for all instances, one wait per chunk for their counts -------------------------------------------
    EventPair assembly;
    PT_HIP(assembly.begin(s->stream));
    std::vector<const KeptMesh *> mesh_of(n_instances);
    for(uint32_t i = 0; i < n_instances; i++) {
        mesh_of[i] = keep.meshes[posed[i].mesh].get();
    }
    keep.counts.assign(n_instances, 0);
    BatchResult batch;
    const size_t at = 9 * static_cast<size_t>(d->n_triangles);
    PT_TRY(assemble_batch(s->stream, keep.scratch, mesh_of, posed.data(), n_instances, keep.table, keep.capacity - d->n_triangles, pos.ptr + at,
                          with_normals ? nrm.ptr + at : nullptr, keep.counts.data(), &batch));
    PT_HIP(assembly.end(s->stream));

    DeviceTriangles assembled;
    assembled.n_triangles = d->n_triangles;
    std::vector<uint32_t> inst_first(n_instances), inst_count(n_instances);
    for(uint32_t i = 0; i < n_instances; i++) {
        const uint32_t kept = keep.counts[i];
        assembled.ranges.push_back(MeshRange{assembled.n_triangles, kept, static_cast<uint8_t>(posed[i].cull_backface != 0 ? 1 : 0), posed[i].material});
        inst_first[i] = d->n_objects + (assembled.n_triangles - d->n_triangles);
        inst_count[i] = kept;
        assembled.n_triangles += kept;
    }
    assembled.ready = assembly.last.e;
    assembled.batch_scratch = &keep.scratch;

    // ---- the scene of these arrays, built aside by the path every scene takes -------------------------------------------------------------
    pt_scene *built = nullptr;
    const int rc = finish_mesh_scene(s->device, d, assembled, pos, nrm, with_normals, inst_first, inst_count, &built);
    if(rc != PT_OK) {
        (void)hipStreamSynchronize(s->stream); // (nothing of the failed pose is in flight when the arrays are used again)
        return rc;
    }
    std::unique_ptr<pt_scene> t(built);
    PT_HIP(hipStreamSynchronize(s->stream));
    float assembly_ms = 0.0F;
    PT_HIP(assembly.ms(&assembly_ms));

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
    if(info != nullptr) {
        info->n_instances = n_instances;
        info->n_triangles = static_cast<uint32_t>(batch.kept);
        info->assembly_syncs = batch.syncs;
        info->assembly_chunks = batch.chunks;
        info->upload_ms = upload_ms;
        info->assembly_ms = assembly_ms;
        info->tree_ms = tree_ms;
        info->rest_ms = std::max(total_ms - upload_ms - assembly_ms - tree_ms, 0.0F);
        info->total_ms = total_ms;
    }
    if(env_int("PT_DEBUG", 0) != 0) {
        std::fprintf(stderr, "[pt] pose: %u instances, %llu triangles kept, %u chunk(s); upload %.1f ms, assembly %.1f ms, tree %.1f ms, total %.1f ms; scratch allocations so far %llu\n",
                     n_instances, static_cast<unsigned long long>(batch.kept), batch.chunks, upload_ms, assembly_ms, tree_ms, total_ms,
                     static_cast<unsigned long long>(keep.scratch.allocations));
    }
    return PT_OK;
}

} // extern "C"
