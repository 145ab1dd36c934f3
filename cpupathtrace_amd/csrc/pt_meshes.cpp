// pt_meshes.cpp -- the entry points of include/pt_mesh.h, and pt_mesh_assemble_batch of include/pt_pose.h: scenes from indexed meshes and
// instances.  The meshes are uploaded once, all instances are transformed, filtered, expanded and smoothed in HBM by the batched assembler
// (pt_mesh_batch.h) behind the description's own triangles, and the arrays go to the device builder where they are (create_scene,
// pt_api.cpp); the host builder gets them downloaded and takes pt_scene_create's path.  pt_scene_pose (pt_pose.cpp) shares both halves.
#include "pt_host.h"

using namespace pth;

namespace {

// All instances through the batched assembler, chunk after chunk, each behind the survivors of the one before: positions and normals at
// pos / nrm (room for `room` triangles), the per-instance counts to counts[n_instances], their sum to *kept.  One wait per chunk; the
// last chunk's sort and smoothing are only enqueued when this returns.  face_of (null: not tracked): the scene-wide face of every
// survivor, written behind every chunk from the flags and ranks the chunk left in the scratch (pt_motion_shapes_kernels.h).
int assemble_batch(hipStream_t stream, PtBatchScratch &scratch, const std::vector<std::unique_ptr<KeptMesh>> &meshes, const pt_mesh_instance *instances, uint32_t n_instances,
                   uint64_t room, float *pos, float *nrm, uint32_t *counts, uint64_t *kept, uint32_t *chunks, uint32_t *face_of = nullptr) {
    std::vector<PtBatchInstance> table(n_instances);
    std::vector<uint32_t> nv(n_instances), nf(n_instances);
    for(uint32_t i = 0; i < n_instances; i++) {
        const KeptMesh &m = *meshes[instances[i].mesh];
        PtBatchInstance &t = table[i];
        t.vertices = m.shape;
        t.faces = m.faces.ptr;
        t.n_vertices = nv[i] = m.n_vertices;
        t.n_faces = nf[i] = m.n_faces;
        t.vertex_base = t.face_base = 0;
        t.smooth = instances[i].smooth != 0 ? 1u : 0u;
        t.pad = 0;
        std::copy(instances[i].transform, instances[i].transform + 16, t.m);
    }
    *kept = 0;
    *chunks = 0;
    const PtBatchLimits limits;
    uint64_t face_base_scene = 0; // the faces of the chunks before
    for(uint32_t first = 0; first < n_instances;) {
        const uint32_t end = pt_mesh_batch_chunk_end(nv.data(), nf.data(), n_instances, first, limits);
        const size_t at = 9 * static_cast<size_t>(*kept);
        uint64_t kept_here = 0;
        const char *what = "";
        const hipError_t e = pt_mesh_batch_chunk(stream, scratch, table.data() + first, end - first, room - *kept, pos + at, nrm != nullptr ? nrm + at : nullptr, counts + first,
                                                 &kept_here, &what);
        if(e != hipSuccess) {
            return fail(PT_ERR_HIP, std::string("batched mesh assembly (") + what + "): " + hipGetErrorString(e));
        }
        uint64_t chunk_faces = 0;
        for(uint32_t i = first; i < end; i++) {
            chunk_faces += nf[i];
        }
        if(face_of != nullptr && chunk_faces > 0) { // (a chunk without faces has not touched the scratch)
            const hipError_t ef = pt_face_table_launch(stream, static_cast<const uint32_t *>(scratch.flag.ptr), static_cast<const uint32_t *>(scratch.rank.ptr),
                                                       static_cast<uint32_t>(chunk_faces), room - *kept, face_of + *kept, static_cast<uint32_t>(face_base_scene));
            if(ef != hipSuccess) {
                return fail(PT_ERR_HIP, std::string("face table kernel: ") + hipGetErrorString(ef));
            }
        }
        face_base_scene += chunk_faces;
        *kept += kept_here;
        (*chunks)++;
        first = end;
    }
    if(*kept > room) {
        return fail(PT_ERR_HIP, "internal: batched mesh assembly kept more triangles than there are faces");
    }
    return PT_OK;
}

} // namespace

namespace pth {

int check_mesh(const pt_mesh_data *m) {
    if((m->n_vertices > 0 && m->vertices == nullptr) || (m->n_faces > 0 && m->faces == nullptr)) {
        return fail(PT_ERR_INVALID, "missing array in mesh");
    }
    if(m->n_faces > PT_MESH_MAX_FACES) {
        return fail(PT_ERR_UNSUPPORTED, "too many faces in one mesh");
    }
    return PT_OK;
}

int KeptMesh::upload(const pt_mesh_data &m) {
    PT_HIP(vertices.ensure(3 * static_cast<size_t>(m.n_vertices)));
    PT_HIP(faces.ensure(3 * static_cast<size_t>(m.n_faces)));
    if(m.n_vertices > 0) {
        PT_HIP(hipMemcpy(vertices.ptr, m.vertices, 3 * static_cast<size_t>(m.n_vertices) * sizeof(float), hipMemcpyHostToDevice));
    }
    if(m.n_faces > 0) {
        PT_HIP(hipMemcpy(faces.ptr, m.faces, 3 * static_cast<size_t>(m.n_faces) * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    n_vertices = m.n_vertices;
    n_faces = m.n_faces;
    shape = vertices.ptr;
    return PT_OK;
}

void DescCopy::assign(const pt_scene_desc &src) {
    auto take = [](auto &to, const auto *from, size_t count) {
        to.clear();
        if(from != nullptr && count > 0) {
            to.assign(from, from + count);
        }
        return to.empty() ? nullptr : to.data();
    };
    d = src;
    d.obj_kind = take(obj_kind, src.obj_kind, src.n_objects);
    d.tri_pos = take(tri_pos, src.tri_pos, 9 * static_cast<size_t>(src.n_triangles));
    d.tri_nrm = take(tri_nrm, src.tri_nrm, 9 * static_cast<size_t>(src.n_triangles));
    d.tri_cull = take(tri_cull, src.tri_cull, src.n_triangles);
    d.tri_material = take(tri_material, src.tri_material, src.n_triangles);
    d.sph = take(sph, src.sph, 4 * static_cast<size_t>(src.n_spheres));
    d.sph_material = take(sph_material, src.sph_material, src.n_spheres);
    d.materials = take(materials, src.materials, src.n_materials);
    d.light_pos = take(light_pos, src.light_pos, 3 * static_cast<size_t>(src.n_point_lights));
    d.light_spectrum = take(light_spectrum, src.light_spectrum, 4 * static_cast<size_t>(src.n_point_lights));
}

int assemble_mesh_scene(hipStream_t stream, const pt_scene_desc *d, const std::vector<std::unique_ptr<KeptMesh>> &meshes, const std::vector<pt_mesh_instance> &instances,
                        PtBatchScratch &scratch, uint64_t capacity, float *pos, float *nrm, MeshAssembly *out, uint32_t *face_of) {
    const uint32_t n_instances = static_cast<uint32_t>(instances.size());
    const size_t front = 9 * static_cast<size_t>(d->n_triangles);
    if(d->n_triangles > 0) {
        PT_HIP(hipMemcpyAsync(pos, d->tri_pos, front * sizeof(float), hipMemcpyHostToDevice, stream));
        if(d->tri_nrm != nullptr) {
            PT_HIP(hipMemcpyAsync(nrm, d->tri_nrm, front * sizeof(float), hipMemcpyHostToDevice, stream));
        }
        else if(nrm != nullptr) {
            PT_HIP(pt_mesh_face_normals(stream, d->n_triangles, pos, nrm));
        }
    }
    out->front_done = std::chrono::steady_clock::now();

    // ---- assembly: one chain of launches for all instances, one wait per chunk for their counts -------------------------------------------
    PT_HIP(out->chain.begin(stream));
    out->inst_first.assign(n_instances, 0);
    out->inst_count.assign(n_instances, 0);
    uint64_t kept = 0;
    PT_TRY(assemble_batch(stream, scratch, meshes, instances.data(), n_instances, capacity - d->n_triangles, pos + front, nrm != nullptr ? nrm + front : nullptr,
                          out->inst_count.data(), &kept, &out->chunks, face_of));
    PT_HIP(out->chain.end(stream));

    DeviceTriangles &t = out->triangles;
    t.pos = pos;
    t.nrm = nrm;
    t.n_triangles = d->n_triangles;
    t.ranges.clear();
    for(uint32_t i = 0; i < n_instances; i++) {
        t.ranges.push_back(PtBatchRange{t.n_triangles, out->inst_count[i], instances[i].material, instances[i].cull_backface != 0 ? 1u : 0u});
        out->inst_first[i] = d->n_objects + (t.n_triangles - d->n_triangles);
        t.n_triangles += out->inst_count[i];
    }
    t.ready = out->chain.last.e;
    t.scratch = &scratch;
    return PT_OK;
}

int finish_mesh_scene(int device, const pt_scene_desc *d, const MeshAssembly &assembly, DevBuf<float> &pos, pt_scene **out) {
    *out = nullptr;
    const DeviceTriangles &assembled = assembly.triangles;
    const bool with_normals = assembled.nrm != nullptr;
    const uint32_t n_mesh_tris = assembled.n_triangles - d->n_triangles, n_objs = d->n_objects + n_mesh_tris;

    pt_scene *scene = nullptr;
    if(builds_on_device(n_objs)) {
        PT_TRY(create_scene(device, d, &assembled, &scene));
    }
    else {
        // ---- the host builder: the assembled arrays come back and the scene is pt_scene_create's of the merged description --------------
        if(assembled.ready != nullptr) {
            PT_HIP(hipEventSynchronize(assembled.ready));
        }
        const size_t n_tris = assembled.n_triangles;
        std::vector<float> h_pos(9 * n_tris), h_nrm(with_normals ? 9 * n_tris : 0);
        std::vector<uint8_t> kind(n_objs, static_cast<uint8_t>(PT_OBJ_TRIANGLE)), cull(n_tris);
        std::vector<uint32_t> material(n_tris);
        if(n_tris > 0) {
            PT_HIP(hipMemcpy(h_pos.data(), assembled.pos, h_pos.size() * sizeof(float), hipMemcpyDeviceToHost));
            if(with_normals) {
                PT_HIP(hipMemcpy(h_nrm.data(), assembled.nrm, h_nrm.size() * sizeof(float), hipMemcpyDeviceToHost));
            }
        }
        std::copy(d->obj_kind, d->obj_kind + d->n_objects, kind.begin());
        std::copy(d->tri_cull, d->tri_cull + d->n_triangles, cull.begin());
        std::copy(d->tri_material, d->tri_material + d->n_triangles, material.begin());
        for(const PtBatchRange &r : assembled.ranges) {
            std::fill(cull.begin() + r.first_tri, cull.begin() + r.first_tri + r.count, static_cast<uint8_t>(r.cull));
            std::fill(material.begin() + r.first_tri, material.begin() + r.first_tri + r.count, r.material);
        }
        pt_scene_desc merged = *d;
        merged.n_objects = n_objs;
        merged.obj_kind = kind.data();
        merged.n_triangles = static_cast<uint32_t>(n_tris);
        merged.tri_pos = h_pos.data();
        merged.tri_nrm = with_normals ? h_nrm.data() : nullptr;
        merged.tri_cull = cull.data();
        merged.tri_material = material.data();
        PT_TRY(create_scene(device, &merged, nullptr, &scene));
    }
    // ---- what pt_scene_instance_ranges and pt_scene_get_triangles answer from ----------------------------------------------------------------
    scene->n_desc_objects = d->n_objects;
    scene->n_desc_tris = d->n_triangles;
    scene->inst_first = assembly.inst_first;
    scene->inst_count = assembly.inst_count;
    scene->desc_ref.resize(d->n_objects);
    {
        uint32_t ti = 0, si = 0;
        for(uint32_t i = 0; i < d->n_objects; i++) {
            scene->desc_ref[i] = d->obj_kind[i] == PT_OBJ_TRIANGLE ? ti++ : (PT_REF_SPHERE | si++);
        }
    }
    take(scene->tri_pos_kept, pos);
    *out = scene;
    return PT_OK;
}

} // namespace pth

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
    DevBuf<float> pos, nrm;
    PT_HIP(pos.ensure(9 * static_cast<size_t>(faces)));
    PT_HIP(nrm.ensure(9 * static_cast<size_t>(faces)));
    PtBatchScratch scratch;
    std::vector<uint32_t> counts(n_instances, 0);
    uint64_t kept = 0;
    uint32_t chunks = 0;
    const int rc = assemble_batch(sg.stream, scratch, uploaded, instances, n_instances, faces, pos.ptr, nrm.ptr, counts.data(), &kept, &chunks);
    const size_t n_out = rc == PT_OK ? static_cast<size_t>(std::min<uint64_t>(kept, capacity)) : 0;
    hipError_t e = hipSuccess;
    if(n_out > 0) {
        e = hipMemcpyAsync(out_pos, pos.ptr, 9 * n_out * sizeof(float), hipMemcpyDeviceToHost, sg.stream);
        if(e == hipSuccess) {
            e = hipMemcpyAsync(out_nrm, nrm.ptr, 9 * n_out * sizeof(float), hipMemcpyDeviceToHost, sg.stream);
        }
    }
    const hipError_t drained = hipStreamSynchronize(sg.stream); // (whatever happened: before the scratch and the arrays go)
    PT_TRY(rc);
    PT_HIP(e);
    PT_HIP(drained);
    if(out_counts != nullptr) {
        std::copy(counts.begin(), counts.end(), out_counts);
    }
    *n_triangles = kept;
    return PT_OK;
}

// A batch of one
int pt_mesh_assemble(int device, const pt_mesh_data *mesh, const pt_mesh_instance *instance, uint64_t capacity, float *out_pos, float *out_nrm, uint64_t *n_triangles) {
    if(mesh == nullptr || instance == nullptr || n_triangles == nullptr || (capacity > 0 && (out_pos == nullptr || out_nrm == nullptr))) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    pt_mesh_instance one = *instance;
    one.mesh = 0; // (the instance's own mesh index is not read: `mesh` is the mesh)
    return pt_mesh_assemble_batch(device, mesh, 1, &one, 1, capacity, out_pos, out_nrm, nullptr, n_triangles);
}

int pt_scene_create_meshes(int device, const pt_scene_desc *d, const pt_mesh_data *meshes, uint32_t n_meshes, const pt_mesh_instance *instances, uint32_t n_instances,
                           pt_scene **out) {
    if(d == nullptr || out == nullptr || (n_meshes > 0 && meshes == nullptr) || (n_instances > 0 && instances == nullptr)) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    *out = nullptr;
    if(n_instances == 0) {
        return create_scene(device, d, nullptr, out);
    }
    if((d->n_materials > 0 && d->materials == nullptr) || (d->n_triangles > 0 && (d->tri_pos == nullptr || d->tri_cull == nullptr || d->tri_material == nullptr)) ||
       (d->n_objects > 0 && d->obj_kind == nullptr)) {
        return fail(PT_ERR_INVALID, "missing array in scene description");
    }
    std::vector<uint8_t> used(n_meshes, 0);
    uint64_t capacity = d->n_triangles; // triangles before any face is rejected
    bool any_smooth = false;
    for(uint32_t i = 0; i < n_instances; i++) {
        const pt_mesh_instance &in = instances[i];
        if(in.mesh >= n_meshes) {
            return fail(PT_ERR_INVALID, "instance names a mesh that is not there");
        }
        if(in.material != PT_NO_MATERIAL && in.material >= d->n_materials) {
            return fail(PT_ERR_INVALID, "instance material index out of range");
        }
        used[in.mesh] = 1;
        capacity += meshes[in.mesh].n_faces;
        any_smooth = any_smooth || in.smooth != 0;
    }
    for(uint32_t m = 0; m < n_meshes; m++) {
        if(used[m] != 0) {
            PT_TRY(check_mesh(&meshes[m]));
        }
    }
    if(capacity > PT_REF_INDEX) {
        return fail(PT_ERR_UNSUPPORTED, "too many objects");
    }
    PT_TRY(check_device(device));
    PT_HIP(hipSetDevice(device));

    using clock = std::chrono::steady_clock;
    const auto t_upload = clock::now();
    StreamGuard sg;
    PT_HIP(hipStreamCreateWithFlags(&sg.stream, hipStreamNonBlocking));
    // ---- upload: every mesh that is used, once (the scene keeps them, with the instance table and a copy of the description, for
    // pt_scene_pose) ----
    std::unique_ptr<PoseKeep> keep(new PoseKeep());
    keep->meshes.resize(n_meshes);
    uint64_t upload_bytes = 0;
    for(uint32_t m = 0; m < n_meshes; m++) {
        if(used[m] != 0) {
            keep->meshes[m].reset(new KeptMesh());
            PT_TRY(keep->meshes[m]->upload(meshes[m]));
            upload_bytes += 12ULL * meshes[m].n_vertices + 12ULL * meshes[m].n_faces;
        }
    }
    keep->instances.assign(instances, instances + n_instances);
    keep->any_smooth = any_smooth;
    keep->capacity = capacity;
    // without normals from the caller and without a smooth instance there is no normal array: the builder makes face normals itself
    const bool with_normals = any_smooth || (d->n_triangles > 0 && d->tri_nrm != nullptr);
    DevBuf<float> pos, nrm;
    PT_HIP(pos.ensure(9 * static_cast<size_t>(capacity)));
    if(with_normals) {
        PT_HIP(nrm.ensure(9 * static_cast<size_t>(capacity)));
    }

    // ---- assembly, with a scratch of this call's own: a scene that is never posed keeps none.  However the call ends, the scratch and
    // the arrays go only when nothing reads them any more: the chain on the assembly stream, and the range fill on the new scene's
    // stream, which reads the scratch's range table (a scene that failed has taken its stream along: then the device is waited for) ----
    PtBatchScratch scratch;
    std::unique_ptr<pt_scene> scene;
    struct Drain {
        hipStream_t assembly, scene;
        PtBatchScratch &scratch;
        ~Drain() {
            (void)hipStreamSynchronize(assembly);
            (void)(scene != nullptr ? hipStreamSynchronize(scene) : hipDeviceSynchronize());
            scratch.release();
        }
    } drain{sg.stream, nullptr, scratch};
    MeshAssembly assembly;
    PT_TRY(assemble_mesh_scene(sg.stream, d, keep->meshes, keep->instances, scratch, capacity, pos.ptr, with_normals ? nrm.ptr : nullptr, &assembly));
    const float upload_ms = std::chrono::duration<float, std::milli>(assembly.front_done - t_upload).count();
    pt_scene *built = nullptr;
    PT_TRY(finish_mesh_scene(device, d, assembly, pos, &built));
    scene.reset(built);
    drain.scene = scene->stream;
    PT_HIP(hipStreamSynchronize(sg.stream));
    PT_HIP(hipStreamSynchronize(scene->stream)); // (an error of either stream is this call's; ~Drain waits again whatever happens)
    float assembly_ms = 0.0F;
    PT_HIP(assembly.chain.ms(&assembly_ms));
    keep->desc.assign(*d);
    scene->pose = std::move(keep);
    if(env_int("PT_DEBUG", 0) != 0) {
        std::fprintf(stderr, "[pt] mesh scene: %u instances, %u of %llu triangles kept; mesh upload %.1f ms (%llu bytes), assembly %.1f ms on the device\n", n_instances,
                     assembly.triangles.n_triangles, static_cast<unsigned long long>(capacity), upload_ms, static_cast<unsigned long long>(upload_bytes), assembly_ms);
    }
    *out = scene.release();
    return PT_OK;
}

int pt_scene_instance_ranges(const pt_scene *scene, uint32_t *first_object, uint32_t *n_objects) {
    if(scene == nullptr) {
        return fail(PT_ERR_INVALID, "null scene");
    }
    for(size_t i = 0; i < scene->inst_first.size(); i++) {
        if(first_object != nullptr) {
            first_object[i] = scene->inst_first[i];
        }
        if(n_objects != nullptr) {
            n_objects[i] = scene->inst_count[i];
        }
    }
    return PT_OK;
}

int pt_scene_get_triangles(pt_scene *s, uint32_t first_object, uint32_t count, float *out_pos, float *out_nrm, uint8_t *out_cull, uint32_t *out_material) {
    if(s == nullptr) {
        return fail(PT_ERR_INVALID, "null scene");
    }
    if(s->tri_pos_kept.ptr == nullptr) {
        return fail(PT_ERR_UNSUPPORTED, "the scene keeps no triangle arrays: it was not made by pt_scene_create_meshes with instances");
    }
    if(static_cast<uint64_t>(first_object) + count > s->n_objects) {
        return fail(PT_ERR_INVALID, "object range outside the scene");
    }
    if(count == 0) {
        return PT_OK;
    }
    // the part of the range in the description (object -> triangle through its table) and the part in the instances (contiguous)
    const uint32_t n_desc = first_object < s->n_desc_objects ? std::min(count, s->n_desc_objects - first_object) : 0U;
    std::vector<uint32_t> idx(n_desc);
    for(uint32_t i = 0; i < n_desc; i++) {
        idx[i] = s->desc_ref[first_object + i];
        if((idx[i] & PT_REF_SPHERE) != 0) {
            return fail(PT_ERR_INVALID, "object range holds a sphere");
        }
    }
    std::lock_guard<std::mutex> lock(s->render_mutex);
    PT_HIP(hipSetDevice(s->device));
    DevBuf<float> d_pos, d_nrm;
    DevBuf<uint8_t> d_cull;
    DevBuf<uint32_t> d_mat, d_idx;
    if(out_pos != nullptr) {
        PT_HIP(d_pos.ensure(9 * static_cast<size_t>(count)));
    }
    if(out_nrm != nullptr) {
        PT_HIP(d_nrm.ensure(9 * static_cast<size_t>(count)));
    }
    if(out_cull != nullptr) {
        PT_HIP(d_cull.ensure(count));
    }
    if(out_material != nullptr) {
        PT_HIP(d_mat.ensure(count));
    }
    const float4 *shade = reinterpret_cast<const float4 *>(s->tri_shade.ptr);
    auto at = [](auto *p, size_t offset) { return p != nullptr ? p + offset : p; };
    if(n_desc > 0) {
        PT_HIP(d_idx.upload(idx));
        PT_HIP(pt_mesh_unpack(s->stream, s->tri_pos_kept.ptr, shade, d_idx.ptr, 0, n_desc, d_pos.ptr, d_nrm.ptr, d_cull.ptr, d_mat.ptr));
    }
    if(count > n_desc) {
        const uint32_t first_tri = s->n_desc_tris + (first_object + n_desc - s->n_desc_objects);
        PT_HIP(pt_mesh_unpack(s->stream, s->tri_pos_kept.ptr, shade, nullptr, first_tri, count - n_desc, at(d_pos.ptr, 9 * static_cast<size_t>(n_desc)),
                              at(d_nrm.ptr, 9 * static_cast<size_t>(n_desc)), at(d_cull.ptr, n_desc), at(d_mat.ptr, n_desc)));
    }
    if(out_pos != nullptr) {
        PT_HIP(hipMemcpyAsync(out_pos, d_pos.ptr, 9 * static_cast<size_t>(count) * sizeof(float), hipMemcpyDeviceToHost, s->stream));
    }
    if(out_nrm != nullptr) {
        PT_HIP(hipMemcpyAsync(out_nrm, d_nrm.ptr, 9 * static_cast<size_t>(count) * sizeof(float), hipMemcpyDeviceToHost, s->stream));
    }
    if(out_cull != nullptr) {
        PT_HIP(hipMemcpyAsync(out_cull, d_cull.ptr, count, hipMemcpyDeviceToHost, s->stream));
    }
    if(out_material != nullptr) {
        PT_HIP(hipMemcpyAsync(out_material, d_mat.ptr, count * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
    }
    PT_HIP(hipStreamSynchronize(s->stream));
    return PT_OK;
}

} // extern "C"
