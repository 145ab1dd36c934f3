// pt_meshes.cpp -- the entry points of include/pt_mesh.h: scenes from indexed meshes and instances.  The meshes are uploaded once, every
// instance is transformed, filtered, smoothed and expanded in HBM (pt_mesh.hip) behind the description's own triangles, and the arrays go
// to the device builder where they are (create_scene, pt_api.cpp); the host builder gets them downloaded and takes pt_scene_create's path.
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

int finish_mesh_scene(int device, const pt_scene_desc *d, DeviceTriangles &assembled, DevBuf<float> &pos, DevBuf<float> &nrm, bool with_normals,
                      const std::vector<uint32_t> &inst_first, const std::vector<uint32_t> &inst_count, pt_scene **out) {
    *out = nullptr;
    assembled.pos = pos.ptr;
    assembled.nrm = with_normals ? nrm.ptr : nullptr;
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
            PT_HIP(hipMemcpy(h_pos.data(), pos.ptr, h_pos.size() * sizeof(float), hipMemcpyDeviceToHost));
            if(with_normals) {
                PT_HIP(hipMemcpy(h_nrm.data(), nrm.ptr, h_nrm.size() * sizeof(float), hipMemcpyDeviceToHost));
            }
        }
        std::copy(d->obj_kind, d->obj_kind + d->n_objects, kind.begin());
        std::copy(d->tri_cull, d->tri_cull + d->n_triangles, cull.begin());
        std::copy(d->tri_material, d->tri_material + d->n_triangles, material.begin());
        for(const MeshRange &r : assembled.ranges) {
            std::fill(cull.begin() + r.first_tri, cull.begin() + r.first_tri + r.count, r.cull);
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
    scene->inst_first = inst_first;
    scene->inst_count = inst_count;
    scene->desc_ref.resize(d->n_objects);
    {
        uint32_t ti = 0, si = 0;
        for(uint32_t i = 0; i < d->n_objects; i++) {
            scene->desc_ref[i] = d->obj_kind[i] == PT_OBJ_TRIANGLE ? ti++ : (PT_REF_SPHERE | si++);
        }
    }
    scene->tri_pos_kept.release();
    scene->tri_pos_kept.ptr = pos.ptr;
    scene->tri_pos_kept.count = pos.count;
    pos.ptr = nullptr;
    pos.count = 0;
    *out = scene;
    return PT_OK;
}

} // namespace pth

extern "C" {

int pt_mesh_assemble(int device, const pt_mesh_data *mesh, const pt_mesh_instance *instance, uint64_t capacity, float *out_pos, float *out_nrm, uint64_t *n_triangles) {
    if(mesh == nullptr || instance == nullptr || n_triangles == nullptr || (capacity > 0 && (out_pos == nullptr || out_nrm == nullptr))) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    *n_triangles = 0;
    PT_TRY(check_mesh(mesh));
    PT_TRY(check_device(device));
    PT_HIP(hipSetDevice(device));
    StreamGuard sg;
    PT_HIP(hipStreamCreateWithFlags(&sg.stream, hipStreamNonBlocking));
    KeptMesh up;
    PT_TRY(up.upload(*mesh));
    DevBuf<float> pos, nrm;
    PT_HIP(pos.ensure(9 * static_cast<size_t>(mesh->n_faces)));
    PT_HIP(nrm.ensure(9 * static_cast<size_t>(mesh->n_faces)));
    uint32_t kept = 0;
    const char *what = "";
    const hipError_t e = pt_mesh_assemble_device(sg.stream, up.view(), instance->transform, instance->smooth != 0, pos.ptr, nrm.ptr, &kept, nullptr, &what);
    if(e != hipSuccess) {
        return fail(PT_ERR_HIP, std::string("mesh assembly (") + what + "): " + hipGetErrorString(e));
    }
    const size_t n_out = static_cast<size_t>(std::min<uint64_t>(kept, capacity));
    if(n_out > 0) {
        PT_HIP(hipMemcpy(out_pos, pos.ptr, 9 * n_out * sizeof(float), hipMemcpyDeviceToHost));
        PT_HIP(hipMemcpy(out_nrm, nrm.ptr, 9 * n_out * sizeof(float), hipMemcpyDeviceToHost));
    }
    *n_triangles = kept;
    return PT_OK;
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
    auto ms_since = [](clock::time_point t0) { return std::chrono::duration<float, std::milli>(clock::now() - t0).count(); };
    const auto t_upload = clock::now();
    StreamGuard sg;
    PT_HIP(hipStreamCreateWithFlags(&sg.stream, hipStreamNonBlocking));
    // ---- upload: every mesh that is used, once; the description's own triangles in front of the arrays the instances are expanded into ----
    // (the scene keeps them, with the instance table and a copy of the description, for pt_scene_pose)
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
    // without normals from the caller and without a smooth instance there is no normal array: the builder makes face normals itself
    const bool with_normals = any_smooth || (d->n_triangles > 0 && d->tri_nrm != nullptr);
    DevBuf<float> pos, nrm;
    PT_HIP(pos.ensure(9 * static_cast<size_t>(capacity)));
    if(with_normals) {
        PT_HIP(nrm.ensure(9 * static_cast<size_t>(capacity)));
    }
    if(d->n_triangles > 0) {
        PT_HIP(hipMemcpy(pos.ptr, d->tri_pos, 9 * static_cast<size_t>(d->n_triangles) * sizeof(float), hipMemcpyHostToDevice));
        if(d->tri_nrm != nullptr) {
            PT_HIP(hipMemcpy(nrm.ptr, d->tri_nrm, 9 * static_cast<size_t>(d->n_triangles) * sizeof(float), hipMemcpyHostToDevice));
        }
        else if(with_normals) {
            PT_HIP(pt_mesh_face_normals(sg.stream, d->n_triangles, pos.ptr, nrm.ptr));
        }
    }
    const float upload_ms = ms_since(t_upload);

    // ---- assembly: instance after instance, each behind the survivors of the one before (its count is read back) --------------------------
    DeviceTriangles assembled;
    assembled.n_triangles = d->n_triangles;
    std::vector<uint32_t> inst_first(n_instances), inst_count(n_instances);
    float assembly_ms = 0.0F;
    for(uint32_t i = 0; i < n_instances; i++) {
        const pt_mesh_instance &in = instances[i];
        const size_t at = 9 * static_cast<size_t>(assembled.n_triangles);
        uint32_t kept = 0;
        float ms = 0.0F;
        const char *what = "";
        const hipError_t e = pt_mesh_assemble_device(sg.stream, keep->meshes[in.mesh]->view(), in.transform, in.smooth != 0, pos.ptr + at,
                                                     with_normals ? nrm.ptr + at : nullptr, &kept, &ms, &what);
        if(e != hipSuccess) {
            return fail(PT_ERR_HIP, std::string("mesh assembly (") + what + "): " + hipGetErrorString(e));
        }
        assembly_ms += ms;
        assembled.ranges.push_back(MeshRange{assembled.n_triangles, kept, static_cast<uint8_t>(in.cull_backface != 0 ? 1 : 0), in.material});
        inst_first[i] = d->n_objects + (assembled.n_triangles - d->n_triangles);
        inst_count[i] = kept;
        assembled.n_triangles += kept;
    }
    PT_HIP(hipStreamSynchronize(sg.stream));
    pt_scene *scene = nullptr;
    PT_TRY(finish_mesh_scene(device, d, assembled, pos, nrm, with_normals, inst_first, inst_count, &scene));
    keep->instances.assign(instances, instances + n_instances);
    keep->desc.assign(*d);
    keep->any_smooth = any_smooth;
    keep->capacity = capacity;
    scene->pose = std::move(keep);
    if(env_int("PT_DEBUG", 0) != 0) {
        std::fprintf(stderr, "[pt] mesh scene: %u instances, %u of %llu triangles kept; mesh upload %.1f ms (%llu bytes), assembly %.1f ms on the device\n", n_instances,
                     assembled.n_triangles, static_cast<unsigned long long>(capacity), upload_ms, static_cast<unsigned long long>(upload_bytes), assembly_ms);
    }
    *out = scene;
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
