// pt_relight.cpp -- pt_scene_relight, pt_scene_get_materials and pt_scene_get_point_lights of include/pt_relight.h: the look of a scene with
// mesh instances replaced in place.  The tree, the records' geometry and the normals stay.  The tables are packed as
// create_scene packs them (pt_api.cpp), the emitter registry is made by the ordered pass of pt_relight.hip over the kept leaf order, and
// the CDF's serial float chain runs on the host over the 8 bytes per emitter that come back.  As in a pose, everything new is built aside
// and the scene adopts it only when it is complete.
#include "pt_host.h"
#include "pt_relight_kernels.h"

using namespace pth;

namespace {

const char *const NO_INSTANCES = "the scene has no instances: it was not made by pt_scene_create_meshes with instances";

// The material word of every triangle of the instances in `which` becomes material[i] (one launch over their ranges)
int write_instance_materials(pt_scene *s, const std::vector<uint32_t> &which, const std::vector<uint32_t> &material, DevBuf<PtRelightRange> &table, uint32_t *rewritten) {
    std::vector<PtRelightRange> ranges;
    uint32_t total = 0;
    for(uint32_t i : which) { // (ascending: the ranges come out sorted by first_tri)
        if(s->inst_count[i] > 0) {
            ranges.push_back(PtRelightRange{s->n_desc_tris + (s->inst_first[i] - s->n_desc_objects), s->inst_count[i], material[i], total});
            total += s->inst_count[i];
        }
    }
    *rewritten = total;
    if(ranges.empty()) {
        return PT_OK;
    }
    PT_HIP(table.ensure(ranges.size()));
    PT_HIP(hipMemcpyAsync(table.ptr, ranges.data(), ranges.size() * sizeof(PtRelightRange), hipMemcpyHostToDevice, s->stream));
    PT_HIP(pt_relight_materials(s->stream, table.ptr, static_cast<uint32_t>(ranges.size()), total, reinterpret_cast<float4 *>(s->recs.ptr),
                                reinterpret_cast<float4 *>(s->tri_shade.ptr)));
    PT_HIP(hipStreamSynchronize(s->stream)); // (`ranges` is pageable memory: the copy has read it when this returns; so has the launch `table`)
    return PT_OK;
}

} // namespace

extern "C" {

int pt_scene_get_materials(const pt_scene *scene, pt_material *out, uint32_t capacity, uint32_t *n_materials) {
    if(scene == nullptr || (capacity > 0 && out == nullptr)) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    if(scene->pose == nullptr) {
        return fail(PT_ERR_UNSUPPORTED, NO_INSTANCES);
    }
    std::lock_guard<std::mutex> lock(const_cast<pt_scene *>(scene)->render_mutex);
    const std::vector<pt_material> &m = scene->pose->desc.materials;
    std::copy(m.begin(), m.begin() + std::min<size_t>(m.size(), capacity), out);
    if(n_materials != nullptr) {
        *n_materials = static_cast<uint32_t>(m.size());
    }
    return PT_OK;
}

int pt_scene_get_point_lights(const pt_scene *scene, float *out_pos, float *out_spectrum, uint32_t capacity, uint32_t *n_point_lights) {
    if(scene == nullptr || (capacity > 0 && (out_pos == nullptr || out_spectrum == nullptr))) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    if(scene->pose == nullptr) {
        return fail(PT_ERR_UNSUPPORTED, NO_INSTANCES);
    }
    std::lock_guard<std::mutex> lock(const_cast<pt_scene *>(scene)->render_mutex);
    const DescCopy &desc = scene->pose->desc;
    const size_t n = std::min<size_t>(desc.d.n_point_lights, capacity);
    std::copy(desc.light_pos.begin(), desc.light_pos.begin() + 3 * n, out_pos);
    std::copy(desc.light_spectrum.begin(), desc.light_spectrum.begin() + 4 * n, out_spectrum);
    if(n_point_lights != nullptr) {
        *n_point_lights = desc.d.n_point_lights;
    }
    return PT_OK;
}

int pt_scene_relight(pt_scene *s, const pt_relight *look, pt_relight_info *info) {
    if(info != nullptr) {
        *info = pt_relight_info{};
    }
    if(s == nullptr || look == nullptr) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    if((look->set_point_lights != 0 && look->n_point_lights > 0 && (look->light_pos == nullptr || look->light_spectrum == nullptr)) ||
       (look->n_instance_materials > 0 && (look->instances == nullptr || look->instance_material == nullptr))) {
        return fail(PT_ERR_INVALID, "null array with a non-zero count");
    }
    // (materials == NULL says that the table stays, whatever n_materials holds)
    std::lock_guard<std::mutex> lock(s->render_mutex);
    if(s->pose == nullptr) {
        return fail(PT_ERR_UNSUPPORTED, NO_INSTANCES);
    }
    PoseKeep &keep = *s->pose;
    DescCopy &desc = keep.desc;
    const uint32_t n_instances = static_cast<uint32_t>(keep.instances.size());
    const bool new_materials = look->materials != nullptr, new_lights = look->set_point_lights != 0;
    const uint32_t n_materials = new_materials ? look->n_materials : desc.d.n_materials;
    const pt_material *materials = new_materials ? look->materials : desc.materials.data();
    const uint32_t n_lights = new_lights ? look->n_point_lights : desc.d.n_point_lights;
    for(uint32_t m = 0; new_materials && m < n_materials; m++) {
        if(materials[m].bsdf < PT_BSDF_LAMBERTIAN || materials[m].bsdf > PT_BSDF_MIRROR) {
            return fail(PT_ERR_INVALID, "unknown BSDF kind");
        }
    }
    std::vector<uint32_t> inst_material(n_instances);
    for(uint32_t i = 0; i < n_instances; i++) {
        inst_material[i] = keep.instances[i].material;
    }
    for(uint32_t k = 0; k < look->n_instance_materials; k++) {
        if(look->instances[k] >= n_instances) {
            return fail(PT_ERR_INVALID, "instance index " + std::to_string(look->instances[k]) + " out of range: the scene has " + std::to_string(n_instances));
        }
        inst_material[look->instances[k]] = look->instance_material[k];
    }
    auto in_table = [n_materials](uint32_t m) { return m == PT_NO_MATERIAL || m < n_materials; };
    for(uint32_t m : desc.tri_material) {
        if(!in_table(m)) {
            return fail(PT_ERR_INVALID, "triangle material index out of range");
        }
    }
    for(uint32_t m : desc.sph_material) {
        if(!in_table(m)) {
            return fail(PT_ERR_INVALID, "sphere material index out of range");
        }
    }
    for(uint32_t m : inst_material) {
        if(!in_table(m)) {
            return fail(PT_ERR_INVALID, "instance material index out of range");
        }
    }
    if(s->live_frames.load() != 0) {
        return fail(PT_ERR_INVALID, "the scene has a live frame: its parked state belongs to the present geometry (pt_frame_destroy first)");
    }

    using clock = std::chrono::steady_clock;
    const auto t_begin = clock::now();
    std::vector<uint32_t> changed; // the instances whose material changes, ascending
    for(uint32_t i = 0; i < n_instances; i++) {
        if(inst_material[i] != keep.instances[i].material) {
            changed.push_back(i);
        }
    }
    bool same_emission = n_materials == desc.d.n_materials;
    for(uint32_t m = 0; same_emission && m < n_materials; m++) {
        same_emission = std::memcmp(materials[m].emission, desc.materials[m].emission, sizeof(materials[m].emission)) == 0;
    }
    const bool rebuild = !changed.empty() || n_lights != desc.d.n_point_lights || !same_emission;

    PT_HIP(hipSetDevice(s->device));
    PT_HIP(hipStreamSynchronize(s->stream));

    // ---- the tables of the new look, aside ---------------------------------------------------------------------------------------------
    DevBuf<F4> d_materials, d_lights, d_emis;
    DevBuf<float> d_cdf;
    if(new_materials || rebuild) { // (a rebuild reads the table it registers from: the new one, or a copy of the one that stays)
        PT_HIP(d_materials.upload(material_table(materials, n_materials)));
    }
    if(new_lights) {
        PT_HIP(d_lights.upload(light_table(look->light_pos, look->light_spectrum, n_lights)));
    }

    std::vector<int32_t> emissive_obj;
    std::vector<float> cdf;
    uint32_t n_candidates = 0, rewritten = 0;
    float registry_ms = 0.0F;
    int object_sample_count = static_cast<int>(s->dev.n_object_samples);
    if(rebuild) {
        // ---- the order of the leaves and the description's object table, uploaded once ---------------------------------------------------
        if(s->leaf_order.ptr == nullptr) {
            std::vector<int32_t> dfs;
            ptb::leaves_depth_first(s->tree, dfs);
            if(dfs.size() != s->n_objects) {
                return fail(PT_ERR_HIP, "internal: the scene keeps neither the device builder's leaf order nor a host tree");
            }
            PT_HIP(s->leaf_order.upload(std::vector<uint32_t>(dfs.begin(), dfs.end())));
        }
        if(s->desc_ref_dev.ptr == nullptr) { // (an empty table occupies one element: DevBuf::ensure, so this holds once for it as well)
            PT_HIP(s->desc_ref_dev.upload(s->desc_ref));
        }
        // ---- the instances' material words: the registry pass reads an object's material from its record.  They are put back if the new
        // look is refused below ----
        DevBuf<PtRelightRange> range_table;
        struct PutBack {
            pt_scene *s;
            const std::vector<uint32_t> &changed;
            std::vector<uint32_t> before;
            DevBuf<PtRelightRange> &table;
            bool armed = true;
            ~PutBack() {
                if(armed) {
                    // (the message of the refusal being returned stays the thread's message, whatever the way back says)
                    const std::string refusal = last_error();
                    uint32_t n = 0;
                    if(write_instance_materials(s, changed, before, table, &n) != PT_OK) {
                        (void)fail(PT_ERR_HIP, refusal);
                    }
                }
            }
        } put_back{s, changed, std::vector<uint32_t>(n_instances), range_table}; // (in place before the first word is written)
        for(uint32_t i = 0; i < n_instances; i++) {
            put_back.before[i] = keep.instances[i].material;
        }
        PT_TRY(write_instance_materials(s, changed, inst_material, range_table, &rewritten));

        // ---- the registry: flags and their scan, the count, then the compacted records ---------------------------------------------------
        PtRelightScene in;
        in.order = s->leaf_order.ptr;
        in.n_objects = s->n_objects;
        in.desc_ref = s->desc_ref_dev.ptr;
        in.n_desc_objects = s->n_desc_objects;
        in.n_desc_tris = s->n_desc_tris;
        in.recs = reinterpret_cast<const float4 *>(s->recs.ptr);
        in.spheres = reinterpret_cast<const float4 *>(s->spheres.ptr);
        in.sph_meta = s->sph_meta.ptr;
        in.tri_pos = s->tri_pos_kept.ptr;
        in.materials = reinterpret_cast<const float4 *>(d_materials.ptr);
        in.n_materials = n_materials;
        DevBuf<unsigned long long> ballots;
        DevBuf<uint32_t> block_first, counts, d_obj;
        DevBuf<float> d_prob;
        PT_HIP(ballots.ensure((static_cast<size_t>(s->n_objects) + 63) / 64));
        PT_HIP(block_first.ensure(pt_relight_blocks(s->n_objects)));
        PT_HIP(counts.ensure(2));
        EventPair timed;
        PT_HIP(timed.begin(s->stream));
        PT_HIP(pt_relight_flag(s->stream, in, ballots.ptr, block_first.ptr, counts.ptr));
        uint32_t h_counts[2] = {0, 0};
        PT_HIP(hipMemcpyAsync(h_counts, counts.ptr, sizeof(h_counts), hipMemcpyDeviceToHost, s->stream));
        PT_HIP(hipStreamSynchronize(s->stream));
        const uint32_t n_emissive = h_counts[0];
        n_candidates = h_counts[1];
        if(n_emissive > s->n_objects) {
            return fail(PT_ERR_HIP, "internal: the registry pass counted more emitters than the scene has objects");
        }
        object_sample_count = object_samples(n_emissive);
        if(n_lights + static_cast<uint32_t>(object_sample_count) > PT_MAX_NEE) {
            return fail(PT_ERR_UNSUPPORTED, "more than 32 light samples per path vertex (" + std::to_string(n_lights) + " point lights + " + std::to_string(object_sample_count) +
                                            " emitter samples): the visibility mask of a path vertex has 32 bits");
        }
        PT_HIP(d_emis.ensure(4 * static_cast<size_t>(n_emissive)));
        PT_HIP(d_prob.ensure(n_emissive));
        PT_HIP(d_obj.ensure(n_emissive));
        PT_HIP(d_cdf.ensure(n_emissive));
        cdf.resize(n_emissive);
        emissive_obj.resize(n_emissive);
        if(n_emissive > 0) {
            PT_HIP(pt_relight_emit(s->stream, in, ballots.ptr, block_first.ptr, reinterpret_cast<float4 *>(d_emis.ptr), d_prob.ptr, d_obj.ptr));
            PT_HIP(hipMemcpyAsync(cdf.data(), d_prob.ptr, n_emissive * sizeof(float), hipMemcpyDeviceToHost, s->stream));
            PT_HIP(hipMemcpyAsync(emissive_obj.data(), d_obj.ptr, n_emissive * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
        }
        PT_HIP(timed.end(s->stream));
        PT_HIP(hipStreamSynchronize(s->stream));
        PT_HIP(timed.ms(&registry_ms));
        {
            // the CDF (scene.cpp:167-180): a serial float chain in registration order, the division afterwards
            float cumulative_probability = 0.0F;
            for(float &v : cdf) {
                const float probability = v;
                v += cumulative_probability;
                cumulative_probability += probability;
            }
            for(float &v : cdf) {
                v /= cumulative_probability;
            }
        }
        if(n_emissive > 0) {
            PT_HIP(hipMemcpy(d_cdf.ptr, cdf.data(), n_emissive * sizeof(float), hipMemcpyHostToDevice));
        }
        put_back.armed = false;
    }

    // ---- adoption: nothing below fails but setup_path, which a scene of these counts has passed before ------------------------------------
    if(new_materials) {
        desc.materials.assign(materials, materials + n_materials);
        desc.d.materials = desc.materials.empty() ? nullptr : desc.materials.data();
        desc.d.n_materials = n_materials;
    }
    if(new_materials || rebuild) {
        take(s->materials, d_materials);
        s->dev.materials = reinterpret_cast<const float4 *>(s->materials.ptr);
        s->dev.n_materials = n_materials;
    }
    if(new_lights) {
        desc.light_pos.assign(look->light_pos, look->light_pos + 3 * static_cast<size_t>(n_lights));
        desc.light_spectrum.assign(look->light_spectrum, look->light_spectrum + 4 * static_cast<size_t>(n_lights));
        desc.d.light_pos = desc.light_pos.empty() ? nullptr : desc.light_pos.data();
        desc.d.light_spectrum = desc.light_spectrum.empty() ? nullptr : desc.light_spectrum.data();
        desc.d.n_point_lights = n_lights;
        take(s->lights, d_lights);
        s->dev.lights = reinterpret_cast<const float4 *>(s->lights.ptr);
        s->dev.n_lights = n_lights;
    }
    for(uint32_t i : changed) {
        keep.instances[i].material = inst_material[i];
    }
    if(rebuild) {
        s->n_emissive = static_cast<uint32_t>(cdf.size());
        s->emissive_obj = std::move(emissive_obj);
        s->emissive_cdf = std::move(cdf);
        take(s->emis, d_emis);
        take(s->emis_cdf, d_cdf);
        s->dev.emis = reinterpret_cast<const float4 *>(s->emis.ptr);
        s->dev.emis_cdf = s->emis_cdf.ptr;
        s->dev.n_emis = s->n_emissive;
        s->dev.n_object_samples = static_cast<uint32_t>(object_sample_count);
        // The emitter count may have crossed the kernel's table size and the slot word may have changed width: what create_scene and
        // setup_path derive from the counts is derived again, as behind a pose (pt_pose.cpp)
        stage_small_scene(s->dev);
        s->path_cfg = PtPathConfig{};
        s->path_blocks_per_cu = 0;
        s->path_slots = s->path_waves = s->path_cap = 0;
        s->host_path_args = PtPathArgs{};
        PT_TRY(setup_path(s));
    }

    const float total_ms = std::chrono::duration<float, std::milli>(clock::now() - t_begin).count();
    if(info != nullptr) {
        info->n_emissive = s->n_emissive;
        info->n_object_samples = s->dev.n_object_samples;
        info->n_candidates = n_candidates;
        info->registry_rebuilt = rebuild ? 1U : 0U;
        info->triangles_rewritten = rewritten;
        info->registry_ms = registry_ms;
        info->total_ms = total_ms;
    }
    if(env_int("PT_DEBUG", 0) != 0) {
        std::fprintf(stderr, "[pt] relight: registry %s, %u emitters of %u candidates, %u triangles rewritten; registry %.2f ms, total %.2f ms\n", rebuild ? "rebuilt" : "kept",
                     s->n_emissive, n_candidates, rewritten, registry_ms, total_ms);
    }
    return PT_OK;
}

} // extern "C"
