// pt_api.cpp -- host side of libpathtrace_hip.so: the C ABI of include/pt_hip.h.  This unit holds the calling thread's error message, the
// helpers every unit starts a call with, and scenes; render calls are in pt_render.cpp, resumable frames in pt_frames.cpp and
// pt_frame_maps.cpp, post-processing, features and denoising in pt_image.cpp (pt_host.h is what they share).
//
// Scene creation flattens the caller's object list into the HBM layout of pt_types.h (building the reference's BVH
// topology on the way, pt_bvh.cpp / pt_build.hip); a render call is ONE launch of the persistent path kernel (pt_path.hip), whose
// wavefronts render the call's streams until none is left.  There is no CPU rendering path in this library.
#include "pt_host.h"

namespace pth {

thread_local std::string g_last_error;

int fail(int code, const std::string &msg) {
    g_last_error = msg;
    return code;
}

const std::string &last_error() {
    return g_last_error;
}

int device_count_quiet() {
    int n = 0;
    if(hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

int check_device(int device) {
    const int n_dev = device_count_quiet();
    if(n_dev <= 0) {
        return fail(PT_ERR_NO_DEVICE, "no HIP device available; libpathtrace_hip has no CPU path");
    }
    if(device < 0 || device >= n_dev) {
        return fail(PT_ERR_NO_DEVICE, "device index out of range");
    }
    return PT_OK;
}

PtDevCamera derive_camera(const pt_camera_params *c) {
    // Camera::Camera, src/camera.cpp:53-76
    PtDevCamera cam{};
    const Vec3 origin = ld(c->origin);
    const Vec3 forward_dir = normalize(sub(ld(c->look_at), origin));
    const Vec3 forward = scale(forward_dir, c->focal_length);
    const Vec3 up_dir = normalize(ld(c->up));
    const float height_half = c->height / 2.0F;
    const Vec3 up = scale(up_dir, height_half);
    const Vec3 right_dir = normalize(cross(forward, up));
    const float width_half = height_half * c->aspect_ratio;
    const Vec3 right = scale(right_dir, width_half);
    const Vec3 v[4] = {origin, forward, up, right};
    float *dst[4] = {cam.origin, cam.forward, cam.up, cam.right};
    for(int i = 0; i < 4; i++) {
        dst[i][0] = v[i].x;
        dst[i][1] = v[i].y;
        dst[i][2] = v[i].z;
    }
    cam.aperture_width_half = c->aperture_width / 2.0F;
    cam.aperture_height_half = c->aperture_height / 2.0F;
    cam.aperture_kind = c->aperture_kind;
    cam.hex_ratio = fmin_std(fmax_std(c->hex_ratio, 0.0F), 1.0F); // camera.cpp:22-24
    cam.focal_plane_dist = c->focal_plane_dist;
    return cam;
}

int derive_options(const pt_options *o, PtDevOptions *out) {
    PtDevOptions d{};
    d.image_width = o->image_width;
    d.image_height = o->image_height;
    d.min_sample_count = o->min_sample_count;
    d.max_sample_count = o->max_sample_count;
    d.overlap_bound = o->max_sample_count;
    d.epsilon = o->epsilon;
    d.pixel_width = 1.0F / static_cast<float>(o->image_width);
    d.pixel_height = 1.0F / static_cast<float>(o->image_height);
    // worker.cpp:158-164
    d.stats_sample_count = std::min(std::max(o->min_sample_count / 4, 1), 64);
    d.candidate_batch_count = std::max(std::max(o->min_sample_count, o->max_sample_count / 4) / d.stats_sample_count, 2);
    d.check_sample_count =
      std::min(std::max({o->min_sample_count / 2, (o->max_sample_count - o->min_sample_count) / 8, 8, d.stats_sample_count}), 1024) / d.stats_sample_count;
    // closed candidates a pixel can accumulate (worker.cpp:214-222).  A candidate closes after candidate_batch_count batches and a pixel
    // has at most max / S of them.  candidate_batch_count is about max / (4 S), which would give 4, but both divisions truncate: max = 11
    // with min <= 2 gives batches of 1 sample, 2 batches per candidate and 11 batches, so 5 candidates close.  That is the most any pair
    // of options reaches (tests/test_shading_cases_cpu.py sweeps 0 <= min, max <= 4096), so the check below is a guard against a change of
    // the formulas above, not a limit a caller can reach (PT_MAX_CANDIDATES = 8).
    const int batches = std::max(o->max_sample_count, 0) / d.stats_sample_count;
    const int closed = batches > 0 ? (batches - 1) / d.candidate_batch_count : 0;
    if(closed > PT_MAX_CANDIDATES) {
        return fail(PT_ERR_UNSUPPORTED, "internal: the estimator's constants allow more than 8 closed candidates per pixel (worker.cpp:158-164 give at most 5)");
    }
    *out = d;
    return PT_OK;
}

int check_render_args(pt_scene *scene, const pt_camera_params *camera, const pt_options *options) {
    if(scene == nullptr || camera == nullptr || options == nullptr) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    if(options->image_width <= 0 || options->image_height <= 0) {
        return fail(PT_ERR_INVALID, "image size must be positive");
    }
    return PT_OK;
}

bool builds_on_device(uint32_t n_objects) {
    // PT_BUILD=device | host forces one; by default scenes of 1024 objects or more are built on the device (pt_build.hip) and smaller
    // ones by the host recursion (pt_bvh.cpp).  Both produce the same arrays, bit for bit.
    bool use_device = n_objects >= static_cast<uint32_t>(std::max(env_int("PT_BUILD_DEVICE_MIN", 1024), 2));
    if(const char *mode = std::getenv("PT_BUILD")) {
        if(std::strcmp(mode, "host") == 0) {
            use_device = false;
        }
        else if(std::strcmp(mode, "device") == 0) {
            use_device = n_objects >= 2;
        }
    }
    return use_device;
}

} // namespace pth

using namespace pth;

extern "C" {

int pt_device_count(void) {
    return device_count_quiet();
}

const char *pt_last_error(void) {
    return last_error().c_str();
}

uint64_t pt_pixel_seed(uint64_t base_seed, int32_t x, int32_t y) {
    // splitmix64 finaliser over (base_seed, x, y); the device computes the same (pt_shading.h pixel_seed)
    uint64_t z = base_seed + 0x9E3779B97F4A7C15ULL * (1ULL + (static_cast<uint64_t>(static_cast<uint32_t>(y)) << 32) + static_cast<uint64_t>(static_cast<uint32_t>(x)));
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

uint64_t pt_rng_seed_to_state(uint64_t seed) {
    return seed ^ (~seed << 32);
}

size_t pt_job_tiles(int32_t image_width, int32_t image_height, pt_tile *out, size_t capacity) {
    // processJob, src/worker.cpp:389-414
    const int width = std::max(image_width, 0);
    const int height = std::max(image_height, 0);
    if(width == 0 || height == 0) {
        return 0;
    }
    const int tile_size = std::max(std::min(std::min(width, height) / 4, 32), 1);
    const int horizontal_tiles = (width + (tile_size - 1)) / tile_size;
    const int vertical_tiles = (height + (tile_size - 1)) / tile_size;
    size_t n = 0;
    for(int ty = 0; ty < vertical_tiles; ty++) {
        for(int tx = 0; tx < horizontal_tiles; tx++) {
            if(out != nullptr && n < capacity) {
                const int ox = tx * tile_size, oy = ty * tile_size;
                out[n] = pt_tile{ox, oy, std::min(width - ox, tile_size), std::min(height - oy, tile_size)};
            }
            n++;
        }
    }
    return n;
}

int pt_scene_create(int device, const pt_scene_desc *d, pt_scene **out) {
    return create_scene(device, d, nullptr, out);
}

} // extern "C"

namespace pth {

std::vector<F4> material_table(const pt_material *materials, uint32_t n) {
    std::vector<F4> table(4 * static_cast<size_t>(n));
    for(uint32_t i = 0; i < n; i++) {
        const pt_material &m = materials[i];
        table[4 * static_cast<size_t>(i) + 0] = {m.diffuse[0], m.diffuse[1], m.diffuse[2], m.diffuse[3]};
        table[4 * static_cast<size_t>(i) + 1] = {m.specular[0], m.specular[1], m.specular[2], m.specular[3]};
        table[4 * static_cast<size_t>(i) + 2] = {m.emission[0], m.emission[1], m.emission[2], m.emission[3]};
        table[4 * static_cast<size_t>(i) + 3] = {m.ior, from_bits(static_cast<uint32_t>(m.bsdf)), from_bits(static_cast<uint32_t>(m.one_way != 0)), 0.0F};
    }
    return table;
}

std::vector<F4> light_table(const float *pos, const float *spectrum, uint32_t n) {
    std::vector<F4> table(2 * static_cast<size_t>(n));
    for(uint32_t i = 0; i < n; i++) {
        const float *p = pos + 3 * static_cast<size_t>(i);
        const float *c = spectrum + 4 * static_cast<size_t>(i);
        table[2 * static_cast<size_t>(i) + 0] = {p[0], p[1], p[2], 0.0F};
        table[2 * static_cast<size_t>(i) + 1] = {c[0], c[1], c[2], c[3]};
    }
    return table;
}

int object_samples(uint32_t n_emissive) {
    const int emissive_object_count = static_cast<int>(n_emissive);
    return std::min(2 + static_cast<int>(std::log10(emissive_object_count + 1)), emissive_object_count); // scene.cpp:226
}

void stage_small_scene(PtDevScene &dev) {
    // LDS staging: a scene whose whole tree and leaf records fit in LDS NEXT TO everything else a workgroup keeps there, four workgroups
    // to the CU, lives in LDS entirely (the path kernel's IN_LDS variant): up to 15.8 KB of records with the small stack window, i.e. about
    // 120 triangles.  Larger ones are read through the caches like any tree: staged at three workgroups per CU they are slower than that
    // (176 triangles: 754 against 785 Msamples/s; at two, 256 triangles: 581 against 715 -- profiles/r03_lds_threshold.txt; round 2 staged up to
    // 24 KB).  An LDS copy of only the top of a larger tree was measured in round 1 and does not pay.  PT_LDS_SMALL_BYTES overrides the limit.
    const size_t small_bytes = (static_cast<size_t>(dev.n_pairs) + dev.pair_base) * 64;
    const int wide_word = dev.n_lights + dev.n_object_samples > 8U ? 1 : 0;
    const size_t other_lds = pt_path_lds_bytes(wide_word, std::min(std::max(env_int("PT_ROWS", 4), 1), PT_MAX_ROWS), 4, 0U, 0U);
    const size_t room = other_lds < 40960 ? 40960 - other_lds : 0;
    if(small_bytes <= static_cast<size_t>(std::max(env_int("PT_LDS_SMALL_BYTES", static_cast<int>(room)), 0)) && env_int("PT_LDS_SMALL", 1) != 0) {
        dev.n_lds_pairs = dev.n_pairs;
        dev.n_lds_tris = dev.n_tris;
    }
    else {
        dev.n_lds_pairs = 0;
        dev.n_lds_tris = 0;
    }
}

} // namespace pth

int pth::create_scene(int device, const pt_scene_desc *d, const DeviceTriangles *assembled, pt_scene **out) {
    if(d == nullptr || out == nullptr) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    *out = nullptr;
    const int device_rc = check_device(device);
    if(device_rc != PT_OK) {
        return device_rc;
    }
    if(d->n_objects != d->n_triangles + d->n_spheres) {
        return fail(PT_ERR_INVALID, "n_objects must equal n_triangles + n_spheres");
    }
    if((d->n_objects > 0 && d->obj_kind == nullptr) || (d->n_triangles > 0 && (d->tri_pos == nullptr || d->tri_cull == nullptr || d->tri_material == nullptr)) ||
       (d->n_spheres > 0 && (d->sph == nullptr || d->sph_material == nullptr)) || (d->n_materials > 0 && d->materials == nullptr) ||
       (d->n_point_lights > 0 && (d->light_pos == nullptr || d->light_spectrum == nullptr))) {
        return fail(PT_ERR_INVALID, "missing array in scene description");
    }
    if(d->n_triangles > PT_REF_INDEX || d->n_spheres > PT_REF_INDEX) {
        return fail(PT_ERR_UNSUPPORTED, "too many objects");
    }
    // all triangles and objects: the description's, and behind them those of the mesh instances (object d->n_objects + k is triangle
    // d->n_triangles + k)
    const uint32_t n_tris = assembled != nullptr ? assembled->n_triangles : d->n_triangles;
    const uint32_t n_objs = d->n_objects + (n_tris - d->n_triangles);
    if(n_tris < d->n_triangles || n_tris > PT_REF_INDEX) {
        return fail(PT_ERR_UNSUPPORTED, "too many objects");
    }

    std::unique_ptr<pt_scene> s(new pt_scene());
    s->device = device;
    PT_HIP(hipSetDevice(device));
    hipDeviceProp_t prop;
    PT_HIP(hipGetDeviceProperties(&prop, device));
    s->cu_count = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    PT_HIP(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
    if(assembled != nullptr && assembled->ready != nullptr) {
        PT_HIP(hipStreamWaitEvent(s->stream, assembled->ready, 0)); // (the arrays are being finished on the assembly's stream)
    }
    s->n_objects = n_objs;
    s->n_desc_objects = d->n_objects;
    s->n_desc_tris = d->n_triangles;

    using clock = std::chrono::steady_clock;
    const auto t_begin = clock::now();
    auto ms_since = [](clock::time_point t0) { return std::chrono::duration<float, std::milli>(clock::now() - t0).count(); };

    // ---- objects in construction order: typed indices and the reference word of every leaf ---------------------------------
    std::vector<uint32_t> leaf_ref(d->n_objects);
    s->tri_obj.resize(d->n_triangles);
    s->sph_obj.resize(d->n_spheres);
    {
        uint32_t ti = 0, si = 0;
        for(uint32_t i = 0; i < d->n_objects; i++) {
            if(d->obj_kind[i] == PT_OBJ_TRIANGLE) {
                if(ti >= d->n_triangles) {
                    return fail(PT_ERR_INVALID, "obj_kind lists more triangles than n_triangles");
                }
                leaf_ref[i] = PT_REF_LEAF | ti;
                s->tri_obj[ti] = i;
                if(d->tri_material[ti] != PT_NO_MATERIAL && d->tri_material[ti] >= d->n_materials) {
                    return fail(PT_ERR_INVALID, "triangle material index out of range");
                }
                ti++;
            }
            else if(d->obj_kind[i] == PT_OBJ_SPHERE) {
                if(si >= d->n_spheres) {
                    return fail(PT_ERR_INVALID, "obj_kind lists more spheres than n_spheres");
                }
                leaf_ref[i] = PT_REF_LEAF | PT_REF_SPHERE | si;
                s->sph_obj[si] = i;
                if(d->sph_material[si] != PT_NO_MATERIAL && d->sph_material[si] >= d->n_materials) {
                    return fail(PT_ERR_INVALID, "sphere material index out of range");
                }
                si++;
            }
            else {
                return fail(PT_ERR_INVALID, "unknown object kind");
            }
        }
    }
    s->n_nodes = n_objs > 0 ? 2ULL * n_objs - 1ULL : 0ULL;

    // Where the tree is built (builds_on_device)
    const bool use_device = builds_on_device(n_objs);
    if(assembled != nullptr && !use_device) {
        return fail(PT_ERR_INVALID, "internal: triangles in device memory need the device builder");
    }
    s->device_built = use_device;
    const bool align_siblings = env_int("PT_ALIGN_SIBLINGS", 1) != 0;

    std::vector<int32_t> dfs; // leaves depth-first, left to right (Scene::registerEmissiveObjects order); device path: only those with an emissive material
    uint32_t n_pairs = 0, root_ref = PT_REF_NONE;
    float root_lo[3] = {0, 0, 0}, root_hi[3] = {0, 0, 0};
    if(use_device) {
        // ---- device: upload the caller's arrays as they are; records, leaf boxes and the tree are made in HBM ----------------------
        s->build_ms[0] = ms_since(t_begin);
        const auto t_upload = clock::now();
        DevBuf<float> raw_pos, raw_nrm, raw_sph;
        DevBuf<uint8_t> raw_cull;
        DevBuf<uint32_t> raw_tri_mat, raw_tri_obj, raw_sph_mat, raw_sph_obj;
        auto up = [](auto &buf, const auto *src, size_t count) -> hipError_t {
            hipError_t e = buf.ensure(count);
            if(e != hipSuccess || count == 0) {
                return e;
            }
            return hipMemcpy(buf.ptr, src, count * sizeof(*src), hipMemcpyHostToDevice);
        };
        if(assembled == nullptr) {
            PT_HIP(up(raw_pos, d->tri_pos, 9 * static_cast<size_t>(d->n_triangles)));
            if(d->tri_nrm != nullptr) {
                PT_HIP(up(raw_nrm, d->tri_nrm, 9 * static_cast<size_t>(d->n_triangles)));
            }
        }
        else {
            // positions and normals are in HBM already; the three small arrays get room for the instances' triangles behind the description's
            PT_HIP(raw_cull.ensure(n_tris));
            PT_HIP(raw_tri_mat.ensure(n_tris));
            PT_HIP(raw_tri_obj.ensure(n_tris));
        }
        PT_HIP(up(raw_cull, d->tri_cull, d->n_triangles));
        PT_HIP(up(raw_tri_mat, d->tri_material, d->n_triangles));
        PT_HIP(up(raw_tri_obj, s->tri_obj.data(), d->n_triangles));
        PT_HIP(up(raw_sph, d->sph, 4 * static_cast<size_t>(d->n_spheres)));
        PT_HIP(up(raw_sph_mat, d->sph_material, d->n_spheres));
        PT_HIP(up(raw_sph_obj, s->sph_obj.data(), d->n_spheres));
        if(assembled != nullptr) {
            // the instances' triangles: one launch for all ranges (pt_mesh_batch.h)
            PT_HIP(pt_mesh_batch_fill_ranges(s->stream, *assembled->scratch, assembled->ranges.data(), static_cast<uint32_t>(assembled->ranges.size()), d->n_triangles,
                                             n_tris - d->n_triangles, d->n_objects, raw_cull.ptr, raw_tri_mat.ptr, raw_tri_obj.ptr));
        }
        PT_HIP(s->tris.ensure(PT_TRI_QUADS * (static_cast<size_t>(n_tris) + 1 + d->n_spheres))); // triangles, a spare record, spheres (pt_types.h)
        PT_HIP(hipMemsetAsync(s->tris.ptr + PT_TRI_QUADS * static_cast<size_t>(n_tris), 0, PT_TRI_QUADS * sizeof(F4), s->stream));
        PT_HIP(s->tri_shade.ensure(8 * static_cast<size_t>(n_tris)));
        PT_HIP(s->spheres.ensure(d->n_spheres));
        PT_HIP(s->sph_meta.ensure(d->n_spheres));
        s->build_ms[1] = ms_since(t_upload);

        PtBuildInput in;
        in.n_objects = n_objs;
        in.n_triangles = n_tris;
        in.n_spheres = d->n_spheres;
        in.tri_pos = assembled != nullptr ? assembled->pos : raw_pos.ptr;
        in.tri_nrm = assembled != nullptr ? assembled->nrm : (d->tri_nrm != nullptr ? raw_nrm.ptr : nullptr);
        in.tri_cull = raw_cull.ptr;
        in.tri_material = raw_tri_mat.ptr;
        in.tri_obj = raw_tri_obj.ptr;
        in.sph = raw_sph.ptr;
        in.sph_material = raw_sph_mat.ptr;
        in.sph_obj = raw_sph_obj.ptr;
        in.align_siblings = align_siblings;
        PtBuildOutput built;
        built.tris = reinterpret_cast<float4 *>(s->tris.ptr);
        built.tri_shade = reinterpret_cast<float4 *>(s->tri_shade.ptr);
        built.spheres = reinterpret_cast<float4 *>(s->spheres.ptr);
        built.sph_meta = s->sph_meta.ptr;
        const char *what = "";
        const hipError_t e = pt_build_scene_device(s->stream, in, built, &what);
        if(e != hipSuccess) {
            return fail(PT_ERR_HIP, std::string("device scene build (") + what + "): " + hipGetErrorString(e));
        }
        s->pairs.ptr = reinterpret_cast<F4 *>(built.pairs);
        s->pairs.count = 4 * static_cast<size_t>(built.n_pairs);
        DevBuf<uint32_t> dfs_dev;
        dfs_dev.ptr = built.dfs;
        dfs_dev.count = n_objs;
        s->build_ms[2] = built.build_ms;
        s->depth = built.depth;
        if(s->depth > PT_MAX_DEPTH) {
            return fail(PT_ERR_UNSUPPORTED, "internal: BVH deeper than 128 levels (impl::constructBVH keeps a child at two thirds of its parent at most: 53 levels for 2^30 objects; tests/test_oracle_golden.py)");
        }
        n_pairs = built.n_pairs;
        root_ref = built.root_ref;
        for(int k = 0; k < 3; k++) {
            root_lo[k] = built.root_lo[k];
            root_hi[k] = built.root_hi[k];
        }
        // Only objects with an emissive material matter to registerEmissiveObjects: pick them out in construction order on the
        // host (sequential reads) and let the device put them into depth-first order.
        std::vector<uint8_t> lit(d->n_materials, 0);
        bool any_lit = false;
        for(uint32_t m = 0; m < d->n_materials; m++) {
            const float *e = d->materials[m].emission;
            lit[m] = (e[0] + e[1] + e[2]) * e[3] > 0.0F ? 1 : 0;
            any_lit = any_lit || lit[m] != 0;
        }
        if(any_lit) {
            std::vector<uint32_t> mask((static_cast<size_t>(n_objs) + 31) / 32, 0U);
            uint32_t n_selected = 0;
            for(uint32_t t = 0; t < d->n_triangles; t++) {
                const uint32_t m = d->tri_material[t];
                if(m != PT_NO_MATERIAL && lit[m] != 0) {
                    const uint32_t o = s->tri_obj[t];
                    mask[o >> 5] |= 1U << (o & 31U);
                    n_selected++;
                }
            }
            for(uint32_t i = 0; i < d->n_spheres; i++) {
                const uint32_t m = d->sph_material[i];
                if(m != PT_NO_MATERIAL && lit[m] != 0) {
                    const uint32_t o = s->sph_obj[i];
                    mask[o >> 5] |= 1U << (o & 31U);
                    n_selected++;
                }
            }
            if(assembled != nullptr) {
                // an instance has one material: a lit one selects its whole range of objects
                for(const PtBatchRange &r : assembled->ranges) {
                    if(r.material != PT_NO_MATERIAL && lit[r.material] != 0) {
                        const uint32_t first = d->n_objects + (r.first_tri - d->n_triangles);
                        for(uint32_t o = first; o < first + r.count; o++) {
                            mask[o >> 5] |= 1U << (o & 31U);
                        }
                        n_selected += r.count;
                    }
                }
            }
            std::vector<uint32_t> ordered;
            PT_HIP(pt_build_order_subset(s->stream, dfs_dev.ptr, n_objs, mask, n_selected, ordered));
            dfs.assign(ordered.begin(), ordered.end());
        }
        if(assembled != nullptr) {
            take(s->leaf_order, dfs_dev); // (a scene with mesh instances keeps the order: pt_scene_relight's registry pass walks it)
        }
    }
    else {
        // ---- host: leaf boxes, the recursion of pt_bvh.cpp, breadth-first flattening, records -----------------------------------
        std::vector<ptb::Box> boxes(d->n_objects);
        for(uint32_t i = 0; i < d->n_objects; i++) {
            ptb::Box &b = boxes[i];
            const uint32_t idx = leaf_ref[i] & PT_REF_INDEX;
            if((leaf_ref[i] & PT_REF_SPHERE) == 0) {
                const float *p = d->tri_pos + 9 * static_cast<size_t>(idx);
                for(int k = 0; k < 3; k++) { // Triangle::getBoundingVolume, object.cpp:184-186
                    b.lo[k] = fmin_std(fmin_std(p[k], p[3 + k]), p[6 + k]);
                    b.hi[k] = fmax_std(fmax_std(p[k], p[3 + k]), p[6 + k]);
                }
            }
            else {
                const float *sp = d->sph + 4 * static_cast<size_t>(idx);
                for(int k = 0; k < 3; k++) { // Sphere::getBoundingVolume, object.cpp:90-93
                    b.lo[k] = sp[k] - sp[3];
                    b.hi[k] = sp[k] + sp[3];
                }
            }
        }
        int threads = env_int("PT_BUILD_THREADS", static_cast<int>(std::thread::hardware_concurrency()));
        threads = std::max(1, std::min(threads, 64));
        s->tree = ptb::build_reference_bvh(boxes, threads);
        s->depth = s->tree.depth;
        if(s->depth > PT_MAX_DEPTH) {
            return fail(PT_ERR_UNSUPPORTED, "internal: BVH deeper than 128 levels (impl::constructBVH keeps a child at two thirds of its parent at most: 53 levels for 2^30 objects; tests/test_oracle_golden.py)");
        }
        ptb::FlatBvh flat = ptb::flatten_breadth_first(s->tree, leaf_ref, align_siblings);
        n_pairs = flat.n_pairs;
        root_ref = flat.root_ref;
        for(int k = 0; k < 3; k++) {
            root_lo[k] = flat.root_box.lo[k];
            root_hi[k] = flat.root_box.hi[k];
        }
        ptb::leaves_depth_first(s->tree, dfs);
        s->build_ms[0] = ms_since(t_begin);
        const auto t_upload = clock::now();

        std::vector<F4> tris(PT_TRI_QUADS * (static_cast<size_t>(d->n_triangles) + 1 + d->n_spheres), F4{0.0F, 0.0F, 0.0F, 0.0F}), shade(8 * static_cast<size_t>(d->n_triangles), F4{0.0F, 0.0F, 0.0F, 0.0F});
        for(uint32_t t = 0; t < d->n_triangles; t++) {
            const float *p = d->tri_pos + 9 * static_cast<size_t>(t);
            const Vec3 a = ld(p), b = ld(p + 3), c = ld(p + 6);
            const Vec3 ab = sub(b, a), ac = sub(c, a);
            const uint32_t obj_cull = s->tri_obj[t] | (d->tri_cull[t] != 0 ? 0x80000000U : 0U);
            tris[PT_TRI_QUADS * static_cast<size_t>(t) + 0] = {a.x, a.y, a.z, ab.x};
            tris[PT_TRI_QUADS * static_cast<size_t>(t) + 1] = {ab.y, ab.z, ac.x, ac.y};
            tris[PT_TRI_QUADS * static_cast<size_t>(t) + 2] = {ac.z, from_bits(d->tri_material[t]), from_bits(obj_cull), 0.0F};
            Vec3 na, nb, nc;
            if(d->tri_nrm != nullptr) {
                const float *q = d->tri_nrm + 9 * static_cast<size_t>(t);
                na = ld(q);
                nb = ld(q + 3);
                nc = ld(q + 6);
            }
            else {
                na = nb = nc = normalize(cross(ab, ac)); // Triangle::Triangle, object.cpp:118-124
            }
            for(int k = 0; k < 3; k++) {
                shade[8 * static_cast<size_t>(t) + k] = tris[PT_TRI_QUADS * static_cast<size_t>(t) + k];
            }
            shade[8 * static_cast<size_t>(t) + 3] = {na.x, na.y, na.z, nb.x};
            shade[8 * static_cast<size_t>(t) + 4] = {nb.y, nb.z, nc.x, nc.y};
            shade[8 * static_cast<size_t>(t) + 5] = {nc.z, 0.0F, 0.0F, 0.0F};
        }
        std::vector<F4> spheres(d->n_spheres);
        std::vector<uint2> sph_meta(d->n_spheres);
        for(uint32_t i = 0; i < d->n_spheres; i++) {
            const float *sp = d->sph + 4 * static_cast<size_t>(i);
            spheres[i] = {sp[0], sp[1], sp[2], sp[3]};
            tris[PT_TRI_QUADS * (static_cast<size_t>(d->n_triangles) + 1 + i)] = spheres[i]; // the record the traversal fetches (pt_types.h)
            sph_meta[i] = make_uint2(d->sph_material[i], s->sph_obj[i]);
        }
        std::vector<F4> pairs(4 * static_cast<size_t>(flat.n_pairs));
        std::memcpy(pairs.data(), flat.pairs.data(), flat.pairs.size() * sizeof(float));
        PT_HIP(s->pairs.upload(pairs));
        PT_HIP(s->tris.upload(tris));
        PT_HIP(s->tri_shade.upload(shade));
        PT_HIP(s->spheres.upload(spheres));
        PT_HIP(s->sph_meta.upload(sph_meta));
        s->build_ms[1] = ms_since(t_upload);
    }
    const auto t_rest = clock::now();

    for(uint32_t i = 0; i < d->n_materials; i++) {
        if(d->materials[i].bsdf < PT_BSDF_LAMBERTIAN || d->materials[i].bsdf > PT_BSDF_MIRROR) {
            return fail(PT_ERR_INVALID, "unknown BSDF kind");
        }
    }
    const std::vector<F4> materials = material_table(d->materials, d->n_materials);
    const std::vector<F4> lights = light_table(d->light_pos, d->light_spectrum, d->n_point_lights);

    // ---- emissive objects: Scene::registerEmissiveObjects + CDF (scene.cpp:183-208, 167-180) -----------------------------------
    std::vector<F4> emis;
    std::vector<float> cdf;
    const float pi = static_cast<float>(M_PI);
    // the positions of the candidates among the instances' triangles (all of them have a lit material) are gathered on the device: E records, not n
    std::vector<float> gathered;
    if(assembled != nullptr) {
        std::vector<uint32_t> wanted;
        for(int32_t obj : dfs) {
            if(static_cast<uint32_t>(obj) >= d->n_objects) {
                wanted.push_back(d->n_triangles + (static_cast<uint32_t>(obj) - d->n_objects));
            }
        }
        if(!wanted.empty()) {
            DevBuf<uint32_t> wanted_dev;
            DevBuf<float> gathered_dev;
            PT_HIP(wanted_dev.upload(wanted));
            PT_HIP(gathered_dev.ensure(9 * wanted.size()));
            PT_HIP(pt_mesh_gather_pos(s->stream, assembled->pos, wanted_dev.ptr, static_cast<uint32_t>(wanted.size()), gathered_dev.ptr));
            gathered.resize(9 * wanted.size());
            PT_HIP(hipMemcpyAsync(gathered.data(), gathered_dev.ptr, gathered.size() * sizeof(float), hipMemcpyDeviceToHost, s->stream));
            PT_HIP(hipStreamSynchronize(s->stream));
        }
    }
    size_t next_gathered = 0;
    for(int32_t obj : dfs) {
        const bool of_instance = static_cast<uint32_t>(obj) >= d->n_objects;
        const uint32_t ref = of_instance ? (PT_REF_LEAF | (d->n_triangles + (static_cast<uint32_t>(obj) - d->n_objects))) : leaf_ref[obj];
        const uint32_t idx = ref & PT_REF_INDEX;
        const bool is_sphere = (ref & PT_REF_SPHERE) != 0;
        const PtBatchRange *range = nullptr;
        const float *tri_p = nullptr; // the triangle's nine coordinates
        if(of_instance) {
            range = &*(std::upper_bound(assembled->ranges.begin(), assembled->ranges.end(), idx, [](uint32_t t, const PtBatchRange &r) { return t < r.first_tri; }) - 1);
            tri_p = gathered.data() + 9 * next_gathered++;
        }
        else if(!is_sphere) {
            tri_p = d->tri_pos + 9 * static_cast<size_t>(idx);
        }
        const uint32_t mat = of_instance ? range->material : (is_sphere ? d->sph_material[idx] : d->tri_material[idx]);
        if(mat == PT_NO_MATERIAL) {
            continue; // default material has no emission
        }
        const float *e = d->materials[mat].emission;
        const float emissive_power = (e[0] + e[1] + e[2]) * e[3];
        if(emissive_power <= 0.0F) {
            continue;
        }
        float area;
        if(is_sphere) {
            const float r = d->sph[4 * static_cast<size_t>(idx) + 3];
            area = 4.0F * pi * (r * r); // object.cpp:95-99
        }
        else {
            const float *p = tri_p;
            const Vec3 c = cross(sub(ld(p + 3), ld(p)), sub(ld(p + 6), ld(p)));
            area = std::sqrt(dot(c, c)) / 2.0F; // object.cpp:188-190
        }
        const float object_probability = emissive_power * area;
        if(object_probability <= 0.0F) {
            continue;
        }
        if(is_sphere) {
            const float *sp = d->sph + 4 * static_cast<size_t>(idx);
            emis.push_back({sp[0], sp[1], sp[2], sp[3]});
            emis.push_back({0.0F, 0.0F, 0.0F, 0.0F});
            emis.push_back({0.0F, from_bits(ref), 0.0F, from_bits(mat)});
        }
        else {
            const float *p = tri_p;
            const bool cull = of_instance ? range->cull != 0 : d->tri_cull[idx] != 0;
            emis.push_back({p[0], p[1], p[2], p[3]});
            emis.push_back({p[4], p[5], p[6], p[7]});
            emis.push_back({p[8], from_bits(ref), from_bits(cull ? 1U : 0U), from_bits(mat)});
        }
        emis.push_back({e[0], e[1], e[2], e[3]});
        cdf.push_back(object_probability);
        s->emissive_obj.push_back(obj);
    }
    {
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
    s->n_emissive = static_cast<uint32_t>(cdf.size());
    s->emissive_cdf = cdf;
    const int object_sample_count = object_samples(s->n_emissive);
    if(d->n_point_lights + static_cast<uint32_t>(object_sample_count) > PT_MAX_NEE) {
        return fail(PT_ERR_UNSUPPORTED, "more than 32 light samples per path vertex (" + std::to_string(d->n_point_lights) + " point lights + " + std::to_string(object_sample_count) +
                                        " emitter samples): the visibility mask of a path vertex has 32 bits");
    }

    // ---- upload --------------------------------------------------------------------------------------------------------------
    PT_HIP(s->materials.upload(materials));
    PT_HIP(s->lights.upload(lights));
    PT_HIP(s->emis.upload(emis));
    PT_HIP(s->emis_cdf.upload(cdf));

    // ---- link: leaf records and pair records become ONE array, and the tree's references indices into it (pt_types.h) --------------
    // (the pair records start on an even record: two sibling nodes on slots 2k, 2k + 1 share one aligned 128-byte line only then)
    const uint32_t sphere_base = n_tris + 1U, leaf_count = sphere_base + d->n_spheres, pair_base = (leaf_count + 1U) & ~1U;
    if(static_cast<uint64_t>(pair_base) + n_pairs > PT_REF_INDEX) {
        return fail(PT_ERR_UNSUPPORTED, "too many records for 30-bit references");
    }
    PT_HIP(s->recs.ensure(4 * (static_cast<size_t>(pair_base) + n_pairs)));
    PT_HIP(hipMemcpyAsync(s->recs.ptr, s->tris.ptr, 4 * static_cast<size_t>(leaf_count) * sizeof(F4), hipMemcpyDeviceToDevice, s->stream));
    if(pair_base > leaf_count) {
        PT_HIP(hipMemsetAsync(s->recs.ptr + 4 * static_cast<size_t>(leaf_count), 0, 4 * sizeof(F4), s->stream));
    }
    if(n_pairs > 0) {
        PT_HIP(hipMemcpyAsync(s->recs.ptr + 4 * static_cast<size_t>(pair_base), s->pairs.ptr, 4 * static_cast<size_t>(n_pairs) * sizeof(F4), hipMemcpyDeviceToDevice, s->stream));
        PT_HIP(pt_link_records(s->stream, reinterpret_cast<float4 *>(s->recs.ptr), pair_base, n_pairs, sphere_base));
    }
    PT_HIP(hipStreamSynchronize(s->stream));
    s->tris.release();
    s->pairs.release();
    if(root_ref != PT_REF_NONE) {
        root_ref += (root_ref & PT_REF_LEAF) == 0 ? pair_base : ((root_ref & PT_REF_SPHERE) != 0 ? sphere_base : 0U);
    }

    PtDevScene &dev = s->dev;
    dev.recs = reinterpret_cast<const float4 *>(s->recs.ptr);
    dev.pairs = dev.recs + 4 * static_cast<size_t>(pair_base);
    dev.tris = dev.recs;
    dev.pair_base = pair_base;
    dev.tri_shade = reinterpret_cast<const float4 *>(s->tri_shade.ptr);
    dev.spheres = reinterpret_cast<const float4 *>(s->spheres.ptr);
    dev.sph_meta = s->sph_meta.ptr;
    dev.materials = reinterpret_cast<const float4 *>(s->materials.ptr);
    dev.lights = reinterpret_cast<const float4 *>(s->lights.ptr);
    dev.emis = reinterpret_cast<const float4 *>(s->emis.ptr);
    dev.emis_cdf = s->emis_cdf.ptr;
    for(int k = 0; k < 3; k++) {
        dev.root_lo[k] = root_lo[k];
        dev.root_hi[k] = root_hi[k];
    }
    dev.root_ref = root_ref;
    dev.n_pairs = n_pairs;
    dev.n_tris = n_tris;
    dev.n_spheres = d->n_spheres;
    dev.n_lights = d->n_point_lights;
    dev.n_emis = s->n_emissive;
    dev.n_materials = d->n_materials;
    dev.n_object_samples = static_cast<uint32_t>(object_sample_count);
    stage_small_scene(dev);

    int rc = setup_path(s.get());
    if(rc != PT_OK) {
        return rc;
    }
    s->build_ms[3] = ms_since(t_rest);
    if(env_int("PT_DEBUG", 0) != 0) {
        std::fprintf(stderr, "[pt] scene build (%s): %u objects, %u pair records, depth %u; host preparation %.1f ms, upload %.1f ms, device tree %.1f ms, rest %.1f ms\n",
                     s->device_built ? "device" : "host", n_objs, n_pairs, s->depth, s->build_ms[0], s->build_ms[1], s->build_ms[2], s->build_ms[3]);
    }
    *out = s.release();
    return PT_OK;
}

extern "C" {

void pt_scene_destroy(pt_scene *scene) {
    if(scene == nullptr) {
        return;
    }
    (void)hipSetDevice(scene->device);
    if(scene->stream != nullptr) {
        (void)hipStreamSynchronize(scene->stream);
    }
    delete scene;
}

int pt_scene_info(const pt_scene *scene, uint64_t *n_nodes, uint32_t *depth, uint32_t *n_emissive) {
    if(scene == nullptr) {
        return fail(PT_ERR_INVALID, "null scene");
    }
    if(n_nodes != nullptr) {
        *n_nodes = scene->n_nodes;
    }
    if(depth != nullptr) {
        *depth = scene->depth;
    }
    if(n_emissive != nullptr) {
        *n_emissive = scene->n_emissive;
    }
    return PT_OK;
}

int pt_scene_emissive(const pt_scene *scene, int32_t *out_obj, float *out_cdf, uint64_t capacity, uint64_t *n_written) {
    if(scene == nullptr) {
        return fail(PT_ERR_INVALID, "null scene");
    }
    const uint64_t n = std::min<uint64_t>(scene->emissive_obj.size(), capacity);
    for(uint64_t i = 0; i < n; i++) {
        if(out_obj != nullptr) {
            out_obj[i] = scene->emissive_obj[i];
        }
        if(out_cdf != nullptr) {
            out_cdf[i] = scene->emissive_cdf[i];
        }
    }
    if(n_written != nullptr) {
        *n_written = scene->emissive_obj.size();
    }
    return PT_OK;
}

int pt_scene_bvh_dump(const pt_scene *scene, int32_t *out_obj, float *out_box, uint64_t capacity, uint64_t *n_written) {
    if(scene == nullptr || out_obj == nullptr || out_box == nullptr) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    std::vector<int32_t> obj;
    std::vector<ptb::Box> box;
    if(!scene->device_built) {
        ptb::dump_preorder(scene->tree, obj, box);
    }
    else {
        // rebuild the pre-order listing from the pair records in HBM
        const uint32_t pair_base = scene->dev.pair_base, sphere_base = scene->dev.n_tris + 1U;
        std::vector<F4> pairs(4 * static_cast<size_t>(scene->dev.n_pairs));
        if(hipSetDevice(scene->device) != hipSuccess ||
           hipMemcpy(pairs.data(), scene->dev.pairs, pairs.size() * sizeof(F4), hipMemcpyDeviceToHost) != hipSuccess) {
            return fail(PT_ERR_HIP, "downloading the pair records failed");
        }
        struct Item {
            uint32_t ref;
            ptb::Box box;
        };
        ptb::Box root;
        for(int k = 0; k < 3; k++) {
            root.lo[k] = scene->dev.root_lo[k];
            root.hi[k] = scene->dev.root_hi[k];
        }
        std::vector<Item> stack{{scene->dev.root_ref, root}};
        obj.reserve(scene->n_nodes);
        box.reserve(scene->n_nodes);
        while(!stack.empty()) {
            const Item it = stack.back();
            stack.pop_back();
            box.push_back(it.box);
            if((it.ref & PT_REF_LEAF) != 0) {
                const uint32_t idx = it.ref & PT_REF_INDEX; // (record indices: pt_types.h)
                obj.push_back(static_cast<int32_t>((it.ref & PT_REF_SPHERE) != 0 ? scene->sph_obj[idx - sphere_base] : scene->tri_object(idx)));
            }
            else {
                obj.push_back(-1);
                const float *q = &pairs[4 * static_cast<size_t>(it.ref - pair_base)].x;
                Item l, r;
                std::memcpy(&l.box, q, 24);
                std::memcpy(&r.box, q + 6, 24);
                std::memcpy(&l.ref, q + 12, 4);
                std::memcpy(&r.ref, q + 13, 4);
                stack.push_back(r);
                stack.push_back(l);
            }
        }
    }
    const uint64_t n = std::min<uint64_t>(obj.size(), capacity);
    for(uint64_t i = 0; i < n; i++) {
        out_obj[i] = obj[i];
        std::memcpy(out_box + 6 * i, &box[i], sizeof(float) * 6);
    }
    if(n_written != nullptr) {
        *n_written = obj.size();
    }
    return PT_OK;
}

int pt_intersect_batch(pt_scene *s, const float *rays, size_t n, float *out_t, int32_t *out_obj) {
    if(s == nullptr || (n > 0 && (rays == nullptr || out_t == nullptr || out_obj == nullptr))) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    if(n == 0) {
        return PT_OK;
    }
    if(n > 0x7fffffffULL) {
        return fail(PT_ERR_INVALID, "too many rays in one batch");
    }
    std::lock_guard<std::mutex> lock(s->render_mutex);
    PT_HIP(hipSetDevice(s->device));
    const uint32_t n32 = static_cast<uint32_t>(n);
    {
        int rc = setup_path(s);
        if(rc != PT_OK) {
            return rc;
        }
        PtPathConfig cfg = s->path_cfg;
        PT_HIP(s->batch_rays.ensure(6 * n));
        PT_HIP(s->closest_out.ensure(n));
        PT_HIP(s->path_spill.ensure(((n + 255) / 256) * 256 * cfg.spill_depth));
        cfg.spill = s->path_spill.ptr;
        hipStream_t st = s->stream;
        PT_HIP(hipMemcpyAsync(s->batch_rays.ptr, rays, 6 * n * sizeof(float), hipMemcpyHostToDevice, st));
        pt_launch_closest(st, s->dev, s->batch_rays.ptr, n32, s->closest_out.ptr, cfg);
        PT_HIP(hipGetLastError());
        std::vector<uint2> hits(n);
        PT_HIP(hipMemcpyAsync(hits.data(), s->closest_out.ptr, n * sizeof(uint2), hipMemcpyDeviceToHost, st));
        PT_HIP(hipStreamSynchronize(st));
        for(size_t i = 0; i < n; i++) {
            const float t = from_bits(hits[i].x);
            const uint32_t ref = hits[i].y;
            out_t[i] = t;
            out_obj[i] = (t < 0.0F || ref == PT_REF_NONE) ? -1 : static_cast<int32_t>((ref & PT_REF_SPHERE) ? s->sph_obj[(ref & PT_REF_INDEX) - (s->dev.n_tris + 1U)] : s->tri_object(ref & PT_REF_INDEX));
        }
        return PT_OK;
    }
}

} // extern "C"
