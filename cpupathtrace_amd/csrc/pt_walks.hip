// pt_walks.hip -- the kernels that trace ONE walk per lane to its end with the path kernel's traversal machinery (pt_trace.h): closest hits
// of a ray batch (pt_closest_kernel), the denoiser's first-hit and followed features (pt_feature_kernel, pt_follow_kernel), the first-hit features with motion (pt_motion_kernel; pt_motion_shapes_kernel for deformed meshes), the scene
// queries (pt_query_kernels.h: pt_query_kernel, pt_query_pixels_kernel, pt_occluded_kernel), the light gathered at points (pt_gather_kernels.h), the light probes (pt_light_probe_kernels.h), radiance along free rays and captures (pt_radiance_kernels.h), light-group passes (pt_light_pass_kernels.h) and two
// diagnostics (pt_steptime_kernel, pt_replay_kernel).  They live apart from pt_path.hip so that an edit here neither recompiles nor
// re-schedules the path kernel.  Written once: the dispatch over the three (stack window, records) routes, the LDS size, and the prologue
// that binds a lane's Tracer (bind_lane) where it leaves a kernel's instructions as they were: the closest-hit and the step-timing kernel.
// The path-sample loop of the gather, probe, radiance and light-pass kernels is written once as well (pt_sample_walk.h).
// The other bodies are deliberately NOT folded further.  Helpers for the root box, the walk to its end and the feature kernels' pixel and sums
// were built and measured ("The split"): every one of them, and bind_lane in the feature kernels, changed the compiler's
// schedule, and the feature passes then exceeded the measurement's tolerance on three rows.  As it stands the instruction text of every
// kernel here is the one it had in pt_path.hip, but for one commutative operand swap in the kViews instantiations (tools/kernel_diff.py).
#include <type_traits>

#include "pt_trace.h"
#include "pt_motion_shapes_kernels.h" // pt_face_table_kernel and its launch: no walk, but the one unit that holds it

using namespace ptd;

namespace {

// LDS of a workgroup: traversal stacks [STACK_LDS][256] | (IN_LDS) every record of the scene, in the order of `recs`
size_t walk_lds_bytes(int stack_lds, bool in_lds, const PtDevScene &scene) {
    return (size_t)stack_lds * 256 * sizeof(uint2) + (in_lds ? ((size_t)scene.n_lds_pairs + scene.pair_base) * 64 : 0);
}

// The head of a kernel: stages the records into LDS (IN_LDS; with the workgroup's barrier, so every thread calls it before it
// may return), points `tr` at the LDS or HBM records, at the thread's column of the stack window and at its part of the spill area.
// Returns the thread's global index.
template<int STACK_LDS, bool IN_LDS>
PT_D size_t bind_lane(Tracer<STACK_LDS, IN_LDS> &tr, const PtDevScene &sc, uint2 *spill, uint32_t spill_depth) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    const int tid = threadIdx.x;
    lds_u2_ptr stack_l = (lds_u2_ptr)reinterpret_cast<uint2 *>(lds_raw) + tid;
    float4 *lds_recs = reinterpret_cast<float4 *>(lds_raw + (size_t)STACK_LDS * 256 * sizeof(uint2));
    if(IN_LDS) {
        for(uint32_t i = tid; i < 4u * (sc.pair_base + sc.n_pairs); i += 256) {
            lds_recs[i] = sc.recs[i];
        }
        __syncthreads();
    }
    if(IN_LDS) {
        tr.recs = (typename RecPtr<IN_LDS>::type)(lds_f4_cptr)lds_recs;
    }
    else {
        tr.recs = (typename RecPtr<IN_LDS>::type)(glb_f4_cptr)sc.recs;
    }
    tr.stack_l = stack_l;
    const size_t gid = (size_t)blockIdx.x * 256 + tid;
    tr.my_spill = (glb_u2_ptr)(spill + gid * spill_depth);
    return gid;
}

// Scene::getIntersection for a batch of rays: one walk per lane, the same traversal machinery
template<int STACK_LDS, bool IN_LDS>
__global__ __launch_bounds__(256) void pt_closest_kernel(PtDevScene sc, const float *__restrict__ rays6, uint32_t n, uint2 *__restrict__ out, uint2 *__restrict__ spill,
                                                         uint32_t spill_depth) {
    Tracer<STACK_LDS, IN_LDS> tr;
    const size_t gid = bind_lane(tr, sc, spill, spill_depth);
    if(gid >= n) {
        return;
    }
    const float *r = rays6 + 6 * gid;
    Walk w;
    typename Tracer<STACK_LDS, IN_LDS>::Rec rec;
    rec.r0 = rec.r1 = rec.r2 = rec.r3 = (f4v){0.0f, 0.0f, 0.0f, 0.0f};
    RootBox root;
    root.ref = sc.root_ref;
    for(int k = 0; k < 3; k++) {
        root.lo[k] = sc.root_lo[k];
        root.hi[k] = sc.root_hi[k];
    }
    tr.start(w, rec, root, make_float4(r[0], r[1], r[2], 0.0f), make_float4(r[3], r[4], r[5], __uint_as_float(0u)));
    uint32_t n_nodes = 0, n_leaves = 0;
    while(tr.step(w, rec, 1, n_nodes, n_leaves)) {
    }
    out[gid] = make_uint2(__float_as_uint(w.best_ref == PT_REF_NONE ? -1.0f : w.best_t), w.best_ref);
}

// First-hit features of a frame for the denoiser (pt_denoise.hip): each pixel traces K = 4 primary rays at the sub-pixel offsets
// (-1/4, -1/4), (+1/4, -1/4), (-1/4, +1/4), (+1/4, +1/4) through a camera without aperture sampling and without pixel jitter (the caller
// passes aperture_kind = none; pixel_width = pixel_height = 0 make camera_shoot's two offsets +0), so the rays are a pure function of
// camera and pixel.  The walk is pt_closest_kernel's.  out[3 p + k], the mean over the rays (summed in ray order, then * 0.25f; a miss adds 0):
//   k = 0: albedo rgb (diffuse for Lambertian, specular for glass and mirror, white for no material), fraction of rays that hit
//   k = 1: shading normal xyz (object_normal), hit distance t
//   k = 2: hit position xyz (o + d * t), luminance of the material's emission
// kViews (pt_render_features_views): `height` is the row count of n views stacked as in a view batch, view_height the rows of one; a pixel's
// camera is views[row / view_height] (aperture none, as `cam`), read per lane, and its row the one inside its view.  Everything else is the
// single frame's, so view v is bit for bit the single frame's result for views[v].  The single-frame instantiations read `cam` and have no
// such test: kViews is a template parameter.
template<int STACK_LDS, bool IN_LDS, bool kViews>
__global__ __launch_bounds__(256) void pt_feature_kernel(PtDevScene sc, PtDevCamera cam, int32_t width, int32_t height, float4 *__restrict__ out, uint2 *__restrict__ spill,
                                                         uint32_t spill_depth, const PtViewCamera *__restrict__ views, int32_t view_height) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    const int tid = threadIdx.x;
    lds_u2_ptr stack_l = (lds_u2_ptr)reinterpret_cast<uint2 *>(lds_raw) + tid;
    float4 *lds_recs = reinterpret_cast<float4 *>(lds_raw + (size_t)STACK_LDS * 256 * sizeof(uint2));
    if(IN_LDS) {
        for(uint32_t i = tid; i < 4u * (sc.pair_base + sc.n_pairs); i += 256) {
            lds_recs[i] = sc.recs[i];
        }
        __syncthreads();
    }
    Tracer<STACK_LDS, IN_LDS> tr;
    if(IN_LDS) {
        tr.recs = (typename RecPtr<IN_LDS>::type)(lds_f4_cptr)lds_recs;
    }
    else {
        tr.recs = (typename RecPtr<IN_LDS>::type)(glb_f4_cptr)sc.recs;
    }
    tr.stack_l = stack_l;
    const size_t gid = (size_t)blockIdx.x * 256 + tid;
    tr.my_spill = (glb_u2_ptr)(spill + gid * spill_depth);
    if(gid >= (size_t)width * (size_t)height) {
        return;
    }
    const int32_t px = (int32_t)(gid % (size_t)width);
    int32_t py = (int32_t)(gid / (size_t)width);
    const PtDevCamera *lane_cam = &cam;
    int32_t frame_height = height;
    if constexpr(kViews) {
        const int32_t view = py / view_height;
        py -= view * view_height;
        lane_cam = &views[view].cam;
        frame_height = view_height;
    }
    RootBox root;
    root.ref = sc.root_ref;
    for(int k = 0; k < 3; k++) {
        root.lo[k] = sc.root_lo[k];
        root.hi[k] = sc.root_hi[k];
    }
    float4 acc0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), acc1 = acc0, acc2 = acc0, emis = acc0;
    for(int k = 0; k < 4; k++) {
        const float dx = (k & 1) ? 0.25f : -0.25f, dy = (k & 2) ? 0.25f : -0.25f;
        // the camera ray of the path kernel (worker.cpp:166-168) with x + 1/2 + dx in place of x + 1/2
        const float one_half = 1.0f / 2.0f;
        const float x_camera = 2 * (((float)px + one_half + dx) / (float)width - one_half);
        float y_camera = 2 * (((float)py + one_half + dy) / (float)frame_height - one_half);
        y_camera = -y_camera;
        uint64_t rng = 0; // (drawn from, never used: both offsets are +0 and there is no aperture)
        const Ray ray = camera_shoot(*lane_cam, x_camera, y_camera, 0.0f, 0.0f, rng);
        Walk w;
        typename Tracer<STACK_LDS, IN_LDS>::Rec rec;
        rec.r0 = rec.r1 = rec.r2 = rec.r3 = (f4v){0.0f, 0.0f, 0.0f, 0.0f};
        tr.start(w, rec, root, make_float4(ray.o.x, ray.o.y, ray.o.z, 0.0f), make_float4(ray.d.x, ray.d.y, ray.d.z, __uint_as_float(0u)));
        uint32_t n_nodes = 0, n_leaves = 0;
        while(tr.step(w, rec, 1, n_nodes, n_leaves)) {
        }
        float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), n4 = a, p4 = a, e4 = a;
        if(w.best_ref != PT_REF_NONE) {
            const float t = w.best_t;
            const V3 pos = ray.o + ray.d * t;
            uint32_t material_index;
            const V3 n = object_normal(sc, w.best_ref, pos, material_index);
            const Material mat = material_load(sc.materials, material_index);
            const bool lambertian = mat.bsdf == 0; // PT_BSDF_LAMBERTIAN
            a = make_float4(lambertian ? mat.diffuse.r : mat.specular.r, lambertian ? mat.diffuse.g : mat.specular.g, lambertian ? mat.diffuse.b : mat.specular.b, 1.0f);
            n4 = make_float4(n.x, n.y, n.z, t);
            p4 = make_float4(pos.x, pos.y, pos.z, 0.0f);
            e4 = make_float4(mat.emission.r, mat.emission.g, mat.emission.b, 0.0f);
        }
        acc0 = make_float4(acc0.x + a.x, acc0.y + a.y, acc0.z + a.z, acc0.w + a.w);
        acc1 = make_float4(acc1.x + n4.x, acc1.y + n4.y, acc1.z + n4.z, acc1.w + n4.w);
        acc2 = make_float4(acc2.x + p4.x, acc2.y + p4.y, acc2.z + p4.z, 0.0f);
        emis = make_float4(emis.x + e4.x, emis.y + e4.y, emis.z + e4.z, 0.0f);
    }
    const float q = 0.25f;
    const float er = emis.x * q, eg = emis.y * q, eb = emis.z * q;
    float4 *o = out + 3 * gid;
    o[0] = make_float4(acc0.x * q, acc0.y * q, acc0.z * q, acc0.w * q);
    o[1] = make_float4(acc1.x * q, acc1.y * q, acc1.z * q, acc1.w * q);
    o[2] = make_float4(acc2.x * q, acc2.y * q, acc2.z * q, (0.2126f * er + 0.7152f * eg) + 0.0722f * eb);
}

// Followed features (include/pt_features.h): the rays, the layout and the order of pt_feature_kernel, but a ray that
// hits glass or a mirror goes on -- bsdf_follow's deterministic branch, tinted by bsdf_spectrum as the path kernel's bounce tints -- to the
// first Lambertian (or material-less) hit or to bounce `max_bounces`, and contributes there: albedo T * albedo, that hit's normal, the
// summed length L of its segments, the unfolded position o0 + d0 * L and T * emission.  A miss at any bounce contributes what a first-hit
// miss does: nothing.  With max_bounces = 0 every operation is pt_feature_kernel's (T = 1 and L = 0 + t are exact): the same bits.
//
// ONE loop of walks per lane, one tr.start / tr.step site: a lane's state is (sub-pixel ray k, bounce b, T, L, o0, d0, the accumulators),
// and a lane whose chain ends starts the chain of its next sub-pixel ray in the same turn of the loop, while its neighbours bounce.  A lane
// accumulates in ray order whatever its neighbours do, so the result does not depend on the wavefront.  The loop is bounded by
// construction: a chain is at most max_bounces + 1 walks, so a lane makes at most 4 * (max_bounces + 1) of them, and that count -- not the
// geometry -- ends the loop; a NaN direction fails the root box's test and its chain ends as a miss.
template<int STACK_LDS, bool IN_LDS, bool kViews>
__global__ __launch_bounds__(256) void pt_follow_kernel(PtDevScene sc, PtDevCamera cam, int32_t width, int32_t height, float4 *__restrict__ out, uint2 *__restrict__ spill,
                                                        uint32_t spill_depth, const PtViewCamera *__restrict__ views, int32_t view_height, int32_t max_bounces,
                                                        float epsilon) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    const int tid = threadIdx.x;
    lds_u2_ptr stack_l = (lds_u2_ptr)reinterpret_cast<uint2 *>(lds_raw) + tid;
    float4 *lds_recs = reinterpret_cast<float4 *>(lds_raw + (size_t)STACK_LDS * 256 * sizeof(uint2));
    if(IN_LDS) {
        for(uint32_t i = tid; i < 4u * (sc.pair_base + sc.n_pairs); i += 256) {
            lds_recs[i] = sc.recs[i];
        }
        __syncthreads();
    }
    Tracer<STACK_LDS, IN_LDS> tr;
    if(IN_LDS) {
        tr.recs = (typename RecPtr<IN_LDS>::type)(lds_f4_cptr)lds_recs;
    }
    else {
        tr.recs = (typename RecPtr<IN_LDS>::type)(glb_f4_cptr)sc.recs;
    }
    tr.stack_l = stack_l;
    const size_t gid = (size_t)blockIdx.x * 256 + tid;
    tr.my_spill = (glb_u2_ptr)(spill + gid * spill_depth);
    if(gid >= (size_t)width * (size_t)height) {
        return;
    }
    const int32_t px = (int32_t)(gid % (size_t)width);
    int32_t py = (int32_t)(gid / (size_t)width);
    const PtDevCamera *lane_cam = &cam;
    int32_t frame_height = height;
    if constexpr(kViews) {
        const int32_t view = py / view_height;
        py -= view * view_height;
        lane_cam = &views[view].cam;
        frame_height = view_height;
    }
    RootBox root;
    root.ref = sc.root_ref;
    for(int k = 0; k < 3; k++) {
        root.lo[k] = sc.root_lo[k];
        root.hi[k] = sc.root_hi[k];
    }
    // the primary ray of sub-pixel k: pt_feature_kernel's
    auto primary = [&](int k) {
        const float dx = (k & 1) ? 0.25f : -0.25f, dy = (k & 2) ? 0.25f : -0.25f;
        const float one_half = 1.0f / 2.0f;
        const float x_camera = 2 * (((float)px + one_half + dx) / (float)width - one_half);
        float y_camera = 2 * (((float)py + one_half + dy) / (float)frame_height - one_half);
        y_camera = -y_camera;
        uint64_t rng = 0; // (drawn from, never used: both offsets are +0 and there is no aperture)
        return camera_shoot(*lane_cam, x_camera, y_camera, 0.0f, 0.0f, rng);
    };
    float4 acc0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), acc1 = acc0, acc2 = acc0, emis = acc0;
    int k = 0, b = 0;
    Ray ray = primary(0);
    V3 o0 = ray.o, d0 = ray.d, T = v3(1.0f, 1.0f, 1.0f);
    float L = 0.0f;
    const int max_walks = 4 * (max_bounces + 1);
    for(int walk = 0; walk < max_walks && k < 4; walk++) {
        Walk w;
        typename Tracer<STACK_LDS, IN_LDS>::Rec rec;
        rec.r0 = rec.r1 = rec.r2 = rec.r3 = (f4v){0.0f, 0.0f, 0.0f, 0.0f};
        tr.start(w, rec, root, make_float4(ray.o.x, ray.o.y, ray.o.z, 0.0f), make_float4(ray.d.x, ray.d.y, ray.d.z, __uint_as_float(0u)));
        uint32_t n_nodes = 0, n_leaves = 0;
        while(tr.step(w, rec, 1, n_nodes, n_leaves)) {
        }
        float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), n4 = a, p4 = a, e4 = a;
        bool chain_ends = true;
        if(w.best_ref != PT_REF_NONE) {
            const float t = w.best_t;
            L = L + t;
            const V3 pos = ray.o + ray.d * t;
            uint32_t material_index;
            const V3 n = object_normal(sc, w.best_ref, pos, material_index);
            const Material mat = material_load(sc.materials, material_index);
            const bool lambertian = mat.bsdf == 0; // PT_BSDF_LAMBERTIAN (a hit without a material loads as one)
            if(lambertian || b == max_bounces) {
                const V3 virt = o0 + d0 * L;
                a = make_float4(T.x * (lambertian ? mat.diffuse.r : mat.specular.r), T.y * (lambertian ? mat.diffuse.g : mat.specular.g),
                                T.z * (lambertian ? mat.diffuse.b : mat.specular.b), 1.0f);
                n4 = make_float4(n.x, n.y, n.z, L);
                p4 = make_float4(virt.x, virt.y, virt.z, 0.0f);
                e4 = make_float4(T.x * mat.emission.r, T.y * mat.emission.g, T.z * mat.emission.b, 0.0f);
            }
            else {
                bool reflected;
                const Ray next = bsdf_follow(mat, ray.d, pos, n, epsilon, reflected);
                float shading_factor, shading_pd;
                const C4 tint = bsdf_spectrum(mat, ray.d, next.d, n, c4(1.0f, 1.0f, 1.0f, 1.0f), false, shading_factor, shading_pd);
                T = v3(T.x * tint.r, T.y * tint.g, T.z * tint.b);
                b += 1;
                ray = next;
                chain_ends = false;
            }
        }
        if(chain_ends) {
            acc0 = make_float4(acc0.x + a.x, acc0.y + a.y, acc0.z + a.z, acc0.w + a.w);
            acc1 = make_float4(acc1.x + n4.x, acc1.y + n4.y, acc1.z + n4.z, acc1.w + n4.w);
            acc2 = make_float4(acc2.x + p4.x, acc2.y + p4.y, acc2.z + p4.z, 0.0f);
            emis = make_float4(emis.x + e4.x, emis.y + e4.y, emis.z + e4.z, 0.0f);
            k += 1;
            if(k < 4) {
                ray = primary(k);
                o0 = ray.o;
                d0 = ray.d;
                T = v3(1.0f, 1.0f, 1.0f);
                L = 0.0f;
                b = 0;
            }
        }
    }
    const float q = 0.25f;
    const float er = emis.x * q, eg = emis.y * q, eb = emis.z * q;
    float4 *o = out + 3 * gid;
    o[0] = make_float4(acc0.x * q, acc0.y * q, acc0.z * q, acc0.w * q);
    o[1] = make_float4(acc1.x * q, acc1.y * q, acc1.z * q, acc1.w * q);
    o[2] = make_float4(acc2.x * q, acc2.y * q, acc2.z * q, (0.2126f * er + 0.7152f * eg) + 0.0722f * eb);
}

// pt_denoise.hip's dot3: (a x + b y) + c z
PT_D float motion_dot3(float a, float b, float c, V3 v) {
    return (a * v.x + b * v.y) + c * v.z;
}

// First-hit features AND motion of a single frame (include/pt_motion.h): the rays, the walk, the accumulators and the
// stores of pt_feature_kernel<.., false>, operation for operation, so `out` has its bits; each hit also adds where its surface point was
// at the previous pose and the normal it had there.  The object of a triangle hit is in its record (the word object_normal's load
// brings anyway); `inst` holds the instances that have objects by ascending first object, so the instance of an object is the last one
// whose first is not above it -- if its range holds the object; objects of the description lie below inst[0].first, spheres are never
// looked up.  n_inst == 0: nothing moved, and motion is the features' position and normal with w = 0.
template<int STACK_LDS, bool IN_LDS>
__global__ __launch_bounds__(256) void pt_motion_kernel(PtDevScene sc, PtDevCamera cam, int32_t width, int32_t height, float4 *__restrict__ out, uint2 *__restrict__ spill,
                                                        uint32_t spill_depth, float4 *__restrict__ motion, const PtMotionInstance *__restrict__ inst, uint32_t n_inst) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    const int tid = threadIdx.x;
    lds_u2_ptr stack_l = (lds_u2_ptr)reinterpret_cast<uint2 *>(lds_raw) + tid;
    float4 *lds_recs = reinterpret_cast<float4 *>(lds_raw + (size_t)STACK_LDS * 256 * sizeof(uint2));
    if(IN_LDS) {
        for(uint32_t i = tid; i < 4u * (sc.pair_base + sc.n_pairs); i += 256) {
            lds_recs[i] = sc.recs[i];
        }
        __syncthreads();
    }
    Tracer<STACK_LDS, IN_LDS> tr;
    if(IN_LDS) {
        tr.recs = (typename RecPtr<IN_LDS>::type)(lds_f4_cptr)lds_recs;
    }
    else {
        tr.recs = (typename RecPtr<IN_LDS>::type)(glb_f4_cptr)sc.recs;
    }
    tr.stack_l = stack_l;
    const size_t gid = (size_t)blockIdx.x * 256 + tid;
    tr.my_spill = (glb_u2_ptr)(spill + gid * spill_depth);
    if(gid >= (size_t)width * (size_t)height) {
        return;
    }
    const int32_t px = (int32_t)(gid % (size_t)width);
    const int32_t py = (int32_t)(gid / (size_t)width);
    RootBox root;
    root.ref = sc.root_ref;
    for(int k = 0; k < 3; k++) {
        root.lo[k] = sc.root_lo[k];
        root.hi[k] = sc.root_hi[k];
    }
    float4 acc0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), acc1 = acc0, acc2 = acc0, emis = acc0, mot0 = acc0, mot1 = acc0;
    for(int k = 0; k < 4; k++) {
        const float dx = (k & 1) ? 0.25f : -0.25f, dy = (k & 2) ? 0.25f : -0.25f;
        const float one_half = 1.0f / 2.0f;
        const float x_camera = 2 * (((float)px + one_half + dx) / (float)width - one_half);
        float y_camera = 2 * (((float)py + one_half + dy) / (float)height - one_half);
        y_camera = -y_camera;
        uint64_t rng = 0; // (drawn from, never used: both offsets are +0 and there is no aperture)
        const Ray ray = camera_shoot(cam, x_camera, y_camera, 0.0f, 0.0f, rng);
        Walk w;
        typename Tracer<STACK_LDS, IN_LDS>::Rec rec;
        rec.r0 = rec.r1 = rec.r2 = rec.r3 = (f4v){0.0f, 0.0f, 0.0f, 0.0f};
        tr.start(w, rec, root, make_float4(ray.o.x, ray.o.y, ray.o.z, 0.0f), make_float4(ray.d.x, ray.d.y, ray.d.z, __uint_as_float(0u)));
        uint32_t n_nodes = 0, n_leaves = 0;
        while(tr.step(w, rec, 1, n_nodes, n_leaves)) {
        }
        float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), n4 = a, p4 = a, e4 = a, m0 = a, m1 = a;
        if(w.best_ref != PT_REF_NONE) {
            const float t = w.best_t;
            const V3 pos = ray.o + ray.d * t;
            uint32_t material_index;
            const V3 n = object_normal(sc, w.best_ref, pos, material_index);
            const Material mat = material_load(sc.materials, material_index);
            const bool lambertian = mat.bsdf == 0; // PT_BSDF_LAMBERTIAN
            a = make_float4(lambertian ? mat.diffuse.r : mat.specular.r, lambertian ? mat.diffuse.g : mat.specular.g, lambertian ? mat.diffuse.b : mat.specular.b, 1.0f);
            n4 = make_float4(n.x, n.y, n.z, t);
            p4 = make_float4(pos.x, pos.y, pos.z, 0.0f);
            e4 = make_float4(mat.emission.r, mat.emission.g, mat.emission.b, 0.0f);
            m0 = p4;
            m1 = make_float4(n.x, n.y, n.z, 0.0f);
            if(n_inst != 0 && !(w.best_ref & PT_REF_SPHERE)) {
                const uint32_t obj = __float_as_uint(sc.tri_shade[8 * (size_t)(w.best_ref & PT_REF_INDEX) + 2].z) & 0x7fffffffu;
                uint32_t lo = 0, hi = n_inst; // the last instance whose first object is <= obj lies in [lo, hi)
                while(hi - lo > 1) {
                    const uint32_t mid = lo + (hi - lo) / 2;
                    if(inst[mid].first <= obj) {
                        lo = mid;
                    }
                    else {
                        hi = mid;
                    }
                }
                const PtMotionInstance *mi = inst + lo;
                const uint32_t first = mi->first;
                if(obj >= first && obj - first < mi->count) {
                    const uint32_t kind = mi->kind;
                    if(kind == 2u) { // PT_MOTION_NONE
                        m0 = make_float4(0.0f, 0.0f, 0.0f, 1.0f);
                        m1 = make_float4(0.0f, 0.0f, 0.0f, 1.0f);
                    }
                    else if(kind == 1u) { // PT_MOTION_MOVED
                        const float4 b0 = *reinterpret_cast<const float4 *>(mi->back), b1 = *reinterpret_cast<const float4 *>(mi->back + 4),
                                     b2 = *reinterpret_cast<const float4 *>(mi->back + 8);
                        const float4 r0 = *reinterpret_cast<const float4 *>(mi->normal), r1 = *reinterpret_cast<const float4 *>(mi->normal + 4),
                                     r2 = *reinterpret_cast<const float4 *>(mi->normal + 8);
                        m0 = make_float4(motion_dot3(b0.x, b0.y, b0.z, pos) + b0.w, motion_dot3(b1.x, b1.y, b1.z, pos) + b1.w, motion_dot3(b2.x, b2.y, b2.z, pos) + b2.w, 1.0f);
                        const V3 v = v3(motion_dot3(r0.x, r0.y, r0.z, n), motion_dot3(r1.x, r1.y, r1.z, n), motion_dot3(r2.x, r2.y, r2.z, n));
                        const float len2 = motion_dot3(v.x, v.y, v.z, v);
                        const float inv = 1.0f / sqrtf(len2);
                        m1 = make_float4(len2 > 0.0f ? v.x * inv : 0.0f, len2 > 0.0f ? v.y * inv : 0.0f, len2 > 0.0f ? v.z * inv : 0.0f, 0.0f);
                    }
                }
            }
        }
        acc0 = make_float4(acc0.x + a.x, acc0.y + a.y, acc0.z + a.z, acc0.w + a.w);
        acc1 = make_float4(acc1.x + n4.x, acc1.y + n4.y, acc1.z + n4.z, acc1.w + n4.w);
        acc2 = make_float4(acc2.x + p4.x, acc2.y + p4.y, acc2.z + p4.z, 0.0f);
        emis = make_float4(emis.x + e4.x, emis.y + e4.y, emis.z + e4.z, 0.0f);
        mot0 = make_float4(mot0.x + m0.x, mot0.y + m0.y, mot0.z + m0.z, mot0.w + m0.w);
        mot1 = make_float4(mot1.x + m1.x, mot1.y + m1.y, mot1.z + m1.z, mot1.w + m1.w);
    }
    const float q = 0.25f;
    const float er = emis.x * q, eg = emis.y * q, eb = emis.z * q;
    float4 *o = out + 3 * gid;
    o[0] = make_float4(acc0.x * q, acc0.y * q, acc0.z * q, acc0.w * q);
    o[1] = make_float4(acc1.x * q, acc1.y * q, acc1.z * q, acc1.w * q);
    o[2] = make_float4(acc2.x * q, acc2.y * q, acc2.z * q, (0.2126f * er + 0.7152f * eg) + 0.0722f * eb);
    float4 *m = motion + 2 * gid;
    m[0] = make_float4(mot0.x * q, mot0.y * q, mot0.z * q, mot0.w * q);
    m[1] = make_float4(mot1.x * q, mot1.y * q, mot1.z * q, mot1.w * q);
}

// A hit on an instance whose mesh was deformed since the mark (include/pt_motion_shapes.h has the formulas as a contract): the face the
// hit triangle came from, its three vertices as they were at the mark through the matrix the instance had then -- kb_transform's
// arithmetic (pt_mesh_batch_kernels.h), so the corners are the marked frame's bit for bit --, the hit's barycentrics as tri_normal
// computes them, and the previous position and normal from those.  The loads of one level (three indices; nine coordinates and the
// matrix) are independent and issued together; they happen once per hit ray, after the walk.
PT_D V3 shape_corner(float4 r0, float4 r1, float4 r2, float4 r3, float x, float y, float z) {
    float h[4];
    const float4 rows[4] = {r0, r1, r2, r3};
    for(int r = 0; r < 4; r++) {
        float d = 0.0f;
        d += rows[r].x * x;
        d += rows[r].y * y;
        d += rows[r].z * z;
        d += rows[r].w * 1.0f;
        h[r] = d;
    }
    const float inv = 1.0f / h[3];
    return v3(h[0] * inv, h[1] * inv, h[2] * inv);
}

PT_D bool shape_finite(float x) {
    return __builtin_fabsf(x) < __builtin_huge_valf(); // (false for NaN)
}

PT_D void shape_motion(const float4 *__restrict__ rec, const PtShapeMotionInstance *__restrict__ mi, uint32_t g, V3 pos, V3 n, float4 &m0, float4 &m1) {
    const int32_t *fi = mi->faces + 3 * (size_t)(g - mi->face_first);
    const int32_t ia = fi[0], ib = fi[1], ic = fi[2]; // (a surviving face's indices are in range: the assembler rejected the others)
    const float *mv = mi->marked;
    const float *pa = mv + 3 * (size_t)ia, *pb = mv + 3 * (size_t)ib, *pc = mv + 3 * (size_t)ic;
    const float ax = pa[0], ay = pa[1], az = pa[2], bx = pb[0], by = pb[1], bz = pb[2], cx = pc[0], cy = pc[1], cz = pc[2];
    const float4 r0 = *reinterpret_cast<const float4 *>(mi->m), r1 = *reinterpret_cast<const float4 *>(mi->m + 4), r2 = *reinterpret_cast<const float4 *>(mi->m + 8),
                 r3 = *reinterpret_cast<const float4 *>(mi->m + 12);
    const TriRec t = tri_unpack(rec[0], rec[1], rec[2]);
    const V3 qa = shape_corner(r0, r1, r2, r3, ax, ay, az), qb = shape_corner(r0, r1, r2, r3, bx, by, bz), qc = shape_corner(r0, r1, r2, r3, cx, cy, cz);
    // tri_normal's barycentrics
    const V3 ap = pos - t.a;
    const float d00 = dot(t.ab, t.ab);
    const float d01 = dot(t.ab, t.ac);
    const float d11 = dot(t.ac, t.ac);
    const float d20 = dot(ap, t.ab);
    const float d21 = dot(ap, t.ac);
    const float inv_d = 1.0f / (d00 * d11 - d01 * d01);
    const float bv = (d11 * d20 - d01 * d21) * inv_d;
    const float bw = (d00 * d21 - d01 * d20) * inv_d;
    const float bu = 1.0f - bv - bw;
    const V3 pp = (qa * bu + qb * bv) + qc * bw;
    const V3 cp = cross(qb - qa, qc - qa), cc = cross(t.ab, t.ac);
    const float lp = motion_dot3(cp.x, cp.y, cp.z, cp), lc = motion_dot3(cc.x, cc.y, cc.z, cc);
    if(!(lp > 0.0f) || !(lc > 0.0f) || !shape_finite(pp.x) || !shape_finite(pp.y) || !shape_finite(pp.z)) { // no previous position
        m0 = make_float4(0.0f, 0.0f, 0.0f, 1.0f);
        m1 = make_float4(0.0f, 0.0f, 0.0f, 1.0f);
        return;
    }
    const V3 ngp = cp * (1.0f / sqrtf(lp)), ng = cc * (1.0f / sqrtf(lc));
    const V3 v = (n - ng) + ngp;
    const float len2 = motion_dot3(v.x, v.y, v.z, v);
    const float inv = 1.0f / sqrtf(len2);
    m0 = make_float4(pp.x, pp.y, pp.z, 1.0f);
    m1 = make_float4(len2 > 0.0f ? v.x * inv : 0.0f, len2 > 0.0f ? v.y * inv : 0.0f, len2 > 0.0f ? v.z * inv : 0.0f, 0.0f);
}

// pt_motion_kernel for a scene with a motion mark in which a mesh was deformed (include/pt_motion_shapes.h): its text
// -- rays, walk, accumulators, stores, the static / moved / none arithmetic operation for operation -- with a fourth kind: an instance
// whose mesh changed shape since the mark takes a hit's previous position and normal from the marked vertices of the hit triangle's face
// (shape_motion).  face_of[t] is the scene-wide face of instance triangle t, which is object first_object + t.
template<int STACK_LDS, bool IN_LDS>
__global__ __launch_bounds__(256) void pt_motion_shapes_kernel(PtDevScene sc, PtDevCamera cam, int32_t width, int32_t height, float4 *__restrict__ out, uint2 *__restrict__ spill,
                                                        uint32_t spill_depth, float4 *__restrict__ motion, const PtShapeMotionInstance *__restrict__ inst, uint32_t n_inst,
                                                               const uint32_t *__restrict__ face_of, uint32_t first_object) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    const int tid = threadIdx.x;
    lds_u2_ptr stack_l = (lds_u2_ptr)reinterpret_cast<uint2 *>(lds_raw) + tid;
    float4 *lds_recs = reinterpret_cast<float4 *>(lds_raw + (size_t)STACK_LDS * 256 * sizeof(uint2));
    if(IN_LDS) {
        for(uint32_t i = tid; i < 4u * (sc.pair_base + sc.n_pairs); i += 256) {
            lds_recs[i] = sc.recs[i];
        }
        __syncthreads();
    }
    Tracer<STACK_LDS, IN_LDS> tr;
    if(IN_LDS) {
        tr.recs = (typename RecPtr<IN_LDS>::type)(lds_f4_cptr)lds_recs;
    }
    else {
        tr.recs = (typename RecPtr<IN_LDS>::type)(glb_f4_cptr)sc.recs;
    }
    tr.stack_l = stack_l;
    const size_t gid = (size_t)blockIdx.x * 256 + tid;
    tr.my_spill = (glb_u2_ptr)(spill + gid * spill_depth);
    if(gid >= (size_t)width * (size_t)height) {
        return;
    }
    const int32_t px = (int32_t)(gid % (size_t)width);
    const int32_t py = (int32_t)(gid / (size_t)width);
    RootBox root;
    root.ref = sc.root_ref;
    for(int k = 0; k < 3; k++) {
        root.lo[k] = sc.root_lo[k];
        root.hi[k] = sc.root_hi[k];
    }
    float4 acc0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), acc1 = acc0, acc2 = acc0, emis = acc0, mot0 = acc0, mot1 = acc0;
    for(int k = 0; k < 4; k++) {
        const float dx = (k & 1) ? 0.25f : -0.25f, dy = (k & 2) ? 0.25f : -0.25f;
        const float one_half = 1.0f / 2.0f;
        const float x_camera = 2 * (((float)px + one_half + dx) / (float)width - one_half);
        float y_camera = 2 * (((float)py + one_half + dy) / (float)height - one_half);
        y_camera = -y_camera;
        uint64_t rng = 0; // (drawn from, never used: both offsets are +0 and there is no aperture)
        const Ray ray = camera_shoot(cam, x_camera, y_camera, 0.0f, 0.0f, rng);
        Walk w;
        typename Tracer<STACK_LDS, IN_LDS>::Rec rec;
        rec.r0 = rec.r1 = rec.r2 = rec.r3 = (f4v){0.0f, 0.0f, 0.0f, 0.0f};
        tr.start(w, rec, root, make_float4(ray.o.x, ray.o.y, ray.o.z, 0.0f), make_float4(ray.d.x, ray.d.y, ray.d.z, __uint_as_float(0u)));
        uint32_t n_nodes = 0, n_leaves = 0;
        while(tr.step(w, rec, 1, n_nodes, n_leaves)) {
        }
        float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), n4 = a, p4 = a, e4 = a, m0 = a, m1 = a;
        if(w.best_ref != PT_REF_NONE) {
            const float t = w.best_t;
            const V3 pos = ray.o + ray.d * t;
            uint32_t material_index;
            const V3 n = object_normal(sc, w.best_ref, pos, material_index);
            const Material mat = material_load(sc.materials, material_index);
            const bool lambertian = mat.bsdf == 0; // PT_BSDF_LAMBERTIAN
            a = make_float4(lambertian ? mat.diffuse.r : mat.specular.r, lambertian ? mat.diffuse.g : mat.specular.g, lambertian ? mat.diffuse.b : mat.specular.b, 1.0f);
            n4 = make_float4(n.x, n.y, n.z, t);
            p4 = make_float4(pos.x, pos.y, pos.z, 0.0f);
            e4 = make_float4(mat.emission.r, mat.emission.g, mat.emission.b, 0.0f);
            m0 = p4;
            m1 = make_float4(n.x, n.y, n.z, 0.0f);
            if(n_inst != 0 && !(w.best_ref & PT_REF_SPHERE)) {
                const uint32_t obj = __float_as_uint(sc.tri_shade[8 * (size_t)(w.best_ref & PT_REF_INDEX) + 2].z) & 0x7fffffffu;
                uint32_t lo = 0, hi = n_inst; // the last instance whose first object is <= obj lies in [lo, hi)
                while(hi - lo > 1) {
                    const uint32_t mid = lo + (hi - lo) / 2;
                    if(inst[mid].first <= obj) {
                        lo = mid;
                    }
                    else {
                        hi = mid;
                    }
                }
                const PtShapeMotionInstance *mi = inst + lo;
                const uint32_t first = mi->first;
                if(obj >= first && obj - first < mi->count) {
                    const uint32_t kind = mi->kind;
                    if(kind == 2u) { // PT_MOTION_NONE
                        m0 = make_float4(0.0f, 0.0f, 0.0f, 1.0f);
                        m1 = make_float4(0.0f, 0.0f, 0.0f, 1.0f);
                    }
                    else if(kind == 1u) { // PT_MOTION_MOVED
                        const float4 b0 = *reinterpret_cast<const float4 *>(mi->back), b1 = *reinterpret_cast<const float4 *>(mi->back + 4),
                                     b2 = *reinterpret_cast<const float4 *>(mi->back + 8);
                        const float4 r0 = *reinterpret_cast<const float4 *>(mi->normal), r1 = *reinterpret_cast<const float4 *>(mi->normal + 4),
                                     r2 = *reinterpret_cast<const float4 *>(mi->normal + 8);
                        m0 = make_float4(motion_dot3(b0.x, b0.y, b0.z, pos) + b0.w, motion_dot3(b1.x, b1.y, b1.z, pos) + b1.w, motion_dot3(b2.x, b2.y, b2.z, pos) + b2.w, 1.0f);
                        const V3 v = v3(motion_dot3(r0.x, r0.y, r0.z, n), motion_dot3(r1.x, r1.y, r1.z, n), motion_dot3(r2.x, r2.y, r2.z, n));
                        const float len2 = motion_dot3(v.x, v.y, v.z, v);
                        const float inv = 1.0f / sqrtf(len2);
                        m1 = make_float4(len2 > 0.0f ? v.x * inv : 0.0f, len2 > 0.0f ? v.y * inv : 0.0f, len2 > 0.0f ? v.z * inv : 0.0f, 0.0f);
                    }
                    else if(kind == 3u) { // PT_MOTION_DEFORMED
                        shape_motion(sc.tri_shade + 8 * (size_t)(w.best_ref & PT_REF_INDEX), mi, face_of[obj - first_object], pos, n, m0, m1);
                    }
                }
            }
        }
        acc0 = make_float4(acc0.x + a.x, acc0.y + a.y, acc0.z + a.z, acc0.w + a.w);
        acc1 = make_float4(acc1.x + n4.x, acc1.y + n4.y, acc1.z + n4.z, acc1.w + n4.w);
        acc2 = make_float4(acc2.x + p4.x, acc2.y + p4.y, acc2.z + p4.z, 0.0f);
        emis = make_float4(emis.x + e4.x, emis.y + e4.y, emis.z + e4.z, 0.0f);
        mot0 = make_float4(mot0.x + m0.x, mot0.y + m0.y, mot0.z + m0.z, mot0.w + m0.w);
        mot1 = make_float4(mot1.x + m1.x, mot1.y + m1.y, mot1.z + m1.z, mot1.w + m1.w);
    }
    const float q = 0.25f;
    const float er = emis.x * q, eg = emis.y * q, eb = emis.z * q;
    float4 *o = out + 3 * gid;
    o[0] = make_float4(acc0.x * q, acc0.y * q, acc0.z * q, acc0.w * q);
    o[1] = make_float4(acc1.x * q, acc1.y * q, acc1.z * q, acc1.w * q);
    o[2] = make_float4(acc2.x * q, acc2.y * q, acc2.z * q, (0.2126f * er + 0.7152f * eg) + 0.0722f * eb);
    float4 *m = motion + 2 * gid;
    m[0] = make_float4(mot0.x * q, mot0.y * q, mot0.z * q, mot0.w * q);
    m[1] = make_float4(mot1.x * q, mot1.y * q, mot1.z * q, mot1.w * q);
}

// ---- diagnostic: where the cycles of a traversal step go -------------------------------------------------------------------------------
// One walk per lane as in pt_closest_kernel, but only the first `lanes_per_wave` lanes of every wavefront get a ray, and every step is
// stamped (s_memtime): cycles spent waiting for the record that was requested at the end of the previous step, and everything else.
// out[ray] = (steps, cycles waiting for records, cycles of the whole walk, cycles of two back-to-back stamps = the stamps' own price).
template<int STACK_LDS, bool STAMP>
__global__ __launch_bounds__(256) void pt_steptime_kernel(PtDevScene sc, const float *__restrict__ rays6, uint32_t n, uint32_t lanes_per_wave, uint4 *__restrict__ out,
                                                          uint2 *__restrict__ spill, uint32_t spill_depth) {
    const int tid = threadIdx.x;
    const uint32_t lane = (uint32_t)tid & 63u;
    const uint32_t wave = blockIdx.x * 4u + ((uint32_t)tid >> 6);
    Tracer<STACK_LDS, false> tr;
    bind_lane(tr, sc, spill, spill_depth);
    const uint32_t ray = wave * lanes_per_wave + lane;
    if(lane >= lanes_per_wave || ray >= n) {
        return;
    }
    const float *r = rays6 + 6 * (size_t)ray;
    Walk w;
    typename Tracer<STACK_LDS, false>::Rec rec;
    rec.r0 = rec.r1 = rec.r2 = rec.r3 = (f4v){0.0f, 0.0f, 0.0f, 0.0f};
    RootBox root;
    root.ref = sc.root_ref;
    for(int k = 0; k < 3; k++) {
        root.lo[k] = sc.root_lo[k];
        root.hi[k] = sc.root_hi[k];
    }
    const unsigned long long t_begin = __builtin_amdgcn_s_memtime();
    const unsigned long long t_again = __builtin_amdgcn_s_memtime();
#ifdef PT_STEP_STAMPS
    tr.stamp_last = t_again;
#endif
    tr.start(w, rec, root, make_float4(r[0], r[1], r[2], 0.0f), make_float4(r[3], r[4], r[5], __uint_as_float(0u)));
    uint32_t n_nodes = 0, n_leaves = 0, steps = 0;
    unsigned long long waiting = 0;
    for(;;) {
        if(STAMP) {
            const unsigned long long t1 = __builtin_amdgcn_s_memtime();
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
            const unsigned long long t2 = __builtin_amdgcn_s_memtime();
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            waiting += t2 - t1;
        }
        if(!tr.step(w, rec, 1, n_nodes, n_leaves)) {
            break;
        }
        steps += 1u;
    }
    const unsigned long long t_end = __builtin_amdgcn_s_memtime();
    out[ray] = make_uint4(steps, (uint32_t)waiting, (uint32_t)(t_end - t_begin), (uint32_t)(t_again - t_begin));
#ifdef PT_STEP_STAMPS
    // (the stamped build reports its segments behind the n results: 8 x 8 bytes per ray)
    unsigned long long *seg = reinterpret_cast<unsigned long long *>(out + n) + 8 * (size_t)ray;
    for(int k = 0; k < 8; k++) {
        seg[k] = tr.stamp_acc[k];
    }
#endif
}

// ---- diagnostic: the traversal alone on the rays of a finished render ----------------------------------------------------------------
// With PT_RING_LOG_RAYS set, the wavefronts' rings are long enough never to wrap, so after a render they hold every ray of the frame
// in the order the wavefront traced them.  This kernel replays them: the same hand-out / burst / leaf-batching loop as the path
// kernel, no shading, results folded into a checksum -- at WAVES wavefronts per SIMD, which the path kernel cannot choose freely
// (the shading code's registers cap it at four).  It answers what a tracer that is not tied to the shading code would deliver.
// Wavefront v replays part (v / n_logs) of `parts` equal parts of ring (v % n_logs).
template<int STACK_LDS, int WAVES>
__global__ __launch_bounds__(256, WAVES) void pt_replay_kernel(PtDevScene sc, PtLocalQueue Q, uint32_t n_logs, uint32_t parts, int refill_idle, int burst_steps,
                                                                int leaf_min, uint2 *__restrict__ spill, uint32_t spill_depth,
                                                                unsigned long long *__restrict__ out) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    const int tid = threadIdx.x;
    const uint32_t lane = (uint32_t)tid & 63u;
    const uint32_t wave = blockIdx.x * 4u + ((uint32_t)tid >> 6);
    if(wave >= n_logs * parts) {
        return;
    }
    Tracer<STACK_LDS, false> tr;
    tr.recs = (glb_f4_cptr)sc.recs;
    tr.stack_l = (lds_u2_ptr)reinterpret_cast<uint2 *>(lds_raw) + tid;
    tr.my_spill = (glb_u2_ptr)(spill + ((size_t)wave * 64 + lane) * spill_depth);
    RootBox root;
    root.ref = sc.root_ref;
    for(int k = 0; k < 3; k++) {
        root.lo[k] = sc.root_lo[k];
        root.hi[k] = sc.root_hi[k];
    }
    const size_t base = (size_t)(wave % n_logs) * Q.cap;
    // rays written: the prefix of the ring whose direction words are not the 0xff fill
    uint32_t lo = 0, hi = Q.cap;
    while(lo < hi) {
        const uint32_t mid = (lo + hi) / 2;
        if(__float_as_uint(Q.ray_d[base + mid].x) == 0xffffffffu) {
            hi = mid;
        }
        else {
            lo = mid + 1;
        }
    }
    const uint32_t part = wave / n_logs;
    uint32_t pos = (uint32_t)((unsigned long long)lo * part / parts);
    const uint32_t end = (uint32_t)((unsigned long long)lo * (part + 1) / parts);

    bool active = false;
    Walk w;
    w.o = v3(0, 0, 0);
    w.d = v3(0, 0, 1);
    w.inv = v3(0, 0, 0);
    w.pack();
    w.thr = 0.0f;
    w.dest = 0;
    w.best_t = 0.0f;
    w.best_ref = PT_REF_NONE;
    w.set_t_max(FLT_MAX);
    w.cur = PT_REF_NONE;
    w.sp = 0;
    w.occluded = false;
    typename Tracer<STACK_LDS, false>::Rec rec;
    rec.r0 = rec.r1 = rec.r2 = rec.r3 = (f4v){0.0f, 0.0f, 0.0f, 0.0f};
    uint32_t n_nodes = 0, n_leaves = 0, n_rays = 0, checksum = 0, w_steps = 0;
    for(;;) {
        if(active && w.cur == PT_REF_NONE) {
            checksum += (w.dest & PT_DEST_SHADOW) ? (w.occluded ? 1u : 2u) : (w.best_ref ^ __float_as_uint(w.best_t));
            active = false;
        }
        const unsigned long long idle_mask = __ballot(!active);
        const uint32_t n_idle = (uint32_t)__popcll(idle_mask);
        if(n_idle >= (uint32_t)refill_idle && pos < end) {
            const uint32_t left = end - pos;
            const uint32_t take = left < n_idle ? left : n_idle;
            if(!active) {
                const uint32_t rank = (uint32_t)__popcll(idle_mask & ((1ULL << lane) - 1ULL));
                if(rank < take) {
                    const float4 ro = Q.ray_o[base + pos + rank];
                    const float4 rd = Q.ray_d[base + pos + rank];
                    if(__float_as_uint(rd.w) != PT_DEST_NULL) {
                        tr.start(w, rec, root, ro, rd);
                        active = true;
                        n_rays++;
                    }
                }
            }
            pos += take;
        }
        if(__ballot(active) == 0ULL) {
            if(pos >= end) {
                break;
            }
            continue;
        }
#pragma unroll 1
        for(int burst = 0; burst < burst_steps; burst++) {
            w_steps++;
            if(!tr.step(w, rec, leaf_min, n_nodes, n_leaves)) {
                w_steps--;
                break;
            }
        }
    }
    for(int off = 32; off > 0; off >>= 1) {
        n_rays += __shfl_down(n_rays, off); // (n_nodes and n_leaves are counted for the whole wavefront: Tracer::step)
        checksum += __shfl_down(checksum, off);
    }
    if(lane == 0) {
        atomicAdd(&out[0], (unsigned long long)n_rays);
        atomicAdd(&out[1], (unsigned long long)n_nodes);
        atomicAdd(&out[2], (unsigned long long)n_leaves);
        atomicAdd(&out[3], (unsigned long long)w_steps);
        atomicAdd(&out[4], (unsigned long long)checksum);
    }
}

template<int STACK_LDS, int WAVES>
int launch_replay(hipStream_t stream, const PtDevScene &scene, const PtLocalQueue &Q, uint32_t n_logs, uint32_t parts, const PtPathConfig &cfg, uint2 *spill,
                  unsigned long long *out) {
    const size_t lds = walk_lds_bytes(STACK_LDS, false, scene);
    int blocks = 0;
    if(hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, pt_replay_kernel<STACK_LDS, WAVES>, 256, lds) != hipSuccess) {
        blocks = -1;
    }
    const uint32_t waves = n_logs * parts;
    hipLaunchKernelGGL((pt_replay_kernel<STACK_LDS, WAVES>), dim3((waves + 3) / 4), dim3(256), lds, stream, scene, Q, n_logs, parts, cfg.refill_idle,
                       cfg.burst_steps, cfg.leaf_min, spill, cfg.spill_depth, out);
    return blocks;
}

// The three routes of a walk kernel, as the path kernel's (PT_DISPATCH_PATH): records in LDS with the small stack window, records in LDS,
// records in HBM.  launch(window, in_lds) gets them as integral constants and the LDS bytes of the route.
template<typename Launch>
void dispatch_route(const PtPathConfig &cfg, const PtDevScene &scene, Launch launch) {
    if(cfg.in_lds && cfg.stack_lds == PT_PATH_STACK_LDS_SMALL) {
        launch(std::integral_constant<int, PT_PATH_STACK_LDS_SMALL>(), std::true_type(), walk_lds_bytes(PT_PATH_STACK_LDS_SMALL, true, scene));
    }
    else if(cfg.in_lds) {
        launch(std::integral_constant<int, PT_PATH_STACK_LDS>(), std::true_type(), walk_lds_bytes(PT_PATH_STACK_LDS, true, scene));
    }
    else {
        launch(std::integral_constant<int, PT_PATH_STACK_LDS>(), std::false_type(), walk_lds_bytes(PT_PATH_STACK_LDS, false, scene));
    }
}

} // namespace

#include "pt_query_kernels.h" // pt_query_kernel, pt_query_pixels_kernel, pt_occluded_kernel and their launches (behind bind_lane and dispatch_route, which they use)
#include "pt_sample_walk.h" // sample_walk: the one path-sample loop of the four files below, with gather_engine and scene_root
#include "pt_gather_kernels.h" // pt_gather_kernel, its reduce and the two kernels that make points, with their launches (behind the same two)
#include "pt_light_probe_kernels.h" // the light probes: sampling, projection and lookup kernels with their launches (behind pt_gather_kernels.h)
#include "pt_radiance_kernels.h" // radiance along free rays and captures: the sampling kernel and its reduction with their launch (behind pt_light_probe_kernels.h)
#include "pt_light_pass_kernels.h" // light-group passes: the sampling kernel with an accumulator per pass, its reduction and the mix (behind pt_radiance_kernels.h)

void pt_launch_closest(hipStream_t stream, const PtDevScene &scene, const float *rays6, uint32_t n, uint2 *out, const PtPathConfig &cfg) {
    if(n == 0) {
        return;
    }
    dispatch_route(cfg, scene, [&](auto window, auto in_lds, size_t lds) {
        hipLaunchKernelGGL((pt_closest_kernel<decltype(window)::value, decltype(in_lds)::value>), dim3((n + 255) / 256), dim3(256), lds, stream, scene, rays6, n, out,
                           cfg.spill, cfg.spill_depth);
    });
}

void pt_launch_features(hipStream_t stream, const PtDevScene &scene, const PtDevCamera &camera, const PtViewCamera *views, int32_t n_views, int32_t width, int32_t height,
                        float4 *out, const PtPathConfig &cfg, const PtFollow *follow) {
    if(width <= 0 || height <= 0 || (views != nullptr && n_views <= 0)) {
        return;
    }
    const int32_t rows = views != nullptr ? n_views * height : height, view_height = views != nullptr ? height : 0;
    const dim3 grid((unsigned)(((size_t)width * (size_t)rows + 255) / 256));
    dispatch_route(cfg, scene, [&](auto window, auto in_lds, size_t lds) {
        constexpr int kWindow = decltype(window)::value;
        constexpr bool kInLds = decltype(in_lds)::value;
        auto launch = [&](auto feature_kernel, auto follow_kernel) {
            if(follow != nullptr) {
                hipLaunchKernelGGL(follow_kernel, grid, dim3(256), lds, stream, scene, camera, width, rows, out, cfg.spill, cfg.spill_depth, views, view_height,
                                   follow->max_bounces, follow->epsilon);
            }
            else {
                hipLaunchKernelGGL(feature_kernel, grid, dim3(256), lds, stream, scene, camera, width, rows, out, cfg.spill, cfg.spill_depth, views, view_height);
            }
        };
        if(views != nullptr) {
            launch(pt_feature_kernel<kWindow, kInLds, true>, pt_follow_kernel<kWindow, kInLds, true>);
        }
        else {
            launch(pt_feature_kernel<kWindow, kInLds, false>, pt_follow_kernel<kWindow, kInLds, false>);
        }
    });
}

void pt_launch_features_motion(hipStream_t stream, const PtDevScene &scene, const PtDevCamera &camera, int32_t width, int32_t height, float4 *out, float4 *motion,
                               const PtMotionInstance *instances, uint32_t n_instances, const PtPathConfig &cfg) {
    if(width <= 0 || height <= 0) {
        return;
    }
    const dim3 grid((unsigned)(((size_t)width * (size_t)height + 255) / 256));
    dispatch_route(cfg, scene, [&](auto window, auto in_lds, size_t lds) {
        hipLaunchKernelGGL((pt_motion_kernel<decltype(window)::value, decltype(in_lds)::value>), grid, dim3(256), lds, stream, scene, camera, width, height, out, cfg.spill,
                           cfg.spill_depth, motion, instances, n_instances);
    });
}

void pt_launch_features_motion_shapes(hipStream_t stream, const PtDevScene &scene, const PtDevCamera &camera, int32_t width, int32_t height, float4 *out, float4 *motion,
                                      const PtShapeMotionInstance *instances, uint32_t n_instances, const uint32_t *face_of, uint32_t first_object, const PtPathConfig &cfg) {
    if(width <= 0 || height <= 0) {
        return;
    }
    const dim3 grid((unsigned)(((size_t)width * (size_t)height + 255) / 256));
    dispatch_route(cfg, scene, [&](auto window, auto in_lds, size_t lds) {
        hipLaunchKernelGGL((pt_motion_shapes_kernel<decltype(window)::value, decltype(in_lds)::value>), grid, dim3(256), lds, stream, scene, camera, width, height, out, cfg.spill,
                           cfg.spill_depth, motion, instances, n_instances, face_of, first_object);
    });
}

void pt_launch_steptime(hipStream_t stream, const PtDevScene &scene, const float *rays6, uint32_t n, uint32_t lanes_per_wave, uint4 *out, uint2 *spill, uint32_t spill_depth, int flags) {
    const uint32_t waves = (n + lanes_per_wave - 1) / lanes_per_wave;
    const size_t lds = walk_lds_bytes(8, false, scene);
    if(flags & 2) { // bit 1: stamp the waits (each stamp is a scalar memory round trip of its own: the totals of such a run are inflated)
        hipLaunchKernelGGL((pt_steptime_kernel<8, true>), dim3((waves + 3) / 4), dim3(256), lds, stream, scene, rays6, n, lanes_per_wave, out, spill, spill_depth);
    }
    else {
        hipLaunchKernelGGL((pt_steptime_kernel<8, false>), dim3((waves + 3) / 4), dim3(256), lds, stream, scene, rays6, n, lanes_per_wave, out, spill, spill_depth);
    }
}

int pt_launch_replay(hipStream_t stream, const PtDevScene &scene, const PtLocalQueue &Q, uint32_t n_logs, uint32_t parts, int waves_per_simd, const PtPathConfig &cfg,
                     uint2 *spill, unsigned long long *out) {
    switch(waves_per_simd) {
    case 4: return launch_replay<8, 4>(stream, scene, Q, n_logs, parts, cfg, spill, out);
    case 5: return launch_replay<8, 5>(stream, scene, Q, n_logs, parts, cfg, spill, out);
    case 6: return launch_replay<8, 6>(stream, scene, Q, n_logs, parts, cfg, spill, out);
    case 7: return launch_replay<8, 7>(stream, scene, Q, n_logs, parts, cfg, spill, out);
    default: return launch_replay<8, 8>(stream, scene, Q, n_logs, parts, cfg, spill, out);
    }
}
