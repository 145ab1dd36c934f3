// unit_probe.hip -- TEST ONLY: the device functions of cpupathtrace_amd/csrc/pt_device.h and pt_libm.h, one at a time.
//
// Built by tests/unit_probe.py into tests/hip/libunit_probe.so with the product's compiler flags; not part of libpathtrace_hip.so.
// The product headers are included unchanged.  Every entry point ptu_* takes the arrays of the matching method of oracle.Checker
// (oracle/__init__.py), copies them to device 0, runs a one-thread-per-case kernel (256-thread workgroups, guarded tail), copies the
// results back and returns the HIP error code (0 = hipSuccess).  ptu_estimator_run (the per-pixel estimator of pt_shading.h) keeps its
// outputs between guard bands (guard_band.h) and returns PT_GUARD_TOUCHED + the buffer's number when one was written.  The libm entries also evaluate the same PT_HD function on the host and
// return the number of inputs whose results differ and the first 16 of them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <thread>
#include <vector>

#include "../../cpupathtrace_amd/csrc/pt_device.h"
#include "../../cpupathtrace_amd/csrc/pt_shading.h"
#include "../../include/pt_hip.h"
#include "guard_band.h"

using namespace ptd;

namespace {

constexpr unsigned WG = 256;

// ---- plumbing ------------------------------------------------------------------------------------------------------

// The first HIP error of an entry point; every later step is skipped once it is set (guard_band.h; the guard part is used by the entries
// that keep their outputs between guard bands).
using Status = GuardStatus;

// A device array of n elements of T, filled from `src` when given; freed when it goes out of scope.
template<typename T>
struct Dev {
    T *p = nullptr;
    size_t n = 0;
    Status &st;
    Dev(Status &status, size_t count, const T *src = nullptr) : n(count), st(status) {
        if(!st.ok()) {
            return;
        }
        st(hipMalloc(reinterpret_cast<void **>(&p), std::max<size_t>(n, 1) * sizeof(T)));
        if(st.ok() && src != nullptr && n > 0) {
            st(hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice));
        }
    }
    Dev(const Dev &) = delete;
    Dev &operator=(const Dev &) = delete;
    ~Dev() {
        if(p != nullptr) {
            (void)hipFree(p);
        }
    }
    void get(T *dst) {
        if(st.ok() && n > 0) {
            st(hipMemcpy(dst, p, n * sizeof(T), hipMemcpyDeviceToHost));
        }
    }
};

dim3 grid_for(uint64_t n) {
    return dim3(static_cast<unsigned>(std::max<uint64_t>((n + WG - 1) / WG, 1)));
}

int finish(Status &st) {
    st(hipGetLastError());
    st(hipDeviceSynchronize());
    return static_cast<int>(st.err);
}

uint64_t seed_to_state(uint64_t seed) {
    return seed ^ (~seed << 32); // RandomEngine(seed), base.h:26
}

PT_D V3 ldv(const float *p, uint64_t i) {
    return ld3(p + 3 * i);
}
PT_D void stv(float *p, V3 v) {
    p[0] = v.x;
    p[1] = v.y;
    p[2] = v.z;
}

// ---- kernels: engine ---------------------------------------------------------------------------------------------------

// sequences of one engine: a single case, so a single thread walks it
__global__ void k_rng_draws(uint64_t state, uint64_t n, uint32_t *out, uint64_t *out_state) {
    if(blockIdx.x * blockDim.x + threadIdx.x != 0) {
        return;
    }
    for(uint64_t i = 0; i < n; i++) {
        out[i] = rng_draw(state);
    }
    *out_state = state;
}

__global__ void k_uniform_floats(uint64_t state, float a, float b, uint64_t n, float *out, uint64_t *out_state) {
    if(blockIdx.x * blockDim.x + threadIdx.x != 0) {
        return;
    }
    for(uint64_t i = 0; i < n; i++) {
        out[i] = rng_uniform(state, a, b);
    }
    *out_state = state;
}

__global__ void k_bernoulli(uint64_t state, double p, uint64_t n, uint8_t *out, uint64_t *out_state) {
    if(blockIdx.x * blockDim.x + threadIdx.x != 0) {
        return;
    }
    for(uint64_t i = 0; i < n; i++) {
        out[i] = rng_bernoulli(state, p) ? 1 : 0;
    }
    *out_state = state;
}

// ---- kernels: primitives -----------------------------------------------------------------------------------------------

template<bool WALK>
__global__ void k_slab(uint64_t n, const float *boxes, const float *rays, float *out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(i >= n) {
        return;
    }
    const V3 lo = ld3(boxes + 6 * i), hi = ld3(boxes + 6 * i + 3), o = ld3(rays + 6 * i), d = ld3(rays + 6 * i + 3);
    const V3 inv = slab_inverse(d);
    out[i] = WALK ? slab_walk(lo, hi, o, inv) : slab_test(lo, hi, o, inv);
}

__global__ void k_tri_intersect(uint64_t n, const float *tri, const uint8_t *cull, const float *rays, float *out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(i >= n) {
        return;
    }
    // the edges are the fp32 differences the reference forms on every call (object.cpp:149-150); the product forms them once, on the host
    const V3 a = ld3(tri + 9 * i), b = ld3(tri + 9 * i + 3), c = ld3(tri + 9 * i + 6);
    out[i] = tri_intersect(a, b - a, c - a, cull[i] != 0, ld3(rays + 6 * i), ld3(rays + 6 * i + 3));
}

__global__ void k_tri_normal(uint64_t n, const float *tri, const float *nrm, const float *pos, float *out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(i >= n) {
        return;
    }
    const V3 a = ld3(tri + 9 * i), b = ld3(tri + 9 * i + 3), c = ld3(tri + 9 * i + 6);
    stv(out + 3 * i, tri_normal(a, b - a, c - a, ld3(nrm + 9 * i), ld3(nrm + 9 * i + 3), ld3(nrm + 9 * i + 6), ldv(pos, i)));
}

__global__ void k_sphere_intersect(uint64_t n, const float *sph, const float *rays, float *out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(i >= n) {
        return;
    }
    out[i] = sphere_intersect(ld3(sph + 4 * i), sph[4 * i + 3], ld3(rays + 6 * i), ld3(rays + 6 * i + 3));
}

// ---- kernels: BSDFs ----------------------------------------------------------------------------------------------------

PT_D Material probe_material(int kind, int one_way, float ior) {
    Material m;
    m.diffuse = c4(1.0f, 1.0f, 1.0f, 1.0f);
    m.specular = c4(1.0f, 1.0f, 1.0f, 1.0f);
    m.emission = c4(0.0f, 0.0f, 0.0f, 0.0f);
    m.ior = ior;
    m.bsdf = kind;
    m.one_way = one_way;
    return m;
}

__global__ void k_bsdf_propagate(int kind, int one_way, uint64_t n, const float *rays, const float *pos, const float *nrm, float epsilon,
                                 const float *ior, const uint64_t *states, float *out_ray, float *out_factor, float *out_pd,
                                 uint64_t *out_states) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(i >= n) {
        return;
    }
    const Material m = probe_material(kind, one_way, ior[i]);
    uint64_t rng = states[i];
    float factor, pd;
    const Ray r = bsdf_propagate(m, ld3(rays + 6 * i + 3), ldv(pos, i), ldv(nrm, i), epsilon, rng, factor, pd);
    stv(out_ray + 6 * i, r.o);
    stv(out_ray + 6 * i + 3, r.d);
    out_factor[i] = factor;
    out_pd[i] = pd;
    out_states[i] = rng;
}

__global__ void k_bsdf_spectrum(int kind, int one_way, uint64_t n, const float *from_dir, const float *to_dir, const float *nrm,
                                const float *light, const float *diffuse, const float *specular, int synthetic, float *out_rgba,
                                float *out_shade, float *out_p) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(i >= n) {
        return;
    }
    Material m = probe_material(kind, one_way, 1.0f);
    m.diffuse = c4(diffuse[4 * i], diffuse[4 * i + 1], diffuse[4 * i + 2], diffuse[4 * i + 3]);
    m.specular = c4(specular[4 * i], specular[4 * i + 1], specular[4 * i + 2], specular[4 * i + 3]);
    const C4 l = c4(light[4 * i], light[4 * i + 1], light[4 * i + 2], light[4 * i + 3]);
    float shade, p;
    const C4 c = bsdf_spectrum(m, ldv(from_dir, i), ldv(to_dir, i), ldv(nrm, i), l, synthetic != 0, shade, p);
    out_rgba[4 * i] = c.r;
    out_rgba[4 * i + 1] = c.g;
    out_rgba[4 * i + 2] = c.b;
    out_rgba[4 * i + 3] = c.a;
    out_shade[i] = shade;
    out_p[i] = p;
}

// ---- kernels: camera ---------------------------------------------------------------------------------------------------

// camera_shoot reads its camera from the kernel arguments, camera_shoot_lane from a table in global memory, as in pt_path.hip
__global__ void k_camera_shoot(PtDevCamera cam, uint64_t n, const float *xy, float pixel_width, float pixel_height, const uint64_t *states,
                               float *out_ray, uint64_t *out_states) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(i >= n) {
        return;
    }
    uint64_t rng = states[i];
    const Ray r = camera_shoot(cam, xy[2 * i], xy[2 * i + 1], pixel_width, pixel_height, rng);
    stv(out_ray + 6 * i, r.o);
    stv(out_ray + 6 * i + 3, r.d);
    out_states[i] = rng;
}

__global__ void k_camera_shoot_lane(const PtViewCamera *views, uint64_t n, const float *xy, float pixel_width, float pixel_height,
                                    const uint64_t *states, float *out_ray, uint64_t *out_states) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(i >= n) {
        return;
    }
    uint64_t rng = states[i];
    const Ray r = camera_shoot_lane(views[0].cam, xy[2 * i], xy[2 * i + 1], pixel_width, pixel_height, rng);
    stv(out_ray + 6 * i, r.o);
    stv(out_ray + 6 * i + 3, r.d);
    out_states[i] = rng;
}

// Camera::Camera (src/camera.cpp:53-76) as derive_camera of pt_api.cpp forms it: the same fp32 operations in the same order
struct H3 {
    float x, y, z;
};
H3 h_ld(const float *p) {
    return H3{p[0], p[1], p[2]};
}
H3 h_scale(H3 a, float f) {
    return H3{a.x * f, a.y * f, a.z * f};
}
H3 h_normalize(H3 a) {
    float d = 0.0f;
    d += a.x * a.x;
    d += a.y * a.y;
    d += a.z * a.z;
    const float inv = 1.0f / std::sqrt(d);
    return h_scale(a, inv);
}
PtDevCamera probe_camera(const pt_camera_params *c) {
    PtDevCamera cam{};
    const H3 origin = h_ld(c->origin);
    const H3 look = h_ld(c->look_at);
    const H3 forward = h_scale(h_normalize(H3{look.x - origin.x, look.y - origin.y, look.z - origin.z}), c->focal_length);
    const float height_half = c->height / 2.0f;
    const H3 up = h_scale(h_normalize(h_ld(c->up)), height_half);
    const H3 right_dir = h_normalize(H3{forward.y * up.z - forward.z * up.y, forward.z * up.x - forward.x * up.z, forward.x * up.y - forward.y * up.x});
    const H3 right = h_scale(right_dir, height_half * c->aspect_ratio);
    const H3 v[4] = {origin, forward, up, right};
    float *dst[4] = {cam.origin, cam.forward, cam.up, cam.right};
    for(int i = 0; i < 4; i++) {
        dst[i][0] = v[i].x;
        dst[i][1] = v[i].y;
        dst[i][2] = v[i].z;
    }
    cam.aperture_width_half = c->aperture_width / 2.0f;
    cam.aperture_height_half = c->aperture_height / 2.0f;
    cam.aperture_kind = c->aperture_kind;
    const float lo = (c->hex_ratio < 0.0f) ? 0.0f : c->hex_ratio; // std::max(hex_ratio, 0), then std::min(.., 1): camera.cpp:22-24
    cam.hex_ratio = (1.0f < lo) ? 1.0f : lo;
    cam.focal_plane_dist = c->focal_plane_dist;
    return cam;
}

// ---- kernels: estimator -------------------------------------------------------------------------------------------------

// One sequence per thread through the loop of the path kernel's finished-sample branch (pt_path.hip): estimator_reset; per sample the
// overlap question, estimator_add if the sample was collected, pixel_sample++; estimator_finish on acceptance or at max_sample_count.
// The estimator and its closed candidates lie in global memory, as PtSlots::est / cand do.
__global__ void k_estimator_run(PtDevOptions opt, uint64_t n, int len, const float *contrib, const uint8_t *collected, PtEstimator *est,
                                PtCandidate *cand_all, float *out_value, uint8_t *out_accepted, uint8_t *out_overlap) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(i >= n) {
        return;
    }
    PtCandidate *cand = cand_all + i * PT_MAX_CANDIDATES;
    estimator_reset(est[i], opt);
    for(;;) {
        PtEstimator e = est[i];
        if(e.pixel_sample >= len) {
            break; // (the host refuses len < max_sample_count; this keeps every read inside the arrays regardless)
        }
        const uint64_t at = i * (uint64_t)len + (uint64_t)e.pixel_sample;
        out_overlap[at] = estimator_safe_to_overlap(e, opt) ? 1 : 0;
        bool accepted = false;
        if(collected[at] != 0) {
            accepted = estimator_add(e, cand, opt, ld4(contrib + 4 * at));
        }
        e.pixel_sample++;
        est[i] = e;
        if(accepted || e.pixel_sample >= opt.max_sample_count) {
            st4(out_value + 4 * i, estimator_finish(e, cand, opt, accepted));
            out_accepted[i] = accepted ? 1 : 0;
            break;
        }
    }
}

// ---- kernels: libm ---------------------------------------------------------------------------------------------------------

// out[4 * i ..]: sinf, cosf, and the two results of sincosf
PT_HD void sincos_case(uint32_t in, uint32_t *out) {
    const float f = ptm::as_f32(in);
    float s, c;
    ptm::sincosf_glibc(f, &s, &c);
    out[0] = ptm::as_u32(ptm::sinf_glibc(f));
    out[1] = ptm::as_u32(ptm::cosf_glibc(f));
    out[2] = ptm::as_u32(s);
    out[3] = ptm::as_u32(c);
}

__global__ void k_libm_sincos(uint64_t n, const uint32_t *in, uint32_t *out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(i >= n) {
        return;
    }
    uint32_t r[4];
    sincos_case(in[i], r);
    out[4 * i] = r[0];
    out[4 * i + 1] = r[1];
    out[4 * i + 2] = r[2];
    out[4 * i + 3] = r[3];
}

PT_HD uint32_t pow_case(int full, uint32_t x, uint32_t y) {
    const float fx = ptm::as_f32(x), fy = ptm::as_f32(y);
    return ptm::as_u32(full ? ptm::powf_glibc_full(fx, fy) : ptm::powf_glibc(fx, fy));
}

// y_stride 1: pairs (x[i], y[i]); y_stride 0: every x[i] with the one exponent y[0]
__global__ void k_libm_pow(int full, uint64_t n, const uint32_t *x, const uint32_t *y, uint64_t y_stride, uint32_t *out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(i >= n) {
        return;
    }
    out[i] = pow_case(full, x[i], y[i * y_stride]);
}

__global__ void k_libm_acos(uint64_t n, const uint32_t *in, uint32_t *out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(i >= n) {
        return;
    }
    out[i] = ptm::as_u32(ptm::acosf_glibc(ptm::as_f32(in[i])));
}

// The host pass: f(i) is true where case i differs.  Up to 16 threads, each over one contiguous share of the cases; the mismatching
// inputs with the lowest indices are the ones reported.
struct Mismatches {
    uint64_t bad = 0;
    std::vector<uint64_t> first; // indices of mismatching cases
};

template<typename F>
Mismatches host_compare(uint64_t n, F differs) {
    const unsigned hw = std::thread::hardware_concurrency();
    const uint64_t n_threads = std::max<uint64_t>(1, std::min<uint64_t>({16, hw == 0 ? 1 : hw, (n + 65535) / 65536}));
    std::vector<Mismatches> part(n_threads);
    std::vector<std::thread> threads;
    for(uint64_t t = 0; t < n_threads; t++) {
        threads.emplace_back([&, t]() {
            const uint64_t begin = n * t / n_threads, end = n * (t + 1) / n_threads;
            for(uint64_t i = begin; i < end; i++) {
                if(differs(i)) {
                    part[t].bad++;
                    if(part[t].first.size() < 16) {
                        part[t].first.push_back(i);
                    }
                }
            }
        });
    }
    for(auto &th : threads) {
        th.join();
    }
    Mismatches all;
    for(const auto &p : part) {
        all.bad += p.bad;
        for(uint64_t i : p.first) {
            if(all.first.size() < 16) {
                all.first.push_back(i);
            }
        }
    }
    return all;
}

// NaN results compare by NaN-ness, everything else by bits
bool bits_differ(uint32_t a, uint32_t b) {
    const bool a_nan = (a & 0x7fffffffu) > 0x7f800000u, b_nan = (b & 0x7fffffffu) > 0x7f800000u;
    return (a_nan || b_nan) ? (a_nan != b_nan) : (a != b);
}

} // namespace

extern "C" {

int ptu_device_count(void) {
    int n = 0;
    if(hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

const char *ptu_error_string(int code) {
    return code >= PT_GUARD_TOUCHED ? "a guard band was written" : hipGetErrorString(static_cast<hipError_t>(code));
}

// ---- engine --------------------------------------------------------------------------------------------------------------

int ptu_rng_draws(uint64_t seed, uint64_t n, uint32_t *out, uint64_t *out_state) {
    Status st;
    Dev<uint32_t> d_out(st, n);
    Dev<uint64_t> d_state(st, 1);
    if(st.ok()) {
        k_rng_draws<<<dim3(1), dim3(WG)>>>(seed_to_state(seed), n, d_out.p, d_state.p);
    }
    d_out.get(out);
    d_state.get(out_state);
    return finish(st);
}

int ptu_uniform_floats(uint64_t seed, float a, float b, uint64_t n, float *out, uint64_t *out_state) {
    Status st;
    Dev<float> d_out(st, n);
    Dev<uint64_t> d_state(st, 1);
    if(st.ok()) {
        k_uniform_floats<<<dim3(1), dim3(WG)>>>(seed_to_state(seed), a, b, n, d_out.p, d_state.p);
    }
    d_out.get(out);
    d_state.get(out_state);
    return finish(st);
}

int ptu_bernoulli(uint64_t seed, double p, uint64_t n, uint8_t *out_flags, uint64_t *out_state) {
    Status st;
    Dev<uint8_t> d_out(st, n);
    Dev<uint64_t> d_state(st, 1);
    if(st.ok()) {
        k_bernoulli<<<dim3(1), dim3(WG)>>>(seed_to_state(seed), p, n, d_out.p, d_state.p);
    }
    d_out.get(out_flags);
    d_state.get(out_state);
    return finish(st);
}

// ---- primitives ------------------------------------------------------------------------------------------------------------

static int slab_entry(bool walk, uint64_t n, const float *boxes, const float *rays, float *out_t) {
    Status st;
    Dev<float> d_boxes(st, 6 * n, boxes), d_rays(st, 6 * n, rays), d_out(st, n);
    if(st.ok()) {
        if(walk) {
            k_slab<true><<<grid_for(n), dim3(WG)>>>(n, d_boxes.p, d_rays.p, d_out.p);
        }
        else {
            k_slab<false><<<grid_for(n), dim3(WG)>>>(n, d_boxes.p, d_rays.p, d_out.p);
        }
    }
    d_out.get(out_t);
    return finish(st);
}

int ptu_aabb_intersect(uint64_t n, const float *boxes, const float *rays, float *out_t) {
    return slab_entry(false, n, boxes, rays, out_t);
}

int ptu_slab_walk(uint64_t n, const float *boxes, const float *rays, float *out_t) {
    return slab_entry(true, n, boxes, rays, out_t);
}

int ptu_tri_intersect(uint64_t n, const float *tri, const uint8_t *cull, const float *rays, float *out_t) {
    Status st;
    Dev<float> d_tri(st, 9 * n, tri), d_rays(st, 6 * n, rays), d_out(st, n);
    Dev<uint8_t> d_cull(st, n, cull);
    if(st.ok()) {
        k_tri_intersect<<<grid_for(n), dim3(WG)>>>(n, d_tri.p, d_cull.p, d_rays.p, d_out.p);
    }
    d_out.get(out_t);
    return finish(st);
}

int ptu_tri_normal(uint64_t n, const float *tri, const float *nrm, const float *pos, float *out_n) {
    Status st;
    Dev<float> d_tri(st, 9 * n, tri), d_nrm(st, 9 * n, nrm), d_pos(st, 3 * n, pos), d_out(st, 3 * n);
    if(st.ok()) {
        k_tri_normal<<<grid_for(n), dim3(WG)>>>(n, d_tri.p, d_nrm.p, d_pos.p, d_out.p);
    }
    d_out.get(out_n);
    return finish(st);
}

int ptu_sphere_intersect(uint64_t n, const float *sph, const float *rays, float *out_t) {
    Status st;
    Dev<float> d_sph(st, 4 * n, sph), d_rays(st, 6 * n, rays), d_out(st, n);
    if(st.ok()) {
        k_sphere_intersect<<<grid_for(n), dim3(WG)>>>(n, d_sph.p, d_rays.p, d_out.p);
    }
    d_out.get(out_t);
    return finish(st);
}

// ---- BSDFs -----------------------------------------------------------------------------------------------------------------

int ptu_bsdf_propagate(int kind, int one_way, uint64_t n, const float *rays, const float *pos, const float *nrm, float epsilon, const float *ior,
                       const uint64_t *states, float *out_ray, float *out_factor, float *out_pd, uint64_t *out_states) {
    Status st;
    Dev<float> d_rays(st, 6 * n, rays), d_pos(st, 3 * n, pos), d_nrm(st, 3 * n, nrm), d_ior(st, n, ior);
    Dev<uint64_t> d_states(st, n, states), d_out_states(st, n);
    Dev<float> d_out_ray(st, 6 * n), d_out_factor(st, n), d_out_pd(st, n);
    if(st.ok()) {
        k_bsdf_propagate<<<grid_for(n), dim3(WG)>>>(kind, one_way, n, d_rays.p, d_pos.p, d_nrm.p, epsilon, d_ior.p, d_states.p, d_out_ray.p,
                                                    d_out_factor.p, d_out_pd.p, d_out_states.p);
    }
    d_out_ray.get(out_ray);
    d_out_factor.get(out_factor);
    d_out_pd.get(out_pd);
    d_out_states.get(out_states);
    return finish(st);
}

int ptu_bsdf_spectrum(int kind, int one_way, uint64_t n, const float *from_dir, const float *to_dir, const float *nrm, const float *light_rgba,
                      const float *diffuse, const float *specular, int synthetic, float *out_rgba, float *out_shade, float *out_p) {
    Status st;
    Dev<float> d_from(st, 3 * n, from_dir), d_to(st, 3 * n, to_dir), d_nrm(st, 3 * n, nrm), d_light(st, 4 * n, light_rgba);
    Dev<float> d_diffuse(st, 4 * n, diffuse), d_specular(st, 4 * n, specular);
    Dev<float> d_rgba(st, 4 * n), d_shade(st, n), d_p(st, n);
    if(st.ok()) {
        k_bsdf_spectrum<<<grid_for(n), dim3(WG)>>>(kind, one_way, n, d_from.p, d_to.p, d_nrm.p, d_light.p, d_diffuse.p, d_specular.p, synthetic,
                                                   d_rgba.p, d_shade.p, d_p.p);
    }
    d_rgba.get(out_rgba);
    d_shade.get(out_shade);
    d_p.get(out_p);
    return finish(st);
}

// ---- camera ------------------------------------------------------------------------------------------------------------------

static int camera_entry(bool lane, const pt_camera_params *cp, uint64_t n, const float *xy, float pixel_width, float pixel_height,
                        const uint64_t *states, float *out_ray, uint64_t *out_states) {
    Status st;
    PtViewCamera view{};
    view.cam = probe_camera(cp);
    Dev<PtViewCamera> d_views(st, 1, &view);
    Dev<float> d_xy(st, 2 * n, xy), d_out_ray(st, 6 * n);
    Dev<uint64_t> d_states(st, n, states), d_out_states(st, n);
    if(st.ok()) {
        if(lane) {
            k_camera_shoot_lane<<<grid_for(n), dim3(WG)>>>(d_views.p, n, d_xy.p, pixel_width, pixel_height, d_states.p, d_out_ray.p, d_out_states.p);
        }
        else {
            k_camera_shoot<<<grid_for(n), dim3(WG)>>>(view.cam, n, d_xy.p, pixel_width, pixel_height, d_states.p, d_out_ray.p, d_out_states.p);
        }
    }
    d_out_ray.get(out_ray);
    d_out_states.get(out_states);
    return finish(st);
}

int ptu_camera_shoot(const pt_camera_params *cp, uint64_t n, const float *xy, float pixel_width, float pixel_height, const uint64_t *states,
                     float *out_ray, uint64_t *out_states) {
    return camera_entry(false, cp, n, xy, pixel_width, pixel_height, states, out_ray, out_states);
}

int ptu_camera_shoot_lane(const pt_camera_params *cp, uint64_t n, const float *xy, float pixel_width, float pixel_height, const uint64_t *states,
                          float *out_ray, uint64_t *out_states) {
    return camera_entry(true, cp, n, xy, pixel_width, pixel_height, states, out_ray, out_states);
}

// ---- estimator ---------------------------------------------------------------------------------------------------------------

// The arguments and results of oracle_estimator_run (oracle/pt_oracle.h; cand_cap is PT_MAX_CANDIDATES here) plus out_overlap [n][len]:
// estimator_safe_to_overlap before every consumed sample, 0 behind the last one.  The options are derived as derive_options of pt_api.cpp
// derives them (worker.cpp:158-164); overlap_bound = stop_bound.
int ptu_estimator_run(int min_sample_count, int max_sample_count, int stop_bound, uint64_t n, int len, const float *contrib,
                      const uint8_t *collected, float *out_value, uint8_t *out_accepted, int32_t *out_consumed, float *out_est_f,
                      int32_t *out_est_i, float *out_cand_f, int32_t *out_cand_count, uint8_t *out_overlap) {
    static_assert(sizeof(PtEstimator) == 128 && sizeof(PtCandidate) == 48, "the probe splits these records into float and int parts");
    if(len < max_sample_count || len < 1 || max_sample_count < 1) {
        return static_cast<int>(hipErrorInvalidValue);
    }
    PtDevOptions d{};
    d.image_width = 1;
    d.image_height = 1;
    d.min_sample_count = min_sample_count;
    d.max_sample_count = max_sample_count;
    d.overlap_bound = stop_bound;
    d.pixel_width = 1.0f;
    d.pixel_height = 1.0f;
    d.stats_sample_count = std::min(std::max(min_sample_count / 4, 1), 64);
    d.candidate_batch_count = std::max(std::max(min_sample_count, max_sample_count / 4) / d.stats_sample_count, 2);
    d.check_sample_count =
      std::min(std::max({min_sample_count / 2, (max_sample_count - min_sample_count) / 8, 8, d.stats_sample_count}), 1024) / d.stats_sample_count;

    Status st;
    const size_t g = WG + 64, steps = (size_t)n * (size_t)len;
    Dev<float> d_contrib(st, 4 * steps, contrib);
    Dev<uint8_t> d_collected(st, steps, collected);
    Guarded<PtEstimator> d_est(st, n, g);
    Guarded<PtCandidate> d_cand(st, n * PT_MAX_CANDIDATES, g);
    Guarded<float> d_value(st, 4 * n, g);
    Guarded<uint8_t> d_accepted(st, n, g), d_overlap(st, steps, g);
    if(st.ok()) {
        k_estimator_run<<<grid_for(n), dim3(WG)>>>(d, n, len, d_contrib.p, d_collected.p, d_est.p(), d_cand.p(), d_value.p(), d_accepted.p(),
                                                   d_overlap.p());
        st(hipGetLastError());
        st(hipDeviceSynchronize());
    }
    std::vector<PtEstimator> est(n);
    std::vector<PtCandidate> cand(n * PT_MAX_CANDIDATES);
    d_est.get(est.data());
    d_cand.get(cand.data());
    d_value.get(out_value);
    d_accepted.get(out_accepted);
    d_overlap.get(out_overlap);
    const int rc = finish(st);
    if(rc != 0) {
        return rc;
    }
    for(uint64_t i = 0; i < n; i++) {
        const PtEstimator &e = est[i];
        const float *f[6] = {e.pixel_value, e.contribution_mean, e.contribution_m2, e.sample_aggregate, e.candidate_mean, e.candidate_m2};
        for(int j = 0; j < 6; j++) {
            std::copy(f[j], f[j] + 4, out_est_f + 24 * i + 4 * j);
        }
        const int32_t v[8] = {e.collected_sample_count, e.contribution_count, e.stats_sample_index, e.candidate_count,
                              e.remaining_checks,       e.n_candidates,       e.pixel_sample,       e.pad};
        std::copy(v, v + 8, out_est_i + 8 * i);
        out_consumed[i] = e.pixel_sample;
        for(int j = 0; j < PT_MAX_CANDIDATES; j++) {
            const PtCandidate &c = cand[i * PT_MAX_CANDIDATES + j];
            std::copy(c.mean, c.mean + 4, out_cand_f + 8 * (i * PT_MAX_CANDIDATES + j));
            std::copy(c.m2, c.m2 + 4, out_cand_f + 8 * (i * PT_MAX_CANDIDATES + j) + 4);
            out_cand_count[i * PT_MAX_CANDIDATES + j] = c.count;
        }
    }
    return st.code();
}

int ptu_max_candidates(void) {
    return PT_MAX_CANDIDATES;
}

// ---- libm: device header against the same header compiled for the host ------------------------------------------------------
//
// out_bad: number of inputs for which any result differs; out_first: up to 16 of them (the inputs' bit patterns; pairs (x, y) for pow),
// unused entries are left alone.  out_bad_libc: number of inputs for which the header's host compile differs from the C library the
// probe runs against (the glibc leg of the chain on the very inputs of the device leg; every caller stays inside the restated domain).

int ptu_libm_sincos(uint64_t n, const uint32_t *in, uint64_t *out_bad, uint32_t *out_first, uint64_t *out_bad_libc) {
    Status st;
    Dev<uint32_t> d_in(st, n, in), d_out(st, 4 * n);
    if(st.ok()) {
        k_libm_sincos<<<grid_for(n), dim3(WG)>>>(n, d_in.p, d_out.p);
    }
    std::vector<uint32_t> got(4 * n);
    d_out.get(got.data());
    const int rc = finish(st);
    if(rc != 0) {
        return rc;
    }
    const Mismatches m = host_compare(n, [&](uint64_t i) {
        uint32_t want[4];
        sincos_case(in[i], want);
        bool bad = false;
        for(int k = 0; k < 4; k++) {
            bad |= bits_differ(got[4 * i + k], want[k]);
        }
        return bad;
    });
    *out_bad = m.bad;
    for(size_t k = 0; k < m.first.size(); k++) {
        out_first[k] = in[m.first[k]];
    }
    *out_bad_libc = host_compare(n, [&](uint64_t i) {
        uint32_t mine[4];
        sincos_case(in[i], mine);
        const float f = ptm::as_f32(in[i]);
        return bits_differ(mine[0], ptm::as_u32(::sinf(f))) || bits_differ(mine[1], ptm::as_u32(::cosf(f)));
    }).bad;
    return 0;
}

// full != 0: powf_glibc_full, else powf_glibc.  paired != 0: the pairs (x[i], y[i]) (nx == ny); otherwise every x with every y (nx * ny
// cases, one launch per exponent so that no more than nx results are held at a time).
int ptu_libm_pow(int full, uint64_t nx, const uint32_t *x, uint64_t ny, const uint32_t *y, int paired, uint64_t *out_bad, uint32_t *out_first,
                 uint64_t *out_bad_libc) {
    Status st;
    if(paired && nx != ny) {
        return static_cast<int>(hipErrorInvalidValue);
    }
    Dev<uint32_t> d_x(st, nx, x), d_y(st, ny, y), d_out(st, nx);
    std::vector<uint32_t> got(nx);
    uint64_t bad = 0, bad_libc = 0, n_first = 0;
    const uint64_t rounds = paired ? 1 : ny;
    for(uint64_t j = 0; j < rounds && st.ok(); j++) {
        k_libm_pow<<<grid_for(nx), dim3(WG)>>>(full, nx, d_x.p, d_y.p + (paired ? 0 : j), paired ? 1 : 0, d_out.p);
        d_out.get(got.data());
        const int rc = finish(st);
        if(rc != 0) {
            return rc;
        }
        const Mismatches m = host_compare(nx, [&](uint64_t i) { return bits_differ(got[i], pow_case(full, x[i], y[paired ? i : j])); });
        bad += m.bad;
        bad_libc += host_compare(nx, [&](uint64_t i) {
            const uint32_t yb = y[paired ? i : j];
            return bits_differ(pow_case(full, x[i], yb), ptm::as_u32(::powf(ptm::as_f32(x[i]), ptm::as_f32(yb))));
        }).bad;
        for(size_t k = 0; k < m.first.size() && n_first < 16; k++, n_first++) {
            out_first[2 * n_first] = x[m.first[k]];
            out_first[2 * n_first + 1] = y[paired ? m.first[k] : j];
        }
    }
    *out_bad = bad;
    *out_bad_libc = bad_libc;
    return static_cast<int>(st.err);
}

int ptu_libm_acos(uint64_t n, const uint32_t *in, uint64_t *out_bad, uint32_t *out_first, uint64_t *out_bad_libc) {
    Status st;
    Dev<uint32_t> d_in(st, n, in), d_out(st, n);
    if(st.ok()) {
        k_libm_acos<<<grid_for(n), dim3(WG)>>>(n, d_in.p, d_out.p);
    }
    std::vector<uint32_t> got(n);
    d_out.get(got.data());
    const int rc = finish(st);
    if(rc != 0) {
        return rc;
    }
    const Mismatches m = host_compare(n, [&](uint64_t i) { return bits_differ(got[i], ptm::as_u32(ptm::acosf_glibc(ptm::as_f32(in[i])))); });
    *out_bad = m.bad;
    for(size_t k = 0; k < m.first.size(); k++) {
        out_first[k] = in[m.first[k]];
    }
    *out_bad_libc = host_compare(n, [&](uint64_t i) {
        const float f = ptm::as_f32(in[i]);
        return bits_differ(ptm::as_u32(ptm::acosf_glibc(f)), ptm::as_u32(::acosf(f)));
    }).bad;
    return 0;
}

} // extern "C"
