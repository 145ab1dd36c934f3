// follow_probe.hip -- TEST ONLY: bsdf_follow of pt_device.h (the deterministic continuation of a followed feature ray, include/pt_features.h)
// behind one entry point, one thread per case, the outputs between guard bands (guard_band.h).  Built by tests/follow_probe.py with the
// product's compiler and flags into tests/hip/libfollow_probe.so; not part of libpathtrace_hip.so.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "../../cpupathtrace_amd/csrc/pt_device.h"
#include "guard_band.h"

using namespace ptd;

namespace {

constexpr unsigned WG = 256;
constexpr size_t GUARD = 1024; // elements on either side of an output

// out_ray[6 i ..] = the ray bsdf_follow returns for case i, out_reflected[i] = its flag; one thread per case, the tail guarded
__global__ void k_bsdf_follow(int kind, int one_way, uint64_t n, const float *rays, const float *pos, const float *nrm, float epsilon, const float *ior,
                              float *out_ray, int32_t *out_reflected) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(i >= n) {
        return;
    }
    Material m;
    m.diffuse = c4(1.0f, 1.0f, 1.0f, 1.0f);
    m.specular = c4(1.0f, 1.0f, 1.0f, 1.0f);
    m.emission = c4(0.0f, 0.0f, 0.0f, 0.0f);
    m.ior = ior[i];
    m.bsdf = kind;
    m.one_way = one_way;
    bool reflected = false;
    const Ray r = bsdf_follow(m, ld3(rays + 6 * i + 3), ld3(pos + 3 * i), ld3(nrm + 3 * i), epsilon, reflected);
    float *o = out_ray + 6 * i;
    o[0] = r.o.x;
    o[1] = r.o.y;
    o[2] = r.o.z;
    o[3] = r.d.x;
    o[4] = r.d.y;
    o[5] = r.d.z;
    out_reflected[i] = reflected ? 1 : 0;
}

} // namespace

extern "C" {

int ptf_device_count(void) {
    int n = 0;
    if(hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

const char *ptf_error_string(int code) {
    return code >= PT_GUARD_TOUCHED ? "a guard band was written" : hipGetErrorString(static_cast<hipError_t>(code));
}

// kind: 1 glass, 2 mirror (bsdf_follow is never called for a Lambertian material).  0, a HIP error, or PT_GUARD_TOUCHED + the array.
int ptf_bsdf_follow(int kind, int one_way, uint64_t n, const float *rays, const float *pos, const float *nrm, float epsilon, const float *ior, float *out_ray,
                    int32_t *out_reflected) {
    if(kind != 1 && kind != 2) {
        return static_cast<int>(hipErrorInvalidValue);
    }
    GuardStatus st;
    Guarded<float> d_rays(st, 6 * n, 0, rays), d_pos(st, 3 * n, 0, pos), d_nrm(st, 3 * n, 0, nrm), d_ior(st, n, 0, ior);
    Guarded<float> d_out_ray(st, 6 * n, GUARD);
    Guarded<int32_t> d_out_reflected(st, n, GUARD);
    if(st.ok() && n > 0) {
        k_bsdf_follow<<<dim3(static_cast<unsigned>((n + WG - 1) / WG)), dim3(WG)>>>(kind, one_way, n, d_rays.p(), d_pos.p(), d_nrm.p(), epsilon, d_ior.p(), d_out_ray.p(),
                                                                                   d_out_reflected.p());
        st(hipGetLastError());
        st(hipDeviceSynchronize());
    }
    d_out_ray.get(out_ray);
    d_out_reflected.get(out_reflected);
    return st.code();
}

} // extern "C"
