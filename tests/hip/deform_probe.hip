// TEST ONLY: the skinning kernel's own source (pt_deform_kernels.h: kernel and launch) compiled for the HOST against
// tests/hip/host_deform, so that it runs where there is no GPU (tests/test_deform_cases_cpu.py).  The arrays are copied into aligned
// "device" memory first, as pt_deform.cpp has them: the kernel's wide loads assume that alignment.
#include "pt_deform_kernels.h"

#include <vector>

extern "C" {

// The largest bone table the product stages in LDS (PT_SKIN_LDS_BONES)
uint32_t deform_probe_lds_bones() {
    return PT_SKIN_LDS_BONES;
}

// pt_skin_launch over host arrays; lds_bones as there (0 forces the cache form).  The result array is filled with 0xA5 before the
// launch.  Returns 0, or 1000 + the error.
int deform_probe_skin(uint32_t n_vertices, const float *rest, uint32_t K, const uint32_t *bone, const float *weight, const float *bones, uint32_t n_bones, uint32_t lds_bones,
                      float *out) {
    void *d_rest = nullptr, *d_bone = nullptr, *d_weight = nullptr, *d_bones = nullptr, *d_out = nullptr;
    const size_t nv = n_vertices, nk = nv * K;
    if(hipMalloc(&d_rest, 12 * nv + 1) != hipSuccess || hipMalloc(&d_bone, 4 * nk + 1) != hipSuccess || hipMalloc(&d_weight, 4 * nk + 1) != hipSuccess ||
       hipMalloc(&d_bones, 48 * static_cast<size_t>(n_bones) + 1) != hipSuccess || hipMalloc(&d_out, 12 * nv + 1) != hipSuccess) {
        return 999;
    }
    memcpy(d_rest, rest, 12 * nv);
    memcpy(d_bone, bone, 4 * nk);
    memcpy(d_weight, weight, 4 * nk);
    memcpy(d_bones, bones, 48 * static_cast<size_t>(n_bones));
    memset(d_out, 0xA5, 12 * nv);
    const hipError_t e = pt_skin_launch(nullptr, n_vertices, static_cast<const float *>(d_rest), K, static_cast<const uint32_t *>(d_bone), static_cast<const float *>(d_weight),
                                        static_cast<const float *>(d_bones), n_bones, lds_bones, static_cast<float *>(d_out));
    memcpy(out, d_out, 12 * nv);
    for(void *p : {d_rest, d_bone, d_weight, d_bones, d_out}) {
        hipFree(p);
    }
    return e == hipSuccess ? 0 : 1000 + static_cast<int>(e);
}

} // extern "C"
