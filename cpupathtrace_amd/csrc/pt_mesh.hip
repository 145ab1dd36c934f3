// pt_mesh.hip -- the small per-triangle kernels around a scene's triangle arrays in HBM (pt_mesh.h): face normals for
// triangles that came without normals, and triangles back out of a built scene.  The assembly of meshes and instances into those arrays
// is pt_mesh_batch.hip.
// Compiled with -ffp-contract=off and correctly rounded divide / sqrt like the rest: every operation is the IEEE operation of the host code.
#include "pt_mesh.h"

namespace {

inline dim3 grid_for(size_t n) {
    return dim3(static_cast<unsigned>((n + 255) / 256));
}

__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) {
    float d = 0.0f; // dot() and getLengthSquared() start from zero and add in index order (detail/linear.h)
    d += ax * bx;
    d += ay * by;
    d += az * bz;
    return d;
}

__global__ void k_face_normals(uint32_t n, const float *__restrict__ pos, float *__restrict__ nrm) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if(t >= n) {
        return;
    }
    const float *v = pos + 9 * static_cast<size_t>(t);
    const float abx = v[3] - v[0], aby = v[4] - v[1], abz = v[5] - v[2];
    const float acx = v[6] - v[0], acy = v[7] - v[1], acz = v[8] - v[2];
    const float cx = aby * acz - abz * acy, cy = abz * acx - abx * acz, cz = abx * acy - aby * acx;
    const float inv = 1.0f / __builtin_sqrtf(dot3(cx, cy, cz, cx, cy, cz));
    const float nv[3] = {cx * inv, cy * inv, cz * inv};
    for(int k = 0; k < 9; k++) {
        nrm[9 * static_cast<size_t>(t) + k] = nv[k % 3];
    }
}

__global__ void k_gather_pos(const float *__restrict__ pos, const uint32_t *__restrict__ idx, uint32_t n, float *__restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if(i >= n) {
        return;
    }
    const float *p = pos + 9 * static_cast<size_t>(idx[i]);
    for(int k = 0; k < 9; k++) {
        out[9 * static_cast<size_t>(i) + k] = p[k];
    }
}

__global__ void k_unpack(const float *__restrict__ pos, const float4 *__restrict__ shade, const uint32_t *__restrict__ idx, uint32_t first, uint32_t n,
                         float *__restrict__ out_pos, float *__restrict__ out_nrm, uint8_t *__restrict__ out_cull, uint32_t *__restrict__ out_material) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if(i >= n) {
        return;
    }
    const size_t t = idx != nullptr ? idx[i] : static_cast<size_t>(first) + i;
    if(out_pos != nullptr) {
        for(int k = 0; k < 9; k++) {
            out_pos[9 * static_cast<size_t>(i) + k] = pos[9 * t + k];
        }
    }
    const float4 *sh = shade + 8 * t; // (pt_build.hip k_triangle_records: material and object | cull in [2], normals in [3] .. [5])
    if(out_nrm != nullptr) {
        const float4 a = sh[3], b = sh[4], c = sh[5];
        const float q[9] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x};
        for(int k = 0; k < 9; k++) {
            out_nrm[9 * static_cast<size_t>(i) + k] = q[k];
        }
    }
    if(out_cull != nullptr || out_material != nullptr) {
        const float4 r2 = sh[2];
        if(out_cull != nullptr) {
            out_cull[i] = (__float_as_uint(r2.z) & 0x80000000u) != 0u ? 1 : 0;
        }
        if(out_material != nullptr) {
            out_material[i] = __float_as_uint(r2.y);
        }
    }
}

} // namespace

hipError_t pt_mesh_face_normals(hipStream_t stream, uint32_t n, const float *pos, float *nrm) {
    if(n == 0) {
        return hipSuccess;
    }
    hipLaunchKernelGGL(k_face_normals, grid_for(n), dim3(256), 0, stream, n, pos, nrm);
    return hipGetLastError();
}

hipError_t pt_mesh_gather_pos(hipStream_t stream, const float *pos, const uint32_t *idx, uint32_t n, float *out) {
    if(n == 0) {
        return hipSuccess;
    }
    hipLaunchKernelGGL(k_gather_pos, grid_for(n), dim3(256), 0, stream, pos, idx, n, out);
    return hipGetLastError();
}

hipError_t pt_mesh_unpack(hipStream_t stream, const float *pos, const float4 *shade, const uint32_t *idx, uint32_t first, uint32_t n, float *out_pos, float *out_nrm,
                          uint8_t *out_cull, uint32_t *out_material) {
    if(n == 0) {
        return hipSuccess;
    }
    hipLaunchKernelGGL(k_unpack, grid_for(n), dim3(256), 0, stream, pos, shade, idx, first, n, out_pos, out_nrm, out_cull, out_material);
    return hipGetLastError();
}
