// pt_mesh.hip -- indexed meshes under transforms, expanded into triangle arrays in HBM: everything io::loadMesh does
// after it has read the numbers (src/scene/mesh.cpp of the reference; src/host/mesh.cpp has the host restatement), so that a mesh is
// handed over once as vertices + faces and every instance of it is made where the builder (pt_build.hip) reads it.
//
// Per instance:
//   1. k_transform   one thread per vertex: v' = M * (x, y, z, 1) row by row with dot() from zero, then * (1 / w')   (matrix.h, mat4::operator*)
//   2. k_face_keep   one thread per face: an index outside [0, n_vertices), two coincident corners (written so that NaN rejects) or a
//                    cross product of squared length <= 0 drop the face -- all on the TRANSFORMED vertices
//   3. an exclusive sum of the keep flags = the survivors' positions: face order is kept, the count comes out of the last element
//   4. k_expand      one thread per face: the survivor's nine coordinates, its unit normal (Triangle::Triangle) three times, its face number
//   5. smooth only:  the (vertex, survivor * 3 + slot) pairs of all corners are sorted by vertex with a STABLE radix sort, so the corners of
//                    a vertex are contiguous and in ascending face order; k_smooth, one thread per vertex, adds the unit face normals
//                    serially in that order (float addition is not associative: neither atomics nor a tree would give the reference's bits),
//                    skips the vertex when the sum's squared length is <= 0, and otherwise writes the normalised sum to every corner.
// Compiled with -ffp-contract=off and correctly rounded divide / sqrt like the rest: every operation is the IEEE operation of the host code.
#include "pt_mesh.h"

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <vector>

namespace {

struct Mat4 {
    float m[16];
};

struct Scratch {
    std::vector<void *> ptrs;
    ~Scratch() {
        for(void *p : ptrs) {
            (void)hipFree(p);
        }
    }
    template<typename T>
    hipError_t get(T **out, size_t count) {
        void *p = nullptr;
        hipError_t e = hipMalloc(&p, std::max<size_t>(count, 1) * sizeof(T));
        if(e == hipSuccess) {
            ptrs.push_back(p);
            *out = static_cast<T *>(p);
        }
        return e;
    }
};

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

__global__ void k_transform(uint32_t n, const float *__restrict__ v, Mat4 M, float *__restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if(i >= n) {
        return;
    }
    const float x = v[3 * static_cast<size_t>(i)], y = v[3 * static_cast<size_t>(i) + 1], z = v[3 * static_cast<size_t>(i) + 2];
    float h[4];
    for(int r = 0; r < 4; r++) {
        float d = 0.0f;
        d += M.m[4 * r + 0] * x;
        d += M.m[4 * r + 1] * y;
        d += M.m[4 * r + 2] * z;
        d += M.m[4 * r + 3] * 1.0f;
        h[r] = d;
    }
    const float inv = 1.0f / h[3];
    out[3 * static_cast<size_t>(i)] = h[0] * inv;
    out[3 * static_cast<size_t>(i) + 1] = h[1] * inv;
    out[3 * static_cast<size_t>(i) + 2] = h[2] * inv;
}

// flag[f] = 1 for a face that stays; flag[n_faces] = 0, so that the exclusive sum's last element is the number of survivors
__global__ void k_face_keep(uint32_t n_faces, uint32_t n_vertices, const int32_t *__restrict__ faces, const float *__restrict__ tv, uint32_t *__restrict__ flag) {
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    if(f > n_faces) {
        return;
    }
    if(f == n_faces) {
        flag[f] = 0u;
        return;
    }
    const int32_t ia = faces[3 * static_cast<size_t>(f)], ib = faces[3 * static_cast<size_t>(f) + 1], ic = faces[3 * static_cast<size_t>(f) + 2];
    const int64_t count = n_vertices;
    uint32_t keep = 0u;
    if(ia >= 0 && ia < count && ib >= 0 && ib < count && ic >= 0 && ic < count) {
        const float *a = tv + 3 * static_cast<size_t>(ia), *b = tv + 3 * static_cast<size_t>(ib), *c = tv + 3 * static_cast<size_t>(ic);
        const float abx = b[0] - a[0], aby = b[1] - a[1], abz = b[2] - a[2];
        const float acx = c[0] - a[0], acy = c[1] - a[1], acz = c[2] - a[2];
        const float bcx = c[0] - b[0], bcy = c[1] - b[1], bcz = c[2] - b[2];
        if(dot3(abx, aby, abz, abx, aby, abz) > 0.0f && dot3(acx, acy, acz, acx, acy, acz) > 0.0f && dot3(bcx, bcy, bcz, bcx, bcy, bcz) > 0.0f) {
            const float cx = aby * acz - abz * acy, cy = abz * acx - abx * acz, cz = abx * acy - aby * acx;
            if(!(dot3(cx, cy, cz, cx, cy, cz) <= 0.0f)) {
                keep = 1u;
            }
        }
    }
    flag[f] = keep;
}

// Survivor `rank[f]` of face f: corners, unit normal (three times into nrm where there is one), and its corners' sort pairs
__global__ void k_expand(uint32_t n_faces, const int32_t *__restrict__ faces, const float *__restrict__ tv, const uint32_t *__restrict__ flag,
                         const uint32_t *__restrict__ rank, float *__restrict__ pos, float *__restrict__ nrm, float *__restrict__ unit, uint32_t *__restrict__ corner_vertex,
                         uint32_t *__restrict__ corner_id) {
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    if(f >= n_faces || flag[f] == 0u) {
        return;
    }
    const size_t j = rank[f];
    float v[9];
    uint32_t index[3];
    for(int s = 0; s < 3; s++) {
        index[s] = static_cast<uint32_t>(faces[3 * static_cast<size_t>(f) + s]);
        const float *p = tv + 3 * static_cast<size_t>(index[s]);
        v[3 * s] = p[0];
        v[3 * s + 1] = p[1];
        v[3 * s + 2] = p[2];
    }
    for(int k = 0; k < 9; k++) {
        pos[9 * j + k] = v[k];
    }
    if(nrm != nullptr) {
        const float abx = v[3] - v[0], aby = v[4] - v[1], abz = v[5] - v[2];
        const float acx = v[6] - v[0], acy = v[7] - v[1], acz = v[8] - v[2];
        const float cx = aby * acz - abz * acy, cy = abz * acx - abx * acz, cz = abx * acy - aby * acx;
        const float inv = 1.0f / __builtin_sqrtf(dot3(cx, cy, cz, cx, cy, cz));
        const float n[3] = {cx * inv, cy * inv, cz * inv};
        for(int k = 0; k < 9; k++) {
            nrm[9 * j + k] = n[k % 3];
        }
        if(unit != nullptr) {
            for(int k = 0; k < 3; k++) {
                unit[3 * j + k] = n[k];
            }
            for(int s = 0; s < 3; s++) {
                corner_vertex[3 * j + s] = index[s];
                corner_id[3 * j + s] = static_cast<uint32_t>(3 * j + s);
            }
        }
    }
}

// The corners of vertex v are sorted_vertex's run of v: [lower bound of v, lower bound of v + 1)
__device__ __forceinline__ uint32_t lower_bound(const uint32_t *__restrict__ a, uint32_t n, uint32_t key) {
    uint32_t lo = 0, hi = n;
    while(lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if(a[mid] < key) {
            lo = mid + 1;
        }
        else {
            hi = mid;
        }
    }
    return lo;
}

__global__ void k_smooth(uint32_t n_vertices, uint32_t n_corners, const uint32_t *__restrict__ sorted_vertex, const uint32_t *__restrict__ sorted_id,
                         const float *__restrict__ unit, float *__restrict__ nrm) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if(v >= n_vertices) {
        return;
    }
    const uint32_t first = lower_bound(sorted_vertex, n_corners, v);
    float sx = 0.0f, sy = 0.0f, sz = 0.0f;
    uint32_t last = first;
    for(; last < n_corners && sorted_vertex[last] == v; last++) {
        const float *n = unit + 3 * static_cast<size_t>(sorted_id[last] / 3u);
        sx = sx + n[0];
        sy = sy + n[1];
        sz = sz + n[2];
    }
    const float length_squared = dot3(sx, sy, sz, sx, sy, sz);
    if(last == first || length_squared <= 0.0f) {
        return; // every corner keeps its face normal (a NaN sum is not <= 0: it is normalised and assigned)
    }
    const float inv = 1.0f / __builtin_sqrtf(length_squared);
    const float nx = sx * inv, ny = sy * inv, nz = sz * inv;
    for(uint32_t k = first; k < last; k++) {
        float *q = nrm + 3 * static_cast<size_t>(sorted_id[k]); // corner id = survivor * 3 + slot, and nrm is [survivor][slot][3]
        q[0] = nx;
        q[1] = ny;
        q[2] = nz;
    }
}

__global__ void k_fill_range(uint32_t first_tri, uint32_t count, uint8_t cull, uint32_t material, uint32_t first_obj, uint8_t *__restrict__ tri_cull,
                             uint32_t *__restrict__ tri_material, uint32_t *__restrict__ tri_obj) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if(i >= count) {
        return;
    }
    const size_t t = static_cast<size_t>(first_tri) + i;
    tri_cull[t] = cull;
    tri_material[t] = material;
    tri_obj[t] = first_obj + i;
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

#define PTM_TRY(call, text)        \
    do {                           \
        hipError_t e_ = (call);    \
        if(e_ != hipSuccess) {     \
            if(what != nullptr) {  \
                *what = text;      \
            }                      \
            return e_;             \
        }                          \
    } while(0)

hipError_t pt_mesh_assemble_device(hipStream_t stream, const PtMeshDevice &mesh, const float *m16, bool smooth, float *pos, float *nrm, uint32_t *n_kept, float *device_ms,
                                   const char **what) {
    *n_kept = 0;
    if(device_ms != nullptr) {
        *device_ms = 0.0f;
    }
    const uint32_t nf = mesh.n_faces, nv = mesh.n_vertices;
    if(nf == 0) {
        return hipSuccess;
    }
    if(nf > PT_MESH_MAX_FACES || (smooth && nrm == nullptr)) {
        if(what != nullptr) {
            *what = "mesh assembly arguments";
        }
        return hipErrorInvalidValue;
    }
    Scratch scratch;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    PTM_TRY(hipEventCreate(&ev0), "event");
    PTM_TRY(hipEventCreate(&ev1), "event");
    struct EventGuard {
        hipEvent_t a, b;
        ~EventGuard() {
            (void)hipEventDestroy(a);
            (void)hipEventDestroy(b);
        }
    } guard{ev0, ev1};
    PTM_TRY(hipEventRecord(ev0, stream), "event");

    Mat4 M;
    std::copy(m16, m16 + 16, M.m);
    float *tv = nullptr;
    uint32_t *flag = nullptr, *rank = nullptr;
    PTM_TRY(scratch.get(&tv, 3 * static_cast<size_t>(nv)), "transformed vertices");
    PTM_TRY(scratch.get(&flag, static_cast<size_t>(nf) + 1), "face flags");
    PTM_TRY(scratch.get(&rank, static_cast<size_t>(nf) + 1), "face ranks");
    if(nv > 0) {
        hipLaunchKernelGGL(k_transform, grid_for(nv), dim3(256), 0, stream, nv, mesh.vertices, M, tv);
    }
    hipLaunchKernelGGL(k_face_keep, grid_for(static_cast<size_t>(nf) + 1), dim3(256), 0, stream, nf, nv, mesh.faces, tv, flag);
    PTM_TRY(hipGetLastError(), "mesh transform and face test kernels");
    {
        size_t bytes = 0;
        PTM_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, flag, rank, static_cast<int>(nf + 1), stream), "scan sizing");
        uint8_t *temp = nullptr;
        PTM_TRY(scratch.get(&temp, bytes), "scan temporary storage");
        PTM_TRY(hipcub::DeviceScan::ExclusiveSum(temp, bytes, flag, rank, static_cast<int>(nf + 1), stream), "face scan");
    }
    uint32_t kept = 0;
    PTM_TRY(hipMemcpyAsync(&kept, rank + nf, sizeof(uint32_t), hipMemcpyDeviceToHost, stream), "reading the survivor count");
    PTM_TRY(hipStreamSynchronize(stream), "face test");
    if(kept > nf) { // cannot happen: nothing is written on the strength of a count that is out of range
        if(what != nullptr) {
            *what = "survivor count";
        }
        return hipErrorUnknown;
    }
    if(kept > 0) {
        const bool do_smooth = smooth && nv > 0;
        float *unit = nullptr;
        uint32_t *corner_vertex = nullptr, *corner_id = nullptr, *sorted_vertex = nullptr, *sorted_id = nullptr;
        const size_t n_corners = 3 * static_cast<size_t>(kept);
        if(do_smooth) {
            PTM_TRY(scratch.get(&unit, n_corners), "unit normals");
            PTM_TRY(scratch.get(&corner_vertex, n_corners), "corner lists");
            PTM_TRY(scratch.get(&corner_id, n_corners), "corner lists");
            PTM_TRY(scratch.get(&sorted_vertex, n_corners), "corner lists");
            PTM_TRY(scratch.get(&sorted_id, n_corners), "corner lists");
        }
        hipLaunchKernelGGL(k_expand, grid_for(nf), dim3(256), 0, stream, nf, mesh.faces, tv, flag, rank, pos, nrm, unit, corner_vertex, corner_id);
        PTM_TRY(hipGetLastError(), "mesh expansion kernel");
        if(do_smooth) {
            int end_bit = 1;
            while(end_bit < 32 && (static_cast<uint64_t>(nv) - 1) >> end_bit != 0) {
                end_bit++;
            }
            size_t bytes = 0;
            PTM_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, corner_vertex, sorted_vertex, corner_id, sorted_id, static_cast<int>(n_corners), 0, end_bit, stream),
                    "sort sizing");
            uint8_t *temp = nullptr;
            PTM_TRY(scratch.get(&temp, bytes), "sort temporary storage");
            PTM_TRY(hipcub::DeviceRadixSort::SortPairs(temp, bytes, corner_vertex, sorted_vertex, corner_id, sorted_id, static_cast<int>(n_corners), 0, end_bit, stream),
                    "corner sort");
            hipLaunchKernelGGL(k_smooth, grid_for(nv), dim3(256), 0, stream, nv, static_cast<uint32_t>(n_corners), sorted_vertex, sorted_id, unit, nrm);
            PTM_TRY(hipGetLastError(), "smoothing kernel");
        }
    }
    PTM_TRY(hipEventRecord(ev1, stream), "event");
    PTM_TRY(hipStreamSynchronize(stream), "mesh assembly");
    if(device_ms != nullptr) {
        PTM_TRY(hipEventElapsedTime(device_ms, ev0, ev1), "event");
    }
    *n_kept = kept;
    return hipSuccess;
}

hipError_t pt_mesh_fill_range(hipStream_t stream, uint32_t first_tri, uint32_t count, uint8_t cull, uint32_t material, uint32_t first_obj, uint8_t *tri_cull,
                              uint32_t *tri_material, uint32_t *tri_obj) {
    if(count == 0) {
        return hipSuccess;
    }
    hipLaunchKernelGGL(k_fill_range, grid_for(count), dim3(256), 0, stream, first_tri, count, cull, material, first_obj, tri_cull, tri_material, tri_obj);
    return hipGetLastError();
}

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
