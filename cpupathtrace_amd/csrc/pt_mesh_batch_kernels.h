// pt_mesh_batch_kernels.h -- the kernels and the launch chain of the mesh assembler (pt_mesh_batch.h): indexed
// meshes under transforms, expanded into triangle arrays in HBM.  It is everything io::loadMesh does after it has read the numbers
// (src/scene/mesh.cpp of the reference; src/host/mesh.cpp has the host restatement), so that a mesh is handed over once as vertices +
// faces and every instance of it is made where the builder (pt_build.hip) reads it.  Included once, by pt_mesh_batch.hip;
// tests/hip/pose_probe.hip includes it as well and, compiled for the host, runs this very source on the CPU.
//
// The index spaces of a chunk's instances are concatenated: global vertex g = vertex_base[i] + v, global face f = face_base[i] + k.
//   1. kb_transform  one thread per global vertex: v' = M * (x, y, z, 1) row by row with dot() from zero, then * (1 / w'), with the
//                    matrix of the vertex's instance   (matrix.h, mat4::operator*)
//   2. kb_face_keep  one thread per global face and one trailing zero flag: an index outside [0, n_vertices) of the face's instance, two
//                    coincident corners (written so that NaN rejects) or a cross product of squared length <= 0 drop the face -- all on
//                    the TRANSFORMED vertices
//   3. ONE exclusive sum over all flags.  Instances are concatenated in order and survivors keep face order, so the rank of a face IS its
//      triangle index in the output; kb_counts takes the per-instance counts as differences of the ranks at the face bases
//   4. kb_expand     one thread per global face: the survivor's nine coordinates, its unit normal (Triangle::Triangle) three times, and
//                    its corners' (key, corner id = survivor * 3 + slot) pairs.  The key of a smooth instance's corner is its GLOBAL
//                    vertex, that of a flat one's the chunk's vertex count, which no vertex has: such corners sort behind all others
//                    and no vertex's run holds them
//   5. smooth only:  one STABLE radix sort of the pairs over the bits of the vertex count, so the corners of a vertex are contiguous and
//                    their ids ascend, and ascending global corner id is ascending face order inside the instance; kb_smooth, one
//                    thread per global vertex of a smooth instance, adds the unit face normals serially in that order (float addition
//                    is not associative: neither atomics nor a tree would give the reference's bits), skips the vertex when the sum's
//                    squared length is <= 0, and otherwise writes the normalised sum to every corner.
// Every thread finds its instance by a binary search of the bases in the instance table.  Indices are 64-bit where 9 * index can pass 2^32.
#ifndef PT_MESH_BATCH_KERNELS_H
#define PT_MESH_BATCH_KERNELS_H

#include "pt_mesh_batch.h"

namespace ptmb {

inline dim3 grid_for(uint64_t n) {
    return dim3(static_cast<unsigned>((n + 255) / 256));
}

__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) {
    float d = 0.0f; // dot() and getLengthSquared() start from zero and add in index order (detail/linear.h)
    d += ax * bx;
    d += ay * by;
    d += az * bz;
    return d;
}

// The instance of global vertex g: the last entry whose vertex_base is <= g (entry 0 has base 0).  Instances without vertices share their
// base with the next one and are never found.
__device__ __forceinline__ uint32_t instance_of_vertex(const PtBatchInstance *__restrict__ table, uint32_t n, uint32_t g) {
    uint32_t lo = 0, hi = n;
    while(hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if(table[mid].vertex_base <= g) {
            lo = mid;
        }
        else {
            hi = mid;
        }
    }
    return lo;
}

__device__ __forceinline__ uint32_t instance_of_face(const PtBatchInstance *__restrict__ table, uint32_t n, uint32_t f) {
    uint32_t lo = 0, hi = n;
    while(hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if(table[mid].face_base <= f) {
            lo = mid;
        }
        else {
            hi = mid;
        }
    }
    return lo;
}

__global__ void kb_transform(uint32_t n_total, const PtBatchInstance *__restrict__ table, uint32_t n_instances, float *__restrict__ out) {
    const uint64_t g64 = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
    if(g64 >= n_total) {
        return;
    }
    const uint32_t g = static_cast<uint32_t>(g64);
    const PtBatchInstance &in = table[instance_of_vertex(table, n_instances, g)];
    const size_t i = g - in.vertex_base;
    const float *v = in.vertices;
    const float x = v[3 * i], y = v[3 * i + 1], z = v[3 * i + 2];
    float h[4];
    for(int r = 0; r < 4; r++) {
        float d = 0.0f;
        d += in.m[4 * r + 0] * x;
        d += in.m[4 * r + 1] * y;
        d += in.m[4 * r + 2] * z;
        d += in.m[4 * r + 3] * 1.0f;
        h[r] = d;
    }
    const float inv = 1.0f / h[3];
    out[3 * static_cast<size_t>(g)] = h[0] * inv;
    out[3 * static_cast<size_t>(g) + 1] = h[1] * inv;
    out[3 * static_cast<size_t>(g) + 2] = h[2] * inv;
}

// flag[f] = 1 for a face that stays; flag[n_total] = 0, so that the exclusive sum's last element is the number of survivors
__global__ void kb_face_keep(uint32_t n_total, const PtBatchInstance *__restrict__ table, uint32_t n_instances, const float *__restrict__ tv, uint32_t *__restrict__ flag) {
    const uint64_t f64 = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
    if(f64 > n_total) {
        return;
    }
    if(f64 == n_total) {
        flag[f64] = 0u;
        return;
    }
    const uint32_t f = static_cast<uint32_t>(f64);
    const PtBatchInstance &in = table[instance_of_face(table, n_instances, f)];
    const size_t k = f - in.face_base;
    const int32_t ia = in.faces[3 * k], ib = in.faces[3 * k + 1], ic = in.faces[3 * k + 2];
    const int64_t count = in.n_vertices;
    uint32_t keep = 0u;
    if(ia >= 0 && ia < count && ib >= 0 && ib < count && ic >= 0 && ic < count) {
        const float *base = tv + 3 * static_cast<size_t>(in.vertex_base);
        const float *a = base + 3 * static_cast<size_t>(ia), *b = base + 3 * static_cast<size_t>(ib), *c = base + 3 * static_cast<size_t>(ic);
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

// counts[i] = survivors of instance i; counts[n_instances] = survivors of the chunk
__global__ void kb_counts(uint32_t n_instances, const PtBatchInstance *__restrict__ table, const uint32_t *__restrict__ rank, uint32_t n_total_faces,
                          uint32_t *__restrict__ counts) {
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
    if(i > n_instances) {
        return;
    }
    if(i == n_instances) {
        counts[i] = rank[n_total_faces];
        return;
    }
    const PtBatchInstance &in = table[i];
    counts[i] = rank[static_cast<size_t>(in.face_base) + in.n_faces] - rank[in.face_base];
}

// Survivor rank[f] of global face f: corners, unit normal (three times into nrm where there is one), and its corners' sort pairs.
// Nothing is written for a rank >= room.
__global__ void kb_expand(uint32_t n_total, const PtBatchInstance *__restrict__ table, uint32_t n_instances, const float *__restrict__ tv, const uint32_t *__restrict__ flag,
                          const uint32_t *__restrict__ rank, uint64_t room, uint32_t flat_key, float *__restrict__ pos, float *__restrict__ nrm, float *__restrict__ unit,
                          uint32_t *__restrict__ corner_vertex, uint32_t *__restrict__ corner_id) {
    const uint64_t f64 = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
    if(f64 >= n_total || flag[f64] == 0u) {
        return;
    }
    const uint32_t f = static_cast<uint32_t>(f64);
    const size_t j = rank[f];
    if(j >= room) {
        return;
    }
    const PtBatchInstance &in = table[instance_of_face(table, n_instances, f)];
    const size_t face = f - in.face_base;
    float v[9];
    uint32_t index[3];
    for(int s = 0; s < 3; s++) {
        index[s] = in.vertex_base + static_cast<uint32_t>(in.faces[3 * face + s]); // (a survivor's indices are inside the instance)
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
                corner_vertex[3 * j + s] = in.smooth != 0u ? index[s] : flat_key;
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

__global__ void kb_smooth(uint32_t n_total, const PtBatchInstance *__restrict__ table, uint32_t n_instances, uint32_t n_corners, const uint32_t *__restrict__ sorted_vertex,
                          const uint32_t *__restrict__ sorted_id, const float *__restrict__ unit, float *__restrict__ nrm) {
    const uint64_t g64 = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
    if(g64 >= n_total) {
        return;
    }
    const uint32_t v = static_cast<uint32_t>(g64);
    if(table[instance_of_vertex(table, n_instances, v)].smooth == 0u) {
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

// Triangle first_tri + i: the constants of the last range that starts at or before it (empty ranges share their start with the next one)
__global__ void kb_fill_ranges(uint32_t n, uint32_t first_tri, uint32_t first_obj, const PtBatchRange *__restrict__ ranges, uint32_t n_ranges, uint8_t *__restrict__ tri_cull,
                               uint32_t *__restrict__ tri_material, uint32_t *__restrict__ tri_obj) {
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
    if(i >= n) {
        return;
    }
    const uint32_t t = first_tri + static_cast<uint32_t>(i);
    uint32_t lo = 0, hi = n_ranges;
    while(hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if(ranges[mid].first_tri <= t) {
            lo = mid;
        }
        else {
            hi = mid;
        }
    }
    tri_cull[t] = static_cast<uint8_t>(ranges[lo].cull);
    tri_material[t] = ranges[lo].material;
    tri_obj[t] = first_obj + static_cast<uint32_t>(i);
}

} // namespace ptmb

#define PTMB_TRY(call, text)       \
    do {                           \
        hipError_t e_ = (call);    \
        if(e_ != hipSuccess) {     \
            if(what != nullptr) {  \
                *what = text;      \
            }                      \
            return e_;             \
        }                          \
    } while(0)

uint32_t pt_mesh_batch_chunk_end(const uint32_t *n_vertices, const uint32_t *n_faces, uint32_t n_instances, uint32_t first, const PtBatchLimits &limits) {
    uint64_t vertices = 0, faces = 0;
    uint32_t end = first;
    while(end < n_instances) {
        const uint64_t v = vertices + n_vertices[end], f = faces + n_faces[end];
        if(end > first && (v > limits.max_vertices || f > limits.max_faces || 3 * f > limits.max_corners)) {
            break;
        }
        vertices = v;
        faces = f;
        end++;
    }
    return end;
}

hipError_t pt_mesh_batch_chunk(hipStream_t stream, PtBatchScratch &sc, PtBatchInstance *table, uint32_t n_instances, uint64_t room, float *pos, float *nrm, uint32_t *counts,
                               uint64_t *kept_out, const char **what) {
    using namespace ptmb;
    *kept_out = 0;
    if(n_instances == 0) {
        return hipSuccess;
    }
    uint64_t nv64 = 0, nf64 = 0;
    bool any_smooth = false;
    for(uint32_t i = 0; i < n_instances; i++) {
        table[i].vertex_base = static_cast<uint32_t>(nv64);
        table[i].face_base = static_cast<uint32_t>(nf64);
        nv64 += table[i].n_vertices;
        nf64 += table[i].n_faces;
        any_smooth = any_smooth || table[i].smooth != 0u;
        counts[i] = 0;
    }
    // (one instance alone may not pass the limits either: the callers refuse a mesh of more than PT_MESH_MAX_FACES faces, pt_mesh.h)
    if(nv64 > 0xffffffffull || 3 * nf64 > 0x7fffffffull || (any_smooth && nrm == nullptr)) {
        if(what != nullptr) {
            *what = "mesh batch arguments";
        }
        return hipErrorInvalidValue;
    }
    if(nf64 == 0) {
        return hipSuccess;
    }
    const uint32_t nv = static_cast<uint32_t>(nv64), nf = static_cast<uint32_t>(nf64);
    const bool do_smooth = any_smooth && nv > 0;
    const size_t max_corners = 3 * static_cast<size_t>(nf);
    int end_bit = 1; // the keys are the global vertices and, for the corners of flat instances, nv itself
    while(end_bit < 32 && static_cast<uint64_t>(nv) >> end_bit != 0) {
        end_bit++;
    }

    // ---- scratch: sized from the faces BEFORE rejection, so that it depends on the meshes and not on the pose --------------------------
    PTMB_TRY(sc.ensure(sc.table, n_instances * sizeof(PtBatchInstance)), "instance table");
    PTMB_TRY(sc.ensure(sc.tv, 3 * static_cast<size_t>(nv) * sizeof(float)), "transformed vertices");
    PTMB_TRY(sc.ensure(sc.flag, (static_cast<size_t>(nf) + 1) * sizeof(uint32_t)), "face flags");
    PTMB_TRY(sc.ensure(sc.rank, (static_cast<size_t>(nf) + 1) * sizeof(uint32_t)), "face ranks");
    PTMB_TRY(sc.ensure(sc.counts, (static_cast<size_t>(n_instances) + 1) * sizeof(uint32_t)), "instance counts");
    size_t scan_bytes = 0, sort_bytes = 0;
    PTMB_TRY(pt_mesh_batch_scan(nullptr, &scan_bytes, nullptr, nullptr, nf + 1, stream), "scan sizing");
    if(do_smooth) {
        PTMB_TRY(sc.ensure(sc.unit, max_corners * sizeof(float)), "unit normals");
        PTMB_TRY(sc.ensure(sc.corner_vertex, max_corners * sizeof(uint32_t)), "corner lists");
        PTMB_TRY(sc.ensure(sc.corner_id, max_corners * sizeof(uint32_t)), "corner lists");
        PTMB_TRY(sc.ensure(sc.sorted_vertex, max_corners * sizeof(uint32_t)), "corner lists");
        PTMB_TRY(sc.ensure(sc.sorted_id, max_corners * sizeof(uint32_t)), "corner lists");
        PTMB_TRY(pt_mesh_batch_sort(nullptr, &sort_bytes, nullptr, nullptr, nullptr, nullptr, static_cast<uint32_t>(max_corners), end_bit, stream), "sort sizing");
    }
    PTMB_TRY(sc.ensure(sc.temp, scan_bytes > sort_bytes ? scan_bytes : sort_bytes), "scan and sort temporary storage");
    const PtBatchInstance *d_table = static_cast<const PtBatchInstance *>(sc.table.ptr);
    float *tv = static_cast<float *>(sc.tv.ptr);
    uint32_t *flag = static_cast<uint32_t *>(sc.flag.ptr), *rank = static_cast<uint32_t *>(sc.rank.ptr), *d_counts = static_cast<uint32_t *>(sc.counts.ptr);
    float *unit = do_smooth ? static_cast<float *>(sc.unit.ptr) : nullptr;
    uint32_t *corner_vertex = do_smooth ? static_cast<uint32_t *>(sc.corner_vertex.ptr) : nullptr, *corner_id = do_smooth ? static_cast<uint32_t *>(sc.corner_id.ptr) : nullptr;
    uint32_t *sorted_vertex = static_cast<uint32_t *>(sc.sorted_vertex.ptr), *sorted_id = static_cast<uint32_t *>(sc.sorted_id.ptr);

    // ---- everything up to the expansion, then the one wait: the counts size the sort ---------------------------------------------------
    PTMB_TRY(hipMemcpyAsync(sc.table.ptr, table, n_instances * sizeof(PtBatchInstance), hipMemcpyHostToDevice, stream), "instance table upload");
    if(nv > 0) {
        hipLaunchKernelGGL(kb_transform, grid_for(nv), dim3(256), 0, stream, nv, d_table, n_instances, tv);
    }
    hipLaunchKernelGGL(kb_face_keep, grid_for(static_cast<uint64_t>(nf) + 1), dim3(256), 0, stream, nf, d_table, n_instances, tv, flag);
    PTMB_TRY(hipGetLastError(), "mesh batch transform and face test kernels");
    PTMB_TRY(pt_mesh_batch_scan(sc.temp.ptr, &scan_bytes, flag, rank, nf + 1, stream), "face scan");
    hipLaunchKernelGGL(kb_counts, grid_for(static_cast<uint64_t>(n_instances) + 1), dim3(256), 0, stream, n_instances, d_table, rank, nf, d_counts);
    PTMB_TRY(hipGetLastError(), "mesh batch count kernel");
    uint32_t kept = 0;
    PTMB_TRY(hipMemcpyAsync(counts, d_counts, n_instances * sizeof(uint32_t), hipMemcpyDeviceToHost, stream), "reading the survivor counts");
    PTMB_TRY(hipMemcpyAsync(&kept, d_counts + n_instances, sizeof(uint32_t), hipMemcpyDeviceToHost, stream), "reading the survivor counts");
    hipLaunchKernelGGL(kb_expand, grid_for(nf), dim3(256), 0, stream, nf, d_table, n_instances, tv, flag, rank, room, nv, pos, nrm, unit, corner_vertex, corner_id);
    PTMB_TRY(hipGetLastError(), "mesh batch expansion kernel");
    PTMB_TRY(hipStreamSynchronize(stream), "mesh batch face test and expansion");
    uint64_t sum = 0;
    for(uint32_t i = 0; i < n_instances; i++) {
        sum += counts[i];
    }
    if(kept > nf || sum != kept) { // cannot happen: nothing more is done on the strength of counts that do not add up
        if(what != nullptr) {
            *what = "survivor counts";
        }
        return hipErrorUnknown;
    }
    *kept_out = kept;
    const uint64_t written = kept < room ? kept : room;
    if(do_smooth && written > 0) {
        const uint32_t n_corners = static_cast<uint32_t>(3 * written);
        // (the library's need is taken for this very count as well: nothing says that fewer items never need more.  Everything enqueued
        // so far that used the storage has been waited for)
        size_t need = 0;
        PTMB_TRY(pt_mesh_batch_sort(nullptr, &need, nullptr, nullptr, nullptr, nullptr, n_corners, end_bit, stream), "sort sizing");
        PTMB_TRY(sc.ensure(sc.temp, need > sort_bytes ? need : sort_bytes), "sort temporary storage");
        sort_bytes = sc.temp.bytes;
        PTMB_TRY(pt_mesh_batch_sort(sc.temp.ptr, &sort_bytes, corner_vertex, sorted_vertex, corner_id, sorted_id, n_corners, end_bit, stream), "corner sort");
        hipLaunchKernelGGL(kb_smooth, grid_for(nv), dim3(256), 0, stream, nv, d_table, n_instances, n_corners, sorted_vertex, sorted_id, unit, nrm);
        PTMB_TRY(hipGetLastError(), "mesh batch smoothing kernel");
    }
    return hipSuccess;
}

hipError_t pt_mesh_batch_fill_ranges(hipStream_t stream, PtBatchScratch &sc, const PtBatchRange *ranges, uint32_t n_ranges, uint32_t first_tri, uint32_t n, uint32_t first_obj,
                                     uint8_t *tri_cull, uint32_t *tri_material, uint32_t *tri_obj) {
    if(n == 0 || n_ranges == 0) {
        return hipSuccess;
    }
    hipError_t e = sc.ensure(sc.ranges, n_ranges * sizeof(PtBatchRange));
    if(e == hipSuccess) {
        e = hipMemcpy(sc.ranges.ptr, ranges, n_ranges * sizeof(PtBatchRange), hipMemcpyHostToDevice);
    }
    if(e != hipSuccess) {
        return e;
    }
    hipLaunchKernelGGL(ptmb::kb_fill_ranges, ptmb::grid_for(n), dim3(256), 0, stream, n, first_tri, first_obj, static_cast<const PtBatchRange *>(sc.ranges.ptr), n_ranges, tri_cull,
                       tri_material, tri_obj);
    return hipGetLastError();
}

#endif
