// pt_nearest.hip -- the launches of the nearest-surface kernel (pt_nearest_kernels.h; include/pt_nearest.h).  A unit of
// its own: the walk is ordered by distance to a box, not by a ray's slabs, and shares nothing with Tracer but the layout of its stack,
// so it stays outside pt_path.hip and pt_walks.hip and an edit here recompiles neither.
#include "pt_nearest_kernels.h"

void pt_launch_nearest_points(hipStream_t stream, const PtDevScene &scene, const float *points4, uint32_t first, uint32_t n, float4 *out, const PtQueryTables &tables, uint2 *spill,
                              uint32_t spill_depth, unsigned long long *counts) {
    if(n == 0) {
        return;
    }
    hipLaunchKernelGGL((pt_nearest_kernel<false>), dim3((n + 255) / 256), dim3(256), 0, stream, scene, tables, points4, PtDistanceGrid{}, 0.0f, first, n, out,
                       static_cast<float *>(nullptr), static_cast<int32_t *>(nullptr), spill, spill_depth, counts);
}

void pt_launch_nearest_grid(hipStream_t stream, const PtDevScene &scene, const PtDistanceGrid &grid, float max_distance, uint32_t first, uint32_t n, float *out_distance,
                            int32_t *out_object, uint2 *spill, uint32_t spill_depth) {
    if(n == 0) {
        return;
    }
    hipLaunchKernelGGL((pt_nearest_kernel<true>), dim3((n + 255) / 256), dim3(256), 0, stream, scene, PtQueryTables{nullptr, 0, 0, nullptr}, static_cast<const float *>(nullptr),
                       grid, max_distance, first, n, static_cast<float4 *>(nullptr), out_distance, out_object, spill, spill_depth, static_cast<unsigned long long *>(nullptr));
}
