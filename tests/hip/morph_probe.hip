// TEST ONLY: the blend-shape kernel's own source (pt_morph_kernels.h: kernel and launch, behind pt_deform_kernels.h) and the host
// transposition of a morph set (pt_morph_rows.h) compiled for the HOST against tests/hip/host_deform, whose launches run a kernel with
// exactly one barrier, so that both run where there is no GPU (tests/test_morph_cases_cpu.py).  The arrays are copied into aligned
// "device" memory first, as pt_morph.cpp has them: the kernel's wide loads assume that alignment.
#include "pt_morph_kernels.h"
#include "pt_morph_rows.h"

#include <vector>

extern "C" {

// The most weights the product stages in LDS (PT_MORPH_LDS_TARGETS)
uint32_t morph_probe_lds_targets() {
    return PT_MORPH_LDS_TARGETS;
}

// pt_morph_rows over checked targets: row_start [n_vertices + 1], and of every entry its target and its delta [3]
void morph_probe_rows(uint32_t n_vertices, const pt_morph_target *targets, uint32_t n_targets, uint32_t *row_start, uint32_t *entry_target, float *entry_delta) {
    std::vector<uint32_t> rows;
    std::vector<PtMorphEntry> entries;
    pt_morph_rows(n_vertices, targets, n_targets, rows, entries);
    memcpy(row_start, rows.data(), rows.size() * sizeof(uint32_t));
    for(size_t e = 0; e < entries.size(); e++) {
        entry_target[e] = entries[e].target;
        entry_delta[3 * e] = entries[e].dx;
        entry_delta[3 * e + 1] = entries[e].dy;
        entry_delta[3 * e + 2] = entries[e].dz;
    }
}

// pt_morph_rows, then pt_morph_launch over host arrays; lds_targets and lds_bones as there (0 forces the cache form); K = 0: no
// skinning, bone / weight / bones may be null.  The result array is filled with 0xA5 before the launch.  Returns 0, or 1000 + the error.
int morph_probe_morph(uint32_t n_vertices, const float *rest, const pt_morph_target *targets, uint32_t n_targets, const float *weights, uint32_t lds_targets, uint32_t K,
                      const uint32_t *bone, const float *weight, const float *bones, uint32_t n_bones, uint32_t lds_bones, float *out) {
    std::vector<uint32_t> rows;
    std::vector<PtMorphEntry> entries;
    pt_morph_rows(n_vertices, targets, n_targets, rows, entries);
    void *d_rest = nullptr, *d_rows = nullptr, *d_entries = nullptr, *d_weights = nullptr, *d_bone = nullptr, *d_weight = nullptr, *d_bones = nullptr, *d_out = nullptr;
    const size_t nv = n_vertices, nk = nv * K;
    if(hipMalloc(&d_rest, 12 * nv + 1) != hipSuccess || hipMalloc(&d_rows, 4 * rows.size()) != hipSuccess || hipMalloc(&d_entries, 16 * entries.size() + 1) != hipSuccess ||
       hipMalloc(&d_weights, 4 * static_cast<size_t>(n_targets) + 1) != hipSuccess || hipMalloc(&d_bone, 4 * nk + 1) != hipSuccess ||
       hipMalloc(&d_weight, 4 * nk + 1) != hipSuccess || hipMalloc(&d_bones, 48 * static_cast<size_t>(n_bones) + 1) != hipSuccess || hipMalloc(&d_out, 12 * nv + 1) != hipSuccess) {
        return 999;
    }
    memcpy(d_rest, rest, 12 * nv);
    memcpy(d_rows, rows.data(), 4 * rows.size());
    memcpy(d_entries, entries.data(), 16 * entries.size());
    memcpy(d_weights, weights, 4 * static_cast<size_t>(n_targets));
    if(K > 0) {
        memcpy(d_bone, bone, 4 * nk);
        memcpy(d_weight, weight, 4 * nk);
        memcpy(d_bones, bones, 48 * static_cast<size_t>(n_bones));
    }
    memset(d_out, 0xA5, 12 * nv);
    const hipError_t e = pt_morph_launch(nullptr, n_vertices, static_cast<const float *>(d_rest), static_cast<const uint32_t *>(d_rows), static_cast<const PtMorphEntry *>(d_entries),
                                         static_cast<const float *>(d_weights), n_targets, lds_targets, K, static_cast<const uint32_t *>(d_bone), static_cast<const float *>(d_weight),
                                         static_cast<const float *>(d_bones), n_bones, lds_bones, static_cast<float *>(d_out));
    memcpy(out, d_out, 12 * nv);
    for(void *p : {d_rest, d_rows, d_entries, d_weights, d_bone, d_weight, d_bones, d_out}) {
        hipFree(p);
    }
    return e == hipSuccess ? 0 : 1000 + static_cast<int>(e);
}

} // extern "C"
