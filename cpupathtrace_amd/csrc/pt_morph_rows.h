// pt_morph_rows.h -- a morph set's target-major lists (include/pt_morph.h) turned into the vertex-major rows the kernel gathers
// (pt_morph_kernels.h), on the host: pt_scene_bind_morphs (pt_morph.cpp) does this once per binding.  tests/hip/morph_probe.hip includes
// it as well, so that the tests run this very source.
#ifndef PT_MORPH_ROWS_H
#define PT_MORPH_ROWS_H

#include "../../include/pt_hip.h"
#include "pt_morph_skin.h"

#include <vector>

// A stable counting sort by vertex: count every vertex's entries, start every row at the running sum, and deal the targets out in
// ascending order, so that a row holds its entries in ascending target order.  The targets must have been checked (every index
// < n_vertices, a dense target of n_vertices deltas, at most 2^31 - 1 entries in all).  row_start: [n_vertices + 1].
inline void pt_morph_rows(uint32_t n_vertices, const pt_morph_target *targets, uint32_t n_targets, std::vector<uint32_t> &row_start, std::vector<PtMorphEntry> &entries) {
    row_start.assign(static_cast<size_t>(n_vertices) + 1, 0);
    for(uint32_t t = 0; t < n_targets; t++) {
        const pt_morph_target &target = targets[t];
        for(uint32_t j = 0; j < target.n_deltas; j++) {
            row_start[static_cast<size_t>(target.vertex != nullptr ? target.vertex[j] : j) + 1]++;
        }
    }
    for(size_t i = 0; i < n_vertices; i++) {
        row_start[i + 1] += row_start[i];
    }
    entries.resize(row_start[n_vertices]);
    std::vector<uint32_t> next(row_start.begin(), row_start.end() - 1);
    for(uint32_t t = 0; t < n_targets; t++) {
        const pt_morph_target &target = targets[t];
        for(uint32_t j = 0; j < target.n_deltas; j++) {
            const float *d = target.delta + 3 * static_cast<size_t>(j);
            entries[next[target.vertex != nullptr ? target.vertex[j] : j]++] = PtMorphEntry{d[0], d[1], d[2], t};
        }
    }
}

#endif
