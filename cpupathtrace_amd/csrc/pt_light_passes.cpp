// pt_light_passes.cpp -- the entry points of include/pt_light_passes.h: the radiance of pt_radiance.h's rays and captures
// split into passes by emitter group and bounce depth, and the mix of such passes.  The kernels are pt_light_pass_kernels.h's (in
// pt_walks.hip); this unit checks the arguments -- pt_radiance.cpp's checks first, then its own --, keeps the workspace -- one per device,
// grown on demand, from pt_sample_host.h's table and launch frame -- and cuts a call into launches of whole rays or pixels: at most PT_RADIANCE_CHUNK / P
// (ray or pixel, sample) pairs each, so that the P + 1 planes of a launch hold about as many cells as a radiance launch's one.  The group
// tables travel per call.  The host mix is plain fp32 on the host (this file is compiled without contraction, like the rest).  Nothing
// here changes the scene, so every call is allowed with a live pt_frame and with or without a motion mark.
#include "pt_sample_host.h"

using namespace pth;

namespace {

const uint64_t PASSES_MAX = 0x7fffffffULL;

// The buffers of the calls on one device beside the workspace of one launch (the total's plane): the host forms' rays and records, the
// group tables of the latest call, and the passes' planes
struct PassWorkspace : SampleWorkspace {
    DevBuf<float> rays;
    DevBuf<pt_light_pass> out_passes;
    DevBuf<pt_radiance_result> out_total;
    DevBuf<uint8_t> groups;
    std::vector<uint8_t> table; // ... as they are uploaded from: the materials' groups, then the point lights'
    DevBuf<F4> passes;
};

int check_shape(const pt_light_groups *g) {
    if(g->n_groups < 1 || g->n_groups > PT_LIGHT_GROUPS_MAX) {
        return fail(PT_ERR_INVALID, "n_groups must be 1..8");
    }
    if(g->split != 0 && g->split != 1) {
        return fail(PT_ERR_INVALID, "split must be 0 or 1");
    }
    return PT_OK;
}

uint32_t passes_of(const pt_light_groups *g) {
    return g->n_groups * (g->split != 0 ? 3U : 1U);
}

// What the header lists behind the radiance call's own refusals; n: the rays or pixels
int check_groups(const pt_light_groups *g, const void *passes, uint64_t n, const pt_radiance_params *params) {
    if(g == nullptr || (n > 0 && passes == nullptr)) {
        return fail(PT_ERR_INVALID, "null argument: groups or passes");
    }
    PT_TRY(check_shape(g));
    if((g->n_materials > 0 && g->material_group == nullptr) || (g->n_point_lights > 0 && g->point_light_group == nullptr)) {
        return fail(PT_ERR_INVALID, "a null group table with a non-zero count");
    }
    for(uint32_t m = 0; m < g->n_materials; m++) {
        if(g->material_group[m] >= g->n_groups) {
            return fail(PT_ERR_INVALID, "a material's group is not below n_groups");
        }
    }
    for(uint32_t l = 0; l < g->n_point_lights; l++) {
        if(g->point_light_group[l] >= g->n_groups) {
            return fail(PT_ERR_INVALID, "a point light's group is not below n_groups");
        }
    }
    // (n x samples <= 0x7fffffff has been checked, so the product fits 64 bits)
    if(n * static_cast<uint64_t>(params->samples) * passes_of(g) > PASSES_MAX) {
        return fail(PT_ERR_INVALID, "too many accumulators in one call: rays or pixels x samples x passes above 0x7fffffff");
    }
    return PT_OK;
}

// A call of n rays (d_rays or, host form, rays) or of the capture's n pixels (both null); host form: d_passes == null, the records go to
// `passes` and `total`
int run(pt_scene *s, const float *rays, const float *d_rays, const pt_capture_desc *capture, size_t n, const pt_light_groups *g, const pt_radiance_params *params,
        pt_light_pass *passes, pt_radiance_result *total, pt_light_pass *d_passes, pt_radiance_result *d_total, void *stream) {
    std::lock_guard<std::mutex> lock(s->render_mutex);
    if(g->n_materials != s->dev.n_materials || g->n_point_lights != s->dev.n_lights) {
        return fail(PT_ERR_INVALID, "the group tables do not fit the scene: it has " + std::to_string(s->dev.n_materials) + " materials and " + std::to_string(s->dev.n_lights) +
                                        " point lights");
    }
    PT_HIP(hipSetDevice(s->device));
    PassWorkspace &ws = sample_workspace<PassWorkspace>(s->device);
    std::lock_guard<std::mutex> ws_lock(ws.mutex);
    const uint32_t n_passes = passes_of(g);
    // PT_RADIANCE_CHUNK / P pairs a launch, so that its P + 1 planes hold about as many cells as a radiance launch's one
    const size_t step = chunk_items("PT_RADIANCE_CHUNK", RADIANCE_CHUNK_DEFAULT, params->samples, n_passes);
    PT_TRY(settle(ws));
    const size_t pairs = std::min(n, step) * static_cast<size_t>(params->samples);
    PtPathConfig cfg;
    PT_TRY(size_launch(s, ws.spill, pairs, &ws.plane, pairs, &cfg));
    PT_HIP(ws.passes.ensure(pairs * n_passes));
    const size_t n_table = static_cast<size_t>(g->n_materials) + g->n_point_lights;
    // (kept in the workspace: a device-form call returns while its copy may still read it; settle() has ended the call before)
    std::vector<uint8_t> &table = ws.table;
    table.assign(g->material_group, g->material_group + g->n_materials);
    table.insert(table.end(), g->point_light_group, g->point_light_group + g->n_point_lights);
    PT_HIP(ws.groups.ensure(n_table));
    const bool host = d_passes == nullptr;
    if(host) {
        PT_HIP(ws.out_passes.ensure(n * n_passes));
        if(total != nullptr) {
            PT_HIP(ws.out_total.ensure(n));
        }
        if(rays != nullptr) {
            PT_HIP(ws.rays.ensure(6 * n));
        }
    }
    const PtCaptureParams cap = radiance_device_capture(capture);
    const float *use_rays = host ? (rays != nullptr ? ws.rays.ptr : nullptr) : d_rays;
    pt_light_pass *out_passes = host ? ws.out_passes.ptr : d_passes;
    pt_radiance_result *out_total = host ? (total != nullptr ? ws.out_total.ptr : nullptr) : d_total;
    auto enqueue_all = [&]() -> int {
        if(n_table > 0) {
            PT_HIP(hipMemcpyAsync(ws.groups.ptr, table.data(), n_table, hipMemcpyHostToDevice, s->stream));
        }
        if(host && rays != nullptr) {
            PT_HIP(hipMemcpyAsync(ws.rays.ptr, rays, 6 * n * sizeof(float), hipMemcpyHostToDevice, s->stream));
        }
        for(size_t first = 0; first < n; first += step) {
            pt_launch_light_passes(s->stream, s->dev, use_rays, cap, static_cast<uint32_t>(first), static_cast<uint32_t>(std::min(step, n - first)),
                                   static_cast<uint32_t>(params->samples), params->epsilon, params->base_seed, ws.groups.ptr, n_passes, g->split != 0 ? 1U : 0U,
                                   reinterpret_cast<float4 *>(ws.plane.ptr), reinterpret_cast<float4 *>(ws.passes.ptr), reinterpret_cast<float4 *>(out_passes),
                                   reinterpret_cast<float4 *>(out_total), cfg);
        }
        if(host) {
            PT_HIP(hipMemcpyAsync(passes, ws.out_passes.ptr, n * n_passes * sizeof(pt_light_pass), hipMemcpyDeviceToHost, s->stream));
            if(total != nullptr) {
                PT_HIP(hipMemcpyAsync(total, ws.out_total.ptr, n * sizeof(pt_radiance_result), hipMemcpyDeviceToHost, s->stream));
            }
        }
        return PT_OK;
    };
    if(host) {
        return run_host(s, enqueue_all);
    }
    return run_device(s, &ws, stream, enqueue_all);
}

} // namespace

extern "C" {

int pt_light_passes_count(const pt_light_groups *groups, uint32_t *n_passes) {
    if(groups == nullptr || n_passes == nullptr) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    PT_TRY(check_shape(groups));
    *n_passes = passes_of(groups);
    return PT_OK;
}

int pt_light_passes_rays(pt_scene *s, const float *rays, size_t n, const pt_light_groups *groups, const pt_radiance_params *params, pt_light_pass *passes, pt_radiance_result *total) {
    PT_TRY(radiance_check_rays(s, rays, n, params, passes));
    PT_TRY(check_groups(groups, passes, n, params));
    if(n == 0) {
        return PT_OK;
    }
    return run(s, rays, nullptr, nullptr, n, groups, params, passes, total, nullptr, nullptr, nullptr);
}

int pt_light_passes_rays_device(pt_scene *s, const float *d_rays, size_t n, const pt_light_groups *groups, const pt_radiance_params *params, pt_light_pass *d_passes,
                                pt_radiance_result *d_total, void *stream) {
    PT_TRY(radiance_check_rays(s, d_rays, n, params, d_passes));
    PT_TRY(check_groups(groups, d_passes, n, params));
    if(n == 0) {
        return PT_OK;
    }
    return run(s, nullptr, d_rays, nullptr, n, groups, params, nullptr, nullptr, d_passes, d_total, stream);
}

int pt_light_passes_capture(pt_scene *s, const pt_capture_desc *capture, const pt_light_groups *groups, const pt_radiance_params *params, pt_light_pass *passes,
                            pt_radiance_result *total) {
    uint64_t n = 0;
    PT_TRY(radiance_check_capture(s, capture, params, passes, &n));
    PT_TRY(check_groups(groups, passes, n, params));
    return run(s, nullptr, nullptr, capture, static_cast<size_t>(n), groups, params, passes, total, nullptr, nullptr, nullptr);
}

int pt_light_passes_capture_device(pt_scene *s, const pt_capture_desc *capture, const pt_light_groups *groups, const pt_radiance_params *params, pt_light_pass *d_passes,
                                   pt_radiance_result *d_total, void *stream) {
    uint64_t n = 0;
    PT_TRY(radiance_check_capture(s, capture, params, d_passes, &n));
    PT_TRY(check_groups(groups, d_passes, n, params));
    return run(s, nullptr, nullptr, capture, static_cast<size_t>(n), groups, params, nullptr, nullptr, d_passes, d_total, stream);
}

int pt_light_passes_mix(const pt_light_pass *passes, size_t n, uint32_t n_passes, const float *gains, const pt_radiance_result *total, float *out) {
    if(n > 0 && (passes == nullptr || gains == nullptr || out == nullptr)) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    if(n_passes < 1 || n_passes > 3 * PT_LIGHT_GROUPS_MAX) {
        return fail(PT_ERR_INVALID, "n_passes must be 1..24");
    }
    for(size_t i = 0; i < n; i++) {
        float acc[3] = {0.0F, 0.0F, 0.0F};
        for(uint32_t p = 0; p < n_passes; p++) {
            for(int c = 0; c < 3; c++) {
                const float product = passes[i * n_passes + p].value[c] * gains[3 * p + c];
                acc[c] = acc[c] + product;
            }
        }
        out[4 * i] = acc[0];
        out[4 * i + 1] = acc[1];
        out[4 * i + 2] = acc[2];
        out[4 * i + 3] = total != nullptr ? total[i].value[3] : 0.0F;
    }
    return PT_OK;
}

int pt_light_passes_mix_device(pt_scene *s, const pt_light_pass *d_passes, size_t n, uint32_t n_passes, const float *d_gains, const pt_radiance_result *d_total, float *d_out,
                               void *stream) {
    if(s == nullptr || (n > 0 && (d_passes == nullptr || d_gains == nullptr || d_out == nullptr))) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    if(n_passes < 1 || n_passes > 3 * PT_LIGHT_GROUPS_MAX) {
        return fail(PT_ERR_INVALID, "n_passes must be 1..24");
    }
    if(n == 0) {
        return PT_OK;
    }
    std::lock_guard<std::mutex> lock(s->render_mutex);
    PT_HIP(hipSetDevice(s->device));
    return run_device(s, nullptr, stream, [&]() -> int {
        pt_launch_light_pass_mix(s->stream, reinterpret_cast<const float4 *>(d_passes), n, n_passes, d_gains, reinterpret_cast<const float4 *>(d_total),
                                 reinterpret_cast<float4 *>(d_out));
        return PT_OK;
    });
}

} // extern "C"
