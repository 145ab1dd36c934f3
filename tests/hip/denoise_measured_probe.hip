// denoise_measured_probe.hip -- TEST ONLY: the measured form of the denoiser (pt_denoise_measured_run, cpupathtrace_amd/csrc/pt_denoise.hip)
// on caller-given frames and planes, whole runs and one kernel at a time.
//
// Built by tests/denoise_measured_probe.py into tests/hip/libdenoise_measured_probe.so with the product's compiler flags; not part of
// libpathtrace_hip.so.  denoise_probe.hip is included unchanged: it brings pt_denoise.hip, its guarded buffers (guard bands of the byte
// 0xA5 of `width + 64` elements around every device array, compared after the run) and its own entry points ptd_*, so that the existing
// filter runs from the same library and the two can be compared device against device.  Every ptm_* entry point takes host arrays and
// returns what the ptd_* ones do: the HIP error code or PTD_GUARD_TOUCHED + the number of the buffer whose guard band was written.
#include "denoise_probe.hip"

extern "C" {

// pt_denoise_measured_run: samples null = the plain stages
int ptm_run(int32_t width, int32_t height, const float *rgba, const float *features, const float *plane, const int32_t *samples, const PtDenoiseParams *params,
            float sigma_measured, int in_place, float *out) {
    Status st;
    Stream stream(st);
    const size_t n = static_cast<size_t>(width) * height, g = static_cast<size_t>(width) + 64;
    Guarded<float4> d_rgba(st, n, g, rgba), d_out(st, in_place ? 0 : n, g), d_feat(st, 3 * n, g, features), d_plane(st, n, g, plane);
    Guarded<int32_t> d_samples(st, samples != nullptr ? n : 0, g, samples);
    Scratch scratch(st, n, g);
    float4 *o = in_place ? d_rgba.p() : d_out.p();
    if(st.ok()) {
        st(pt_denoise_measured_run(stream.s, d_rgba.p(), d_feat.p(), d_plane.p(), samples != nullptr ? d_samples.p() : nullptr, width, height, *params,
                                   sigma_measured, scratch.get(), o));
    }
    stream.wait();
    if(st.ok()) {
        st(hipMemcpy(out, o, n * sizeof(float4), hipMemcpyDeviceToHost));
    }
    d_rgba.check();
    d_out.check();
    d_feat.check();
    d_plane.check();
    d_samples.check();
    scratch.check();
    return st.code();
}

int ptm_variance(int masked, int32_t width, int32_t height, const float *col, const float *guide, const uint32_t *cls, const float *features, const float *plane,
                 float sigma_normal, float sigma_depth, float *grad, float *var) {
    Status st;
    Stream stream(st);
    const size_t n = static_cast<size_t>(width) * height, g = static_cast<size_t>(width) + 64;
    Guarded<float4> d_col(st, n, g, col), d_guide(st, n, g, guide), d_feat(st, 3 * n, g, features), d_plane(st, n, g, plane);
    Guarded<uint32_t> d_cls(st, n, g, cls);
    Guarded<float2> d_grad(st, n, g);
    Guarded<float> d_var(st, n, g);
    if(st.ok()) {
        const dim3 grid = grid_of(width, height), block(16, 16);
        const PtMeasuredPixel mp{d_plane.p(), d_feat.p(), 0.0f};
        if(masked) {
            hipLaunchKernelGGL(pt_denoise_variance_measured_kernel<true>, grid, block, 0, stream.s, d_col.p(), d_guide.p(), d_cls.p(), width, height, sigma_normal,
                               sigma_depth, d_grad.p(), d_var.p(), mp);
        }
        else {
            hipLaunchKernelGGL(pt_denoise_variance_measured_kernel<false>, grid, block, 0, stream.s, d_col.p(), d_guide.p(), d_cls.p(), width, height, sigma_normal,
                               sigma_depth, d_grad.p(), d_var.p(), mp);
        }
    }
    stream.wait();
    d_grad.get(grad);
    d_var.get(var);
    d_col.check();
    d_guide.check();
    d_feat.check();
    d_plane.check();
    d_cls.check();
    d_grad.check();
    d_var.check();
    return st.code();
}

// one a-trous launch at `step`
int ptm_atrous(int masked, int32_t width, int32_t height, const float *col, const float *var, const float *guide, const uint32_t *cls, const float *grad,
               const float *plane, int32_t step, float sigma_luminance, float sigma_normal, float sigma_depth, float sigma_measured, float *col_out,
               float *var_out) {
    Status st;
    Stream stream(st);
    const size_t n = static_cast<size_t>(width) * height, g = static_cast<size_t>(width) + 64;
    Guarded<float4> d_col(st, n, g, col), d_guide(st, n, g, guide), d_col_out(st, n, g), d_plane(st, n, g, plane);
    Guarded<float> d_var(st, n, g, var), d_var_out(st, n, g);
    Guarded<uint32_t> d_cls(st, n, g, cls);
    Guarded<float2> d_grad(st, n, g, grad);
    if(st.ok()) {
        const dim3 grid = grid_of(width, height), block(16, 16);
        const PtMeasuredPixel mp{d_plane.p(), nullptr, sigma_measured};
        if(masked) {
            hipLaunchKernelGGL(pt_denoise_atrous_measured_kernel<true>, grid, block, 0, stream.s, d_col.p(), d_var.p(), d_guide.p(), d_cls.p(), d_grad.p(), width,
                               height, step, sigma_luminance, sigma_normal, sigma_depth, d_col_out.p(), d_var_out.p(), mp);
        }
        else {
            hipLaunchKernelGGL(pt_denoise_atrous_measured_kernel<false>, grid, block, 0, stream.s, d_col.p(), d_var.p(), d_guide.p(), d_cls.p(), d_grad.p(), width,
                               height, step, sigma_luminance, sigma_normal, sigma_depth, d_col_out.p(), d_var_out.p(), mp);
        }
    }
    stream.wait();
    d_col_out.get(col_out);
    d_var_out.get(var_out);
    d_col.check();
    d_guide.check();
    d_col_out.check();
    d_plane.check();
    d_var.check();
    d_var_out.check();
    d_cls.check();
    d_grad.check();
    return st.code();
}

} // extern "C"
