// pt_motion.cpp -- the entry points of include/pt_motion.h that describe motion: the per-instance table that takes a point
// of the current pose back to the previous one (pt_motion_table: host arithmetic in double, no device), and the feature pass that also
// writes every pixel's previous position and normal (pt_walks.hip: pt_motion_kernel).  The temporal push that reads them is with the other
// pushes in pt_image.cpp.
#include "pt_host.h"

using namespace pth;

namespace {

double det3(const double m[9]) {
    return m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}

// inverse by adjugate / determinant
void inv3(const double m[9], double det, double out[9]) {
    out[0] = (m[4] * m[8] - m[5] * m[7]) / det;
    out[1] = (m[2] * m[7] - m[1] * m[8]) / det;
    out[2] = (m[1] * m[5] - m[2] * m[4]) / det;
    out[3] = (m[5] * m[6] - m[3] * m[8]) / det;
    out[4] = (m[0] * m[8] - m[2] * m[6]) / det;
    out[5] = (m[2] * m[3] - m[0] * m[5]) / det;
    out[6] = (m[3] * m[7] - m[4] * m[6]) / det;
    out[7] = (m[1] * m[6] - m[0] * m[7]) / det;
    out[8] = (m[0] * m[4] - m[1] * m[3]) / det;
}

void mul3(const double a[9], const double b[9], double out[9]) {
    for(int r = 0; r < 3; r++) {
        for(int c = 0; c < 3; c++) {
            out[3 * r + c] = (a[3 * r] * b[c] + a[3 * r + 1] * b[3 + c]) + a[3 * r + 2] * b[6 + c];
        }
    }
}

} // namespace

namespace pth {

// One instance of pt_motion_table: the kind, and for a moved instance back[12] and normal[9]
uint8_t motion_of(const float *c, const float *p, float back[12], float normal[9]) {
    if(std::memcmp(c, p, 16 * sizeof(float)) == 0) {
        return PT_MOTION_STATIC;
    }
    for(int i = 0; i < 16; i++) {
        if(!std::isfinite(c[i]) || !std::isfinite(p[i])) {
            return PT_MOTION_NONE;
        }
    }
    for(const float *m : {c, p}) {
        if(!(m[12] == 0.0F && m[13] == 0.0F && m[14] == 0.0F && m[15] == 1.0F)) {
            return PT_MOTION_NONE;
        }
    }
    double a[9], b[9];
    for(int r = 0; r < 3; r++) {
        for(int k = 0; k < 3; k++) {
            a[3 * r + k] = c[4 * r + k];
            b[3 * r + k] = p[4 * r + k];
        }
    }
    const double det_a = det3(a), det_b = det3(b);
    if(!std::isfinite(det_a) || det_a == 0.0 || !std::isfinite(det_b) || det_b == 0.0) {
        return PT_MOTION_NONE;
    }
    double a_inv[9], b_inv[9], l[9], nt[9];
    inv3(a, det_a, a_inv);
    inv3(b, det_b, b_inv);
    mul3(b, a_inv, l);
    mul3(a, b_inv, nt);
    for(int r = 0; r < 3; r++) {
        for(int k = 0; k < 3; k++) {
            back[4 * r + k] = static_cast<float>(l[3 * r + k]);
            normal[3 * r + k] = static_cast<float>(nt[3 * k + r]); // the transpose
        }
        const double lc = (l[3 * r] * c[3] + l[3 * r + 1] * c[7]) + l[3 * r + 2] * c[11];
        back[4 * r + 3] = static_cast<float>(p[4 * r + 3] - lc);
    }
    for(int i = 0; i < 12; i++) {
        if(!std::isfinite(back[i])) {
            return PT_MOTION_NONE;
        }
    }
    for(int i = 0; i < 9; i++) {
        if(!std::isfinite(normal[i])) {
            return PT_MOTION_NONE;
        }
    }
    return PT_MOTION_MOVED;
}

void motion_identity(uint8_t kind, float back[12], float normal[9]) {
    const float d = kind == PT_MOTION_STATIC ? 1.0F : 0.0F;
    std::fill(back, back + 12, 0.0F);
    std::fill(normal, normal + 9, 0.0F);
    back[0] = back[5] = back[10] = d;
    normal[0] = normal[4] = normal[8] = d;
}

// The arguments of the two entries, checked without a device
int motion_check(pt_scene *s, const pt_camera_params *camera, const pt_options *options, const float *out_features, const float *out_motion) {
    if(options != nullptr && options->image_width > 0 && options->image_height > 0 &&
       static_cast<uint64_t>(options->image_height) * static_cast<uint64_t>(options->image_width) > 0x0fffffffULL) {
        return fail(PT_ERR_INVALID, "more than 0x0fffffff pixels");
    }
    PT_TRY(check_render_args(s, camera, options));
    if(out_features == nullptr || out_motion == nullptr) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    return PT_OK;
}

// The device table of the call (render_mutex held): the instances that have objects, each with the way back from the scene's pose to
// `previous`.  *n_out = 0 when nothing moved: no table is needed then.  No device work before the last refusal.
int motion_instances(pt_scene *s, const float *previous, uint32_t *n_out) {
    *n_out = 0;
    if(previous == nullptr) {
        return PT_OK;
    }
    if(s->pose == nullptr) {
        return fail(PT_ERR_UNSUPPORTED, "the scene has no instances: it was not made by pt_scene_create_meshes with instances");
    }
    const std::vector<pt_mesh_instance> &instances = s->pose->instances;
    std::vector<PtMotionInstance> table;
    bool any_moved = false;
    for(size_t i = 0; i < instances.size(); i++) {
        if(s->inst_count[i] == 0) { // (shares its first object with a neighbour: never looked up)
            continue;
        }
        PtMotionInstance m{};
        float back[12], normal[9];
        const uint8_t kind = motion_of(instances[i].transform, previous + 16 * i, back, normal);
        if(kind != PT_MOTION_MOVED) {
            motion_identity(kind, back, normal);
        }
        any_moved = any_moved || kind != PT_MOTION_STATIC;
        m.first = s->inst_first[i];
        m.count = s->inst_count[i];
        m.kind = kind;
        std::copy(back, back + 12, m.back);
        for(int r = 0; r < 3; r++) {
            std::copy(normal + 3 * r, normal + 3 * r + 3, m.normal + 4 * r);
        }
        table.push_back(m);
    }
    if(!any_moved) {
        return PT_OK;
    }
    PT_HIP(hipSetDevice(s->device));
    PT_HIP(s->motion_instances.ensure(table.size()));
    PT_HIP(hipMemcpyAsync(s->motion_instances.ptr, table.data(), table.size() * sizeof(PtMotionInstance), hipMemcpyHostToDevice, s->stream));
    PT_HIP(hipStreamSynchronize(s->stream)); // the table is this function's vector
    *n_out = static_cast<uint32_t>(table.size());
    return PT_OK;
}

// Enqueues the pass on the scene's stream (render_mutex held), as features_views_launch does for one view
int motion_launch(pt_scene *s, const pt_camera_params *camera, const pt_options *options, uint32_t n_instances, float4 *d_features, float4 *d_motion) {
    PT_TRY(setup_path(s));
    PtDevCamera cam = derive_camera(camera);
    cam.aperture_kind = PT_APERTURE_NONE; // the rays are a pure function of camera and pixel
    PtPathConfig cfg = s->path_cfg;
    const size_t n = static_cast<size_t>(options->image_width) * static_cast<size_t>(options->image_height);
    PT_HIP(s->feature_spill.ensure(((n + 255) / 256) * 256 * cfg.spill_depth));
    cfg.spill = s->feature_spill.ptr;
    pt_launch_features_motion(s->stream, s->dev, cam, options->image_width, options->image_height, d_features, d_motion, s->motion_instances.ptr, n_instances, cfg);
    PT_HIP(hipGetLastError());
    return PT_OK;
}

} // namespace pth

extern "C" {

int pt_motion_table(const float *current, const float *previous, uint32_t n, uint8_t *out_kind, float *out_back, float *out_normal) {
    if(n > 0 && (current == nullptr || previous == nullptr || out_kind == nullptr || out_back == nullptr || out_normal == nullptr)) {
        return fail(PT_ERR_INVALID, "null argument");
    }
    for(size_t i = 0; i < n; i++) {
        float back[12], normal[9];
        const uint8_t kind = motion_of(current + 16 * i, previous + 16 * i, back, normal);
        if(kind != PT_MOTION_MOVED) {
            motion_identity(kind, back, normal);
        }
        out_kind[i] = kind;
        std::copy(back, back + 12, out_back + 12 * i);
        std::copy(normal, normal + 9, out_normal + 9 * i);
    }
    return PT_OK;
}

int pt_render_features_motion(pt_scene *s, const pt_camera_params *camera, const pt_options *options, const float *previous_transforms, float *out_features,
                              float *out_motion) {
    PT_TRY(motion_check(s, camera, options, out_features, out_motion));
    const size_t n = static_cast<size_t>(options->image_width) * static_cast<size_t>(options->image_height);
    std::lock_guard<std::mutex> lock(s->render_mutex);
    uint32_t n_instances = 0;
    PT_TRY(motion_instances(s, previous_transforms, &n_instances));
    PT_HIP(hipSetDevice(s->device));
    PT_HIP(s->features.ensure(3 * n));
    PT_HIP(s->motion.ensure(2 * n));
    PT_TRY(motion_launch(s, camera, options, n_instances, reinterpret_cast<float4 *>(s->features.ptr), reinterpret_cast<float4 *>(s->motion.ptr)));
    PT_HIP(hipMemcpyAsync(out_features, s->features.ptr, 3 * n * sizeof(F4), hipMemcpyDeviceToHost, s->stream));
    PT_HIP(hipMemcpyAsync(out_motion, s->motion.ptr, 2 * n * sizeof(F4), hipMemcpyDeviceToHost, s->stream));
    PT_HIP(hipStreamSynchronize(s->stream));
    return PT_OK;
}

int pt_render_features_motion_device(pt_scene *s, const pt_camera_params *camera, const pt_options *options, const float *previous_transforms, float *d_out_features,
                                     float *d_out_motion, void *stream) {
    PT_TRY(motion_check(s, camera, options, d_out_features, d_out_motion));
    std::lock_guard<std::mutex> lock(s->render_mutex);
    uint32_t n_instances = 0;
    PT_TRY(motion_instances(s, previous_transforms, &n_instances));
    PT_HIP(hipSetDevice(s->device));
    // order after the caller's stream, trace on the library's stream, then make the caller's stream wait for it
    StreamOrder order;
    PT_TRY(order.begin(stream, s->stream));
    PT_TRY(motion_launch(s, camera, options, n_instances, reinterpret_cast<float4 *>(d_out_features), reinterpret_cast<float4 *>(d_out_motion)));
    PT_TRY(order.end());
    if(order.caller == nullptr) {
        PT_HIP(hipStreamSynchronize(s->stream));
    }
    return PT_OK;
}

} // extern "C"
