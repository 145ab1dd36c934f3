// tests/cpp/features_test.cpp -- followed features through the C++ API (PathTrace/denoise.h, FrameRender / ViewBatchRender::setFeatureParams)
// and the C ABI (include/pt_features.h).  tests/test_features_follow_cpu.py compiles and links it; with a device it also runs:
// denoise(..., FeatureParams{0}) equals denoise(...) bit for bit, and FeatureParams{8} changes a frame that shows a mirror.
#include <PathTrace/camera.h>
#include <PathTrace/denoise.h>
#include <PathTrace/frame_render.h>
#include <PathTrace/scene/light.h>
#include <PathTrace/scene/mesh.h>
#include <PathTrace/scene/object.h>
#include <PathTrace/scene/scene.h>
#include <PathTrace/view_batch_render.h>

#include "../../include/pt_hip.h"

#include <cstdio>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <vector>

namespace {

int failures = 0;

void expect(bool ok, const char *what) {
    std::printf("%s: %s\n", what, ok ? "ok" : "FAILED");
    if(!ok) {
        failures++;
    }
}

bool same(const Image<> &a, const Image<> &b) {
    return a.getWidth() == b.getWidth() && a.getHeight() == b.getHeight() &&
           std::memcmp(a.data(), b.data(), a.size() * sizeof(Color<float>)) == 0;
}

} // namespace

int main() {
    pt_feature_params p{};
    expect(pt_feature_params_default(&p) == PT_OK && p.max_bounces == 8 && p.flags == 0, "pt_feature_params_default");
    expect(pt_feature_params_default(nullptr) == PT_ERR_INVALID, "pt_feature_params_default(null)");
    expect(FeatureParams{}.max_bounces == 8, "FeatureParams default");
    float dummy[12];
    expect(pt_render_features_followed(nullptr, nullptr, nullptr, nullptr, dummy) == PT_ERR_INVALID, "null arguments are refused");
    expect(pt_frame_set_feature_params(nullptr, &p) == PT_ERR_INVALID, "a null frame is refused");
    // (taken, not called: the members exist with these signatures)
    void (FrameRender::*set_frame)(const pt_feature_params *) = &FrameRender::setFeatureParams;
    void (ViewBatchRender::*set_views)(const pt_feature_params *) = &ViewBatchRender::setFeatureParams;
    expect(set_frame != nullptr && set_views != nullptr, "setFeatureParams members");
    if(pt_device_count() < 1) {
        std::printf("no device: the rest is skipped\n");
        return failures == 0 ? 0 : 1;
    }
    // a mirror sphere in the Box benchmark scene, seen from inside the box
    std::vector<std::unique_ptr<Object>> objects;
    std::vector<std::unique_ptr<LightSource>> lights;
    auto walls = makeBox(vec3<float>{-1.0F, -1.0F, -1.0F}, vec3<float>{1.0F, 1.0F, 1.0F});
    auto paint = std::make_shared<ConstantMaterialHandler>(std::make_shared<ConstantMaterial>(Color<float>(0.8F, 0.3F, 0.2F, 1.0F)), std::make_shared<LambertianBRDF>());
    for(auto &t : walls) {
        t.setMaterialHandler(paint);
    }
    moveObjects(objects, walls);
    auto ball = std::make_unique<Sphere>(vec3<float>{0.1F, -0.2F, 0.3F}, 0.5F);
    ball->setMaterialHandler(std::make_shared<ConstantMaterialHandler>(std::make_shared<ConstantMaterial>(), std::make_shared<MirrorBRDF>(false)));
    objects.push_back(std::move(ball));
    Scene scene(std::move(objects), std::move(lights));
    Camera camera({0.0F, 0.0F, -0.9F}, {0.0F, 0.0F, 0.0F}, {0.0F, 1.0F, 0.0F}, 1.0F, 1.0F, -1.0F);
    RenderOptions options{32, 24, 1, 1, 1E-3F};
    Image<> frame(32, 24);
    for(int y = 0; y < 24; y++) {
        for(int x = 0; x < 32; x++) {
            frame(x, y) = Color<float>{static_cast<float>((x * 7 + y * 3) % 5) * 0.2F, 0.5F, static_cast<float>(x % 3) * 0.3F, 1.0F};
        }
    }
    const Image<> first = denoise(frame, scene, camera, options);
    expect(same(denoise(frame, scene, camera, options, DenoiseParams{}, FeatureParams{0}), first), "max_bounces 0 equals the first-hit denoise");
    expect(!same(denoise(frame, scene, camera, options, DenoiseParams{}, FeatureParams{8}), first), "followed features change a frame with a mirror");
    bool threw = false;
    try {
        denoise(frame, scene, camera, options, DenoiseParams{}, FeatureParams{33});
    }
    catch(const std::invalid_argument &) {
        threw = true;
    }
    expect(threw, "max_bounces 33 throws");
    return failures == 0 ? 0 : 1;
}
