// tests/cpp/view_batch_render_test.cpp -- ViewBatchRender (include/PathTrace/view_batch_render.h) on the GPU: a batch sliced by
// RenderControl::setBudget until complete equals processViews with the same $PATHTRACE_SEED bit for bit, and its denoised preview once
// complete equals processViews with allow_bias.  Prints one line per check; exit status 0 = every check passed.
#include <PathTrace/camera.h>
#include <PathTrace/render_control.h>
#include <PathTrace/scene/light.h>
#include <PathTrace/scene/mesh.h>
#include <PathTrace/scene/object.h>
#include <PathTrace/scene/scene.h>
#include <PathTrace/view_batch.h>
#include <PathTrace/view_batch_render.h>
#include <PathTrace/worker.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

namespace {

    using Objects = std::vector<std::unique_ptr<Object>>;
    using Lights = std::vector<std::unique_ptr<LightSource>>;

    Scene boxScene() {
        Objects objects;
        Lights lights;
        auto walls = makeBox(vec3<float>{-1.0F, -1.0F, -1.0F}, vec3<float>{1.0F, 1.0F, 1.0F});
        moveObjects(objects, walls);
        auto lamp = makePlane(vec3<float>{-0.25F, 0.99F, -0.25F}, vec3<float>{0.25F, 0.99F, 0.25F});
        auto glow = std::make_shared<ConstantMaterial>(Color<float>(1.0F, 1.0F, 1.0F, 1.0F), 1.0F, Spectrum(Color<float>{1.0F, 1.0F, 1.0F, 1.0F}));
        auto handler = std::make_shared<ConstantMaterialHandler>(glow, std::make_shared<LambertianBRDF>());
        for(auto &t : lamp) {
            t.setMaterialHandler(handler);
        }
        moveObjects(objects, lamp);
        return Scene(std::move(objects), std::move(lights));
    }

    int failures = 0;

    void expect(bool ok, const char *what) {
        std::printf("%s %s\n", ok ? "[ OK ]" : "[FAIL]", what);
        failures += ok ? 0 : 1;
    }

    bool same(const std::vector<Image<>> &a, const std::vector<Image<>> &b) {
        bool ok = a.size() == b.size();
        for(size_t v = 0; ok && v < a.size(); v++) {
            ok = a[v].getWidth() == b[v].getWidth() && a[v].getHeight() == b[v].getHeight() &&
                 std::memcmp(a[v].data(), b[v].data(), a[v].size() * sizeof(Color<float>)) == 0;
        }
        return ok;
    }

} // namespace

int main() {
    setenv("PATHTRACE_SEED", "2468", 1);
    const int side = 256, n_views = 8;
    Scene scene = boxScene();
    std::vector<Camera> cameras;
    for(int v = 0; v < n_views; v++) {
        cameras.emplace_back(vec3<float>{0.08F * static_cast<float>(v) - 0.3F, 0.05F * static_cast<float>(v % 3), -3.0F}, vec3<float>{0.0F, 0.0F, 0.0F},
                             vec3<float>{0.0F, 1.0F, 0.0F}, 1.0F, 1.0F, 1.0F);
    }
    std::vector<const Camera *> views;
    for(const Camera &c : cameras) {
        views.push_back(&c);
    }
    RenderOptions options{side, side, 512, 512, 1E-3F};

    ViewBatchRender batch(scene, views, options);
    bool complete = false;
    int calls = 0, stopped_with_parked = 0;
    auto budget = std::chrono::milliseconds(40);
    while(!complete && calls < 200) {
        RenderControl control;
        control.setBudget(budget);
        complete = batch.render(control);
        calls++;
        const pt_frame_info info = batch.info();
        if(!complete && info.streams_parked > 0) {
            stopped_with_parked++;
        }
        else if(!complete) {
            budget *= 2; // (a budget shorter than the launch's start-up parks nothing)
        }
    }
    std::printf("%d calls, %d of them stopped with parked pixels\n", calls, stopped_with_parked);
    expect(complete && batch.complete() && stopped_with_parked > 0, "budgeted calls stop, resume and complete the batch");

    std::vector<std::uint64_t> seeds;
    const std::vector<Image<>> want = processViews(scene, views, options, [](int, int) {}, 0, &seeds);
    expect(seeds == batch.seeds() && same(batch.images(), want), "the sliced batch equals processViews with the same PATHTRACE_SEED bit for bit");

    pt_denoise_params params{};
    pt_denoise_params_default(&params);
    std::vector<Image<>> preview;
    batch.preview(preview, nullptr, &params);
    RenderOptions biased = options;
    biased.allow_bias = true;
    expect(same(preview, processViews(scene, views, biased)), "the denoised preview of the complete batch equals processViews with allow_bias bit for bit");
    return failures == 0 ? 0 : 1;
}
