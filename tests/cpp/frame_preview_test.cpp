// tests/cpp/frame_preview_test.cpp -- FrameRender::preview (include/PathTrace/frame_render.h) on the GPU: the sample classes of a stopped
// frame's preview match info(), the preview of the complete frame is image() bit for bit, and its denoised preview equals processJob with
// allow_bias and the same $PATHTRACE_SEED bit for bit.  Prints one line per check; exit status 0 = every check passed.
#include <PathTrace/camera.h>
#include <PathTrace/frame_render.h>
#include <PathTrace/render_control.h>
#include <PathTrace/scene/light.h>
#include <PathTrace/scene/mesh.h>
#include <PathTrace/scene/object.h>
#include <PathTrace/scene/scene.h>
#include <PathTrace/worker.h>

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

    bool same(const Image<> &a, const Image<> &b) {
        return a.getWidth() == b.getWidth() && a.getHeight() == b.getHeight() && std::memcmp(a.data(), b.data(), a.size() * sizeof(Color<float>)) == 0;
    }

} // namespace

int main() {
    setenv("PATHTRACE_SEED", "1357", 1);
    const int side = 2048; // more streams than the device has slots: a stop leaves finished, parked and untouched pixels
    Camera camera({0.0F, 0.0F, -3.0F}, {0.0F, 0.0F, 0.0F}, {0.0F, 1.0F, 0.0F}, 1.0F, 1.0F, 1.0F);
    Scene scene = boxScene();
    RenderOptions options{side, side, 32, 32, 1E-3F};
    FrameRenderJob job{camera, scene, options};

    FrameRender frame(job);
    Image<> preview;
    std::vector<std::int32_t> samples;
    frame.preview(preview, &samples);
    bool all_holes = preview.getWidth() == side && samples.size() == static_cast<size_t>(side) * side;
    for(size_t i = 0; i < samples.size() && all_holes; i++) {
        all_holes = samples[i] == 0;
    }
    expect(all_holes, "before the first render every pixel is a hole");

    bool complete = false;
    {
        RenderControl control;
        int reports = 0;
        complete = frame.render(control, [&](int, int) {
            if(++reports == 1) {
                control.cancel();
            }
        });
    }
    const pt_frame_info info = frame.info();
    frame.preview(preview, &samples);
    std::uint64_t finished = 0, parked = 0, untouched = 0, carried = 0;
    for(std::int32_t s : samples) {
        finished += s == -1 ? 1 : 0;
        parked += s >= 1 ? 1 : 0;
        untouched += s == 0 ? 1 : 0;
        carried += s >= 1 ? static_cast<std::uint64_t>(s) : 0;
    }
    std::printf("after the cancel: preview %llu finished, %llu parked (%llu samples), %llu untouched; info %llu, %llu (%llu), %llu\n",
                static_cast<unsigned long long>(finished), static_cast<unsigned long long>(parked), static_cast<unsigned long long>(carried),
                static_cast<unsigned long long>(untouched), static_cast<unsigned long long>(info.streams_finished),
                static_cast<unsigned long long>(info.streams_parked), static_cast<unsigned long long>(info.samples_carried),
                static_cast<unsigned long long>(info.streams_untouched));
    expect(!complete && info.streams_parked > 0, "the cancel parks half-finished pixels");
    expect(finished == info.streams_finished && parked == info.streams_parked && untouched == info.streams_untouched && carried == info.samples_carried,
           "the preview's sample classes match info()");

    int calls = 1;
    while(!complete && calls < 200) {
        RenderControl control;
        control.setBudget(std::chrono::milliseconds(60));
        complete = frame.render(control);
        calls++;
    }
    expect(complete, "budgeted calls complete the frame");
    frame.preview(preview, &samples);
    bool all_finished = true;
    for(std::int32_t s : samples) {
        all_finished = all_finished && s == -1;
    }
    expect(same(preview, frame.image()) && all_finished, "the preview of the complete frame is image() bit for bit");

    pt_denoise_params params{};
    pt_denoise_params_default(&params);
    frame.preview(preview, nullptr, &params);
    RenderOptions biased = options;
    biased.allow_bias = true;
    const Image<> clean = processJob(FrameRenderJob{camera, scene, biased});
    expect(same(preview, clean), "the denoised preview of the complete frame equals processJob with allow_bias bit for bit");
    return failures == 0 ? 0 : 1;
}
