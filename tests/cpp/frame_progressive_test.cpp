// tests/cpp/frame_progressive_test.cpp -- FrameRender::setProgressive / progress and the same on ViewBatchRender (include/PathTrace/frame_render.h,
// view_batch_render.h) on the GPU: a pass brings every pixel to the quantum, the preview has samples everywhere, the finished frame equals
// processJob / processViews with the same $PATHTRACE_SEED bit for bit.  Prints one line per check; exit status 0 = every check passed.
#include <PathTrace/camera.h>
#include <PathTrace/frame_render.h>
#include <PathTrace/render_control.h>
#include <PathTrace/scene/light.h>
#include <PathTrace/scene/mesh.h>
#include <PathTrace/scene/object.h>
#include <PathTrace/scene/scene.h>
#include <PathTrace/view_batch.h>
#include <PathTrace/view_batch_render.h>
#include <PathTrace/worker.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <stdexcept>
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
    setenv("PATHTRACE_SEED", "2468", 1);
    Camera camera({0.0F, 0.0F, -3.0F}, {0.0F, 0.0F, 0.0F}, {0.0F, 1.0F, 0.0F}, 1.0F, 1.0F, 1.0F);
    Scene scene = boxScene();
    RenderOptions options{512, 384, 16, 16, 1E-3F};
    FrameRenderJob job{camera, scene, options};

    FrameRender frame(job);
    frame.setProgressive(4, 1);
    bool complete = true;
    {
        RenderControl control;
        complete = frame.render(control);
    }
    pt_frame_progress progress = frame.progress();
    std::printf("after one pass: %d passes, target %d, samples %d..%d, %llu streams at the target\n", progress.passes_completed, progress.target,
                progress.min_samples, progress.max_samples, static_cast<unsigned long long>(progress.streams_at_target));
    expect(!complete && progress.passes_completed == 1 && progress.target == 4 && progress.pass_in_progress == 0 && progress.min_samples == 4 &&
             progress.max_samples == 4 && progress.samples_lost == 0 && progress.streams_at_target == 512ULL * 384ULL,
           "one pass brings every pixel to the quantum and stops");

    Image<> preview;
    std::vector<std::int32_t> samples;
    frame.preview(preview, &samples);
    bool all_four = samples.size() == 512U * 384U;
    for(std::int32_t s : samples) {
        all_four = all_four && s == 4;
    }
    expect(all_four, "the preview has 4 samples on every pixel");

    bool thrown = false;
    try {
        frame.setProgressive(-1);
    }
    catch(const std::invalid_argument &) {
        thrown = true;
    }
    expect(thrown && frame.progress().quantum == 4, "a negative quantum is refused and changes nothing");

    frame.setProgressive(6);
    {
        RenderControl control;
        complete = frame.render(control);
    }
    progress = frame.progress();
    expect(complete && progress.passes_completed == 3 && progress.target == 16 && same(frame.image(), processJob(job)),
           "passes of another quantum complete the frame; it equals processJob bit for bit");

    Camera second({0.3F, 0.1F, -3.0F}, {0.0F, 0.0F, 0.0F}, {0.0F, 1.0F, 0.0F}, 1.0F, 1.0F, 1.0F);
    const std::vector<const Camera *> cameras{&camera, &second};
    RenderOptions small{160, 128, 8, 8, 1E-3F};
    ViewBatchRender batch(scene, cameras, small);
    batch.setProgressive(3, 1);
    int calls = 0;
    bool even = true;
    for(bool done = false; !done && calls < 10; calls++) {
        RenderControl control;
        done = batch.render(control);
        const pt_frame_progress p = batch.progress();
        even = even && p.passes_completed == calls + 1 && (done || (p.min_samples == p.target && p.max_samples == p.target));
    }
    const std::vector<Image<>> got = batch.images(), want = processViews(scene, cameras, small);
    expect(batch.complete() && calls == 3 && even && got.size() == 2 && same(got[0], want[0]) && same(got[1], want[1]),
           "a progressive view batch advances evenly and equals processViews bit for bit");
    return failures == 0 ? 0 : 1;
}
