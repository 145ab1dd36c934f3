// tests/cpp/frame_noise_test.cpp -- FrameRender::setNoiseTarget / noise / errorMap / noiseTargetReached and the same on ViewBatchRender
// (include/PathTrace/frame_render.h, view_batch_render.h) on the GPU: the summary agrees with the map, a progressive frame with a target
// stops once enough of it is finished or held, and with the target cleared it finishes equal to processJob / processViews with the same
// $PATHTRACE_SEED bit for bit.  Prints one line per check; exit status 0 = every check passed.
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

#include <cmath>
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
    RenderOptions options{32, 32, 8, 64, 1E-3F};
    FrameRenderJob job{camera, scene, options};

    FrameRender frame(job);
    frame.setProgressive(8, 1);
    for(int pass = 0; pass < 2; pass++) {
        RenderControl control;
        frame.render(control);
    }
    const pt_frame_noise before = frame.noise();
    const std::vector<float> map = frame.errorMap();
    std::uint64_t finished = 0, rated = 0, unrated = 0;
    float largest = 0.0F;
    for(float e : map) {
        finished += e == -1.0F ? 1 : 0;
        unrated += std::isinf(e) ? 1 : 0;
        if(e >= 0.0F && std::isfinite(e)) {
            rated++;
            largest = e > largest ? e : largest;
        }
    }
    std::printf("after two passes: %llu finished, %llu rated, %llu unrated, largest error %g\n", static_cast<unsigned long long>(finished),
                static_cast<unsigned long long>(rated), static_cast<unsigned long long>(unrated), largest);
    expect(map.size() == 32U * 32U && before.streams_total == 32U * 32U && before.streams_finished == finished && before.streams_rated == rated &&
             before.streams_unrated == unrated && before.max_error == largest && rated > 0 && before.streams_held == 0 && before.target_reached == 0 &&
             !frame.noiseTargetReached(),
           "noise() agrees with errorMap(); nothing is held without a target");

    bool thrown = false;
    try {
        frame.setNoiseTarget(0.1F, 1E-5F, 0.0F);
    }
    catch(const std::invalid_argument &) {
        thrown = true;
    }
    expect(thrown && frame.noise().target_error == 0.0F, "a fraction of 0 is refused and changes nothing");

    // half the largest error, on half the frame: reached at once or after a few passes, and long before the frame is complete
    frame.setNoiseTarget(largest * 0.5F, 1E-5F, 0.5F);
    int calls = 0;
    bool complete = false;
    while(!complete && !frame.noiseTargetReached() && calls < 16) {
        RenderControl control;
        complete = frame.render(control);
        calls++;
    }
    const pt_frame_noise reached = frame.noise();
    const int launches = frame.info().launches;
    bool stopped_again = false;
    {
        RenderControl control;
        stopped_again = !frame.render(control) && control.cancelled();
    }
    std::printf("target %g reached after %d more calls: %llu finished, %llu held of %llu\n", reached.target_error, calls,
                static_cast<unsigned long long>(reached.streams_finished), static_cast<unsigned long long>(reached.streams_held),
                static_cast<unsigned long long>(reached.streams_total));
    expect(!complete && reached.target_reached == 1 && reached.streams_held > 0 &&
             2 * (reached.streams_finished + reached.streams_held) >= reached.streams_total && stopped_again && frame.info().launches == launches &&
             frame.progress().samples_lost == 0,
           "a frame with a target stops when half of it is finished or held, and stays stopped without a launch");

    frame.setNoiseTarget(0.0F);
    frame.setProgressive(8, 0);
    {
        RenderControl control;
        complete = frame.render(control);
    }
    expect(complete && !frame.noiseTargetReached() && same(frame.image(), processJob(job)), "with the target cleared the frame finishes equal to processJob bit for bit");

    Camera second({0.3F, 0.1F, -3.0F}, {0.0F, 0.0F, 0.0F}, {0.0F, 1.0F, 0.0F}, 1.0F, 1.0F, 1.0F);
    const std::vector<const Camera *> cameras{&camera, &second};
    ViewBatchRender batch(scene, cameras, options);
    batch.setProgressive(8, 1);
    for(int pass = 0; pass < 2; pass++) {
        RenderControl control;
        batch.render(control);
    }
    // (the seed of view 0 is the frame's: its map is the single frame's)
    const std::vector<float> maps = batch.errorMap();
    const bool first_view = maps.size() == 2U * map.size() && std::memcmp(maps.data(), map.data(), map.size() * sizeof(float)) == 0;
    batch.setNoiseTarget(largest * 0.5F, 1E-5F, 0.5F);
    bool batch_complete = false;
    for(calls = 0; !batch_complete && !batch.noiseTargetReached() && calls < 16; calls++) {
        RenderControl control;
        batch_complete = batch.render(control);
    }
    const bool batch_reached = !batch_complete && batch.noiseTargetReached() && batch.noise().streams_held > 0;
    batch.setNoiseTarget(0.0F);
    batch.setProgressive(8, 0);
    {
        RenderControl control;
        batch_complete = batch.render(control);
    }
    const std::vector<Image<>> got = batch.images(), want = processViews(scene, cameras, options);
    expect(first_view && batch_reached && batch_complete && got.size() == 2 && same(got[0], want[0]) && same(got[1], want[1]),
           "a view batch rates view 0 as the single frame, reaches its target, and finishes equal to processViews");
    return failures == 0 ? 0 : 1;
}
