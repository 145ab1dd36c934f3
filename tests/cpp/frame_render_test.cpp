// tests/cpp/frame_render_test.cpp -- FrameRender (include/PathTrace/frame_render.h) on the GPU: a frame rendered in slices -- a cancel
// from the progress callback, then budgeted calls -- equals processJob's frame with the same $PATHTRACE_SEED bit for bit.  Prints one line
// per check; exit status 0 = every check passed.
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

} // namespace

int main() {
    setenv("PATHTRACE_SEED", "8642", 1); // the sliced and the full render draw the same samples
    const int side = 2048;               // more streams than the device has slots: a stop finds most pixels half-way
    Camera camera({0.0F, 0.0F, -3.0F}, {0.0F, 0.0F, 0.0F}, {0.0F, 1.0F, 0.0F}, 1.0F, 1.0F, 1.0F);
    Scene scene = boxScene();
    RenderOptions options{side, side, 32, 32, 1E-3F};
    FrameRenderJob job{camera, scene, options};
    const Image<> full = processJob(job);

    FrameRender frame(job);
    bool complete = false;
    {
        RenderControl control;
        int reports = 0;
        complete = frame.render(control, [&](int, int) {
            if(++reports == 1) {
                control.cancel();
            }
        });
        expect(!complete && control.cancelled() && control.finishedTiles().size() < control.tileCount(), "a cancel from the progress callback stops the frame");
        const pt_frame_info info = frame.info();
        expect(info.streams_parked > 0 && info.samples_carried > 0, "the stop parks half-finished pixels");
        std::printf("after the cancel: %llu finished, %llu parked (%llu samples), %llu untouched\n", static_cast<unsigned long long>(info.streams_finished),
                    static_cast<unsigned long long>(info.streams_parked), static_cast<unsigned long long>(info.samples_carried),
                    static_cast<unsigned long long>(info.streams_untouched));
    }
    int calls = 1;
    while(!complete && calls < 200) {
        RenderControl control; // (a fresh control per call)
        control.setBudget(std::chrono::milliseconds(60));
        complete = frame.render(control);
        calls++;
    }
    std::printf("complete after %d calls\n", calls);
    expect(complete && frame.complete(), "budgeted calls complete the frame");
    expect(frame.info().streams_finished == static_cast<std::uint64_t>(side) * side, "every stream finished");
    expect(std::memcmp(frame.image().data(), full.data(), full.size() * sizeof(Color<float>)) == 0, "the frame equals processJob's bit for bit");
    return failures == 0 ? 0 : 1;
}
