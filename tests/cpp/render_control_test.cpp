// tests/cpp/render_control_test.cpp -- processJob under a RenderControl (include/PathTrace/render_control.h) on the GPU: a cancel from the
// progress callback stops the render early, the tiles it reports as finished are exactly those of a full render, and a control that is
// never cancelled renders the whole frame bit for bit.  Prints one line per check; exit status 0 = every check passed.
#include <PathTrace/camera.h>
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

    bool sameTile(const Image<> &a, const Image<> &b, const RenderControl::Tile &t) {
        for(int y = t.offset_y; y < t.offset_y + t.height; y++) {
            for(int x = t.offset_x; x < t.offset_x + t.width; x++) {
                const std::size_t at = static_cast<std::size_t>(y) * static_cast<std::size_t>(a.getWidth()) + static_cast<std::size_t>(x);
                if(std::memcmp(a.data() + at, b.data() + at, sizeof(Color<float>)) != 0) {
                    return false;
                }
            }
        }
        return true;
    }

} // namespace

int main() {
    setenv("PATHTRACE_SEED", "4321", 1); // the controlled and the full render draw the same samples
    const int side = 2048;               // 4 M pixels: many more streams than the device has slots, so tiles finish one after another
    Camera camera({0.0F, 0.0F, -3.0F}, {0.0F, 0.0F, 0.0F}, {0.0F, 1.0F, 0.0F}, 1.0F, 1.0F, 1.0F);
    Scene scene = boxScene();
    RenderOptions options{side, side, 16, 16, 1E-3F};
    FrameRenderJob job{camera, scene, options};
    const Image<> full = processJob(job);

    RenderControl control;
    int reports = 0;
    const Image<> part = processJob(job, control, [&](int, int) {
        if(++reports == 1) {
            control.cancel();
        }
    });
    const std::vector<RenderControl::Tile> &done = control.finishedTiles();
    expect(control.cancelled(), "a cancel from the progress callback stops the render");
    expect(!done.empty() && done.size() < control.tileCount(), "some tiles finished, not all");
    bool exact = true;
    for(const RenderControl::Tile &t : done) {
        exact = exact && sameTile(part, full, t);
    }
    expect(exact, "every finished tile equals the full render");
    expect(control.streamsFinished() + control.streamsAbandoned() + control.streamsUnclaimed() == static_cast<std::uint64_t>(side) * side,
           "every stream is finished, abandoned or unclaimed");
    std::printf("tiles finished %zu of %zu; streams finished %llu, abandoned %llu, unclaimed %llu; drain %.3f ms\n", done.size(), control.tileCount(),
                static_cast<unsigned long long>(control.streamsFinished()), static_cast<unsigned long long>(control.streamsAbandoned()),
                static_cast<unsigned long long>(control.streamsUnclaimed()), control.drainMilliseconds());

    RenderControl calm;
    calm.setBudget(std::chrono::seconds(600));
    const Image<> whole = processJob(job, calm);
    expect(!calm.cancelled() && calm.finishedTiles().size() == calm.tileCount(), "an uncancelled control finishes every tile");
    expect(std::memcmp(whole.data(), full.data(), full.size() * sizeof(Color<float>)) == 0, "... and renders the frame bit for bit");
    expect(calm.streamsAbandoned() == 0 && calm.streamsUnclaimed() == 0 && calm.drainMilliseconds() == 0.0, "... with no stream dropped");
    return failures == 0 ? 0 : 1;
}
