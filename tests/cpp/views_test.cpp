// tests/cpp/views_test.cpp -- processViews (include/PathTrace/view_batch.h): four cameras of one scene rendered in one call; each returned
// Image<> equals processJob for that camera with $PATHTRACE_SEED set to the view's seed, bit for bit; bad camera lists are refused.  Prints
// one line per check; exit status 0 = every check passed.
#include <PathTrace/camera.h>
#include <PathTrace/scene/light.h>
#include <PathTrace/scene/mesh.h>
#include <PathTrace/scene/object.h>
#include <PathTrace/scene/scene.h>
#include <PathTrace/view_batch.h>
#include <PathTrace/worker.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
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

    template<typename F>
    bool throwsInvalid(F f) {
        try {
            f();
        }
        catch(const std::invalid_argument &) {
            return true;
        }
        catch(...) {
            return false;
        }
        return false;
    }

} // namespace

int main() {
    RenderOptions options{40, 28, 2, 12, 1E-3F};
    setenv("PATHTRACE_SEED", "4242", 1);
    Scene scene = boxScene();
    Camera pinhole({0.0F, 0.0F, -3.0F}, {0.0F, 0.0F, 0.0F}, {0.0F, 1.0F, 0.0F}, 1.0F, 1.0F, -1.0F);
    Camera moved({0.3F, 0.1F, -2.8F}, {0.0F, 0.0F, 0.0F}, {0.0F, 1.0F, 0.0F}, 1.0F, 1.0F, -1.0F);
    Camera lens({-0.2F, 0.0F, -3.0F}, {0.0F, 0.0F, 0.0F}, {0.0F, 1.0F, 0.0F}, 1.0F, 1.0F, -1.0F, 0.06F, 0.06F, std::make_unique<CircularApertureSampler>(), 3.2F);
    Camera hexagon({0.1F, -0.1F, -3.1F}, {0.0F, 0.0F, 0.0F}, {0.0F, 1.0F, 0.0F}, 1.0F, 1.0F, -1.0F, 0.05F, 0.05F, std::make_unique<HexagonalApertureSampler>(0.4F),
                   3.0F);
    const std::vector<const Camera *> cameras{&pinhole, &moved, &lens, &hexagon};
    std::vector<std::uint64_t> seeds;
    int reports = 0, last = 0;
    bool increasing = true;
    const std::vector<Image<>> views = processViews(scene, cameras, options, [&](int completed, int) {
        increasing = increasing && completed == last + 1;
        last = completed;
        reports++;
    }, 0, &seeds);
    expect(views.size() == 4 && seeds.size() == 4 && seeds[0] == 4242 && seeds[3] == 4245, "four views, seeded from $PATHTRACE_SEED on");
    expect(increasing && reports > 0 && reports % 4 == 0, "progress counts the tiles of every view in order");
    bool same = true;
    for(size_t v = 0; v < views.size(); v++) {
        setenv("PATHTRACE_SEED", std::to_string(seeds[v]).c_str(), 1);
        const FrameRenderJob job{*cameras[v], scene, options};
        const Image<> single = processJob(job);
        const bool equal = views[v].getWidth() == single.getWidth() && views[v].getHeight() == single.getHeight() &&
                           std::memcmp(views[v].data(), single.data(), single.size() * sizeof(Color<float>)) == 0;
        std::printf("view %zu (seed %llu): %s\n", v, static_cast<unsigned long long>(seeds[v]), equal ? "equal" : "DIFFERENT");
        same = same && equal;
    }
    expect(same, "every view equals processJob with its camera and seed bit for bit");
    expect(std::memcmp(views[0].data(), views[1].data(), views[0].size() * sizeof(Color<float>)) != 0, "the views differ");
    expect(throwsInvalid([&] { processViews(scene, {}, options); }), "an empty camera list is refused");
    expect(throwsInvalid([&] { processViews(scene, {&pinhole, nullptr}, options); }), "a null camera is refused");
    return failures == 0 ? 0 : 1;
}
