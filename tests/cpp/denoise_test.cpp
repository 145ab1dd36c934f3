// tests/cpp/denoise_test.cpp -- RenderOptions::allow_bias (include/PathTrace/worker.h, denoise.h, view_batch.h): processJob with the flag
// equals denoise(processJob without it) bit for bit, processViews with the flag equals processJob with the flag per view, processItem
// ignores it, and denoise refuses a frame of the wrong size.  With an argument, the unbiased and the biased frame are written to that file
// (raw float32, one after the other) for tests/test_gpu_denoise.py.  Prints one line per check; exit status 0 = every check passed.
#include <PathTrace/camera.h>
#include <PathTrace/denoise.h>
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

    // scenes.box_scene(): the reference's Box benchmark scene
    Scene boxScene() {
        Objects objects;
        Lights lights;
        auto walls = makeBox(vec3<float>{-1.0F, -1.0F, -1.0F}, vec3<float>{1.0F, 1.0F, 1.0F});
        moveObjects(objects, walls);
        auto lamp = makePlane(vec3<float>{-0.25F, 1.0F - 0.01F, -0.25F}, vec3<float>{0.25F, 1.0F - 0.01F, 0.25F});
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

int main(int argc, char **argv) {
    setenv("PATHTRACE_SEED", "4242", 1);
    Scene scene = boxScene();
    Camera pinhole({0.0F, 0.0F, -3.0F}, {0.0F, 0.0F, 0.0F}, {0.0F, 1.0F, 0.0F}, 1.0F, 1.0F, -1.0F);
    Camera lens({-0.2F, 0.0F, -3.0F}, {0.0F, 0.0F, 0.0F}, {0.0F, 1.0F, 0.0F}, 1.0F, 1.0F, -1.0F, 0.06F, 0.06F, std::make_unique<CircularApertureSampler>(), 3.2F);
    RenderOptions plain{48, 40, 8, 8, 1E-3F};
    RenderOptions biased = plain;
    biased.allow_bias = true;

    const Image<> noisy = processJob(FrameRenderJob{pinhole, scene, plain});
    const Image<> clean = processJob(FrameRenderJob{pinhole, scene, biased});
    const Image<> by_hand = denoise(noisy, scene, pinhole, plain);
    expect(same(clean, by_hand), "processJob with allow_bias equals denoise(processJob without it) bit for bit");
    expect(!same(clean, noisy), "allow_bias changes the frame");
    expect(same(processJob(FrameRenderJob{pinhole, scene, plain}), noisy), "without allow_bias the frame is the same as before");
    expect(same(denoise(noisy, scene, pinhole, biased), by_hand), "denoise does not depend on the flag itself");

    std::vector<std::uint64_t> seeds;
    const std::vector<Image<>> views = processViews(scene, {&pinhole, &lens}, biased, [](int, int) {}, 0, &seeds);
    bool views_equal = views.size() == 2;
    for(size_t v = 0; v < views.size() && views_equal; v++) {
        setenv("PATHTRACE_SEED", std::to_string(seeds[v]).c_str(), 1);
        views_equal = same(views[v], processJob(FrameRenderJob{v == 0 ? pinhole : lens, scene, biased}));
    }
    setenv("PATHTRACE_SEED", "4242", 1);
    expect(views_equal, "processViews with allow_bias equals processJob with allow_bias per view");

    const FrameRenderJob plain_job{pinhole, scene, plain}, biased_job{pinhole, scene, biased};
    RandomEngine a(77), b(77);
    const Image<> tile_plain = processItem(WorkItem(&plain_job, 8, 4, 16, 12), a);
    const Image<> tile_biased = processItem(WorkItem(&biased_job, 8, 4, 16, 12), b);
    expect(same(tile_plain, tile_biased), "processItem ignores allow_bias");

    bool refused = false;
    try {
        denoise(Image<>(10, 10), scene, pinhole, plain);
    }
    catch(const std::invalid_argument &) {
        refused = true;
    }
    expect(refused, "denoise refuses a frame of another size");

    if(argc > 1) {
        std::FILE *f = std::fopen(argv[1], "wb");
        const bool written = f != nullptr && std::fwrite(noisy.data(), sizeof(Color<float>), noisy.size(), f) == noisy.size() &&
                             std::fwrite(clean.data(), sizeof(Color<float>), clean.size(), f) == clean.size();
        expect(f != nullptr && std::fclose(f) == 0 && written, "frames written");
    }
    return failures == 0 ? 0 : 1;
}
