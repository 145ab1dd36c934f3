// tests/cpp/temporal_test.cpp -- TemporalDenoiser and denoiseSequence (include/PathTrace/temporal_denoise.h): the first push and the first
// after reset() equal denoise() bit for bit, denoiseSequence equals the pushes, a later push differs from the spatial filter, and a frame of
// the wrong size or bad parameters are refused.  With an argument, the 3 noisy frames of a pan and their 3 temporal outputs are written to
// that file (raw float32) for tests/test_gpu_temporal.py.  Prints one line per check; exit status 0 = every check passed.
#include <PathTrace/camera.h>
#include <PathTrace/denoise.h>
#include <PathTrace/scene/light.h>
#include <PathTrace/scene/mesh.h>
#include <PathTrace/scene/object.h>
#include <PathTrace/scene/scene.h>
#include <PathTrace/temporal_denoise.h>
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
    Camera c0({0.0F, 0.0F, -3.0F}, {0.0F, 0.0F, 0.0F}, {0.0F, 1.0F, 0.0F}, 1.0F, 1.0F, -1.0F);
    Camera c1({0.02F, 0.0F, -3.0F}, {0.02F, 0.0F, 0.0F}, {0.0F, 1.0F, 0.0F}, 1.0F, 1.0F, -1.0F);
    Camera c2({0.04F, 0.01F, -3.0F}, {0.04F, 0.01F, 0.0F}, {0.0F, 1.0F, 0.0F}, 1.0F, 1.0F, -1.0F);
    const std::vector<const Camera *> cams{&c0, &c1, &c2};
    RenderOptions plain{48, 40, 8, 8, 1E-3F};
    const std::vector<Image<>> frames = processViews(scene, cams, plain, [](int, int) {});

    TemporalDenoiser denoiser(scene, plain);
    std::vector<Image<>> pushed;
    for(size_t v = 0; v < frames.size(); v++) {
        pushed.push_back(denoiser.push(frames[v], *cams[v]));
    }
    expect(same(pushed[0], denoise(frames[0], scene, c0, plain)), "the first push equals denoise() bit for bit");
    expect(!same(pushed[2], denoise(frames[2], scene, c2, plain)), "a later push is not the spatial filter");
    denoiser.reset();
    expect(same(denoiser.push(frames[1], c1), denoise(frames[1], scene, c1, plain)), "the first push after reset() equals denoise() bit for bit");
    const std::vector<Image<>> seq = denoiseSequence(frames, scene, cams, plain);
    bool seq_same = seq.size() == pushed.size();
    for(size_t v = 0; v < seq.size() && seq_same; v++) {
        seq_same = same(seq[v], pushed[v]);
    }
    expect(seq_same, "denoiseSequence equals the pushes");

    bool refused = false;
    try {
        denoiser.push(Image<>(10, 10), c0);
    }
    catch(const std::invalid_argument &) {
        refused = true;
    }
    expect(refused, "push refuses a frame of another size");
    refused = false;
    try {
        TemporalDenoiseParams bad;
        bad.alpha_color = 0.0F;
        TemporalDenoiser never(scene, plain, bad);
    }
    catch(const std::invalid_argument &) {
        refused = true;
    }
    expect(refused, "TemporalDenoiser refuses an alpha outside (0, 1]");

    if(argc > 1) {
        std::FILE *f = std::fopen(argv[1], "wb");
        bool written = f != nullptr;
        for(const std::vector<Image<>> *set : {&frames, static_cast<const std::vector<Image<>> *>(&pushed)}) {
            for(const Image<> &im : *set) {
                written = written && std::fwrite(im.data(), sizeof(Color<float>), im.size(), f) == im.size();
            }
        }
        expect(f != nullptr && std::fclose(f) == 0 && written, "frames written");
    }
    return failures == 0 ? 0 : 1;
}
