// tests/cpp/motion_shapes_test.cpp -- TemporalDenoiseParams::follow_motion across Scene::deform (include/PathTrace/temporal_denoise.h,
// include/pt_motion_shapes.h): a Scene with one mesh instance, a card of 8 faces, is posed and deformed between the pushes of two
// TemporalDenoisers, one that follows the motion -- it marks the scene after every push and reprojects per vertex at the next -- and one
// that does not.  The 3 noisy frames, the 3 outputs with follow_motion and the 3 without are written to the file named by the argument
// (raw float32) for tests/test_gpu_motion_shapes.py, which repeats the first route as a loop over the C ABI through the Python binding.
// Prints one line per check; exit status 0 = every check passed.
#include <PathTrace/camera.h>
#include <PathTrace/denoise.h>
#include <PathTrace/scene/light.h>
#include <PathTrace/scene/mesh.h>
#include <PathTrace/scene/object.h>
#include <PathTrace/scene/scene.h>
#include <PathTrace/temporal_denoise.h>
#include <PathTrace/worker.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

namespace {

    using Objects = std::vector<std::unique_ptr<Object>>;
    using Lights = std::vector<std::unique_ptr<LightSource>>;

    int failures = 0;

    void expect(bool ok, const char *what) {
        std::printf("%s %s\n", ok ? "[ OK ]" : "[FAIL]", what);
        failures += ok ? 0 : 1;
    }

    bool same(const Image<> &a, const Image<> &b) {
        return a.getWidth() == b.getWidth() && a.getHeight() == b.getHeight() && std::memcmp(a.data(), b.data(), a.size() * sizeof(Color<float>)) == 0;
    }

    mat4<float> placement(float x, float y, float z) {
        return mat4<float>{vec4<float>{1.0F, 0.0F, 0.0F, x}, vec4<float>{0.0F, 1.0F, 0.0F, y}, vec4<float>{0.0F, 0.0F, 1.0F, z}, vec4<float>{0.0F, 0.0F, 0.0F, 1.0F}};
    }

    // the card's 3 x 3 vertices, its middle column pushed toward the camera by `bow` and its top row sideways by `lean`
    std::vector<vec3<float>> shape(float bow, float lean) {
        std::vector<vec3<float>> v;
        for(int j = 0; j < 3; j++) {
            for(int i = 0; i < 3; i++) {
                v.push_back(vec3<float>{-0.25F + 0.3125F * static_cast<float>(i) + (j == 2 ? lean : 0.0F), -0.25F + 0.25F * static_cast<float>(j), i == 1 ? -bow : 0.0F});
            }
        }
        return v;
    }

} // namespace

int main(int argc, char **argv) {
    setenv("PATHTRACE_SEED", "4242", 1);
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
    std::ostringstream obj;
    for(const vec3<float> &v : shape(0.0F, 0.0F)) {
        obj << "v " << v.x() << " " << v.y() << " " << v.z() << "\n";
    }
    for(int j = 0; j < 2; j++) {
        for(int i = 0; i < 2; i++) {
            const int a = 3 * j + i + 1, b = a + 1, c = a + 4, d = a + 3;
            obj << "f " << a << " " << c << " " << b << "\nf " << a << " " << d << " " << c << "\n";
        }
    }
    std::istringstream text(obj.str());
    auto mesh = std::make_shared<const io::MeshData>(io::loadMeshData(text));
    std::vector<MeshInstance> instances(1);
    instances[0].mesh = mesh;
    instances[0].transformation = placement(-0.125F, 0.0F, 0.5F);
    instances[0].cull_backface = false;
    instances[0].smooth = false;
    Scene scene(std::move(objects), std::move(lights), std::move(instances));
    Camera camera({0.0F, 0.0F, -0.875F}, {0.0F, 0.0F, 1.0F}, {0.0F, 1.0F, 0.0F}, 0.625F, 1.0F, -1.25F);
    RenderOptions options{40, 32, 8, 8, 1E-3F};

    TemporalDenoiseParams follow;
    follow.follow_motion = true;
    TemporalDenoiser followed(scene, options, follow), plain(scene, options);
    std::vector<Image<>> frames, with_motion, without, spatial;
    for(size_t v = 0; v < 3; v++) {
        if(v == 1) { // a new shape under a new matrix
            scene.pose(std::vector<mat4<float>>{placement(0.0F, 0.0625F, 0.5F)});
            scene.deform(mesh, shape(0.125F, 0.0F));
        }
        if(v == 2) { // ... and a new shape alone
            scene.deform(mesh, shape(0.1875F, 0.0625F));
        }
        frames.push_back(processJob(FrameRenderJob{camera, scene, options}));
        with_motion.push_back(followed.push(frames[v], camera));
        without.push_back(plain.push(frames[v], camera));
        spatial.push_back(denoise(frames[v], scene, camera, options));
    }
    expect(same(with_motion[0], without[0]) && same(with_motion[0], spatial[0]), "the first push has no previous frame");
    expect(!same(with_motion[1], without[1]) && !same(with_motion[2], without[2]), "following the deformation changes the later pushes");
    scene.unmarkMotion();
    expect(same(followed.push(frames[2], camera), spatial[2]), "a push after Scene::unmarkMotion has no previous frame");
    scene.markMotion();
    scene.unmarkMotion();
    scene.unmarkMotion(); // (nothing to forget)
    bool refused = false;
    try {
        Objects none;
        Lights no_lights;
        auto box = makeBox(vec3<float>{-1.0F, -1.0F, -1.0F}, vec3<float>{1.0F, 1.0F, 1.0F});
        moveObjects(none, box);
        Scene bare(std::move(none), std::move(no_lights));
        bare.markMotion();
    }
    catch(const std::invalid_argument &) {
        refused = true;
    }
    expect(refused, "Scene::markMotion on a Scene without mesh instances throws std::invalid_argument");

    if(argc > 1) {
        std::FILE *f = std::fopen(argv[1], "wb");
        bool written = f != nullptr;
        for(const std::vector<Image<>> *set : {static_cast<const std::vector<Image<>> *>(&frames), static_cast<const std::vector<Image<>> *>(&with_motion),
                                               static_cast<const std::vector<Image<>> *>(&without)}) {
            for(const Image<> &im : *set) {
                written = written && std::fwrite(im.data(), sizeof(Color<float>), im.size(), f) == im.size();
            }
        }
        expect(f != nullptr && std::fclose(f) == 0 && written, "frames written");
    }
    return failures == 0 ? 0 : 1;
}
