// tests/cpp/relight_scene_test.cpp -- Scene::relight: a Scene of MeshInstances whose material handlers and light sources are replaced in
// place against Scenes CONSTRUCTED with the new handlers and lights, one of MeshInstances and one made the reference's way (io::loadMesh +
// setMaterialHandler + moveObjects) from the same OBJ text: the same light samples draw for draw and the same processJob image under one
// PATHTRACE_SEED.
#include <PathTrace/camera.h>
#include <PathTrace/scene/light.h>
#include <PathTrace/scene/mesh.h>
#include <PathTrace/scene/object.h>
#include <PathTrace/scene/scene.h>
#include <PathTrace/worker.h>

#include <gmock/gmock.h>
#include <gtest/gtest.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sstream>
#include <stdexcept>
#include <string>

namespace {

    using Objects = std::vector<std::unique_ptr<Object>>;
    using Lights = std::vector<std::unique_ptr<LightSource>>;
    using Handler = std::shared_ptr<MaterialHandler>;

    // A closed, slightly bumpy UV sphere of radius 40 around (0, 50, 0) as OBJ text
    std::string sphereText(int nu, int nv) {
        std::string text;
        char line[128];
        auto vertex = [&](double x, double y, double z) {
            std::snprintf(line, sizeof(line), "v %.9g %.9g %.9g\n", static_cast<float>(x), static_cast<float>(y), static_cast<float>(z));
            text += line;
        };
        auto face = [&](int a, int b, int c) {
            std::snprintf(line, sizeof(line), "f %d %d %d\n", a + 1, b + 1, c + 1);
            text += line;
        };
        vertex(0.0, 90.0, 0.0);
        for(int j = 1; j < nv; j++) {
            for(int i = 0; i < nu; i++) {
                const double theta = 2.0 * M_PI * i / nu, phi = M_PI * j / nv;
                const double r = 40.0 * (1.0 + 0.2 * std::sin(5.0 * theta) * std::sin(7.0 * phi));
                vertex(r * std::sin(phi) * std::cos(theta), 50.0 + r * std::cos(phi), r * std::sin(phi) * std::sin(theta));
            }
        }
        vertex(0.0, 10.0, 0.0);
        const int bottom = 1 + nu * (nv - 1);
        auto ring = [&](int j, int i) { return 1 + j * nu + (i % nu); };
        for(int i = 0; i < nu; i++) {
            face(0, ring(0, i + 1), ring(0, i));
        }
        for(int j = 0; j + 2 < nv; j++) {
            for(int i = 0; i < nu; i++) {
                face(ring(j, i), ring(j, i + 1), ring(j + 1, i + 1));
                face(ring(j, i), ring(j + 1, i + 1), ring(j + 1, i));
            }
        }
        for(int i = 0; i < nu; i++) {
            face(bottom, ring(nv - 2, i), ring(nv - 2, i + 1));
        }
        return text;
    }

    Handler handlerOf(Color<float> diffuse, float ior, Color<float> emission, std::shared_ptr<BSDF> bsdf) {
        return std::make_shared<ConstantMaterialHandler>(std::make_shared<ConstantMaterial>(diffuse, ior, Spectrum(emission)), std::move(bsdf));
    }

    mat4<float> placement(float scale, float x, float y, float z) {
        return mat4<float>{vec4<float>{scale, 0.0F, 0.0F, x}, vec4<float>{0.0F, scale, 0.0F, y}, vec4<float>{0.0F, 0.0F, scale, z}, vec4<float>{0.0F, 0.0F, 0.0F, 1.0F}};
    }

    // The handlers of a look: the light quad's, the sphere's, and one per mesh instance (the third instance keeps the default handler)
    struct Look {
        Handler quad, ball, first, second;
    };

    Look lookA() {
        return Look{handlerOf(Color<float>(1.0F, 1.0F, 1.0F, 1.0F), 1.0F, Color<float>{1.0F, 1.0F, 1.0F, 1.0F}, std::make_shared<LambertianBRDF>()),
                    handlerOf(Color<float>(0.0F, 0.0F, 1.0F, 1.0F), 1.0F, Color<float>{0.0F, 0.0F, 0.0F, 0.0F}, std::make_shared<MirrorBRDF>()),
                    handlerOf(Color<float>(1.0F, 1.0F, 1.0F, 1.0F), 1.5F, Color<float>{0.0F, 0.0F, 0.0F, 0.0F}, std::make_shared<GlassBDF>()),
                    handlerOf(Color<float>(0.8F, 0.7F, 0.6F, 1.0F), 1.0F, Color<float>{0.0F, 0.0F, 0.0F, 0.0F}, std::make_shared<LambertianBRDF>())};
    }

    // the quad dimmed, the sphere glowing, the glass instance dull and the dull instance a lamp
    Look lookB() {
        return Look{handlerOf(Color<float>(1.0F, 1.0F, 1.0F, 1.0F), 1.0F, Color<float>{1.0F, 0.8F, 0.6F, 0.25F}, std::make_shared<LambertianBRDF>()),
                    handlerOf(Color<float>(0.2F, 0.2F, 0.9F, 1.0F), 1.0F, Color<float>{0.1F, 0.2F, 0.9F, 1.5F}, std::make_shared<LambertianBRDF>()),
                    handlerOf(Color<float>(0.3F, 0.9F, 0.4F, 1.0F), 1.0F, Color<float>{0.0F, 0.0F, 0.0F, 0.0F}, std::make_shared<LambertianBRDF>()),
                    handlerOf(Color<float>(1.0F, 1.0F, 1.0F, 1.0F), 1.0F, Color<float>{1.0F, 0.9F, 0.8F, 2.0F}, std::make_shared<LambertianBRDF>())};
    }

    Lights lightsA() {
        Lights lights;
        lights.emplace_back(std::make_unique<PointLightSource>(vec3<float>{-0.6F, 0.7F, -0.6F}, Spectrum(Color<float>{0.5F, 0.5F, 0.4F, 1.0F})));
        return lights;
    }
    Lights lightsB() {
        Lights lights;
        lights.emplace_back(std::make_unique<PointLightSource>(vec3<float>{0.5F, 0.6F, -0.7F}, Spectrum(Color<float>{0.2F, 0.5F, 0.9F, 1.0F})));
        lights.emplace_back(std::make_unique<PointLightSource>(vec3<float>{-0.5F, -0.6F, -0.2F}, Spectrum(Color<float>{0.9F, 0.3F, 0.1F, 1.0F})));
        return lights;
    }

    void addBase(Objects &objects, const Look &look) {
        auto walls = makeBox(vec3<float>{-1.0F, -1.0F, -1.0F}, vec3<float>{1.0F, 1.0F, 1.0F});
        moveObjects(objects, walls);
        auto lamp = makePlane(vec3<float>{-0.25F, 0.99F, -0.25F}, vec3<float>{0.25F, 0.99F, 0.25F});
        for(auto &t : lamp) {
            t.setMaterialHandler(look.quad);
        }
        moveObjects(objects, lamp);
        auto ball = std::make_unique<Sphere>(vec3<float>{0.55F, -0.7F, -0.3F}, 0.3F);
        ball->setMaterialHandler(look.ball);
        objects.emplace_back(std::move(ball));
    }

    struct Placed {
        bool cull_backface, smooth;
        Handler handler;
        mat4<float> at;
    };

    std::vector<Placed> placed(const Look &look) {
        return {Placed{false, true, look.first, placement(0.01F, -0.3F, -0.8F, 0.2F)}, Placed{true, false, look.second, placement(0.004F, 0.4F, 0.2F, -0.2F)},
                Placed{true, true, nullptr, placement(0.005F, 0.3F, -0.9F, 0.5F)}};
    }

    std::unique_ptr<Scene> meshScene(const std::string &text, const Look &look, Lights &&lights) {
        Objects objects;
        addBase(objects, look);
        std::istringstream stream(text);
        auto data = std::make_shared<const io::MeshData>(io::loadMeshData(stream));
        std::vector<MeshInstance> instances;
        for(const Placed &p : placed(look)) {
            instances.push_back(MeshInstance{data, p.at, p.cull_backface, p.smooth, p.handler});
        }
        return std::make_unique<Scene>(std::move(objects), std::move(lights), std::move(instances));
    }

    std::unique_ptr<Scene> flatScene(const std::string &text, const Look &look, Lights &&lights) {
        Objects objects;
        addBase(objects, look);
        for(const Placed &p : placed(look)) {
            std::istringstream stream(text);
            auto triangles = io::loadMesh(stream, p.at, p.cull_backface, p.smooth);
            if(p.handler != nullptr) {
                for(auto &t : triangles) {
                    t.setMaterialHandler(p.handler);
                }
            }
            moveObjects(objects, triangles);
        }
        return std::make_unique<Scene>(std::move(objects), std::move(lights));
    }

    bool sameBits(const Image<> &a, const Image<> &b) {
        return a.getWidth() == b.getWidth() && a.getHeight() == b.getHeight() && std::memcmp(a.data(), b.data(), a.size() * sizeof(Color<float>)) == 0;
    }

    bool sameVector(const vec3<float> &a, const vec3<float> &b) {
        return std::memcmp(&a, &b, sizeof(a)) == 0;
    }

    Image<> render(const Scene &scene) {
        Camera camera({0.0F, 0.0F, -3.0F}, {0.0F, 0.0F, 0.0F}, {0.0F, 1.0F, 0.0F}, 1.0F, 1.0F, -1.0F);
        RenderOptions options{32, 32, 4, 8, 1E-3F};
        setenv("PATHTRACE_SEED", "77", 1);
        auto image = processJob(FrameRenderJob{camera, scene, options});
        unsetenv("PATHTRACE_SEED");
        return image;
    }

    // the number of light samples of 200 positions that differ between two scenes, draw for draw, and the number compared
    std::pair<int, int> differingLightSamples(const Scene &a_scene, const Scene &b_scene) {
        RandomEngine ra(1234), rb(1234);
        int differing = 0, samples = 0;
        for(int k = 0; k < 200; k++) {
            const vec3<float> pos{0.01F * static_cast<float>(k % 50) - 0.2F, -0.5F + 0.005F * static_cast<float>(k), 0.1F};
            const auto a = a_scene.sampleLights(pos, vec3<float>{0.0F, 1.0F, 0.0F}, ra);
            const auto b = b_scene.sampleLights(pos, vec3<float>{0.0F, 1.0F, 0.0F}, rb);
            differing += a.size() != b.size() || ra.state() != rb.state();
            for(size_t i = 0; i < a.size() && i < b.size(); i++) {
                const auto ca = std::get<1>(a[i]).getColor(), cb = std::get<1>(b[i]).getColor();
                differing += !sameVector(std::get<0>(a[i]), std::get<0>(b[i])) || std::memcmp(&ca, &cb, sizeof(ca)) != 0 ||
                             std::memcmp(&std::get<2>(a[i]), &std::get<2>(b[i]), sizeof(float)) != 0;
                samples++;
            }
        }
        return {differing, samples};
    }

    std::vector<std::pair<Handler, Handler>> replacements(const Look &from, const Look &to) {
        return {{from.quad, to.quad}, {from.ball, to.ball}, {from.first, to.first}, {from.second, to.second}};
    }

} // namespace

TEST(RelightScene, HandlersReplacedEqualASceneConstructedWithThem) {
    for(const auto &[nu, nv] : {std::pair<int, int>{24, 16}, std::pair<int, int>{48, 24}}) { // the host builder; the device builder
        const std::string text = sphereText(nu, nv);
        const Look a = lookA(), b = lookB();
        auto relit = meshScene(text, a, lightsA());
        const auto first = render(*relit); // (the workspace is sized for look A)
        relit->relight(replacements(a, b));
        auto fresh = meshScene(text, b, lightsA());
        auto flat = flatScene(text, b, lightsA());
        const auto [differing, samples] = differingLightSamples(*relit, *flat);
        EXPECT_THAT(differing, testing::Eq(0));
        EXPECT_THAT(samples > 400, testing::Eq(true));
        const auto image = render(*relit);
        EXPECT_THAT(sameBits(image, render(*fresh)), testing::Eq(true));
        EXPECT_THAT(sameBits(image, render(*flat)), testing::Eq(true));
        EXPECT_THAT(sameBits(image, first), testing::Eq(false));
        // ... and back: the first frame's bits
        relit->relight(replacements(b, a));
        EXPECT_THAT(sameBits(render(*relit), first), testing::Eq(true));
    }
}

TEST(RelightScene, LightsReplacedEqualASceneConstructedWithThem) {
    const std::string text = sphereText(24, 16);
    const Look a = lookA();
    auto relit = meshScene(text, a, lightsA());
    relit->relight(lightsB());
    auto flat = flatScene(text, a, lightsB());
    const auto [differing, samples] = differingLightSamples(*relit, *flat);
    EXPECT_THAT(differing, testing::Eq(0));
    EXPECT_THAT(samples > 400, testing::Eq(true));
    EXPECT_THAT(sameBits(render(*relit), render(*flat)), testing::Eq(true));
    // handlers after lights, and a pose in between: the look stays
    const Look b = lookB();
    relit->relight(replacements(a, b));
    auto matrices = std::vector<mat4<float>>{};
    for(const Placed &p : placed(b)) {
        matrices.push_back(p.at);
    }
    relit->pose(matrices);
    EXPECT_THAT(sameBits(render(*relit), render(*flatScene(text, b, lightsB()))), testing::Eq(true));
}

TEST(RelightScene, ThrowsWhatPoseThrows) {
    const std::string text = sphereText(24, 16);
    const Look a = lookA(), b = lookB();
    auto relit = meshScene(text, a, lightsA());
    auto flat = flatScene(text, a, lightsA());
    const auto before = render(*relit);
    int thrown = 0;
    try {
        flat->relight(replacements(a, b)); // a Scene without mesh instances
    } catch(const std::invalid_argument &) {
        thrown++;
    }
    try {
        flat->relight(lightsB());
    } catch(const std::invalid_argument &) {
        thrown++;
    }
    try {
        relit->relight(std::vector<std::pair<Handler, Handler>>{{b.quad, a.quad}}); // a handler the Scene does not use
    } catch(const std::invalid_argument &) {
        thrown++;
    }
    try {
        relit->relight(std::vector<std::pair<Handler, Handler>>{{a.quad, nullptr}});
    } catch(const std::invalid_argument &) {
        thrown++;
    }
    EXPECT_THAT(thrown, testing::Eq(4));
    EXPECT_THAT(sameBits(render(*relit), before), testing::Eq(true));
}

TEST(RelightScene, AHandlerAlreadyInUseTakesTheSlotsOfWhatItReplaces) {
    // the issue's own workflow: switch a mesh to the lamp's handler, then dim the lamp -- the mesh must dim with it
    const std::string text = sphereText(24, 16);
    const Look a = lookA(), b = lookB();
    auto relit = meshScene(text, a, lightsA());
    (void)render(*relit);
    relit->relight(std::vector<std::pair<Handler, Handler>>{{a.first, a.quad}}); // instance 0 glows like the quad: a.quad holds two slots
    Look both = a;
    both.first = a.quad;
    {
        auto flat = flatScene(text, both, lightsA());
        EXPECT_THAT(differingLightSamples(*relit, *flat).first, testing::Eq(0));
        EXPECT_THAT(sameBits(render(*relit), render(*flat)), testing::Eq(true));
    }
    relit->relight(std::vector<std::pair<Handler, Handler>>{{a.quad, b.quad}}); // ... and both dim
    both.quad = both.first = b.quad;
    {
        auto flat = flatScene(text, both, lightsA());
        const auto [differing, samples] = differingLightSamples(*relit, *flat);
        EXPECT_THAT(differing, testing::Eq(0));
        EXPECT_THAT(samples > 400, testing::Eq(true));
        EXPECT_THAT(sameBits(render(*relit), render(*flat)), testing::Eq(true));
    }
    // a chain inside one call through a handler in use: second -> ball's handler, ball's handler -> a lamp
    relit->relight(std::vector<std::pair<Handler, Handler>>{{a.second, a.ball}, {a.ball, b.second}});
    both.second = both.ball = b.second;
    {
        auto flat = flatScene(text, both, lightsA());
        EXPECT_THAT(differingLightSamples(*relit, *flat).first, testing::Eq(0));
        EXPECT_THAT(sameBits(render(*relit), render(*flat)), testing::Eq(true));
        // a pose rebuilds from the kept description: the look stays
        auto matrices = std::vector<mat4<float>>{};
        for(const Placed &p : placed(both)) {
            matrices.push_back(p.at);
        }
        relit->pose(matrices);
        EXPECT_THAT(sameBits(render(*relit), render(*flat)), testing::Eq(true));
    }
}

int main(int argc, char **argv) {
    testing::InitGoogleTest(&argc, argv);
    return RUN_ALL_TESTS();
}
