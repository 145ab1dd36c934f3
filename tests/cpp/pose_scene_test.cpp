// tests/cpp/pose_scene_test.cpp -- Scene::pose: a Scene of MeshInstances moved to new matrices against Scenes CONSTRUCTED at those matrices,
// one of MeshInstances and one made the reference's way (io::loadMesh + setMaterialHandler + moveObjects) from the same OBJ text: the same
// processJob image under one PATHTRACE_SEED, Triangles at the new positions behind the hits, the same light samples draw for draw after an
// emissive instance moved.
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

    // A closed, slightly bumpy UV sphere of radius 40 around (0, 50, 0) as OBJ text, with a repeated index every few faces
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
                if(i % 7 == 3) {
                    face(ring(j, i), ring(j, i), ring(j + 1, i));
                }
            }
        }
        for(int i = 0; i < nu; i++) {
            face(bottom, ring(nv - 2, i), ring(nv - 2, i + 1));
        }
        return text;
    }

    std::shared_ptr<MaterialHandler> handlerOf(Color<float> diffuse, float ior, Color<float> emission, std::shared_ptr<BSDF> bsdf) {
        return std::make_shared<ConstantMaterialHandler>(std::make_shared<ConstantMaterial>(diffuse, ior, Spectrum(emission)), std::move(bsdf));
    }

    mat4<float> placement(float scale, float x, float y, float z) {
        return mat4<float>{vec4<float>{scale, 0.0F, 0.0F, x}, vec4<float>{0.0F, scale, 0.0F, y}, vec4<float>{0.0F, 0.0F, scale, z}, vec4<float>{0.0F, 0.0F, 0.0F, 1.0F}};
    }

    struct Placed {
        bool cull_backface, smooth;
        std::shared_ptr<MaterialHandler> handler;
    };

    void addBase(Objects &objects, Lights &lights) {
        auto walls = makeBox(vec3<float>{-1.0F, -1.0F, -1.0F}, vec3<float>{1.0F, 1.0F, 1.0F});
        moveObjects(objects, walls);
        auto lamp = makePlane(vec3<float>{-0.25F, 0.99F, -0.25F}, vec3<float>{0.25F, 0.99F, 0.25F});
        auto glow = handlerOf(Color<float>(1.0F, 1.0F, 1.0F, 1.0F), 1.0F, Color<float>{1.0F, 1.0F, 1.0F, 1.0F}, std::make_shared<LambertianBRDF>());
        for(auto &t : lamp) {
            t.setMaterialHandler(glow);
        }
        moveObjects(objects, lamp);
        objects.emplace_back(std::make_unique<Sphere>(vec3<float>{0.55F, -0.7F, -0.3F}, 0.3F));
        lights.emplace_back(std::make_unique<PointLightSource>(vec3<float>{-0.6F, 0.7F, -0.6F}, Spectrum(Color<float>{0.5F, 0.5F, 0.4F, 1.0F})));
    }

    std::vector<Placed> placed() {
        auto glass = handlerOf(Color<float>(1.0F, 1.0F, 1.0F, 1.0F), 1.5F, Color<float>{0.0F, 0.0F, 0.0F, 0.0F}, std::make_shared<GlassBDF>());
        auto lamp = handlerOf(Color<float>(1.0F, 1.0F, 1.0F, 1.0F), 1.0F, Color<float>{1.0F, 0.9F, 0.8F, 2.0F}, std::make_shared<LambertianBRDF>());
        return {Placed{false, true, glass}, Placed{true, false, lamp}, Placed{true, true, nullptr}};
    }

    std::vector<mat4<float>> poseA() {
        return {placement(0.01F, -0.3F, -0.8F, 0.2F), placement(0.004F, 0.4F, 0.2F, -0.2F), placement(0.005F, 0.3F, -0.9F, 0.5F)};
    }
    std::vector<mat4<float>> poseB() {
        return {placement(0.012F, 0.2F, -0.9F, -0.1F), placement(0.006F, -0.4F, -0.3F, 0.3F), placement(0.005F, 0.3F, -0.9F, 0.5F)};
    }

    std::unique_ptr<Scene> meshScene(const std::string &text, const std::vector<mat4<float>> &pose) {
        Objects objects;
        Lights lights;
        addBase(objects, lights);
        std::istringstream stream(text);
        auto data = std::make_shared<const io::MeshData>(io::loadMeshData(stream));
        std::vector<MeshInstance> instances;
        const auto p = placed();
        for(size_t i = 0; i < p.size(); i++) {
            instances.push_back(MeshInstance{data, pose[i], p[i].cull_backface, p[i].smooth, p[i].handler});
        }
        return std::make_unique<Scene>(std::move(objects), std::move(lights), std::move(instances));
    }

    std::unique_ptr<Scene> flatScene(const std::string &text, const std::vector<mat4<float>> &pose) {
        Objects objects;
        Lights lights;
        addBase(objects, lights);
        const auto p = placed();
        for(size_t i = 0; i < p.size(); i++) {
            std::istringstream stream(text);
            auto triangles = io::loadMesh(stream, pose[i], p[i].cull_backface, p[i].smooth);
            if(p[i].handler != nullptr) {
                for(auto &t : triangles) {
                    t.setMaterialHandler(p[i].handler);
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
        RenderOptions options{64, 64, 4, 8, 1E-3F};
        setenv("PATHTRACE_SEED", "77", 1);
        auto image = processJob(FrameRenderJob{camera, scene, options});
        unsetenv("PATHTRACE_SEED");
        return image;
    }

} // namespace

TEST(PoseScene, RendersTheImageOfASceneConstructedAtThePose) {
    for(const auto &[nu, nv] : {std::pair<int, int>{24, 16}, std::pair<int, int>{48, 24}}) { // the host builder; the device builder
        const std::string text = sphereText(nu, nv);
        auto posed = meshScene(text, poseA());
        (void)render(*posed); // (the workspace is sized for pose A)
        posed->pose(poseB());
        const auto image = render(*posed);
        EXPECT_THAT(sameBits(image, render(*meshScene(text, poseB()))), testing::Eq(true));
        EXPECT_THAT(sameBits(image, render(*flatScene(text, poseB()))), testing::Eq(true));
        // the subset form: instance 1 back to where it was, the others stay
        posed->pose(std::vector<uint32_t>{1}, std::vector<mat4<float>>{poseA()[1]});
        auto mixed = poseB();
        mixed[1] = poseA()[1];
        EXPECT_THAT(sameBits(render(*posed), render(*flatScene(text, mixed))), testing::Eq(true));
    }
}

TEST(PoseScene, HitsReturnTrianglesAtTheNewPositions) {
    const std::string text = sphereText(48, 24);
    auto posed = meshScene(text, poseA());
    RandomEngine warm(9);
    std::uniform_real_distribution<float> dist(-0.9F, 0.9F);
    for(int k = 0; k < 50; k++) { // Triangles of pose A are handed out and cached: they must not survive the pose
        const vec3<float> origin{dist(warm), dist(warm), dist(warm)};
        (void)posed->getIntersection(Ray{origin, vec3<float>(vec3<float>{dist(warm), dist(warm), dist(warm)}.normalize())});
    }
    posed->pose(poseB());
    auto flat = flatScene(text, poseB());
    RandomEngine re(5);
    int on_mesh = 0, differing = 0;
    for(int k = 0; k < 400; k++) {
        const vec3<float> origin{dist(re), dist(re), dist(re)};
        const vec3<float> dir = vec3<float>(vec3<float>{dist(re), dist(re), dist(re)}.normalize());
        const auto [ta, oa] = posed->getIntersection(Ray{origin, dir});
        const auto [tb, ob] = flat->getIntersection(Ray{origin, dir});
        differing += std::memcmp(&ta, &tb, sizeof(float)) != 0 || (oa == nullptr) != (ob == nullptr);
        const auto *a = dynamic_cast<const Triangle *>(oa);
        const auto *b = dynamic_cast<const Triangle *>(ob);
        if((a == nullptr) != (b == nullptr)) {
            differing++;
            continue;
        }
        if(a == nullptr) {
            continue;
        }
        const bool same = sameVector(a->a, b->a) && sameVector(a->b, b->b) && sameVector(a->c, b->c) && sameVector(a->normal_a, b->normal_a) &&
                          sameVector(a->normal_b, b->normal_b) && sameVector(a->normal_c, b->normal_c) && a->cullsBackface() == b->cullsBackface();
        differing += same ? 0 : 1;
        on_mesh += (a->b - a->a).getLengthSquared() < 0.25F ? 1 : 0; // (a wall triangle of the box spans more than 1.9)
    }
    EXPECT_THAT(differing, testing::Eq(0));
    EXPECT_THAT(on_mesh > 50, testing::Eq(true));
}

TEST(PoseScene, LightSamplesFollowAnEmissiveInstance) {
    const std::string text = sphereText(24, 16);
    auto posed = meshScene(text, poseA());
    posed->pose(poseB()); // instance 1 is the lamp: it moves and grows
    auto flat = flatScene(text, poseB());
    RandomEngine ra(1234), rb(1234);
    int differing = 0, samples = 0;
    for(int k = 0; k < 200; k++) {
        const vec3<float> pos{0.01F * static_cast<float>(k % 50) - 0.2F, -0.5F + 0.005F * static_cast<float>(k), 0.1F};
        const auto a = posed->sampleLights(pos, vec3<float>{0.0F, 1.0F, 0.0F}, ra);
        const auto b = flat->sampleLights(pos, vec3<float>{0.0F, 1.0F, 0.0F}, rb);
        differing += a.size() != b.size() || ra.state() != rb.state();
        for(size_t i = 0; i < a.size() && i < b.size(); i++) {
            const auto ca = std::get<1>(a[i]).getColor(), cb = std::get<1>(b[i]).getColor();
            differing += !sameVector(std::get<0>(a[i]), std::get<0>(b[i])) || std::memcmp(&ca, &cb, sizeof(ca)) != 0 ||
                         std::memcmp(&std::get<2>(a[i]), &std::get<2>(b[i]), sizeof(float)) != 0;
            samples++;
        }
    }
    EXPECT_THAT(differing, testing::Eq(0));
    EXPECT_THAT(samples > 400, testing::Eq(true));
    // what the constructor throws: a wrong count, an index that is not there, a Scene without instances
    int thrown = 0;
    try {
        posed->pose(std::vector<mat4<float>>{poseA()[0]});
    } catch(const std::invalid_argument &) {
        thrown++;
    }
    try {
        posed->pose(std::vector<uint32_t>{3}, std::vector<mat4<float>>{poseA()[0]});
    } catch(const std::invalid_argument &) {
        thrown++;
    }
    try {
        flat->pose(poseA());
    } catch(const std::invalid_argument &) {
        thrown++;
    }
    EXPECT_THAT(thrown, testing::Eq(3));
}

int main(int argc, char **argv) {
    testing::InitGoogleTest(&argc, argv);
    return RUN_ALL_TESTS();
}
