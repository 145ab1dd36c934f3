// tests/cpp/morph_scene_test.cpp -- Scene::bindMorphs and Scene::morph: a Scene of MeshInstances whose mesh is morphed on the device --
// alone, or in front of the rig of Scene::bindSkin -- against Scenes CONSTRUCTED from a MeshData with those vertices: the same processJob
// image under one PATHTRACE_SEED.  The morphed and skinned vertices are computed here with the arithmetic include/pt_morph.h and
// include/pt_deform.h state, in float, operation by operation (this file is compiled with -ffp-contract=off).
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

    std::shared_ptr<MaterialHandler> handlerOf(Color<float> diffuse, float ior, Color<float> emission, std::shared_ptr<BSDF> bsdf) {
        return std::make_shared<ConstantMaterialHandler>(std::make_shared<ConstantMaterial>(diffuse, ior, Spectrum(emission)), std::move(bsdf));
    }

    mat4<float> placement(float scale, float x, float y, float z) {
        return mat4<float>{vec4<float>{scale, 0.0F, 0.0F, x}, vec4<float>{0.0F, scale, 0.0F, y}, vec4<float>{0.0F, 0.0F, scale, z}, vec4<float>{0.0F, 0.0F, 0.0F, 1.0F}};
    }

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

    // Two instances of `face` under different matrices (one of them a lamp) and one of `still`, which no morph names
    std::unique_ptr<Scene> meshScene(const std::shared_ptr<const io::MeshData> &face, const std::shared_ptr<const io::MeshData> &still) {
        Objects objects;
        Lights lights;
        addBase(objects, lights);
        auto glass = handlerOf(Color<float>(1.0F, 1.0F, 1.0F, 1.0F), 1.5F, Color<float>{0.0F, 0.0F, 0.0F, 0.0F}, std::make_shared<GlassBDF>());
        auto lamp = handlerOf(Color<float>(1.0F, 1.0F, 1.0F, 1.0F), 1.0F, Color<float>{1.0F, 0.9F, 0.8F, 2.0F}, std::make_shared<LambertianBRDF>());
        std::vector<MeshInstance> instances;
        instances.push_back(MeshInstance{face, placement(0.008F, -0.3F, -0.8F, 0.2F), false, true, glass});
        instances.push_back(MeshInstance{still, placement(0.005F, 0.3F, -0.9F, 0.5F), true, true, nullptr});
        instances.push_back(MeshInstance{face, placement(0.004F, 0.4F, 0.2F, -0.2F), true, false, lamp});
        return std::make_unique<Scene>(std::move(objects), std::move(lights), std::move(instances));
    }

    std::shared_ptr<const io::MeshData> meshOf(const std::string &text) {
        std::istringstream stream(text);
        return std::make_shared<const io::MeshData>(io::loadMeshData(stream));
    }

    std::shared_ptr<const io::MeshData> withVertices(const io::MeshData &mesh, const std::vector<vec3<float>> &vertices) {
        io::MeshData copy = mesh;
        copy.vertices = vertices;
        return std::make_shared<const io::MeshData>(std::move(copy));
    }

    // Three targets: a dense stretch along x that grows with height, a sparse bulge of every third vertex of the upper half, and an
    // empty one between them
    std::vector<MorphTarget> targetsOf(const io::MeshData &mesh) {
        MorphTarget stretch, nothing, bulge;
        for(uint32_t i = 0; i < mesh.vertices.size(); i++) {
            const auto &v = mesh.vertices[i];
            stretch.deltas.push_back(vec3<float>{0.25F * v[0] * (v[1] - 10.0F) / 80.0F, 0.0F, 0.05F * v[2]});
            if(i % 3 == 0 && v[1] > 50.0F) {
                bulge.vertices.push_back(i);
                bulge.deltas.push_back(vec3<float>{0.1F * v[0], 4.0F, 0.1F * v[2]});
            }
        }
        return {stretch, nothing, bulge};
    }

    // include/pt_morph.h's arithmetic: target after target, only the vertices a target lists, product and sum rounded on their own
    std::vector<vec3<float>> morphed(const io::MeshData &mesh, const std::vector<MorphTarget> &targets, const std::vector<float> &weights) {
        std::vector<vec3<float>> out = mesh.vertices;
        for(size_t t = 0; t < targets.size(); t++) {
            for(size_t j = 0; j < targets[t].deltas.size(); j++) {
                const size_t i = targets[t].vertices.empty() ? j : targets[t].vertices[j];
                float m[3] = {out[i][0], out[i][1], out[i][2]};
                for(int c = 0; c < 3; c++) {
                    const float product = weights[t] * targets[t].deltas[j][c];
                    m[c] += product;
                }
                out[i] = vec3<float>{m[0], m[1], m[2]};
            }
        }
        return out;
    }

    // two bones, K = 2: the upper half follows bone 1, the lower bone 0, blended by height
    struct Rig {
        std::vector<uint32_t> bone;
        std::vector<float> weight;
    };
    Rig rigOf(const io::MeshData &mesh) {
        Rig rig;
        for(const auto &v : mesh.vertices) {
            const float t = std::min(std::max((v[1] - 10.0F) / 80.0F, 0.0F), 1.0F);
            rig.bone.insert(rig.bone.end(), {0U, 1U});
            rig.weight.insert(rig.weight.end(), {1.0F - t, t});
        }
        return rig;
    }
    std::vector<mat4<float>> bonesOf(float lean) {
        return {mat4_identity<float>,
                mat4<float>{vec4<float>{1.0F, lean, 0.0F, -50.0F * lean}, vec4<float>{0.0F, 1.0F, 0.0F, 5.0F}, vec4<float>{0.0F, 0.0F, 1.1F, 0.0F}, vec4<float>{0.0F, 0.0F, 0.0F, 1.0F}}};
    }
    std::vector<vec3<float>> skinned(const std::vector<vec3<float>> &vertices, const Rig &rig, const std::vector<mat4<float>> &bones) {
        std::vector<vec3<float>> out;
        for(size_t i = 0; i < vertices.size(); i++) {
            const auto &v = vertices[i];
            float acc[3] = {0.0F, 0.0F, 0.0F};
            for(size_t k = 0; k < 2; k++) {
                const mat4<float> &b = bones[rig.bone[2 * i + k]];
                for(int c = 0; c < 3; c++) {
                    float d = 0.0F;
                    d += b.rows[c][0] * v[0];
                    d += b.rows[c][1] * v[1];
                    d += b.rows[c][2] * v[2];
                    d += b.rows[c][3] * 1.0F;
                    acc[c] += rig.weight[2 * i + k] * d;
                }
            }
            out.push_back(vec3<float>{acc[0], acc[1], acc[2]});
        }
        return out;
    }

    bool sameBits(const Image<> &a, const Image<> &b) {
        return a.getWidth() == b.getWidth() && a.getHeight() == b.getHeight() && std::memcmp(a.data(), b.data(), a.size() * sizeof(Color<float>)) == 0;
    }

    Image<> render(const Scene &scene) {
        Camera camera({0.0F, 0.0F, -3.0F}, {0.0F, 0.0F, 0.0F}, {0.0F, 1.0F, 0.0F}, 1.0F, 1.0F, -1.0F);
        RenderOptions options{32, 32, 4, 8, 1E-3F};
        setenv("PATHTRACE_SEED", "77", 1);
        auto image = processJob(FrameRenderJob{camera, scene, options});
        unsetenv("PATHTRACE_SEED");
        return image;
    }

} // namespace

TEST(MorphScene, WeightsRenderTheImageOfASceneConstructedFromTheMorphedVertices) {
    const auto face = meshOf(sphereText(24, 12)), still = meshOf(sphereText(8, 4));
    auto scene = meshScene(face, still);
    const auto created = render(*scene);
    const auto targets = targetsOf(*face);
    scene->bindMorphs(face, targets);
    EXPECT_THAT(sameBits(render(*scene), created), testing::Eq(true)); // (binding changes no geometry)
    scene->morph(face, {1.0F, 3.0F, 0.0F});
    scene->morph(face, {0.6F, -2.0F, 1.5F}); // (from the rest vertices again: the first weights leave no trace)
    const auto image = render(*scene);
    EXPECT_THAT(sameBits(image, created), testing::Eq(false));
    EXPECT_THAT(sameBits(image, render(*meshScene(withVertices(*face, morphed(*face, targets, {0.6F, -2.0F, 1.5F})), still))), testing::Eq(true));
    scene->restShape(face);
    EXPECT_THAT(sameBits(render(*scene), created), testing::Eq(true));
}

TEST(MorphScene, WeightsAndBonesRenderTheImageOfTheSkinnedMorphedVertices) {
    const auto face = meshOf(sphereText(24, 12)), still = meshOf(sphereText(8, 4));
    auto scene = meshScene(face, still);
    const auto targets = targetsOf(*face);
    const Rig rig = rigOf(*face);
    scene->bindMorphs(face, targets);
    scene->bindSkin(face, rig.bone, rig.weight, 2);
    const std::vector<float> weights{0.8F, 0.0F, -0.5F};
    scene->morph(face, weights, bonesOf(0.3F));
    const auto expected = skinned(morphed(*face, targets, weights), rig, bonesOf(0.3F));
    EXPECT_THAT(sameBits(render(*scene), render(*meshScene(withVertices(*face, expected), still))), testing::Eq(true));
    // bones alone afterwards skin the REST vertices, not the morphed ones
    scene->deform(face, bonesOf(0.3F));
    EXPECT_THAT(sameBits(render(*scene), render(*meshScene(withVertices(*face, skinned(face->vertices, rig, bonesOf(0.3F))), still))), testing::Eq(true));
    // a pose after the morph keeps the shape
    scene->morph(face, weights, bonesOf(-0.2F));
    const auto moved = placement(0.006F, -0.2F, -0.7F, 0.1F);
    scene->pose(std::vector<uint32_t>{0}, std::vector<mat4<float>>{moved});
    auto fresh = meshScene(withVertices(*face, skinned(morphed(*face, targets, weights), rig, bonesOf(-0.2F))), still);
    fresh->pose(std::vector<uint32_t>{0}, std::vector<mat4<float>>{moved});
    EXPECT_THAT(sameBits(render(*scene), render(*fresh)), testing::Eq(true));
}

TEST(MorphScene, RefusalsThrowInvalidArgument) {
    const auto face = meshOf(sphereText(8, 4)), still = meshOf(sphereText(8, 4)), stranger = meshOf(sphereText(8, 4));
    auto scene = meshScene(face, still);
    const auto before = render(*scene);
    int thrown = 0;
    auto refused = [&](auto call) {
        try {
            call();
        } catch(const std::invalid_argument &) {
            thrown++;
        }
    };
    const auto targets = targetsOf(*face);
    const uint32_t n = static_cast<uint32_t>(face->vertices.size());
    refused([&] { scene->bindMorphs(stranger, targets); });                                                              // a mesh no instance uses
    refused([&] { scene->morph(face, {1.0F, 1.0F, 1.0F}); });                                                           // no bound targets
    refused([&] { scene->bindMorphs(face, {MorphTarget{{}, std::vector<vec3<float>>(n - 1)}}); });                      // a dense target of another length
    refused([&] { scene->bindMorphs(face, {MorphTarget{{2, 1}, std::vector<vec3<float>>(2)}}); });                      // indices that do not ascend
    refused([&] { scene->bindMorphs(face, {MorphTarget{{1, n}, std::vector<vec3<float>>(2)}}); });                      // an index that names no vertex
    refused([&] { scene->bindMorphs(face, {MorphTarget{{1, 2}, std::vector<vec3<float>>(3)}}); });                      // deltas that do not match the indices
    scene->bindMorphs(face, targets);
    refused([&] { scene->morph(face, {1.0F, 1.0F}); });                                                                 // a wrong weight count
    refused([&] { scene->morph(face, {1.0F, 1.0F, 1.0F}, bonesOf(0.1F)); });                                            // bones without a rig
    const Rig rig = rigOf(*face);
    scene->bindSkin(face, rig.bone, rig.weight, 2);
    refused([&] { scene->morph(face, {1.0F, 1.0F, 1.0F}, std::vector<mat4<float>>(3, mat4_identity<float>)); });         // a wrong bone count
    scene->bindMorphs(face, {});
    refused([&] { scene->morph(face, {1.0F, 1.0F, 1.0F}); });                                                           // unbound again
    Objects objects;
    Lights lights;
    addBase(objects, lights);
    Scene plain(std::move(objects), std::move(lights));
    refused([&] { plain.bindMorphs(face, targets); });                                                                  // a Scene without mesh instances
    EXPECT_THAT(thrown, testing::Eq(11));
    EXPECT_THAT(sameBits(render(*scene), before), testing::Eq(true));
}

int main(int argc, char **argv) {
    testing::InitGoogleTest(&argc, argv);
    return RUN_ALL_TESTS();
}
