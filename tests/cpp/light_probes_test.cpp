// tests/cpp/light_probes_test.cpp -- Scene::lightProbes, Scene::lightProbeGrid and Scene::shadeWithLightProbes
// (include/PathTrace/light_probes.h, include/pt_light_probes.h) on tests/cpp/gather_test.cpp's scene: a wall, a sphere, two instances of a
// two-face card and a point light.  Every call returns one record per probe, node or point, the arguments the device would refuse are
// argument errors, and every record is printed as "RECORD <call> <index> <hex words>" for tests/test_cpp_light_probes.py, which compares
// them with what the Python binding returns for the same scene.
#include <PathTrace/camera.h>
#include <PathTrace/light_probes.h>
#include <PathTrace/scene/light.h>
#include <PathTrace/scene/mesh.h>
#include <PathTrace/scene/object.h>
#include <PathTrace/scene/scene.h>
#include <PathTrace/worker.h>

#include <gmock/gmock.h>
#include <gtest/gtest.h>

#include <cstdio>
#include <cstring>
#include <limits>
#include <sstream>
#include <stdexcept>

namespace {

    using Objects = std::vector<std::unique_ptr<Object>>;
    using Lights = std::vector<std::unique_ptr<LightSource>>;

    mat4<float> placement(float x, float y, float z) {
        return mat4<float>{vec4<float>{1.0F, 0.0F, 0.0F, x}, vec4<float>{0.0F, 1.0F, 0.0F, y}, vec4<float>{0.0F, 0.0F, 1.0F, z}, vec4<float>{0.0F, 0.0F, 0.0F, 1.0F}};
    }

    std::unique_ptr<Scene> cardScene() {
        Objects objects;
        Lights lights;
        auto wall = makePlane(vec3<float>{-2.0F, -2.0F, 1.0F}, vec3<float>{2.0F, 2.0F, 1.0F});
        moveObjects(objects, wall);
        objects.emplace_back(std::make_unique<Sphere>(vec3<float>{-0.5F, -0.5F, 0.5F}, 0.2F));
        lights.emplace_back(std::make_unique<PointLightSource>(vec3<float>{0.3F, 0.8F, -0.5F}, Spectrum(Color<float>{0.5F, 0.75F, 1.0F, 1.0F})));
        std::istringstream text("v -0.2 -0.2 0\nv 0.2 -0.2 0\nv 0.2 0.2 0\nv -0.2 0.2 0\nf 1 3 2\nf 1 4 3\n");
        auto mesh = std::make_shared<const io::MeshData>(io::loadMeshData(text));
        std::vector<MeshInstance> instances(2);
        for(int i = 0; i < 2; i++) {
            instances[i].mesh = mesh;
            instances[i].transformation = placement(i == 0 ? -0.4F : 0.4F, 0.3F, 0.5F);
            instances[i].cull_backface = false;
            instances[i].smooth = false;
        }
        return std::make_unique<Scene>(std::move(objects), std::move(lights), std::move(instances));
    }

    LightProbeOptions probeOptions() {
        LightProbeOptions o;
        o.samples = 65;
        o.base_seed = 43;
        return o;
    }

    LightProbeGrid someGrid() {
        LightProbeGrid g;
        g.origin = vec3<float>{-0.75F, -0.5F, -0.25F};
        g.step = vec3<float>{0.5F, 0.75F, 0.5F};
        g.count = {3, 2, 2};
        return g;
    }

    void print(const char *call, size_t index, const LightProbe &r) {
        std::printf("RECORD %s %zu", call, index);
        for(size_t k = 0; k < 9; k++) {
            for(size_t c = 0; c < 3; c++) {
                uint32_t w;
                std::memcpy(&w, &r.sh[k][c], 4);
                std::printf(" %08x", w);
            }
        }
        std::printf(" %08x %08x %08x\n", r.samples, r.missed, r.backfacing);
    }

    // the positions the Python side probes as well: in front of the wall, between the cards, behind the wall
    std::vector<vec3<float>> somePositions() {
        std::vector<vec3<float>> positions;
        for(int k = 0; k < 9; k++) {
            positions.push_back(vec3<float>{-1.0F + 0.25F * static_cast<float>(k), -0.5F + 0.125F * static_cast<float>(k), k % 3 == 0 ? 1.5F : (k % 3 == 1 ? 0.5F : 0.0F)});
        }
        return positions;
    }

    std::vector<GatherPoint> somePoints() {
        std::vector<GatherPoint> points;
        for(int k = 0; k < 11; k++) {
            GatherPoint p;
            p.position = vec3<float>{-1.0F + 0.25F * static_cast<float>(k), -0.75F + 0.25F * static_cast<float>(k), -0.5F + 0.125F * static_cast<float>(k)};
            p.normal = k % 2 == 0 ? vec3<float>{0.0F, 0.0F, -1.0F} : vec3<float>{0.0F, 1.0F, 0.0F};
            points.push_back(p);
        }
        return points;
    }

} // namespace

TEST(LightProbeScene, EveryCallReturnsItsRecords) {
    auto scene = cardScene();
    const LightProbeOptions o = probeOptions();
    const std::vector<vec3<float>> positions = somePositions();
    const std::vector<LightProbe> at_positions = scene->lightProbes(positions, o);
    EXPECT_THAT(at_positions.size(), testing::Eq(positions.size()));
    for(size_t i = 0; i < at_positions.size(); i++) {
        print("points", i, at_positions[i]);
        EXPECT_THAT(at_positions[i].samples == 65U && at_positions[i].missed + at_positions[i].backfacing <= 65U, testing::Eq(true));
    }
    const LightProbeGrid grid = someGrid();
    const std::vector<LightProbe> nodes = scene->lightProbeGrid(grid, o);
    EXPECT_THAT(nodes.size(), testing::Eq(12U));
    for(size_t i = 0; i < nodes.size(); i++) {
        print("grid", i, nodes[i]);
    }
    const std::vector<GatherPoint> points = somePoints();
    const std::vector<Color<float>> shaded = scene->shadeWithLightProbes(grid, nodes, points, o);
    EXPECT_THAT(shaded.size(), testing::Eq(points.size()));
    for(size_t i = 0; i < shaded.size(); i++) {
        uint32_t w[4];
        std::memcpy(w, &shaded[i], sizeof(w));
        std::printf("RECORD shade %zu %08x %08x %08x %08x\n", i, w[0], w[1], w[2], w[3]);
        EXPECT_THAT(shaded[i][3] >= 0.0F && shaded[i][3] <= 1.0001F, testing::Eq(true));
    }
}

TEST(LightProbeScene, RefusedArgumentsAreArgumentErrors) {
    auto scene = cardScene();
    int thrown = 0;
    auto refused = [&](auto call) {
        try {
            call();
        } catch(const std::invalid_argument &) {
            thrown++;
        }
    };
    LightProbeOptions o = probeOptions();
    o.samples = 0;
    refused([&] { scene->lightProbes(somePositions(), o); });
    o = probeOptions();
    o.epsilon = -1.0F;
    refused([&] { scene->lightProbeGrid(someGrid(), o); });
    o = probeOptions();
    o.max_backfacing = std::numeric_limits<float>::quiet_NaN();
    refused([&] { scene->lightProbes(somePositions(), o); });
    LightProbeGrid g = someGrid();
    g.count[1] = 0;
    refused([&] { scene->lightProbeGrid(g, probeOptions()); });
    g = someGrid();
    g.step[2] = 0.0F;
    refused([&] { scene->lightProbeGrid(g, probeOptions()); });
    g.step[2] = std::numeric_limits<float>::infinity();
    refused([&] { scene->shadeWithLightProbes(g, std::vector<LightProbe>(12), somePoints(), probeOptions()); });
    refused([&] { scene->shadeWithLightProbes(someGrid(), std::vector<LightProbe>(11), somePoints(), probeOptions()); });
    EXPECT_THAT(thrown, testing::Eq(7));
    EXPECT_THAT(scene->lightProbes({}, probeOptions()).size(), testing::Eq(0U));
}

int main(int argc, char **argv) {
    testing::InitGoogleTest(&argc, argv);
    return RUN_ALL_TESTS();
}
