// tests/cpp/gather_test.cpp -- Scene::gather, Scene::gatherFrame and Scene::bakeInstance (include/PathTrace/gather.h, include/pt_gather.h):
// a Scene of a wall, a sphere, two instances of a two-face card and a point light.  Every call returns one record per point, pixel or
// corner, the options the device would refuse are argument errors, and every record is printed as "RECORD <call> <kind> <index> <eight
// hex words>" for tests/test_cpp_gather.py, which compares them with what the Python binding returns for the same scene.
#include <PathTrace/camera.h>
#include <PathTrace/gather.h>
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

    // tests/cpp/query_test.cpp's scene with a light: a wall at z = 1, a sphere in front of its lower left, a card of two faces twice
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

    const int W = 12, H = 10;
    Camera camera() { return Camera({0.0F, 0.0F, -2.0F}, {0.0F, 0.0F, 1.0F}, {0.0F, 1.0F, 0.0F}, 1.0F, 1.0F, -static_cast<float>(W) / static_cast<float>(H)); }
    RenderOptions options() { return RenderOptions{W, H, 1, 1, 1E-3F}; }

    const GatherKind kinds[3] = {GatherKind::occlusion, GatherKind::direct, GatherKind::paths};

    GatherOptions gatherOptions(GatherKind kind) {
        GatherOptions o;
        o.kind = kind;
        o.samples = 3;
        o.distance = kind == GatherKind::occlusion ? 0.75F : std::numeric_limits<float>::infinity();
        o.base_seed = 41;
        return o;
    }

    void print(const char *call, GatherKind kind, size_t index, const GatherResult &r) {
        uint32_t w[4];
        std::memcpy(w, &r.value, sizeof(w));
        std::printf("RECORD %s %d %zu %08x %08x %08x %08x %08x %08x %08x %08x\n", call, static_cast<int>(kind), index, w[0], w[1], w[2], w[3], r.samples, r.occluded, 0U, 0U);
    }

    // the points the Python side gathers at as well: on the wall, on the cards, in front of the sphere, in empty space
    std::vector<GatherPoint> somePoints() {
        std::vector<GatherPoint> points;
        for(int k = 0; k < 9; k++) {
            GatherPoint p;
            p.position = vec3<float>{-1.0F + 0.25F * static_cast<float>(k), -0.5F + 0.125F * static_cast<float>(k), k % 3 == 0 ? 1.0F : (k % 3 == 1 ? 0.5F : 0.0F)};
            p.normal = vec3<float>{0.0F, 0.0F, -1.0F};
            points.push_back(p);
        }
        points[4].normal = vec3<float>{0.0F, 1.0F, 0.0F};
        return points;
    }

} // namespace

TEST(GatherScene, EveryCallReturnsItsRecords) {
    auto scene = cardScene();
    for(GatherKind kind : kinds) {
        const GatherOptions o = gatherOptions(kind);
        const std::vector<GatherPoint> points = somePoints();
        const std::vector<GatherResult> at_points = scene->gather(points, o);
        EXPECT_THAT(at_points.size(), testing::Eq(points.size()));
        for(size_t i = 0; i < at_points.size(); i++) {
            print("points", kind, i, at_points[i]);
            EXPECT_THAT(at_points[i].samples == 3U && at_points[i].value[3] == 1.0F && at_points[i].occluded <= (kind == GatherKind::occlusion ? 3U : 0U), testing::Eq(true));
        }
        // a frame: one record per pixel in row order (the wall fills the frame: every pixel hits)
        const std::vector<GatherResult> frame = scene->gatherFrame(camera(), options(), o);
        EXPECT_THAT(frame.size(), testing::Eq(static_cast<size_t>(W * H)));
        int taken = 0;
        for(size_t i = 0; i < frame.size(); i++) {
            print("frame", kind, i, frame[i]);
            taken += frame[i].samples == 3U && frame[i].value[3] == 1.0F ? 1 : 0;
        }
        EXPECT_THAT(taken, testing::Eq(W * H));
        // a bake: two triangles of three corners per card
        for(size_t instance = 0; instance < 2; instance++) {
            const auto baked = scene->bakeInstance(instance, o);
            EXPECT_THAT(baked.size(), testing::Eq(2U));
            int positions = 0;
            for(size_t t = 0; t < baked.size(); t++) {
                for(size_t c = 0; c < 3; c++) {
                    print(instance == 0 ? "bake0" : "bake1", kind, 3 * t + c, baked[t][c]);
                    positions += baked[t][c].samples == 3U ? 1 : 0;
                }
            }
            EXPECT_THAT(positions, testing::Eq(6));
        }
    }
}

TEST(GatherScene, RefusedOptionsAreArgumentErrors) {
    auto scene = cardScene();
    int thrown = 0;
    auto refused = [&](auto call) {
        try {
            call();
        } catch(const std::invalid_argument &) {
            thrown++;
        }
    };
    GatherOptions o = gatherOptions(GatherKind::direct);
    o.samples = 0;
    refused([&] { scene->gather(somePoints(), o); });
    o = gatherOptions(GatherKind::paths);
    o.epsilon = -1.0F;
    refused([&] { scene->gatherFrame(camera(), options(), o); });
    o = gatherOptions(GatherKind::occlusion);
    o.distance = 0.0F;
    refused([&] { scene->gather(somePoints(), o); });
    o.distance = std::numeric_limits<float>::quiet_NaN();
    refused([&] { scene->bakeInstance(0, o); });
    refused([&] { scene->bakeInstance(2, gatherOptions(GatherKind::direct)); });
    refused([&] { scene->gatherFrame(camera(), RenderOptions{0, H, 1, 1, 1E-3F}, gatherOptions(GatherKind::direct)); });
    EXPECT_THAT(thrown, testing::Eq(6));
    EXPECT_THAT(scene->gather({}, gatherOptions(GatherKind::paths)).size(), testing::Eq(0U));
}

int main(int argc, char **argv) {
    testing::InitGoogleTest(&argc, argv);
    return RUN_ALL_TESTS();
}
