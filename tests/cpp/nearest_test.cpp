// tests/cpp/nearest_test.cpp -- Scene::nearest and Scene::distanceGrid (include/PathTrace/nearest.h, include/pt_nearest.h): in a Scene
// of a wall, a sphere and two instances of a two-face card, points in front of each are answered with that object, its instance and
// face, the closest point and the side; a threshold turns far answers into misses; and a grid is the same queries at its nodes.
#include <PathTrace/nearest.h>
#include <PathTrace/scene/light.h>
#include <PathTrace/scene/mesh.h>
#include <PathTrace/scene/object.h>
#include <PathTrace/scene/scene.h>

#include <gmock/gmock.h>
#include <gtest/gtest.h>

#include <cmath>
#include <limits>
#include <sstream>
#include <stdexcept>

namespace {

    using Objects = std::vector<std::unique_ptr<Object>>;
    using Lights = std::vector<std::unique_ptr<LightSource>>;

    mat4<float> placement(float x, float y, float z) {
        return mat4<float>{vec4<float>{1.0F, 0.0F, 0.0F, x}, vec4<float>{0.0F, 1.0F, 0.0F, y}, vec4<float>{0.0F, 0.0F, 1.0F, z}, vec4<float>{0.0F, 0.0F, 0.0F, 1.0F}};
    }

    // a wall at z = 1 (2 triangles), a sphere in front of its lower left, and a card of two faces twice: left and right of the centre
    std::unique_ptr<Scene> cardScene() {
        Objects objects;
        Lights lights;
        auto wall = makePlane(vec3<float>{-2.0F, -2.0F, 1.0F}, vec3<float>{2.0F, 2.0F, 1.0F});
        moveObjects(objects, wall);
        objects.emplace_back(std::make_unique<Sphere>(vec3<float>{-0.5F, -0.5F, 0.5F}, 0.2F));
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

} // namespace

TEST(NearestScene, NamesObjectInstanceFaceAndClosestPoint) {
    auto scene = cardScene();
    const std::vector<vec3<float>> points = {{1.5F, -1.5F, 0.9F},   // in front of the wall
                                             {-0.5F, -0.5F, 0.1F},  // in front of the sphere
                                             {-0.5F, -0.5F, 0.5F},  // its centre
                                             {-0.45F, 0.35F, 0.4F}, // in front of the left card
                                             {0.45F, 0.25F, 0.6F},  // behind the right card
                                             {0.7F, 0.3F, 0.5F}};   // in the right card's plane, past its edge
    const std::vector<NearestResult> r = scene->nearest(points);
    EXPECT_THAT(r.size(), testing::Eq(points.size()));
    if(r.size() != points.size()) {
        return;
    }
    for(const NearestResult &n : r) {
        EXPECT_THAT(n.found && n.object != nullptr, testing::Eq(true));
    }
    EXPECT_THAT(r[0].object_index < 2 && r[0].instance == -1 && r[0].face == NearestResult::no_face && std::abs(r[0].distance - 0.1F) <= 1E-6F, testing::Eq(true));
    EXPECT_THAT(std::abs(r[0].position[2] - 1.0F) <= 1E-6F && r[0].feature == NearestFeature::face, testing::Eq(true));
    EXPECT_THAT(r[1].object_index == 2 && r[1].feature == NearestFeature::sphere && r[1].side == 1 && std::abs(r[1].distance - 0.2F) <= 1E-6F, testing::Eq(true));
    EXPECT_THAT(std::abs(r[1].position[2] - 0.3F) <= 1E-6F && std::abs(r[1].geometric_normal[2] + 1.0F) <= 1E-6F, testing::Eq(true));
    EXPECT_THAT(r[2].object_index == 2 && r[2].side == -1 && r[2].distance == 0.2F && r[2].geometric_normal[0] == 1.0F, testing::Eq(true));
    EXPECT_THAT(r[3].instance == 0 && r[3].face < 2 && r[3].object_index == 3 + static_cast<int>(r[3].face) && std::abs(r[3].distance - 0.1F) <= 1E-6F, testing::Eq(true));
    EXPECT_THAT(r[4].instance == 1 && r[4].face < 2 && r[4].object_index == 5 + static_cast<int>(r[4].face) && r[4].side == -r[3].side && r[3].side != 0, testing::Eq(true));
    EXPECT_THAT(r[3].b1 >= 0.0F && r[3].b2 >= 0.0F && r[3].b1 + r[3].b2 <= 1.0F && std::abs(r[3].position[2] - 0.5F) <= 1E-6F, testing::Eq(true));
    EXPECT_THAT(r[5].instance == 1 && r[5].feature != NearestFeature::face && r[5].side == 0 && std::abs(r[5].distance - 0.1F) <= 1E-6F, testing::Eq(true));
    // the object is the one Scene::getIntersection reports for the ray from the point to the card
    const auto [t, object] = scene->getIntersection(Ray{points[3], vec3<float>{0.0F, 0.0F, 1.0F}});
    EXPECT_THAT(object == r[3].object && std::abs(t - r[3].distance) <= 1E-6F, testing::Eq(true));
    // a threshold: the answers at 0.1 stay, the ones at 0.2 become misses
    const std::vector<NearestResult> close = scene->nearest(points, 0.15F);
    EXPECT_THAT(close[0].found && !close[1].found && !close[2].found && close[3].found && close[5].found, testing::Eq(true));
    EXPECT_THAT(close[1].object == nullptr && close[1].object_index == -1 && std::isinf(close[1].distance), testing::Eq(true));
    EXPECT_THAT(scene->nearest({}).empty(), testing::Eq(true));
    EXPECT_THAT(scene->nearest({vec3<float>{std::numeric_limits<float>::quiet_NaN(), 0.0F, 0.0F}})[0].found, testing::Eq(false));
}

TEST(NearestScene, DistanceGridIsNearestAtItsNodes) {
    auto scene = cardScene();
    DistanceGrid grid;
    grid.origin = vec3<float>{-1.0F, -1.0F, 0.0F};
    grid.step = vec3<float>{0.5F, 0.5F, 0.25F};
    grid.count = {5, 5, 4};
    const DistanceField field = scene->distanceGrid(grid, 0.45F);
    EXPECT_THAT(field.distance.size() == 100 && field.object.size() == 100, testing::Eq(true));
    if(field.distance.size() != 100 || field.object.size() != 100) {
        return;
    }
    std::vector<vec3<float>> nodes;
    for(uint32_t z = 0; z < 4; z++) {
        for(uint32_t y = 0; y < 5; y++) {
            for(uint32_t x = 0; x < 5; x++) {
                nodes.push_back(vec3<float>{-1.0F + static_cast<float>(x) * 0.5F, -1.0F + static_cast<float>(y) * 0.5F, 0.0F + static_cast<float>(z) * 0.25F});
            }
        }
    }
    const std::vector<NearestResult> want = scene->nearest(nodes, 0.45F);
    int same = 0, missed = 0;
    for(size_t i = 0; i < nodes.size(); i++) {
        same += field.distance[i] == want[i].distance && field.object[i] == want[i].object_index ? 1 : 0;
        missed += field.object[i] < 0 ? 1 : 0;
    }
    EXPECT_THAT(same, testing::Eq(100));
    EXPECT_THAT(missed > 10 && missed < 90, testing::Eq(true));
    int thrown = 0;
    for(const std::array<uint32_t, 3> &count : {std::array<uint32_t, 3>{0, 1, 1}, {1, 0, 1}, {1, 1, 0}, {65536, 65536, 1}}) {
        grid.count = count;
        try {
            scene->distanceGrid(grid);
        } catch(const std::invalid_argument &) {
            thrown++;
        }
    }
    EXPECT_THAT(thrown, testing::Eq(4));
}

int main(int argc, char **argv) {
    testing::InitGoogleTest(&argc, argv);
    return RUN_ALL_TESTS();
}
