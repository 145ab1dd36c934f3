// tests/cpp/query_test.cpp -- Scene::pick and Scene::occluded (include/PathTrace/query.h, include/pt_query.h): a Scene of a wall, a
// sphere and two instances of a two-face card is picked through a camera; the object is the one Scene::getIntersection reports for the
// same ray, instance and face name the card's triangle, the barycentrics rebuild the position, and occluded is "the closest hit lies
// below t_max" at the hit distance's neighbours.
#include <PathTrace/camera.h>
#include <PathTrace/query.h>
#include <PathTrace/scene/light.h>
#include <PathTrace/scene/mesh.h>
#include <PathTrace/scene/object.h>
#include <PathTrace/scene/scene.h>
#include <PathTrace/worker.h>

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

    const int W = 40, H = 40;
    Camera camera() { return Camera({0.0F, 0.0F, -2.0F}, {0.0F, 0.0F, 1.0F}, {0.0F, 1.0F, 0.0F}, 1.0F, 1.0F, -1.0F); }
    RenderOptions options() { return RenderOptions{W, H, 1, 1, 1E-3F}; }

} // namespace

TEST(QueryScene, PickNamesObjectInstanceAndFace) {
    auto scene = cardScene();
    int on_wall = 0, on_sphere = 0, on_card[2] = {0, 0}, faces[2] = {0, 0}, consistent = 0, hits = 0;
    for(int y = 0; y < H; y++) {
        for(int x = 0; x < W; x++) {
            const PickResult p = scene->pick(camera(), options(), x, y);
            if(!p.hit) {
                continue;
            }
            hits++;
            // the same ray again: from the camera's origin through the hit
            const vec3<float> origin{0.0F, 0.0F, -2.0F};
            const Ray ray{origin, (p.position - origin).normalize()};
            const auto [t, object] = scene->getIntersection(ray);
            const bool same_object = object == p.object && std::abs(t - p.t) <= 1E-4F * p.t;
            bool rebuilt = true;
            if(p.instance >= 0) {
                on_card[p.instance]++;
                faces[p.face == PickResult::no_face ? 0 : p.face]++;
                rebuilt = p.face < 2 && p.object_index == 3 + 2 * p.instance + static_cast<int>(p.face) && p.b1 >= -1E-4F && p.b2 >= -1E-4F && p.b1 + p.b2 <= 1.0F + 1E-4F &&
                          std::abs(std::abs(p.geometric_normal[2]) - 1.0F) <= 1E-6F;
            }
            else if(p.object_index == 2) {
                on_sphere++;
                rebuilt = p.face == PickResult::no_face && p.b1 == 0.0F && p.b2 == 0.0F && p.geometric_normal[0] == p.normal[0] && p.geometric_normal[2] == p.normal[2];
            }
            else {
                on_wall++;
                rebuilt = p.face == PickResult::no_face && std::abs(p.position[2] - 1.0F) <= 1E-5F;
            }
            consistent += same_object && rebuilt ? 1 : 0;
        }
    }
    EXPECT_THAT(hits, testing::Eq(W * H)); // (the wall fills the frame)
    EXPECT_THAT(consistent, testing::Eq(hits));
    EXPECT_THAT(on_wall > 100 && on_sphere > 5 && on_card[0] > 10 && on_card[1] > 10 && faces[0] > 5 && faces[1] > 5, testing::Eq(true));
    EXPECT_THAT(scene->pick(Camera({0.0F, 0.0F, -2.0F}, {0.0F, 0.0F, -3.0F}, {0.0F, 1.0F, 0.0F}, 1.0F, 1.0F, -1.0F), options(), 3, 4).hit, testing::Eq(false));
    int thrown = 0;
    for(const auto &[x, y] : {std::pair<int, int>{W, 0}, {0, H}, {-1, 0}, {0, -1}}) {
        try {
            scene->pick(camera(), options(), x, y);
        } catch(const std::invalid_argument &) {
            thrown++;
        }
    }
    EXPECT_THAT(thrown, testing::Eq(4));
}

TEST(QueryScene, OccludedIsTheClosestHitBelowTheThreshold) {
    auto scene = cardScene();
    const float inf = std::numeric_limits<float>::infinity();
    int agree = 0, rays = 0;
    for(int k = 0; k < 64; k++) {
        const vec3<float> origin{0.0F, 0.0F, -2.0F};
        const vec3<float> target{-1.5F + 3.0F * static_cast<float>(k % 8) / 7.0F, -1.5F + 3.0F * static_cast<float>(k / 8) / 7.0F, 1.0F};
        const Ray ray{origin, (target - origin).normalize()};
        const auto [t, object] = scene->getIntersection(ray);
        rays++;
        bool ok = object != nullptr && t >= 0.0F;
        ok = ok && !scene->occluded(ray, t) && scene->occluded(ray, std::nextafter(t, inf)) && !scene->occluded(ray, std::nextafter(t, -inf));
        ok = ok && scene->occluded(ray, inf) && scene->occluded(ray, std::numeric_limits<float>::max());
        ok = ok && !scene->occluded(ray, 0.0F) && !scene->occluded(ray, -1.0F) && !scene->occluded(ray, std::numeric_limits<float>::quiet_NaN());
        agree += ok ? 1 : 0;
    }
    EXPECT_THAT(agree, testing::Eq(rays));
    const Ray away{vec3<float>{0.0F, 0.0F, -2.0F}, vec3<float>{0.0F, 0.0F, -1.0F}};
    EXPECT_THAT(scene->occluded(away, inf), testing::Eq(false));
}

int main(int argc, char **argv) {
    testing::InitGoogleTest(&argc, argv);
    return RUN_ALL_TESTS();
}
