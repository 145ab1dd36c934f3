// tests/cpp/light_passes_test.cpp -- Scene::lightPasses, Scene::captureLightPasses and mixLightPasses (include/PathTrace/light_passes.h,
// include/pt_light_passes.h) on tests/cpp/gather_test.cpp's scene: a wall, a sphere, two instances of a two-face card and a point light.
// The Scene gives its objects' shared default handler one slot of the material table, and there is one point light: the slot is in group 0,
// the light in group 1 (the Python side describes the same scene without a table: objects without a material are in group 0 as well).  Every pass and every
// mixed value is printed as "RECORD <call> <index> <hex words>" for tests/test_cpp_light_passes.py, which compares them with what the
// Python binding returns for the same scene; the arguments the device would refuse are argument errors.
#include <PathTrace/camera.h>
#include <PathTrace/light_passes.h>
#include <PathTrace/radiance.h>
#include <PathTrace/scene/light.h>
#include <PathTrace/scene/mesh.h>
#include <PathTrace/scene/object.h>
#include <PathTrace/scene/scene.h>
#include <PathTrace/worker.h>

#include <gmock/gmock.h>
#include <gtest/gtest.h>

#include <cstdio>
#include <cstring>
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

    RadianceOptions someOptions() {
        RadianceOptions o;
        o.samples = 65;
        o.base_seed = 47;
        return o;
    }

    // the rays the Python side traces as well: along +z towards the front of the sphere, which the point light reaches, and past its rim
    // onto the wall (the steps are powers of two: the same floats on both sides)
    std::vector<Ray> someRays() {
        std::vector<Ray> rays;
        for(int k = 0; k < 11; k++) {
            Ray r;
            r.origin = vec3<float>{-0.5F + 0.03125F * static_cast<float>(k), -0.5F + 0.015625F * static_cast<float>(k), -1.0F};
            r.dir = vec3<float>{0.0F, 0.0F, 1.0F};
            rays.push_back(r);
        }
        return rays;
    }

    Capture someCapture() {
        Capture c;
        c.model = CaptureModel::fisheye;
        c.width = 5;
        c.height = 5;
        c.lookAt(vec3<float>{0.1F, 0.2F, -1.0F}, vec3<float>{0.0F, 0.0F, 1.0F}, vec3<float>{0.0F, 1.0F, 0.0F});
        c.fov = 2.5F;
        return c;
    }

    LightGroups someGroups() {
        LightGroups g;
        g.n_groups = 2;
        g.split = true;
        g.material_group = {0};
        g.point_light_group = {1};
        return g;
    }

    // one gain per pass, none of them 1
    std::vector<std::array<float, 3>> someGains(size_t n_passes) {
        std::vector<std::array<float, 3>> gains(n_passes);
        for(size_t p = 0; p < n_passes; p++) {
            gains[p] = {0.5F + 0.25F * static_cast<float>(p), 1.5F, 2.0F - 0.125F * static_cast<float>(p)};
        }
        return gains;
    }

    void print(const char *call, size_t index, const float *value, size_t n) {
        std::printf("RECORD %s %zu", call, index);
        for(size_t k = 0; k < n; k++) {
            uint32_t w;
            std::memcpy(&w, value + k, sizeof(w));
            std::printf(" %08x", w);
        }
        std::printf("\n");
    }

    void printAll(const char *name, const LightPasses &passes) {
        const std::string pass = std::string(name) + "_pass", total = std::string(name) + "_total", mix = std::string(name) + "_mix";
        for(size_t i = 0; i < passes.value.size(); i++) {
            print(pass.c_str(), i, passes.value[i].data(), 3);
        }
        for(size_t i = 0; i < passes.total.size(); i++) {
            const Color<float> v = passes.total[i].value;
            const float rgba[4] = {v[0], v[1], v[2], v[3]};
            print(total.c_str(), i, rgba, 4);
        }
        const std::vector<Color<float>> mixed = mixLightPasses(passes, someGains(passes.n_passes));
        for(size_t i = 0; i < mixed.size(); i++) {
            const float rgba[4] = {mixed[i][0], mixed[i][1], mixed[i][2], mixed[i][3]};
            print(mix.c_str(), i, rgba, 4);
        }
    }

} // namespace

TEST(LightPassScene, EveryCallReturnsItsPasses) {
    auto scene = cardScene();
    const LightGroups groups = someGroups();
    EXPECT_THAT(groups.passes(), testing::Eq(6U));
    EXPECT_THAT(groups.pass(1, LightPassComponent::direct), testing::Eq(4U));
    const std::vector<Ray> rays = someRays();
    const LightPasses along = scene->lightPasses(rays, groups, someOptions());
    EXPECT_THAT(along.size() == rays.size() && along.n_passes == 6U && along.total.size() == rays.size() && along.width == 0, testing::Eq(true));
    printAll("rays", along);
    // the point light's group holds the light; the objects emit nothing and a point light is never seen along the ray itself
    bool lit = false;
    for(size_t i = 0; i < along.size(); i++) {
        for(size_t p = 0; p < 4; p++) {
            EXPECT_THAT(along.at(i, p)[0] == 0.0F && along.at(i, p)[1] == 0.0F && along.at(i, p)[2] == 0.0F, testing::Eq(true));
        }
        lit = lit || along.at(i, groups.pass(1, LightPassComponent::direct))[0] > 0.0F;
    }
    EXPECT_THAT(lit, testing::Eq(true));
    const LightPasses image = scene->captureLightPasses(someCapture(), groups, someOptions());
    EXPECT_THAT(image.size() == 25U && image.width == 5 && image.height == 5 && image.total.size() == 25U, testing::Eq(true));
    printAll("capture", image);
    const LightPasses bare = scene->lightPasses(rays, groups, someOptions(), false);
    EXPECT_THAT(bare.total.empty() && bare.value == along.value, testing::Eq(true));
    EXPECT_THAT(mixLightPasses(bare, someGains(6))[0][3], testing::Eq(0.0F));
}

TEST(LightPassScene, RefusedArgumentsAreErrors) {
    auto scene = cardScene();
    int thrown = 0, refused_by_device = 0;
    auto refused = [&](auto call) {
        try {
            call();
        } catch(const std::invalid_argument &) {
            thrown++;
        } catch(const std::runtime_error &) {
            refused_by_device++;
        }
    };
    LightGroups g = someGroups();
    g.n_groups = 9;
    refused([&] { scene->lightPasses(someRays(), g, someOptions()); });
    g = someGroups();
    g.n_groups = 0;
    refused([&] { scene->captureLightPasses(someCapture(), g, someOptions()); });
    g = someGroups();
    g.point_light_group = {2};
    refused([&] { scene->lightPasses(someRays(), g, someOptions()); });
    RadianceOptions o = someOptions();
    o.samples = 0;
    refused([&] { scene->lightPasses(someRays(), someGroups(), o); });
    Capture c = someCapture();
    c.width = 4;
    refused([&] { scene->captureLightPasses(c, someGroups(), someOptions()); });
    LightPasses p;
    p.n_passes = 2;
    p.value.resize(4);
    refused([&] { mixLightPasses(p, someGains(3)); });
    EXPECT_THAT(thrown, testing::Eq(6));
    // tables that do not fit the scene's counts: the device's refusal, under its lock
    g = someGroups();
    g.point_light_group = {1, 1};
    refused([&] { scene->lightPasses(someRays(), g, someOptions()); });
    g = someGroups();
    g.material_group = {};
    refused([&] { scene->captureLightPasses(someCapture(), g, someOptions()); });
    EXPECT_THAT(refused_by_device, testing::Eq(2));
    EXPECT_THAT(scene->lightPasses({}, someGroups(), someOptions()).size(), testing::Eq(0U));
}

int main(int argc, char **argv) {
    testing::InitGoogleTest(&argc, argv);
    return RUN_ALL_TESTS();
}
