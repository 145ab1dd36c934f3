// tests/cpp/radiance_test.cpp -- Scene::radiance and Scene::capture (include/PathTrace/radiance.h, include/pt_radiance.h) on
// tests/cpp/gather_test.cpp's scene: a wall, a sphere, two instances of a two-face card and a point light.  Every call returns one record
// per ray or one value per pixel, the arguments the device would refuse are argument errors, and every record is printed as
// "RECORD <call> <index> <hex words>" for tests/test_cpp_radiance.py, which compares them with what the Python binding returns for the
// same scene.
#include <PathTrace/camera.h>
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

    RadianceOptions someOptions() {
        RadianceOptions o;
        o.samples = 65;
        o.base_seed = 47;
        return o;
    }

    // the rays the Python side traces as well: from in front of the wall towards it, spread over the cards, the sphere and past the wall's edge
    std::vector<Ray> someRays() {
        std::vector<Ray> rays;
        for(int k = 0; k < 11; k++) {
            Ray r;
            r.origin = vec3<float>{-0.5F + 0.125F * static_cast<float>(k), 0.25F, -1.0F};
            r.dir = vec3<float>{-1.25F + 0.25F * static_cast<float>(k), -0.75F + 0.125F * static_cast<float>(k), 1.0F}; // (not of unit length: taken as it is)
            rays.push_back(r);
        }
        return rays;
    }

    Capture someCapture(CaptureModel model, int width, int height) {
        Capture c;
        c.model = model;
        c.width = width;
        c.height = height;
        c.lookAt(vec3<float>{0.1F, 0.2F, -1.0F}, vec3<float>{0.0F, 0.0F, 1.0F}, vec3<float>{0.0F, 1.0F, 0.0F});
        c.fov = 2.5F;
        c.extent_x = 1.5F;
        c.extent_y = 0.75F;
        return c;
    }

    void print(const char *call, size_t index, const Color<float> &value) {
        uint32_t w[4];
        std::memcpy(w, &value, sizeof(w));
        std::printf("RECORD %s %zu %08x %08x %08x %08x\n", call, index, w[0], w[1], w[2], w[3]);
    }

} // namespace

TEST(RadianceScene, EveryCallReturnsItsRecords) {
    auto scene = cardScene();
    const RadianceOptions o = someOptions();
    const std::vector<Ray> rays = someRays();
    const std::vector<RadianceResult> along = scene->radiance(rays, o);
    EXPECT_THAT(along.size(), testing::Eq(rays.size()));
    for(size_t i = 0; i < along.size(); i++) {
        print("rays", i, along[i].value);
        std::printf("COUNTS rays %zu %u %u %u\n", i, along[i].samples, along[i].missed, along[i].outside);
        EXPECT_THAT(along[i].samples == 65U && (along[i].missed == 0U || along[i].missed == 65U) && along[i].outside == 0U, testing::Eq(true));
    }
    const struct {
        const char *name;
        CaptureModel model;
        int width, height;
    } captures[] = {{"equirect", CaptureModel::equirect, 8, 4}, {"cube", CaptureModel::cube, 18, 3}, {"fisheye", CaptureModel::fisheye, 5, 5}, {"ortho", CaptureModel::ortho, 7, 3}};
    for(const auto &c : captures) {
        const Image<Color<float>> image = scene->capture(someCapture(c.model, c.width, c.height), o);
        EXPECT_THAT(image.getWidth() == c.width && image.getHeight() == c.height, testing::Eq(true));
        for(size_t i = 0; i < image.size(); i++) {
            print(c.name, i, image.data()[i]);
            EXPECT_THAT(image.data()[i][3] >= 0.0F && image.data()[i][3] <= 1.0F, testing::Eq(true));
        }
    }
}

TEST(RadianceScene, RefusedArgumentsAreArgumentErrors) {
    auto scene = cardScene();
    int thrown = 0;
    auto refused = [&](auto call) {
        try {
            call();
        } catch(const std::invalid_argument &) {
            thrown++;
        }
    };
    RadianceOptions o = someOptions();
    o.samples = 0;
    refused([&] { scene->radiance(someRays(), o); });
    o = someOptions();
    o.epsilon = -1.0F;
    refused([&] { scene->capture(someCapture(CaptureModel::equirect, 8, 4), o); });
    o = someOptions();
    refused([&] { scene->capture(someCapture(CaptureModel::equirect, 0, 4), o); });
    refused([&] { scene->capture(someCapture(CaptureModel::cube, 12, 3), o); });
    refused([&] { scene->capture(someCapture(CaptureModel::fisheye, 5, 4), o); });
    Capture c = someCapture(CaptureModel::fisheye, 5, 5);
    c.fov = 7.0F;
    refused([&] { scene->capture(c, o); });
    c = someCapture(CaptureModel::ortho, 7, 3);
    c.extent_y = 0.0F;
    refused([&] { scene->capture(c, o); });
    c = someCapture(CaptureModel::equirect, 8, 4);
    c.up[1] = std::numeric_limits<float>::infinity();
    refused([&] { scene->capture(c, o); });
    c = someCapture(static_cast<CaptureModel>(4), 8, 4);
    refused([&] { scene->capture(c, o); });
    EXPECT_THAT(thrown, testing::Eq(9));
    EXPECT_THAT(scene->radiance({}, someOptions()).size(), testing::Eq(0U));
}

int main(int argc, char **argv) {
    testing::InitGoogleTest(&argc, argv);
    return RUN_ALL_TESTS();
}
