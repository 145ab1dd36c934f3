// tests/cpp/frame_checkpoint_test.cpp -- FrameRender::save / load and ViewBatchRender::save / load (include/PathTrace/frame_render.h,
// view_batch_render.h; include/pt_checkpoint.h) on the GPU: a progressive frame saved after two passes and loaded onto a scene built
// again finishes as processJob's frame with the same $PATHTRACE_SEED bit for bit, as does the frame it was saved from; the same for a
// batch of views; a damaged blob and a blob of the other kind are refused.  Prints one line per check; exit status 0 = every check passed.
#include <PathTrace/camera.h>
#include <PathTrace/frame_render.h>
#include <PathTrace/render_control.h>
#include <PathTrace/scene/light.h>
#include <PathTrace/scene/mesh.h>
#include <PathTrace/scene/object.h>
#include <PathTrace/scene/scene.h>
#include <PathTrace/view_batch.h>
#include <PathTrace/view_batch_render.h>
#include <PathTrace/worker.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <vector>

namespace {

    using Objects = std::vector<std::unique_ptr<Object>>;
    using Lights = std::vector<std::unique_ptr<LightSource>>;

    Scene boxScene() {
        Objects objects;
        Lights lights;
        auto walls = makeBox(vec3<float>{-1.0F, -1.0F, -1.0F}, vec3<float>{1.0F, 1.0F, 1.0F});
        moveObjects(objects, walls);
        auto lamp = makePlane(vec3<float>{-0.25F, 0.99F, -0.25F}, vec3<float>{0.25F, 0.99F, 0.25F});
        auto glow = std::make_shared<ConstantMaterial>(Color<float>(1.0F, 1.0F, 1.0F, 1.0F), 1.0F, Spectrum(Color<float>{1.0F, 1.0F, 1.0F, 1.0F}));
        auto handler = std::make_shared<ConstantMaterialHandler>(glow, std::make_shared<LambertianBRDF>());
        for(auto &t : lamp) {
            t.setMaterialHandler(handler);
        }
        moveObjects(objects, lamp);
        return Scene(std::move(objects), std::move(lights));
    }

    int failures = 0;

    void expect(bool ok, const char *what) {
        std::printf("%s %s\n", ok ? "[ OK ]" : "[FAIL]", what);
        failures += ok ? 0 : 1;
    }

    bool same(const Image<> &a, const Image<> &b) {
        return a.getWidth() == b.getWidth() && a.getHeight() == b.getHeight() &&
               std::memcmp(a.data(), b.data(), a.getWidth() * a.getHeight() * 4 * sizeof(float)) == 0;
    }

    bool same(const std::vector<Image<>> &a, const std::vector<Image<>> &b) {
        bool ok = a.size() == b.size();
        for(size_t v = 0; ok && v < a.size(); v++) {
            ok = same(a[v], b[v]);
        }
        return ok;
    }

    template<typename Render>
    void passes(Render &r, int n) {
        r.setProgressive(8, 1);
        for(int i = 0; i < n; i++) {
            RenderControl control;
            r.render(control);
        }
    }

    template<typename Render>
    bool finish(Render &r) {
        r.setProgressive(0, 0);
        RenderControl control;
        return r.render(control);
    }

    template<typename Load>
    bool refused(Load load) {
        try {
            load();
        } catch(const std::runtime_error &) {
            return true;
        }
        return false;
    }

} // namespace

int main() {
    setenv("PATHTRACE_SEED", "97531", 1);
    Camera camera({0.0F, 0.0F, -3.0F}, {0.0F, 0.0F, 0.0F}, {0.0F, 1.0F, 0.0F}, 1.0F, 1.0F, 1.0F);
    Scene scene = boxScene(), again = boxScene();
    RenderOptions options{96, 64, 32, 32, 1E-3F};
    std::vector<std::uint8_t> frame_blob, batch_blob;
    {
        FrameRenderJob job{camera, scene, options};
        const Image<> full = processJob(job);
        FrameRender frame(job);
        passes(frame, 2);
        frame.save(frame_blob);
        std::vector<std::uint8_t> twice;
        frame.save(twice);
        FrameRender loaded = FrameRender::load(again, frame_blob);
        std::vector<std::uint8_t> resaved;
        loaded.save(resaved);
        const pt_frame_info a = frame.info(), b = loaded.info();
        const bool as_saved = !loaded.complete() && loaded.seed() == frame.seed() && a.streams_parked == b.streams_parked && b.streams_parked == 96 * 64 &&
                              a.samples_carried == b.samples_carried && loaded.progress().passes_completed == 2 && twice == frame_blob && resaved == frame_blob;
        expect(as_saved && finish(loaded) && same(loaded.image(), full) && finish(frame) && same(frame.image(), full),
               "a frame saved after two passes and loaded onto a scene built again: both finish as processJob bit for bit");
    }
    {
        std::vector<Camera> cameras;
        for(int v = 0; v < 3; v++) {
            cameras.emplace_back(vec3<float>{0.1F * static_cast<float>(v), 0.05F * static_cast<float>(v), -3.0F}, vec3<float>{0.0F, 0.0F, 0.0F}, vec3<float>{0.0F, 1.0F, 0.0F},
                                 1.0F, 1.0F, 1.0F);
        }
        std::vector<const Camera *> views;
        for(const Camera &c : cameras) {
            views.push_back(&c);
        }
        RenderOptions small{64, 48, 24, 24, 1E-3F};
        std::vector<std::uint64_t> seeds;
        const std::vector<Image<>> want = processViews(scene, views, small, [](int, int) {}, 0, &seeds);
        ViewBatchRender batch(scene, views, small);
        passes(batch, 1);
        batch.save(batch_blob);
        ViewBatchRender loaded = ViewBatchRender::load(again, batch_blob);
        const bool as_saved = !loaded.complete() && loaded.seeds() == seeds && loaded.viewCount() == 3 && loaded.info().streams_parked == 3 * 64 * 48;
        expect(as_saved && finish(loaded) && same(loaded.images(), want) && finish(batch) && same(batch.images(), want),
               "a batch of three views saved after one pass and loaded: both finish as processViews bit for bit");
    }
    {
        std::vector<std::uint8_t> damaged = frame_blob;
        damaged[damaged.size() / 2] ^= 0x04;
        const bool a = refused([&] { FrameRender::load(again, damaged); });
        const bool b = refused([&] { FrameRender::load(again, batch_blob); });
        const bool c = refused([&] { ViewBatchRender::load(again, frame_blob); });
        const bool d = refused([&] { FrameRender::load(again, std::vector<std::uint8_t>(100, 0)); });
        // ... and nothing of them is left on the scene: it still takes a frame
        FrameRender after = FrameRender::load(again, frame_blob);
        expect(a && b && c && d && !after.complete(), "a damaged blob, a blob of the other kind and a short one are refused");
    }
    return failures == 0 ? 0 : 1;
}
