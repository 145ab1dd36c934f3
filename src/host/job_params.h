// job_params.h -- what processJob, FrameRender and processViews (worker.cpp, frame_render.cpp, view_batch.cpp) share: the translation of a FrameRenderJob into the C ABI
// of pt_hip.h, the job's tiles and seed, and the forwarding of progress reports.  Internal to libPathTrace.so.
#ifndef PATHTRACE_HOST_JOB_PARAMS_H
#define PATHTRACE_HOST_JOB_PARAMS_H

#include <PathTrace/worker.h>

#include "../../include/pt_hip.h"

#include <algorithm>
#include <cstdlib>
#include <exception>
#include <functional>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>

namespace pathtrace_host {

    inline pt_camera_params cameraParams(const Camera &camera) {
        const Camera::Parameters &p = camera.parameters();
        if(p.aperture_kind < 0) {
            throw std::invalid_argument("PathTrace: user-defined ApertureSampler classes cannot be rendered on the device");
        }
        pt_camera_params c{};
        for(int k = 0; k < 3; k++) {
            c.origin[k] = p.origin[k];
            c.look_at[k] = p.look_at[k];
            c.up[k] = p.up[k];
        }
        c.focal_length = p.focal_length;
        c.height = p.height;
        c.aspect_ratio = p.aspect_ratio;
        c.aperture_width = p.aperture_width;
        c.aperture_height = p.aperture_height;
        c.aperture_kind = p.aperture_kind;
        c.hex_ratio = p.hex_ratio;
        c.focal_plane_dist = p.focal_plane_dist;
        return c;
    }

    inline pt_options renderOptions(const RenderOptions &o) {
        return pt_options{o.image_width, o.image_height, o.min_sample_count, o.max_sample_count, o.epsilon};
    }

    inline void check(int status, const char *what) {
        if(status != PT_OK) {
            throw std::runtime_error(std::string("PathTrace: ") + what + " failed: " + pt_last_error());
        }
    }

    inline std::vector<pt_tile> jobTiles(int width, int height) {
        std::vector<pt_tile> tiles(pt_job_tiles(width, height, nullptr, 0));
        pt_job_tiles(width, height, tiles.data(), tiles.size());
        return tiles;
    }

    // one random base seed per call, like the reference's std::random_device-seeded workers; $PATHTRACE_SEED pins it
    inline uint64_t jobSeed() {
        if(const char *fixed = std::getenv("PATHTRACE_SEED")) {
            return std::strtoull(fixed, nullptr, 0);
        }
        std::random_device device;
        return (static_cast<uint64_t>(device()) << 32) | device();
    }

    // the seeds of a batch of n views (processViews): view v takes jobSeed() + v, so that processJob with $PATHTRACE_SEED = seeds[v] renders it again
    inline std::vector<uint64_t> viewSeeds(size_t n) {
        const uint64_t base = jobSeed();
        std::vector<uint64_t> seeds(n);
        for(size_t v = 0; v < n; v++) {
            seeds[v] = base + static_cast<uint64_t>(v);
        }
        return seeds;
    }

    // An exception thrown by the progress callback must not cross the C ABI (with several devices it would be thrown on a library thread
    // and end the program): it is kept, the remaining calls are skipped, and it is thrown again once the devices have finished.
    struct ForwardProgress {
        const std::function<void(int, int)> *fn;
        std::exception_ptr failure;

        static void call(int completed, int total, void *user) {
            ForwardProgress *f = static_cast<ForwardProgress *>(user);
            if(f->failure) {
                return;
            }
            try {
                (*f->fn)(completed, total);
            }
            catch(...) {
                f->failure = std::current_exception();
            }
        }
    };

    // the device of a Scene's first replica: Scene::Scene creates it on $PATHTRACE_DEVICE (0 by default), src/host/scene.cpp
    inline int sceneDevice() {
        const char *device_env = std::getenv("PATHTRACE_DEVICE");
        return device_env != nullptr ? std::atoi(device_env) : 0;
    }

    // worker_count (worker.h:83-84; threads in the reference, 0 = as many as the machine has): at most that many of the scene's device
    // replicas take part.  Every device runs one persistent launch, so there is nothing else for the count to choose.
    inline int replicaCount(const std::vector<pt_scene *> &replicas, int worker_count) {
        return worker_count > 0 ? std::min(worker_count, static_cast<int>(replicas.size())) : static_cast<int>(replicas.size());
    }

    // the number of mesh instances of `scene` (src/host/scene.cpp; 0 for a Scene without any)
    size_t sceneInstanceCount(const Scene &scene);

} // namespace pathtrace_host

#endif
