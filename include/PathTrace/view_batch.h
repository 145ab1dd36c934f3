// PathTrace/view_batch.h -- processJob for many cameras of one scene at once (an extension of PathTrace/worker.h).
#ifndef PATHTRACE_VIEW_BATCH_H
#define PATHTRACE_VIEW_BATCH_H

#include <PathTrace/camera.h>
#include <PathTrace/image/image.h>
#include <PathTrace/scene/scene.h>
#include <PathTrace/worker.h>

#include <cstdint>
#include <functional>
#include <vector>

// Renders one frame per camera -- a turntable, a camera path, a stereo pair -- with the same options, all in one persistent launch per
// device replica of the scene: small frames rendered one at a time leave most of the device idle.  Image v is bit for bit what processJob
// gives for cameras[v] with $PATHTRACE_SEED = seeds[v]; the seeds are jobSeed() + v, where the base follows $PATHTRACE_SEED or is random
// as in processJob.  With options.allow_bias every view is denoised as processJob denoises its frame, bit for bit, the whole batch in one launch per stage.  `seeds` (may be
// null) receives them.  progress_callback(completed, total) counts the tiles of all views, from the
// calling thread with one replica.  worker_count as in processJob.  Throws std::invalid_argument for an empty camera list or a null
// camera, std::runtime_error if the device fails.
std::vector<Image<>> processViews(
  const Scene &scene, const std::vector<const Camera *> &cameras, const RenderOptions &options,
  const std::function<void(int, int)> &progress_callback = [](int, int) {}, int worker_count = 0, std::vector<std::uint64_t> *seeds = nullptr);

#endif
