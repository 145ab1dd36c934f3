"""ctypes binding of libpathtrace_hip.so (include/pt_hip.h), named after the reference's interface.

``Scene``            Scene::Scene / Scene::getIntersection        (reference include/PathTrace/scene/scene.h:32,41)
``process_item``     processItem(WorkItem, RandomEngine&)          (include/PathTrace/worker.h:69)
``process_job``      processJob(FrameRenderJob)                    (include/PathTrace/worker.h:83-84)
``process_job_controlled``  processJob that can be cancelled or given a time budget (include/PathTrace/render_control.h)
``Frame``            a controlled processJob that can be continued: each call resumes where the last one stopped (include/PathTrace/frame_render.h)
                     ``Frame.preview`` shows it between two calls, optionally denoised
``process_views``    processJob for many cameras of one scene in one launch (include/PathTrace/view_batch.h)
``ViewsFrame``       process_views that can be stopped, continued and previewed: a Frame over a view batch (include/PathTrace/view_batch_render.h)
``denoise_views``    denoise for a whole view batch, one launch per stage; ``Scene.render_features_views`` gives its features
``denoise``          feature-guided denoising of a finished frame, what RenderOptions::allow_bias asks for (include/PathTrace/denoise.h);
                     ``Scene.render_features`` gives the features, ``Scene.process_job(..., allow_bias=True)`` does both
``TemporalDenoiser`` the same over a sequence of frames, with the history of the earlier ones reprojected (include/PathTrace/temporal_denoise.h);
                     ``Scene.denoise_sequence`` renders the features and pushes every frame

The library is the only implementation behind these calls: if it is missing or no HIP device is usable they raise.
"""
import ctypes as C
import os

import numpy as np

from . import build as _build
from .scenes import MATERIAL_DTYPE

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PT_LIB_OVERRIDE") or os.path.join(HERE, "libpathtrace_hip.so")  # override: A/B builds of the same ABI

PT_OK = 0
PT_ERR_CANCELLED = 6
ERRORS = {1: "PT_ERR_INVALID", 2: "PT_ERR_NO_DEVICE", 3: "PT_ERR_HIP", 4: "PT_ERR_UNSUPPORTED", 5: "PT_ERR_NOMEM", 6: "PT_ERR_CANCELLED"}

EXPORTS = ["pt_device_count", "pt_last_error", "pt_scene_create", "pt_scene_destroy", "pt_scene_info", "pt_scene_emissive", "pt_scene_bvh_dump", "pt_intersect_batch",
           "pt_render_streams", "pt_render_item", "pt_render_tiles", "pt_render_tiles_progress", "pt_render_tiles_multi", "pt_render_tiles_device", "pt_render_tiles_ctl", "pt_render_cancel", "pt_job_tiles", "pt_pixel_seed", "pt_rng_seed_to_state", "pt_post_process", "pt_post_process_device"]
FRAME_EXPORTS = ["pt_frame_create", "pt_frame_render", "pt_frame_get_info", "pt_frame_destroy"]
PREVIEW_EXPORTS = ["pt_frame_preview"]
EXPORTS += PREVIEW_EXPORTS
EXPORTS += FRAME_EXPORTS
VIEW_EXPORTS = ["pt_render_views", "pt_render_views_device"]
EXPORTS += VIEW_EXPORTS
DENOISE_EXPORTS = ["pt_denoise_params_default", "pt_render_features", "pt_render_features_device", "pt_denoise", "pt_denoise_device"]
EXPORTS += DENOISE_EXPORTS
VIEWS_FRAME_EXPORTS = ["pt_frame_create_views", "pt_render_features_views", "pt_render_features_views_device", "pt_denoise_views", "pt_denoise_views_device"]
EXPORTS += VIEWS_FRAME_EXPORTS
PROGRESSIVE_EXPORTS = ["pt_frame_set_progressive", "pt_frame_get_progress"]
EXPORTS += PROGRESSIVE_EXPORTS
TEMPORAL_EXPORTS = ["pt_temporal_params_default", "pt_temporal_create", "pt_temporal_denoise", "pt_temporal_denoise_device", "pt_temporal_reset",
                    "pt_temporal_destroy"]
EXPORTS += TEMPORAL_EXPORTS
# (EXPORTS is what include/pt_hip.h itself declares; these two are declared in include/pt_frame_noise.h, which it includes)
NOISE_EXPORTS = ["pt_frame_get_noise", "pt_frame_set_noise_target"]
# (... and these in include/pt_frame_variance.h)
VARIANCE_EXPORTS = ["pt_denoise_measured_params_default", "pt_frame_get_variance", "pt_denoise_measured", "pt_denoise_measured_device", "pt_frame_preview_measured"]
# (... and these in include/pt_features.h)
FEATURES_EXPORTS = ["pt_feature_params_default", "pt_render_features_followed", "pt_render_features_followed_device", "pt_render_features_followed_views",
                    "pt_render_features_followed_views_device", "pt_frame_set_feature_params"]
# (... and these in include/pt_mesh.h)
MESH_EXPORTS = ["pt_scene_create_meshes", "pt_mesh_assemble", "pt_scene_instance_ranges", "pt_scene_get_triangles"]
# ... and these in include/pt_pose.h
POSE_EXPORTS = ["pt_scene_pose", "pt_scene_get_pose", "pt_mesh_assemble_batch"]
# ... and these in include/pt_motion.h
MOTION_EXPORTS = ["pt_motion_table", "pt_render_features_motion", "pt_render_features_motion_device", "pt_temporal_denoise_motion", "pt_temporal_denoise_motion_device"]
# ... and these in include/pt_relight.h
RELIGHT_EXPORTS = ["pt_scene_relight", "pt_scene_get_materials", "pt_scene_get_point_lights"]
# ... and these in include/pt_deform.h
DEFORM_EXPORTS = ["pt_scene_bind_skin", "pt_scene_deform", "pt_scene_get_mesh_vertices"]
# ... and these in include/pt_morph.h
MORPH_EXPORTS = ["pt_scene_bind_morphs", "pt_scene_morph", "pt_scene_get_morphs"]
DEFORM_VERTICES, DEFORM_BONES, DEFORM_REST = 0, 1, 2
SKIN_MAX_INFLUENCES = 8
MOTION_STATIC, MOTION_MOVED, MOTION_NONE = 0, 1, 2
# ... and these in include/pt_motion_shapes.h
MOTION_SHAPES_EXPORTS = ["pt_scene_motion_mark", "pt_scene_motion_unmark", "pt_scene_get_motion_mark", "pt_scene_get_triangle_faces", "pt_render_features_motion_marked",
                         "pt_render_features_motion_marked_device"]
MOTION_DEFORMED = 3
# scene queries (include/pt_query.h): hit records for rays, pixels and frames, and occlusion tests
QUERY_EXPORTS = ["pt_query_rays", "pt_query_rays_device", "pt_query_pixels", "pt_query_pixels_device", "pt_query_frame", "pt_query_frame_device", "pt_occluded_rays",
                 "pt_occluded_rays_device"]
QUERY_NO_FACE = 0xFFFFFFFF
# nearest-surface queries (include/pt_nearest.h): the closest point of the scene to free points, and distance grids
NEAREST_EXPORTS = ["pt_nearest_points", "pt_nearest_points_device", "pt_distance_grid_fill", "pt_distance_grid_fill_device"]
NEAREST_FACE, NEAREST_EDGE_AB, NEAREST_EDGE_BC, NEAREST_EDGE_CA, NEAREST_VERTEX_A, NEAREST_VERTEX_B, NEAREST_VERTEX_C, NEAREST_SPHERE = range(8)
# light gathered at points (include/pt_gather.h): occlusion, direct light, full paths
GATHER_EXPORTS = ["pt_gather_params_default", "pt_gather_points", "pt_gather_points_device", "pt_gather_frame", "pt_gather_frame_device", "pt_gather_instance"]
GATHER_OCCLUSION, GATHER_DIRECT, GATHER_PATHS = 0, 1, 2
# light probes (include/pt_light_probes.h): SH radiance at free points, probe grids, the lookup that shades points from a grid
LIGHT_PROBE_EXPORTS = ["pt_light_probe_params_default", "pt_light_probes_points", "pt_light_probes_points_device", "pt_light_probes_grid", "pt_light_probes_shade",
                       "pt_light_probes_shade_device"]
# radiance along free rays and captures (include/pt_radiance.h): per-ray means, and images made by four camera models on the device
RADIANCE_EXPORTS = ["pt_radiance_params_default", "pt_radiance_rays", "pt_radiance_rays_device", "pt_radiance_capture", "pt_radiance_capture_device"]
CAPTURE_EQUIRECT, CAPTURE_CUBE, CAPTURE_FISHEYE, CAPTURE_ORTHO = 0, 1, 2, 3
# light-group passes (include/pt_light_passes.h): the same samples split by emitter group and bounce depth, and the mix of such passes
LIGHT_PASSES_EXPORTS = ["pt_light_passes_count", "pt_light_passes_rays", "pt_light_passes_rays_device", "pt_light_passes_capture", "pt_light_passes_capture_device",
                        "pt_light_passes_mix", "pt_light_passes_mix_device"]
LIGHT_GROUPS_MAX = 8
PASS_EMITTED, PASS_DIRECT, PASS_INDIRECT = 0, 1, 2
# checkpoints of a frame (include/pt_checkpoint.h, which pt_hip.h includes as it includes pt_frame_noise.h)
CHECKPOINT_EXPORTS = ["pt_checkpoint_inspect", "pt_frame_checkpoint_size", "pt_frame_checkpoint_save", "pt_frame_checkpoint_load"]
CHECKPOINT_HEADER_BYTES = 352
CHECKPOINT_FINISHED, CHECKPOINT_UNTOUCHED, CHECKPOINT_RECORD = 0, 1, 2
# pt_hit: 64 bytes.  A miss: t -1, object -1, instance -1, face QUERY_NO_FACE, material NO_MATERIAL, every other float 0
Hit = np.dtype([("t", "<f4"), ("object", "<i4"), ("instance", "<i4"), ("face", "<u4"), ("position", "<f4", 3), ("material", "<u4"), ("normal", "<f4", 3), ("b1", "<f4"),
                ("geometric_normal", "<f4", 3), ("b2", "<f4")])

# pt_nearest: 64 bytes.  A miss: distance and squared_distance +inf, object -1, instance -1, face QUERY_NO_FACE, material NO_MATERIAL,
# every other word 0.  pt_distance_grid: 36 bytes
Nearest = np.dtype([("distance", "<f4"), ("object", "<i4"), ("instance", "<i4"), ("face", "<u4"), ("position", "<f4", 3), ("material", "<u4"),
                    ("geometric_normal", "<f4", 3), ("b1", "<f4"), ("squared_distance", "<f4"), ("feature", "<u4"), ("side", "<i4"), ("b2", "<f4")])
DistanceGrid = np.dtype([("origin", "<f4", 3), ("step", "<f4", 3), ("count", "<u4", 3)])

# pt_gather_result: 32 bytes.  A frame's pixel without a first hit: all zero
GatherResult = np.dtype([("value", "<f4", 4), ("samples", "<u4"), ("occluded", "<u4"), ("pad", "<u4", 2)])

# pt_light_probe: 128 bytes; sh[k][c]: coefficient k (bands 0..2) of colour channel c.  pt_light_probe_grid: 36 bytes
LightProbe = np.dtype([("sh", "<f4", (9, 3)), ("samples", "<u4"), ("missed", "<u4"), ("backfacing", "<u4"), ("pad", "<u4", 2)])
LightProbeGrid = np.dtype([("origin", "<f4", 3), ("step", "<f4", 3), ("count", "<u4", 3)])


class LightProbeParams(C.Structure):
    """pt_light_probe_params"""
    _fields_ = [("samples", C.c_int32), ("epsilon", C.c_float), ("base_seed", C.c_uint64), ("max_backfacing", C.c_float), ("pad", C.c_uint32)]

# pt_radiance_result: 32 bytes; value: the mean radiance and its alpha
RadianceResult = np.dtype([("value", "<f4", 4), ("samples", "<u4"), ("missed", "<u4"), ("outside", "<u4"), ("pad", "<u4")])


class RadianceParams(C.Structure):
    """pt_radiance_params"""
    _fields_ = [("samples", C.c_int32), ("epsilon", C.c_float), ("base_seed", C.c_uint64)]


class CaptureDesc(C.Structure):
    """pt_capture_desc"""
    _fields_ = [("model", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("jitter", C.c_int32), ("origin", C.c_float * 3), ("right", C.c_float * 3), ("up", C.c_float * 3),
                ("forward", C.c_float * 3), ("fov", C.c_float), ("extent", C.c_float * 2), ("pad", C.c_uint32)]


# pt_light_pass: 16 bytes; value: the rgb of one pass
LightPass = np.dtype([("value", "<f4", 3), ("pad", "<u4")])


class LightGroups(C.Structure):
    """pt_light_groups (light_groups makes one and keeps its tables alive)"""
    _fields_ = [("n_groups", C.c_uint32), ("split", C.c_int32), ("material_group", C.c_void_p), ("n_materials", C.c_uint32), ("point_light_group", C.c_void_p),
                ("n_point_lights", C.c_uint32)]

    @property
    def n_passes(self):
        """P = n_groups * (split ? 3 : 1), by pt_light_passes_count"""
        n = C.c_uint32(0)
        _check(load().pt_light_passes_count(C.byref(self), C.byref(n)))
        return int(n.value)


class GatherParams(C.Structure):
    """pt_gather_params"""
    _fields_ = [("kind", C.c_int32), ("samples", C.c_int32), ("epsilon", C.c_float), ("distance", C.c_float), ("base_seed", C.c_uint64)]


class MotionMarkInfo(C.Structure):
    """pt_motion_mark_info"""
    _fields_ = [("n_instances", C.c_uint32), ("n_meshes_copied", C.c_uint32), ("bytes_copied", C.c_uint64), ("allocations", C.c_uint32), ("total_ms", C.c_float)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}




class PtError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("%s: %s" % (ERRORS.get(code, code), message))
        self.code = code


POST_TONE_MAP, POST_GAMMA = 1, 2


def post_process(image, steps=POST_TONE_MAP | POST_GAMMA, gamma=1.8, device=0):
    """toneMap / gammaCorrect / postProcess (post_processing.h:14,22,30) of an (h, w, 4) float32 frame on the GPU; returns a new array."""
    img = np.array(image, dtype=np.float32, order="C", copy=True)
    h, w = img.shape[:2]
    _check(load().pt_post_process(C.c_int(device), _ptr(img), C.c_int32(w), C.c_int32(h), C.c_uint32(steps), C.c_float(gamma)))
    return img


class DenoiseParams(C.Structure):
    """pt_denoise_params: a-trous passes (0..10) and the three edge-stopping sigmas (>= 0; 0 turns a term off)."""
    _fields_ = [("iterations", C.c_int32), ("sigma_luminance", C.c_float), ("sigma_normal", C.c_float), ("sigma_depth", C.c_float)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


def denoise_params_default():
    """The library's default parameters (pt_denoise_params_default) as a dict."""
    p = DenoiseParams()
    _check(load().pt_denoise_params_default(C.byref(p)))
    return p.as_dict()


def _denoise_params(params):
    """None = the library's defaults (a NULL pointer); otherwise a dict whose missing keys take the defaults."""
    if params is None:
        return None
    unknown = set(params) - {k for k, _ in DenoiseParams._fields_}
    if unknown:
        raise ValueError("unknown denoise parameters: %s" % ", ".join(sorted(unknown)))
    p = DenoiseParams()
    _check(load().pt_denoise_params_default(C.byref(p)))
    for k, v in params.items():
        setattr(p, k, v)
    return C.byref(p)


def denoise(image, features, params=None, device=0):
    """Feature-guided denoising (pt_denoise) of an (h, w, 4) float32 frame with the (h, w, 3, 4) features of Scene.render_features for the
    same camera; returns a new array (alpha copied).  params: None = defaults, or a dict of DenoiseParams fields."""
    img = np.ascontiguousarray(image, dtype=np.float32)
    feat = np.ascontiguousarray(features, dtype=np.float32)
    if img.ndim != 3 or img.shape[2] != 4 or feat.shape != img.shape[:2] + (3, 4):
        raise ValueError("image must be (h, w, 4) and features (h, w, 3, 4)")
    out = np.empty_like(img)
    h, w = img.shape[:2]
    _check(load().pt_denoise(C.c_int(device), _ptr(img), _ptr(feat), C.c_int32(w), C.c_int32(h), _denoise_params(params), _ptr(out)))
    return out


def denoise_device(d_rgba_ptr, d_features_ptr, width, height, d_out_ptr, stream_ptr=0, params=None, device=0):
    """pt_denoise_device on device memory (e.g. torch tensors' data_ptr()): rgba and out width*height*4 floats (out may equal rgba), features
    width*height*12 floats; ordered on stream_ptr (0 = the default stream), which is synchronised before the call returns."""
    _check(load().pt_denoise_device(C.c_int(device), C.c_void_p(d_rgba_ptr), C.c_void_p(d_features_ptr), C.c_int32(width), C.c_int32(height),
                                    _denoise_params(params), C.c_void_p(d_out_ptr), C.c_void_p(stream_ptr)))


def denoise_views(images, features, params=None, device=0):
    """denoise for a view batch (pt_denoise_views): (V, h, w, 4) float32 frames with the (V, h, w, 3, 4) features of
    Scene.render_features_views, 3 + iterations launches whatever V is; view v of the result equals denoise(images[v], features[v]) bit for
    bit.  Returns a new array."""
    img = np.ascontiguousarray(images, dtype=np.float32)
    feat = np.ascontiguousarray(features, dtype=np.float32)
    if img.ndim != 4 or img.shape[3] != 4 or feat.shape != img.shape[:3] + (3, 4):
        raise ValueError("images must be (V, h, w, 4) and features (V, h, w, 3, 4)")
    out = np.empty_like(img)
    v, h, w = img.shape[:3]
    _check(load().pt_denoise_views(C.c_int(device), _ptr(img), _ptr(feat), C.c_int32(w), C.c_int32(h), C.c_int32(v), _denoise_params(params), _ptr(out)))
    return out


def denoise_views_device(d_rgba_ptr, d_features_ptr, width, height, n_views, d_out_ptr, stream_ptr=0, params=None, device=0):
    """pt_denoise_views_device on device memory: as denoise_device, every array holding n_views frames."""
    _check(load().pt_denoise_views_device(C.c_int(device), C.c_void_p(d_rgba_ptr), C.c_void_p(d_features_ptr), C.c_int32(width), C.c_int32(height),
                                          C.c_int32(n_views), _denoise_params(params), C.c_void_p(d_out_ptr), C.c_void_p(stream_ptr)))


class FeatureParams(C.Structure):
    """pt_feature_params: how far a followed feature ray goes through mirrors and glass (max_bounces, 0..32); flags must be 0."""
    _fields_ = [("max_bounces", C.c_int32), ("flags", C.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


def feature_params_default():
    """The library's default parameters of the followed features (pt_feature_params_default) as a dict."""
    p = FeatureParams()
    _check(load().pt_feature_params_default(C.byref(p)))
    return p.as_dict()


def _feature_params(params):
    """A FeatureParams as it is; otherwise a dict whose missing keys take the library's defaults."""
    if isinstance(params, FeatureParams):
        return params
    unknown = set(params) - {k for k, _ in FeatureParams._fields_}
    if unknown:
        raise ValueError("unknown feature parameters: %s" % ", ".join(sorted(unknown)))
    p = FeatureParams()
    _check(load().pt_feature_params_default(C.byref(p)))
    for k, v in params.items():
        setattr(p, k, v)
    return p


class DenoiseMeasuredParams(C.Structure):
    """pt_denoise_measured_params: DenoiseParams and the luminance sigma of the pixels whose variance is measured."""
    _fields_ = [("base", DenoiseParams), ("sigma_measured", C.c_float)]

    def as_dict(self):
        d = self.base.as_dict()
        d["sigma_measured"] = self.sigma_measured
        return d


def denoise_measured_params_default():
    """The library's default parameters of the measured form (pt_denoise_measured_params_default) as a flat dict: DenoiseParams' fields
    and sigma_measured."""
    p = DenoiseMeasuredParams()
    _check(load().pt_denoise_measured_params_default(C.byref(p)))
    return p.as_dict()


def _denoise_measured_params(params):
    """None = the library's defaults (a NULL pointer); otherwise a flat dict whose missing keys take the defaults."""
    if params is None:
        return None
    unknown = set(params) - {k for k, _ in DenoiseParams._fields_} - {"sigma_measured"}
    if unknown:
        raise ValueError("unknown denoise parameters: %s" % ", ".join(sorted(unknown)))
    p = DenoiseMeasuredParams()
    _check(load().pt_denoise_measured_params_default(C.byref(p)))
    for k, v in params.items():
        setattr(p if k == "sigma_measured" else p.base, k, v)
    return C.byref(p)


def denoise_measured(image, features, variance, mask=None, params=None, device=0):
    """denoise with a plane of measured variances (pt_denoise_measured): variance (h, w, 4) float32 as Frame.variance() gives it -- the
    variance of the mean of r, g, b and the batch means B; a pixel with B >= 2 filters with that variance and sigma_measured, the others as
    denoise does.  mask: None, or (h, w) int32 sample counts whose zeros are holes, as Frame.preview's.  Returns a new array."""
    img = np.ascontiguousarray(image, dtype=np.float32)
    feat = np.ascontiguousarray(features, dtype=np.float32)
    var = np.ascontiguousarray(variance, dtype=np.float32)
    if img.ndim != 3 or img.shape[2] != 4 or feat.shape != img.shape[:2] + (3, 4) or var.shape != img.shape:
        raise ValueError("image and variance must be (h, w, 4) and features (h, w, 3, 4)")
    m = None
    if mask is not None:
        m = np.ascontiguousarray(mask, dtype=np.int32)
        if m.shape != img.shape[:2]:
            raise ValueError("mask must be (h, w)")
    out = np.empty_like(img)
    h, w = img.shape[:2]
    _check(load().pt_denoise_measured(C.c_int(device), _ptr(img), _ptr(feat), _ptr(var), _ptr(m), C.c_int32(w), C.c_int32(h), _denoise_measured_params(params),
                                      _ptr(out)))
    return out


def denoise_measured_device(d_rgba_ptr, d_features_ptr, d_variance_ptr, width, height, d_out_ptr, d_mask_ptr=0, stream_ptr=0, params=None, device=0):
    """pt_denoise_measured_device on device memory: as denoise_device, with the variance plane (width*height*4 floats) and an optional mask
    (width*height int32, 0 = none)."""
    _check(load().pt_denoise_measured_device(C.c_int(device), C.c_void_p(d_rgba_ptr), C.c_void_p(d_features_ptr), C.c_void_p(d_variance_ptr),
                                             C.c_void_p(d_mask_ptr or None), C.c_int32(width), C.c_int32(height), _denoise_measured_params(params),
                                             C.c_void_p(d_out_ptr), C.c_void_p(stream_ptr)))


class TemporalParams(C.Structure):
    """pt_temporal_params: the spatial filter's DenoiseParams and the temporal step's fields."""
    _fields_ = [("spatial", DenoiseParams), ("alpha_color", C.c_float), ("alpha_moments", C.c_float), ("max_history", C.c_int32),
                ("moments_min_history", C.c_int32), ("sigma_luminance_temporal", C.c_float), ("normal_min", C.c_float),
                ("position_tolerance", C.c_float)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_[1:]}
        d["spatial"] = self.spatial.as_dict()
        return d


def temporal_params_default():
    """The library's default temporal parameters (pt_temporal_params_default) as a dict; "spatial" is a dict of DenoiseParams fields."""
    p = TemporalParams()
    _check(load().pt_temporal_params_default(C.byref(p)))
    return p.as_dict()


def _temporal_params(params):
    """None = the library's defaults (a NULL pointer); otherwise a dict whose missing keys (and missing "spatial" keys) take the defaults."""
    if params is None:
        return None
    unknown = set(params) - {k for k, _ in TemporalParams._fields_}
    if unknown:
        raise ValueError("unknown temporal parameters: %s" % ", ".join(sorted(unknown)))
    p = TemporalParams()
    _check(load().pt_temporal_params_default(C.byref(p)))
    for k, v in params.items():
        if k == "spatial":
            unknown = set(v) - {f for f, _ in DenoiseParams._fields_}
            if unknown:
                raise ValueError("unknown denoise parameters: %s" % ", ".join(sorted(unknown)))
            for f, x in v.items():
                setattr(p.spatial, f, x)
        else:
            setattr(p, k, v)
    return p


class TemporalDenoiser:
    """A pt_temporal handle: denoises the frames of one sequence (one scene, one image size) one push at a time, each with the
    reprojected history of the ones before; a scene posed between the frames is followed through the `motion` of
    Scene.render_features_motion.  params: None = defaults, or a dict of TemporalParams fields."""

    def __init__(self, width, height, params=None, device=0):
        self.width, self.height, self.device = int(width), int(height), device
        p = _temporal_params(params)
        h = C.c_void_p()
        _check(load().pt_temporal_create(C.c_int(device), C.c_int32(self.width), C.c_int32(self.height), C.byref(p) if p is not None else None,
                                         C.byref(h)))
        self._h = h

    def denoise(self, image, features, camera, motion=None):
        """One push: the (h, w, 4) frame, its (h, w, 3, 4) features and its camera (dict).  Returns (out, history): the denoised frame and
        the (h, w) int32 history length of every pixel (0 where no ray hit, 1 where the pixel has no history).  motion: the frame's
        (h, w, 2, 4) motion (Scene.render_features_motion) reprojects where every pixel's surface was at the previous pose
        (pt_temporal_denoise_motion); None = the scene did not move."""
        img = np.ascontiguousarray(image, dtype=np.float32)
        feat = np.ascontiguousarray(features, dtype=np.float32)
        if img.shape != (self.height, self.width, 4) or feat.shape != (self.height, self.width, 3, 4):
            raise ValueError("image must be (%d, %d, 4) and features (%d, %d, 3, 4)" % (self.height, self.width, self.height, self.width))
        out = np.empty_like(img)
        hist = np.empty((self.height, self.width), np.int32)
        cp = _camera(camera)
        if motion is not None:
            mot = np.ascontiguousarray(motion, dtype=np.float32)
            if mot.shape != (self.height, self.width, 2, 4):
                raise ValueError("motion must be (%d, %d, 2, 4)" % (self.height, self.width))
            _check(load().pt_temporal_denoise_motion(self._h, _ptr(img), _ptr(feat), _ptr(mot), C.byref(cp), _ptr(out), _ptr(hist)))
            return out, hist
        _check(load().pt_temporal_denoise(self._h, _ptr(img), _ptr(feat), C.byref(cp), _ptr(out), _ptr(hist)))
        return out, hist

    def denoise_device(self, d_rgba_ptr, d_features_ptr, camera, d_out_ptr, d_history_ptr=0, stream_ptr=0, motion=None):
        """One push on device memory (e.g. torch tensors' data_ptr()): rgba and out h*w*4 floats (out may equal rgba), features h*w*12 floats,
        history h*w int32 (0 = not written); ordered on stream_ptr (0 = the default stream), which is synchronised before the call returns.
        motion: the device address of the frame's h*w*8 floats of motion (None = the scene did not move)."""
        cp = _camera(camera)
        if motion is not None:
            _check(load().pt_temporal_denoise_motion_device(self._h, C.c_void_p(d_rgba_ptr), C.c_void_p(d_features_ptr), C.c_void_p(motion), C.byref(cp),
                                                            C.c_void_p(d_out_ptr), C.c_void_p(d_history_ptr or None), C.c_void_p(stream_ptr)))
            return
        _check(load().pt_temporal_denoise_device(self._h, C.c_void_p(d_rgba_ptr), C.c_void_p(d_features_ptr), C.byref(cp), C.c_void_p(d_out_ptr),
                                                 C.c_void_p(d_history_ptr or None), C.c_void_p(stream_ptr)))

    def reset(self):
        """Forget the history: the next push has none."""
        _check(load().pt_temporal_reset(self._h))

    def close(self):
        if getattr(self, "_h", None):
            load().pt_temporal_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def motion_table(current, previous):
    """pt_motion_table: for n instances with the matrices current and previous ((n, 4, 4) or (n, 16), rows) the way from the current pose
    back to the previous one: (kind (n,) uint8 -- MOTION_STATIC | MOTION_MOVED | MOTION_NONE, back (n, 3, 4), normal (n, 3, 3)).  Host
    arithmetic: needs no device."""
    cur = np.ascontiguousarray(current, dtype=np.float32).reshape(-1, 16)
    prev = np.ascontiguousarray(previous, dtype=np.float32).reshape(-1, 16)
    if cur.shape != prev.shape:
        raise ValueError("motion_table: %d current and %d previous matrices" % (len(cur), len(prev)))
    n = len(cur)
    kind, back, normal = np.zeros(n, np.uint8), np.zeros((n, 3, 4), np.float32), np.zeros((n, 3, 3), np.float32)
    _check(load().pt_motion_table(_ptr(cur), _ptr(prev), C.c_uint32(n), _ptr(kind), _ptr(back), _ptr(normal)))
    return kind, back, normal


class SceneDesc(C.Structure):
    _fields_ = [("n_objects", C.c_uint32), ("obj_kind", C.c_void_p),
                ("n_triangles", C.c_uint32), ("tri_pos", C.c_void_p), ("tri_nrm", C.c_void_p), ("tri_cull", C.c_void_p),
                ("tri_material", C.c_void_p),
                ("n_spheres", C.c_uint32), ("sph", C.c_void_p), ("sph_material", C.c_void_p),
                ("n_materials", C.c_uint32), ("materials", C.c_void_p),
                ("n_point_lights", C.c_uint32), ("light_pos", C.c_void_p), ("light_spectrum", C.c_void_p)]


class MeshData(C.Structure):
    _fields_ = [("n_vertices", C.c_uint32), ("vertices", C.c_void_p), ("n_faces", C.c_uint32), ("faces", C.c_void_p)]


class MeshInstance(C.Structure):
    _fields_ = [("mesh", C.c_uint32), ("transform", C.c_float * 16), ("smooth", C.c_int32), ("cull_backface", C.c_int32), ("material", C.c_uint32)]


def _mesh_data(vertices, faces):
    """pt_mesh_data over (n, 3) float32 vertices and (m, 3) int32 faces; returns it with the arrays it points into."""
    v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
    f = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
    return MeshData(len(v), v.ctypes.data, len(f), f.ctypes.data), (v, f)


def _mesh_instance(mesh=0, transform=None, smooth=True, cull=True, material=0xFFFFFFFF):
    inst = MeshInstance()
    inst.mesh = mesh
    m = np.eye(4, dtype=np.float32) if transform is None else np.asarray(transform, dtype=np.float32).reshape(16)
    inst.transform[:] = [float(x) for x in m.reshape(16)]
    inst.smooth, inst.cull_backface, inst.material = int(bool(smooth)), int(bool(cull)), int(material)
    return inst


def mesh_assemble(vertices, faces, transform=None, smooth=True, capacity=None, device=0, out_pos=None, out_nrm=None):
    """pt_mesh_assemble: one instance of an indexed mesh expanded on the device, as io::loadMesh returns it.  Returns (count, positions,
    normals), each (min(count, capacity), 9); capacity defaults to the number of faces.  out_pos / out_nrm: arrays to write into
    (at least capacity rows); the returned arrays are views of them."""
    md, keep = _mesh_data(vertices, faces)
    capacity = md.n_faces if capacity is None else int(capacity)
    pos = np.zeros((capacity, 9), np.float32) if out_pos is None else out_pos
    nrm = np.zeros((capacity, 9), np.float32) if out_nrm is None else out_nrm
    inst = _mesh_instance(0, transform, smooth)
    n = C.c_uint64()
    _check(load().pt_mesh_assemble(C.c_int(device), C.byref(md), C.byref(inst), C.c_uint64(capacity), _ptr(pos), _ptr(nrm), C.byref(n)))
    del keep
    k = min(n.value, capacity)
    return n.value, pos[:k], nrm[:k]


class PoseInfo(C.Structure):  # pt_pose_info
    _fields_ = [("n_instances", C.c_uint32), ("n_triangles", C.c_uint32), ("assembly_syncs", C.c_uint32), ("assembly_chunks", C.c_uint32),
                ("upload_ms", C.c_float), ("assembly_ms", C.c_float), ("tree_ms", C.c_float), ("rest_ms", C.c_float), ("total_ms", C.c_float)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class Skin(C.Structure):  # pt_skin
    _fields_ = [("mesh", C.c_uint32), ("n_bones", C.c_uint32), ("influences", C.c_uint32), ("bone", C.c_void_p), ("weight", C.c_void_p)]


class MeshDeform(C.Structure):  # pt_mesh_deform
    _fields_ = [("mesh", C.c_uint32), ("kind", C.c_uint32), ("data", C.c_void_p), ("count", C.c_uint32)]


class DeformInfo(C.Structure):  # pt_deform_info
    _fields_ = PoseInfo._fields_ + [("n_meshes_deformed", C.c_uint32), ("n_vertices_skinned", C.c_uint32), ("skin_ms", C.c_float), ("vertex_upload_ms", C.c_float),
                                    ("allocations", C.c_uint32)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class MorphTarget(C.Structure):  # pt_morph_target
    _fields_ = [("n_deltas", C.c_uint32), ("vertex", C.c_void_p), ("delta", C.c_void_p)]


class MorphSet(C.Structure):  # pt_morph_set
    _fields_ = [("mesh", C.c_uint32), ("n_targets", C.c_uint32), ("targets", C.c_void_p)]


class MeshMorph(C.Structure):  # pt_mesh_morph
    _fields_ = [("mesh", C.c_uint32), ("weights", C.c_void_p), ("n_weights", C.c_uint32), ("bones", C.c_void_p), ("n_bones", C.c_uint32)]


class MorphInfo(C.Structure):  # pt_morph_info
    _fields_ = DeformInfo._fields_ + [("n_vertices_morphed", C.c_uint32), ("morph_ms", C.c_float), ("n_entries_read", C.c_uint64)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class Relight(C.Structure):  # pt_relight
    _fields_ = [("materials", C.c_void_p), ("n_materials", C.c_uint32), ("set_point_lights", C.c_int32), ("light_pos", C.c_void_p), ("light_spectrum", C.c_void_p),
                ("n_point_lights", C.c_uint32), ("instances", C.c_void_p), ("instance_material", C.c_void_p), ("n_instance_materials", C.c_uint32)]


class RelightInfo(C.Structure):  # pt_relight_info
    _fields_ = [("n_emissive", C.c_uint32), ("n_object_samples", C.c_uint32), ("n_candidates", C.c_uint32), ("registry_rebuilt", C.c_uint32),
                ("triangles_rewritten", C.c_uint32), ("registry_ms", C.c_float), ("total_ms", C.c_float)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


def mesh_assemble_batch(meshes, instances, capacity=None, device=0, out_pos=None, out_nrm=None):
    """pt_mesh_assemble_batch: every instance of `instances` expanded on the device by one chain of launches, the survivors of instance
    0, 1, ... end to end.  meshes: [(vertices, faces), ...]; instances: [(mesh index, transform, smooth), ...].  Returns (total count,
    per-instance counts, positions, normals), the arrays (min(total, capacity), 9); capacity defaults to the faces of all instances.
    out_pos / out_nrm: arrays to write into (at least capacity rows); the returned arrays are views of them."""
    mesh_keep = [_mesh_data(v, f) for v, f in meshes]
    md = (MeshData * max(len(mesh_keep), 1))(*[m for m, _ in mesh_keep])
    insts = (MeshInstance * max(len(instances), 1))(*[_mesh_instance(m, t, s) for m, t, s in instances])
    if capacity is None:
        capacity = sum(mesh_keep[m][0].n_faces for m, _, _ in instances)
    capacity = int(capacity)
    pos = np.zeros((capacity, 9), np.float32) if out_pos is None else out_pos
    nrm = np.zeros((capacity, 9), np.float32) if out_nrm is None else out_nrm
    counts = np.zeros(len(instances), np.uint32)
    n = C.c_uint64()
    _check(load().pt_mesh_assemble_batch(C.c_int(device), md, C.c_uint32(len(mesh_keep)), insts, C.c_uint32(len(instances)), C.c_uint64(capacity), _ptr(pos), _ptr(nrm),
                                         _ptr(counts), C.byref(n)))
    del mesh_keep
    k = min(n.value, capacity)
    return n.value, counts, pos[:k], nrm[:k]


class CameraParams(C.Structure):
    _fields_ = [("origin", C.c_float * 3), ("look_at", C.c_float * 3), ("up", C.c_float * 3), ("focal_length", C.c_float),
                ("height", C.c_float), ("aspect_ratio", C.c_float), ("aperture_width", C.c_float), ("aperture_height", C.c_float),
                ("aperture_kind", C.c_int32), ("hex_ratio", C.c_float), ("focal_plane_dist", C.c_float)]


class Options(C.Structure):
    _fields_ = [("image_width", C.c_int32), ("image_height", C.c_int32), ("min_sample_count", C.c_int32),
                ("max_sample_count", C.c_int32), ("epsilon", C.c_float)]


class Stats(C.Structure):
    _fields_ = [("samples", C.c_uint64), ("rays_traced", C.c_uint64), ("shadow_rays_traced", C.c_uint64), ("node_visits", C.c_uint64),
                ("leaf_tests", C.c_uint64), ("vertices", C.c_uint64), ("launches", C.c_uint64), ("kernel_ms", C.c_double),
                ("wave_steps", C.c_uint64), ("shading_passes", C.c_uint64), ("wavefronts", C.c_uint64), ("slot_rows", C.c_uint64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class RenderControl(C.Structure):
    """pt_render_control: the stop and the outcome of one controlled render.  cancel() may be called from a progress callback or from any
    other thread while the render runs; a control that was cancelled stays cancelled (use a new one for the next render)."""
    _fields_ = [("budget_ms", C.c_double), ("tile_done", C.c_void_p), ("streams_finished", C.c_uint64), ("streams_abandoned", C.c_uint64),
                ("streams_unclaimed", C.c_uint64), ("drain_ms", C.c_double), ("cancel_requested", C.c_int32)]

    def cancel(self):
        _check(load().pt_render_cancel(C.byref(self)))


class FrameInfo(C.Structure):
    """pt_frame_info: where a resumable frame stands."""
    _fields_ = [("streams_total", C.c_uint64), ("streams_finished", C.c_uint64), ("streams_parked", C.c_uint64), ("streams_untouched", C.c_uint64),
                ("tiles_total", C.c_uint64), ("tiles_done", C.c_uint64), ("samples_carried", C.c_uint64), ("parked_with_candidates", C.c_uint64),
                ("park_bytes", C.c_uint64), ("launches", C.c_int32), ("status", C.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class FrameProgress(C.Structure):
    """pt_frame_progress: where a progressive frame stands."""
    _fields_ = [("quantum", C.c_int32), ("max_passes_per_call", C.c_int32), ("passes_completed", C.c_int32), ("target", C.c_int32),
                ("pass_in_progress", C.c_int32), ("min_samples", C.c_int32), ("max_samples", C.c_int32), ("streams_at_target", C.c_uint64),
                ("samples_lost", C.c_uint64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class FrameNoise(C.Structure):
    """pt_frame_noise: how noisy the unfinished pixels of a frame are."""
    _fields_ = [("target_error", C.c_float), ("floor", C.c_float), ("fraction", C.c_float), ("target_reached", C.c_int32), ("streams_total", C.c_uint64),
                ("streams_finished", C.c_uint64), ("streams_rated", C.c_uint64), ("streams_unrated", C.c_uint64), ("streams_held", C.c_uint64),
                ("max_error", C.c_float), ("histogram", C.c_uint32 * 64)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_}
        d["histogram"] = np.array(self.histogram, np.uint32)
        return NoiseSummary(d)


class CheckpointFingerprint(C.Structure):
    """pt_checkpoint_fingerprint: what a checkpoint remembers of its scene."""
    _fields_ = [("triangles", C.c_uint64), ("spheres", C.c_uint64), ("materials", C.c_uint64), ("point_lights", C.c_uint64), ("emitters", C.c_uint64),
                ("tree_nodes", C.c_uint64), ("root_box", C.c_uint32 * 6)]


class CheckpointInfo(C.Structure):
    """pt_checkpoint_info: what pt_checkpoint_inspect reports of a blob."""
    _fields_ = [("total_bytes", C.c_uint64), ("n_tiles", C.c_uint64), ("n_streams", C.c_uint64), ("streams_finished", C.c_uint64), ("streams_untouched", C.c_uint64),
                ("streams_with_record", C.c_uint64), ("streams_with_candidates", C.c_uint64), ("bytes_header", C.c_uint64), ("bytes_tables", C.c_uint64),
                ("bytes_tiles", C.c_uint64), ("bytes_map", C.c_uint64), ("bytes_pixels", C.c_uint64), ("bytes_records", C.c_uint64), ("samples_lost", C.c_uint64),
                ("fingerprint", CheckpointFingerprint), ("options", Options), ("version", C.c_uint32), ("n_views", C.c_int32), ("quantum", C.c_int32),
                ("max_passes_per_call", C.c_int32), ("passes_completed", C.c_int32), ("target", C.c_int32), ("pass_in_progress", C.c_int32),
                ("noise_target", C.c_float), ("noise_floor", C.c_float), ("noise_fraction", C.c_float), ("follow_features", C.c_int32), ("launches", C.c_int32)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if k not in ("fingerprint", "options")}
        d["options"] = {k: getattr(self.options, k) for k, _ in Options._fields_}
        d["fingerprint"] = {k: getattr(self.fingerprint, k) for k, _ in CheckpointFingerprint._fields_ if k != "root_box"}
        d["fingerprint"]["root_box"] = np.array(self.fingerprint.root_box, np.uint32)
        return d


def _blob(blob_or_path):
    """A checkpoint as a contiguous uint8 array: the bytes of a file, or of anything bytes-like."""
    if isinstance(blob_or_path, (str, os.PathLike)):
        return np.fromfile(blob_or_path, np.uint8)
    return np.ascontiguousarray(np.frombuffer(blob_or_path, np.uint8) if not isinstance(blob_or_path, np.ndarray) else blob_or_path.view(np.uint8).ravel())


def checkpoint_inspect(blob):
    """pt_checkpoint_inspect as a dict: validates a checkpoint (bytes-like, or a path) and says what it holds -- the job's sizes, n_views,
    the streams of each class, the bytes of each section, the mode, the counters and the scene's fingerprint.  Needs no device; raises
    PtError (PT_ERR_INVALID, naming the field) for a blob that is not a valid checkpoint."""
    b = _blob(blob)
    info = CheckpointInfo()
    _check(load().pt_checkpoint_inspect(_ptr(b) if len(b) else None, C.c_size_t(len(b)), C.byref(info)))
    return info.as_dict()


def error_bin(error):
    """The histogram bin of an error (pixel_error_bin, csrc/pt_noise.h): clamp(exponent of the float32 - 127 + 32, 0, 63), so bin 32 is
    [1, 2), zero and the denormals fall in bin 0, 2^31 and everything above in bin 63.  Scalar or array."""
    bits = np.asarray(error, np.float32).view(np.uint32)
    return np.clip(((bits >> np.uint32(23)) & np.uint32(0xff)).astype(np.int32) - 127 + 32, 0, 63)


class NoiseSummary(dict):
    """Frame.noise(): pt_frame_noise as a dict (histogram: 64 counts as a numpy array), with percentile()."""

    def percentile(self, p):
        """An upper bound of the error that p percent (0 < p <= 100) of the rated streams do not exceed, from the histogram: the upper
        edge 2^(bin - 31) of the first bin at which the running count reaches them, or max_error if that is less (0.0 for bin 0 of a
        frame whose max_error is 0, and when nothing is rated)."""
        if not 0 < p <= 100:
            raise ValueError("p must be in (0, 100]")
        hist = np.asarray(self["histogram"], np.uint64)
        rated = int(hist.sum())
        if rated == 0:
            return 0.0
        b = int(np.searchsorted(np.cumsum(hist), max(int(np.ceil(rated * p / 100.0)), 1)))
        return min(float(2.0 ** (b - 31)), float(self["max_error"]))


TILE_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("w", "<i4"), ("h", "<i4")])
STREAM_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("w", "<i4"), ("h", "<i4"), ("rng_state", "<u8")])

_lib = None


def load(build_if_missing=True):
    """Load libpathtrace_hip.so; raises if it cannot be built/loaded (there is no fallback implementation)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        if not build_if_missing:
            raise FileNotFoundError(LIB_PATH + " is missing: run python -c 'import __graft_entry__ as g; g.build()'")
        _build.build()
    lib = C.CDLL(LIB_PATH)
    lib.pt_last_error.restype = C.c_char_p
    lib.pt_job_tiles.restype = C.c_size_t
    lib.pt_pixel_seed.restype = C.c_uint64
    lib.pt_rng_seed_to_state.restype = C.c_uint64
    lib.pt_scene_destroy.restype = None
    _lib = lib
    return lib


def _check(rc):
    if rc != PT_OK:
        raise PtError(rc, load().pt_last_error().decode())


def _ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def device_count():
    return load().pt_device_count()


def seed_to_state(seed):
    return load().pt_rng_seed_to_state(C.c_uint64(seed & 0xFFFFFFFFFFFFFFFF))


def pixel_seed(base_seed, x, y):
    return load().pt_pixel_seed(C.c_uint64(base_seed), C.c_int32(x), C.c_int32(y))


def job_tiles(width, height):
    """The WorkItem list processJob builds (reference src/worker.cpp:398-414)."""
    lib = load()
    n = lib.pt_job_tiles(C.c_int32(width), C.c_int32(height), None, C.c_size_t(0))
    tiles = np.zeros(n, dtype=TILE_DTYPE)
    lib.pt_job_tiles(C.c_int32(width), C.c_int32(height), _ptr(tiles), C.c_size_t(n))
    return tiles


def _camera(cam):
    p = CameraParams()
    p.origin[:] = [float(v) for v in cam["origin"]]
    p.look_at[:] = [float(v) for v in cam["look_at"]]
    p.up[:] = [float(v) for v in cam["up"]]
    p.focal_length, p.height, p.aspect_ratio = cam["focal_length"], cam["height"], cam["aspect_ratio"]
    p.aperture_width, p.aperture_height = cam.get("aperture_width", 0.0), cam.get("aperture_height", 0.0)
    p.aperture_kind, p.hex_ratio = cam.get("aperture_kind", 0), cam.get("hex_ratio", 0.0)
    p.focal_plane_dist = cam.get("focal_plane_dist", 0.0)
    return p


def _options(opt):
    return Options(int(opt["image_width"]), int(opt["image_height"]), int(opt["min_sample_count"]), int(opt["max_sample_count"]),
                   float(opt["epsilon"]))


def gather_params(kind, samples, epsilon, distance=np.inf, base_seed=0):
    return GatherParams(int(kind), int(samples), float(epsilon), float(distance), int(base_seed) & 0xFFFFFFFFFFFFFFFF)


def gather_params_default():
    gp = GatherParams()
    _check(load().pt_gather_params_default(C.byref(gp)))
    return gp


def light_probe_params(samples, epsilon, base_seed=0, max_backfacing=0.25):
    return LightProbeParams(int(samples), float(epsilon), int(base_seed) & 0xFFFFFFFFFFFFFFFF, float(max_backfacing), 0)


def light_probe_params_default():
    lp = LightProbeParams()
    _check(load().pt_light_probe_params_default(C.byref(lp)))
    return lp


def light_probe_grid(origin, step, count):
    """A pt_light_probe_grid as a 0-d array of dtype LightProbeGrid; a grid made by this function passes through unchanged."""
    if isinstance(origin, np.ndarray) and origin.dtype == LightProbeGrid:
        return np.ascontiguousarray(origin).reshape(())
    g = np.zeros((), LightProbeGrid)
    g["origin"], g["step"], g["count"] = np.asarray(origin, np.float32), np.asarray(step, np.float32), np.asarray(count, np.int64)
    return g


def distance_grid(origin, step, count):
    """A pt_distance_grid as a 0-d array of dtype DistanceGrid; a grid made by this function passes through unchanged."""
    if isinstance(origin, np.ndarray) and origin.dtype == DistanceGrid:
        return np.ascontiguousarray(origin).reshape(())
    g = np.zeros((), DistanceGrid)
    g["origin"], g["step"], g["count"] = np.asarray(origin, np.float32), np.asarray(step, np.float32), np.asarray(count, np.int64)
    return g


def radiance_params(samples, epsilon, base_seed=0):
    return RadianceParams(int(samples), float(epsilon), int(base_seed) & 0xFFFFFFFFFFFFFFFF)


def radiance_params_default():
    rp = RadianceParams()
    _check(load().pt_radiance_params_default(C.byref(rp)))
    return rp


def capture_desc(model, width, height, origin, look_at, up, fov=np.pi, extent=(1.0, 1.0), jitter=True):
    """A pt_capture_desc that looks from origin at look_at: the basis is made in numpy float32, forward = normalize(look_at - origin),
    right = normalize(cross(forward, up)), and up re-made as cross(right, forward).  fov: FISHEYE's full angle, radians; extent: ORTHO's
    half width and half height."""
    f32 = np.float32

    def normalize(v):  # (vec3::normalize's arithmetic: the C++ Capture::lookAt makes the same basis, bit for bit)
        total = f32(0.0)
        for x in v:
            total = f32(total + f32(x * x))
        return (v * f32(f32(1.0) / np.sqrt(total))).astype(f32)

    origin = np.asarray(origin, f32).reshape(3)
    forward = normalize((np.asarray(look_at, f32).reshape(3) - origin).astype(f32))
    right = normalize(np.cross(forward, np.asarray(up, f32).reshape(3)).astype(f32))
    true_up = np.cross(right, forward).astype(f32)
    extent = np.asarray(extent, f32).reshape(2)
    return CaptureDesc(int(model), int(width), int(height), int(bool(jitter)), (C.c_float * 3)(*origin), (C.c_float * 3)(*right), (C.c_float * 3)(*true_up), (C.c_float * 3)(*forward),
                       float(f32(fov)), (C.c_float * 2)(*extent), 0)


def light_groups(n_groups, material_group, point_light_group, split=False):
    """A pt_light_groups: the group (0 .. n_groups - 1) of every material of the scene's table and of every point light; split: three
    passes per group (emitted, direct, indirect) instead of one."""
    materials = np.ascontiguousarray(np.asarray(material_group, np.uint8).reshape(-1))
    lights = np.ascontiguousarray(np.asarray(point_light_group, np.uint8).reshape(-1))
    g = LightGroups(int(n_groups), int(split), materials.ctypes.data if len(materials) else None, len(materials), lights.ctypes.data if len(lights) else None, len(lights))
    g._tables = (materials, lights)  # (the struct points into them)
    return g


def mix_light_passes(passes, gains, total=None):
    """pt_light_passes_mix, on the host: passes (..., P) records of dtype LightPass, gains (P, 3), total (...) records of dtype
    RadianceResult or None -> (..., 4) float32: the passes weighed by the gains and added in order; alpha from total, or 0."""
    passes = np.ascontiguousarray(passes, LightPass)
    shape, n_passes = passes.shape[:-1], passes.shape[-1]
    gains = np.ascontiguousarray(np.asarray(gains, np.float32).reshape(n_passes, 3))
    n = int(np.prod(shape, dtype=np.int64))
    if total is not None:
        total = np.ascontiguousarray(total, RadianceResult)
        if total.shape != shape:
            raise ValueError("total must have one record per ray or pixel")
    out = np.zeros(shape + (4,), np.float32)
    _check(load().pt_light_passes_mix(_ptr(passes), C.c_size_t(n), C.c_uint32(n_passes), _ptr(gains), _ptr(total), _ptr(out)))
    return out


def _gather_points(points, normals):
    """(n, 6) float32: position, normal"""
    points = np.asarray(points, np.float32).reshape(-1, 3)
    normals = np.asarray(normals, np.float32).reshape(-1, 3)
    if len(points) != len(normals):
        raise ValueError("as many normals as points")
    return np.ascontiguousarray(np.concatenate([points, normals], axis=1), dtype=np.float32)


class Scene:
    """A scene resident on one MI355X (the reference's Scene: objects + lights + BVH)."""

    def __init__(self, scene, device=0):
        lib = load()
        keep = {
            "obj_kind": np.ascontiguousarray(scene["obj_kind"], dtype=np.uint8),
            "tri_pos": np.ascontiguousarray(scene["tri_pos"], dtype=np.float32).reshape(-1, 9),
            "tri_nrm": None if scene.get("tri_nrm") is None else np.ascontiguousarray(scene["tri_nrm"], dtype=np.float32).reshape(-1, 9),
            "tri_cull": np.ascontiguousarray(scene["tri_cull"], dtype=np.uint8),
            "tri_material": np.ascontiguousarray(scene["tri_material"], dtype=np.uint32),
            "sph": np.ascontiguousarray(scene["sph"], dtype=np.float32).reshape(-1, 4),
            "sph_material": np.ascontiguousarray(scene["sph_material"], dtype=np.uint32),
            "materials": np.ascontiguousarray(scene["materials"], dtype=MATERIAL_DTYPE),
            "light_pos": np.ascontiguousarray(scene["light_pos"], dtype=np.float32).reshape(-1, 3),
            "light_spectrum": np.ascontiguousarray(scene["light_spectrum"], dtype=np.float32).reshape(-1, 4),
        }
        d = SceneDesc()
        d.n_objects, d.obj_kind = len(keep["obj_kind"]), _ptr(keep["obj_kind"])
        d.n_triangles, d.tri_pos, d.tri_nrm = len(keep["tri_pos"]), _ptr(keep["tri_pos"]), _ptr(keep["tri_nrm"])
        d.tri_cull, d.tri_material = _ptr(keep["tri_cull"]), _ptr(keep["tri_material"])
        d.n_spheres, d.sph, d.sph_material = len(keep["sph"]), _ptr(keep["sph"]), _ptr(keep["sph_material"])
        d.n_materials, d.materials = len(keep["materials"]), _ptr(keep["materials"])
        d.n_point_lights, d.light_pos, d.light_spectrum = len(keep["light_pos"]), _ptr(keep["light_pos"]), _ptr(keep["light_spectrum"])
        self.n_objects = self._n_desc_objects = d.n_objects
        self._h = C.c_void_p()
        instances = scene.get("instances") or []
        self.n_instances = len(instances)
        if instances:
            # meshes and instances recorded by SceneBuilder.mesh: assembled on the device behind the objects above
            mesh_keep = [_mesh_data(v, f) for v, f in scene["meshes"]]
            meshes = (MeshData * len(mesh_keep))(*[m for m, _ in mesh_keep])
            insts = (MeshInstance * len(instances))(*[_mesh_instance(i["mesh"], i["transform"], i["smooth"], i["cull"], i["material"]) for i in instances])
            _check(lib.pt_scene_create_meshes(C.c_int(device), C.byref(d), meshes, C.c_uint32(len(mesh_keep)), insts, C.c_uint32(len(instances)), C.byref(self._h)))
            first, count = self._instance_ranges()
            self.n_objects = d.n_objects + int(count.sum())
        else:
            _check(lib.pt_scene_create(C.c_int(device), C.byref(d), C.byref(self._h)))
        self.device = device

    def _instance_ranges(self):
        first, count = np.zeros(self.n_instances, np.uint32), np.zeros(self.n_instances, np.uint32)
        _check(load().pt_scene_instance_ranges(self._h, _ptr(first), _ptr(count)))
        return first, count

    def instance_ranges(self):
        """(first object, number of objects) of every mesh instance: its surviving triangles, in instance order."""
        return self._instance_ranges()

    def pose(self, transforms, instances=None):
        """pt_scene_pose: new matrices ((n, 4, 4) or (n, 16), rows) for the instances named by `instances` (all of them, in order, by
        default).  The scene is then what a new Scene of the same description with these matrices would be, bit for bit; it keeps its
        handle, stream and workspace.  Returns the pt_pose_info as a dict and updates n_objects."""
        m = np.ascontiguousarray(transforms, dtype=np.float32).reshape(-1, 16)
        idx = None if instances is None else np.ascontiguousarray(instances, dtype=np.uint32).reshape(-1)
        if idx is not None and len(idx) != len(m):
            raise ValueError("pose: %d instance indices for %d matrices" % (len(idx), len(m)))
        info = PoseInfo()
        _check(load().pt_scene_pose(self._h, _ptr(idx), C.c_uint32(len(m)), _ptr(m), C.byref(info)))
        self.n_objects = self._n_desc_objects + int(info.n_triangles)
        return info.as_dict()

    def pose_transforms(self):
        """pt_scene_get_pose: the current matrices of all instances, (n_instances, 4, 4)."""
        out = np.zeros((self.n_instances, 4, 4), np.float32)
        _check(load().pt_scene_get_pose(self._h, _ptr(out)))
        return out

    def bind_skin(self, mesh, bones, weights, n_bones=None):
        """pt_scene_bind_skin: a rig for mesh `mesh` of the scene's mesh list: bones (n_vertices, K) indices and weights (n_vertices, K),
        used as given.  n_bones defaults to the largest index + 1; bones=None unbinds.  Every index is checked on the host."""
        skin = Skin()
        skin.mesh = mesh
        if bones is not None:
            b = np.ascontiguousarray(bones, dtype=np.uint32)
            w = np.ascontiguousarray(weights, dtype=np.float32)
            if b.ndim != 2 or b.shape != w.shape:
                raise ValueError("bind_skin: bones and weights must both be (n_vertices, K)")
            skin.n_bones = int(b.max()) + 1 if n_bones is None else int(n_bones)
            skin.influences, skin.bone, skin.weight = b.shape[1], b.ctypes.data, w.ctypes.data
        _check(load().pt_scene_bind_skin(self._h, C.byref(skin)))

    def deform(self, vertices=None, bones=None, rest=(), transforms=None, instances=None):
        """pt_scene_deform: new shapes for meshes, then what pose() does.  vertices: {mesh: (n_vertices, 3)} replaces a mesh's vertices;
        bones: {mesh: (n_bones, 3, 4) or (n_bones, 4, 4) matrices} skins its rest vertices with the rig of bind_skin on the device (of a
        4 x 4 matrix rows 0 .. 2 are used); rest: meshes that go back to the vertices they were created with.  A mesh named more than
        once takes the last of vertices, bones, rest.  transforms / instances: as pose(); None = the pose stays.  All instances of a
        mesh share its shape.  Returns the pt_deform_info as a dict and updates n_objects."""
        entries, keep = [], []
        for mesh, v in (vertices or {}).items():
            a = np.ascontiguousarray(v, dtype=np.float32).reshape(-1, 3)
            backing = a if len(a) > 0 else np.zeros((1, 3), np.float32)
            keep += [a, backing]
            entries.append(MeshDeform(int(mesh), DEFORM_VERTICES, backing.ctypes.data, len(a)))
        for mesh, m in (bones or {}).items():
            a = np.asarray(m, dtype=np.float32)
            if a.ndim == 3 and a.shape[1:] == (4, 4):
                a = a[:, :3, :]
            a = np.ascontiguousarray(a).reshape(-1, 12)
            backing = a if len(a) > 0 else np.zeros((1, 12), np.float32)
            keep += [a, backing]
            entries.append(MeshDeform(int(mesh), DEFORM_BONES, backing.ctypes.data, len(a)))
        for mesh in rest:
            entries.append(MeshDeform(int(mesh), DEFORM_REST, None, 0))
        table = (MeshDeform * max(len(entries), 1))(*entries)
        m = np.zeros((0, 16), np.float32) if transforms is None else np.ascontiguousarray(transforms, dtype=np.float32).reshape(-1, 16)
        idx = None if instances is None else np.ascontiguousarray(instances, dtype=np.uint32).reshape(-1)
        if idx is not None and len(idx) != len(m):
            raise ValueError("deform: %d instance indices for %d matrices" % (len(idx), len(m)))
        info = DeformInfo()
        _check(load().pt_scene_deform(self._h, table, C.c_uint32(len(entries)), _ptr(idx), C.c_uint32(len(m)), _ptr(m) if len(m) > 0 else None, C.byref(info)))
        del keep
        self.n_objects = self._n_desc_objects + int(info.n_triangles)
        return info.as_dict()

    def mesh_vertices(self, mesh):
        """pt_scene_get_mesh_vertices: the vertices the scene's instances of mesh `mesh` are made of at the moment, (n_vertices, 3)."""
        n = C.c_uint32()
        _check(load().pt_scene_get_mesh_vertices(self._h, C.c_uint32(mesh), None, C.byref(n)))
        out = np.zeros((n.value, 3), np.float32)
        _check(load().pt_scene_get_mesh_vertices(self._h, C.c_uint32(mesh), _ptr(out), None))
        return out

    def bind_morphs(self, mesh, targets):
        """pt_scene_bind_morphs: a set of morph targets for mesh `mesh`: targets is a list of (indices or None, deltas) -- sparse, with
        strictly ascending vertex indices and deltas (n, 3), or dense (indices None), with deltas (n_vertices, 3).  None or [] unbinds.
        Every index is checked on the host; the set is uploaded once, vertex-major."""
        ms, keep = MorphSet(), []
        ms.mesh = mesh
        if targets:
            table = (MorphTarget * len(targets))()
            for t, (indices, deltas) in enumerate(targets):
                d = np.ascontiguousarray(deltas, dtype=np.float32).reshape(-1, 3)
                backing = d if len(d) > 0 else np.zeros((1, 3), np.float32)
                keep += [d, backing]
                table[t].n_deltas, table[t].delta = len(d), backing.ctypes.data
                if indices is not None:
                    idx = np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1)
                    if len(idx) != len(d):
                        raise ValueError("bind_morphs: target %d has %d indices for %d deltas" % (t, len(idx), len(d)))
                    backing = idx if len(idx) > 0 else np.zeros(1, np.uint32)
                    keep += [idx, backing]
                    table[t].vertex = backing.ctypes.data
            ms.n_targets, ms.targets = len(targets), C.addressof(table)
        _check(load().pt_scene_bind_morphs(self._h, C.byref(ms)))
        del keep

    def morph(self, weights=None, bones=None, transforms=None, instances=None):
        """pt_scene_morph: weights: {mesh: (n_targets,)} makes a mesh's vertices from its REST vertices and the set of bind_morphs on the
        device; bones: {mesh: (n_bones, 3, 4) or (n_bones, 4, 4) matrices} sends the morphed vertices of a mesh named in `weights`
        through the rig of bind_skin in the same launch.  transforms / instances: as pose(); None = the pose stays.  All instances of a
        mesh share its shape.  Returns the pt_morph_info as a dict and updates n_objects."""
        entries, keep = [], []
        bones = dict(bones or {})
        for mesh, w in (weights or {}).items():
            a = np.ascontiguousarray(w, dtype=np.float32).reshape(-1)
            backing = a if len(a) > 0 else np.zeros(1, np.float32)
            keep += [a, backing]
            entry = MeshMorph(int(mesh), backing.ctypes.data, len(a), None, 0)
            if mesh in bones:
                b = np.asarray(bones.pop(mesh), dtype=np.float32)
                if b.ndim == 3 and b.shape[1:] == (4, 4):
                    b = b[:, :3, :]
                b = np.ascontiguousarray(b).reshape(-1, 12)
                backing = b if len(b) > 0 else np.zeros((1, 12), np.float32)
                keep += [b, backing]
                entry.bones, entry.n_bones = backing.ctypes.data, len(b)
            entries.append(entry)
        if bones:
            raise ValueError("morph: bones for meshes %s without weights" % sorted(bones))
        table = (MeshMorph * max(len(entries), 1))(*entries)
        m = np.zeros((0, 16), np.float32) if transforms is None else np.ascontiguousarray(transforms, dtype=np.float32).reshape(-1, 16)
        idx = None if instances is None else np.ascontiguousarray(instances, dtype=np.uint32).reshape(-1)
        if idx is not None and len(idx) != len(m):
            raise ValueError("morph: %d instance indices for %d matrices" % (len(idx), len(m)))
        info = MorphInfo()
        _check(load().pt_scene_morph(self._h, table, C.c_uint32(len(entries)), _ptr(idx), C.c_uint32(len(m)), _ptr(m) if len(m) > 0 else None, C.byref(info)))
        del keep
        self.n_objects = self._n_desc_objects + int(info.n_triangles)
        return info.as_dict()

    def morphs(self, mesh):
        """pt_scene_get_morphs: (targets, listed (vertex, delta) pairs) of the set bound to mesh `mesh`; (0, 0) for none."""
        n_targets, n_entries = C.c_uint32(), C.c_uint64()
        _check(load().pt_scene_get_morphs(self._h, C.c_uint32(mesh), C.byref(n_targets), C.byref(n_entries)))
        return n_targets.value, n_entries.value

    def relight(self, materials=None, point_lights=None, instance_materials=None):
        """pt_scene_relight: a new look in place.  materials: the whole new table (MATERIAL_DTYPE), None = it stays; point_lights:
        (positions (n, 3), spectra (n, 4)), None = they stay; instance_materials: {instance: material index or 0xFFFFFFFF} or a list of
        such pairs (a repeated instance gets the last).  The tree is not touched; the scene is then what a new Scene of the same geometry
        with this look would be, bit for bit.  Returns the RelightInfo."""
        look, keep = Relight(), []
        if materials is not None:
            m = np.ascontiguousarray(materials, dtype=MATERIAL_DTYPE).reshape(-1)
            backing = m if len(m) > 0 else np.zeros(1, MATERIAL_DTYPE)  # (a NULL pointer would say "the table stays": an empty table has an address too)
            keep += [m, backing]
            look.materials, look.n_materials = backing.ctypes.data, len(m)
        if point_lights is not None:
            pos = np.ascontiguousarray(point_lights[0], dtype=np.float32).reshape(-1, 3)
            spectrum = np.ascontiguousarray(point_lights[1], dtype=np.float32).reshape(-1, 4)
            if len(pos) != len(spectrum):
                raise ValueError("relight: %d light positions for %d spectra" % (len(pos), len(spectrum)))
            keep += [pos, spectrum]
            look.set_point_lights, look.light_pos, look.light_spectrum, look.n_point_lights = 1, pos.ctypes.data, spectrum.ctypes.data, len(pos)
        if instance_materials is not None:
            pairs = list(instance_materials.items()) if isinstance(instance_materials, dict) else list(instance_materials)
            idx = np.array([p[0] for p in pairs], dtype=np.uint32)
            mat = np.array([p[1] for p in pairs], dtype=np.uint32)
            keep += [idx, mat]
            look.instances, look.instance_material, look.n_instance_materials = idx.ctypes.data, mat.ctypes.data, len(idx)
        info = RelightInfo()
        _check(load().pt_scene_relight(self._h, C.byref(look), C.byref(info)))
        del keep
        return info

    def materials(self):
        """pt_scene_get_materials: the current material table (MATERIAL_DTYPE)."""
        n = C.c_uint32()
        _check(load().pt_scene_get_materials(self._h, None, C.c_uint32(0), C.byref(n)))
        out = np.zeros(n.value, MATERIAL_DTYPE)
        _check(load().pt_scene_get_materials(self._h, _ptr(out), C.c_uint32(n.value), None))
        return out

    def point_lights(self):
        """pt_scene_get_point_lights: (positions (n, 3), spectra (n, 4))."""
        n = C.c_uint32()
        _check(load().pt_scene_get_point_lights(self._h, None, None, C.c_uint32(0), C.byref(n)))
        pos, spectrum = np.zeros((n.value, 3), np.float32), np.zeros((n.value, 4), np.float32)
        _check(load().pt_scene_get_point_lights(self._h, _ptr(pos), _ptr(spectrum), C.c_uint32(n.value), None))
        return pos, spectrum

    def triangles(self, first, count):
        """pt_scene_get_triangles: the triangle objects first .. first + count - 1 of a scene with mesh instances, as the builder took
        them: positions (count, 9), normals (count, 9), cull flags, materials."""
        pos, nrm = np.zeros((count, 9), np.float32), np.zeros((count, 9), np.float32)
        cull, mat = np.zeros(count, np.uint8), np.zeros(count, np.uint32)
        _check(load().pt_scene_get_triangles(self._h, C.c_uint32(first), C.c_uint32(count), _ptr(pos), _ptr(nrm), _ptr(cull), _ptr(mat)))
        return pos, nrm, cull, mat

    def close(self):
        if getattr(self, "_h", None):
            load().pt_scene_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self):
        n, depth, ne = C.c_uint64(), C.c_uint32(), C.c_uint32()
        _check(load().pt_scene_info(self._h, C.byref(n), C.byref(depth), C.byref(ne)))
        return {"n_nodes": n.value, "depth": depth.value, "n_emissive": ne.value}

    def emissive(self):
        """Emissive objects in Scene::registerEmissiveObjects order (scene.cpp:183-208) and their normalised CDF."""
        n = self.info()["n_emissive"]
        obj, cdf = np.empty(max(n, 1), np.int32), np.empty(max(n, 1), np.float32)
        written = C.c_uint64()
        _check(load().pt_scene_emissive(self._h, _ptr(obj), _ptr(cdf), C.c_uint64(n), C.byref(written)))
        return obj[:n], cdf[:n]

    def bvh_dump(self):
        n = max(2 * self.n_objects - 1, 1)
        obj, box = np.empty(n, np.int32), np.empty((n, 6), np.float32)
        written = C.c_uint64()
        _check(load().pt_scene_bvh_dump(self._h, _ptr(obj), _ptr(box), C.c_uint64(n), C.byref(written)))
        return obj[:written.value], box[:written.value]

    def get_intersection(self, rays):
        """Scene::getIntersection for a batch: rays (n, 6) -> (t, object index or -1)."""
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
        t, obj = np.empty(len(rays), np.float32), np.empty(len(rays), np.int32)
        _check(load().pt_intersect_batch(self._h, _ptr(rays), C.c_size_t(len(rays)), _ptr(t), _ptr(obj)))
        return t, obj

    def query(self, rays):
        """pt_query_rays: rays (n, 6) -> (n,) records of dtype Hit: what get_intersection reports (t, object, bit for bit) and the hit's
        instance, mesh face, position, material, shading and geometric normal and barycentrics."""
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
        out = np.zeros(len(rays), Hit)
        _check(load().pt_query_rays(self._h, _ptr(rays), C.c_size_t(len(rays)), _ptr(out)))
        return out

    def query_device(self, d_rays_ptr, n, d_out_ptr, stream_ptr=0):
        """pt_query_rays_device: n rays (6 floats each) and n records (64 bytes each) in device memory, ordered on stream_ptr."""
        _check(load().pt_query_rays_device(self._h, C.c_void_p(d_rays_ptr), C.c_size_t(n), C.c_void_p(d_out_ptr), C.c_void_p(stream_ptr)))

    def occluded(self, rays, t_max):
        """pt_occluded_rays: rays (n, 6) and t_max (n,) or a scalar -> (n,) bool: whether the closest hit of ray i has 0 <= t < t_max[i].
        The walk ends at the first such hit it meets; +inf asks whether the ray hits anything, a NaN or negative t_max gives False."""
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
        seg = np.empty((len(rays), 7), np.float32)
        seg[:, :6], seg[:, 6] = rays, np.asarray(t_max, np.float32)
        out = np.zeros(len(rays), np.uint8)
        _check(load().pt_occluded_rays(self._h, _ptr(seg), C.c_size_t(len(seg)), _ptr(out)))
        return out.astype(bool)

    def occluded_device(self, d_segments_ptr, n, d_out_ptr, stream_ptr=0):
        """pt_occluded_rays_device: n segments (origin, direction, t_max: 7 floats) and n bytes in device memory, ordered on stream_ptr."""
        _check(load().pt_occluded_rays_device(self._h, C.c_void_p(d_segments_ptr), C.c_size_t(n), C.c_void_p(d_out_ptr), C.c_void_p(stream_ptr)))

    def pick(self, camera, options, pixels):
        """pt_query_pixels: pixels (n, 2) of (x, y) -> (n,) records of dtype Hit for the rays through the pixels' centres (no aperture, no
        jitter: a pure function of camera and pixel).  A pixel outside the frame is refused."""
        xy = np.ascontiguousarray(pixels, dtype=np.int32).reshape(-1, 2)
        out = np.zeros(len(xy), Hit)
        cp, op = _camera(camera), _options(options)
        _check(load().pt_query_pixels(self._h, C.byref(cp), C.byref(op), _ptr(xy), C.c_size_t(len(xy)), _ptr(out)))
        return out

    def pick_device(self, camera, options, d_pixels_ptr, n, d_out_ptr, stream_ptr=0):
        """pt_query_pixels_device: n pixels (two int32 each) and n records in device memory, ordered on stream_ptr."""
        cp, op = _camera(camera), _options(options)
        _check(load().pt_query_pixels_device(self._h, C.byref(cp), C.byref(op), C.c_void_p(d_pixels_ptr), C.c_size_t(n), C.c_void_p(d_out_ptr), C.c_void_p(stream_ptr)))

    def id_map(self, camera, options):
        """pt_query_frame: the record of every pixel's centre ray, an (H, W) array of dtype Hit: the frame's object, instance, face and
        attribute map."""
        out = np.zeros((options["image_height"], options["image_width"]), Hit)
        cp, op = _camera(camera), _options(options)
        _check(load().pt_query_frame(self._h, C.byref(cp), C.byref(op), _ptr(out)))
        return out

    def id_map_device(self, camera, options, d_out_ptr, stream_ptr=0):
        """pt_query_frame_device: H*W records in device memory, ordered on stream_ptr."""
        cp, op = _camera(camera), _options(options)
        _check(load().pt_query_frame_device(self._h, C.byref(cp), C.byref(op), C.c_void_p(d_out_ptr), C.c_void_p(stream_ptr)))

    def nearest(self, points, max_distance=np.inf):
        """pt_nearest_points: the closest point of the scene's surfaces to each point (n, 3) within max_distance (a scalar or (n,)):
        (n,) records of dtype Nearest -- distance, object, instance, face, position, barycentrics, the feature (NEAREST_*) and the side
        of that primitive.  A miss has distance +inf and object -1."""
        pts = np.asarray(points, np.float32).reshape(-1, 3)
        q = np.empty((len(pts), 4), np.float32)
        q[:, :3], q[:, 3] = pts, np.asarray(max_distance, np.float32)
        out = np.zeros(len(q), Nearest)
        _check(load().pt_nearest_points(self._h, _ptr(q), C.c_size_t(len(q)), _ptr(out)))
        return out

    def nearest_device(self, d_points_ptr, n, d_out_ptr, stream_ptr=0):
        """pt_nearest_points_device: n queries (xyz, max_distance: 4 floats each) and n records (64 bytes each) in device memory,
        ordered on stream_ptr."""
        _check(load().pt_nearest_points_device(self._h, C.c_void_p(d_points_ptr), C.c_size_t(n), C.c_void_p(d_out_ptr), C.c_void_p(stream_ptr)))

    def distance_grid(self, origin, step, count, max_distance=np.inf, want_object=True):
        """pt_distance_grid_fill: the unsigned distance to the nearest surface at origin + i * step, count = (nx, ny, nz): (distance
        (nz, ny, nx) float32, +inf where nothing lies within max_distance; object (nz, ny, nx) int32, -1 there -- None without
        want_object).  The positions are made on the device."""
        grid = distance_grid(origin, step, count)
        nx, ny, nz = (int(c) for c in grid["count"])
        distance = np.zeros((nz, ny, nx), np.float32)
        obj = np.zeros((nz, ny, nx), np.int32) if want_object else None
        _check(load().pt_distance_grid_fill(self._h, _ptr(grid), C.c_float(max_distance), _ptr(distance), _ptr(obj)))
        return distance, obj

    def distance_grid_device(self, grid, d_distance_ptr, d_object_ptr=0, max_distance=np.inf, stream_ptr=0):
        """pt_distance_grid_fill_device: nx * ny * nz floats and (d_object_ptr not 0) as many int32 in device memory, ordered on stream_ptr."""
        grid = distance_grid(grid, None, None)
        _check(load().pt_distance_grid_fill_device(self._h, _ptr(grid), C.c_float(max_distance), C.c_void_p(d_distance_ptr), C.c_void_p(d_object_ptr or None),
                                                   C.c_void_p(stream_ptr)))

    def gather(self, points, normals, kind, samples, epsilon, distance=np.inf, base_seed=0):
        """pt_gather_points: the light that arrives at the points (n, 3) with the unit normals (n, 3), `samples` samples each, as (n,)
        records of dtype GatherResult.  kind: GATHER_OCCLUSION (the share of cosine-distributed rays that meet nothing within
        `distance`), GATHER_DIRECT (the light samples of one vertex) or GATHER_PATHS (whole paths from the point)."""
        pts = _gather_points(points, normals)
        out = np.zeros(len(pts), GatherResult)
        gp = gather_params(kind, samples, epsilon, distance, base_seed)
        _check(load().pt_gather_points(self._h, _ptr(pts), C.c_size_t(len(pts)), C.byref(gp), _ptr(out)))
        return out

    def gather_device(self, d_points_ptr, n, d_out_ptr, kind, samples, epsilon, distance=np.inf, base_seed=0, stream_ptr=0):
        """pt_gather_points_device: n points (6 floats each) and n records (32 bytes each) in device memory, ordered on stream_ptr."""
        gp = gather_params(kind, samples, epsilon, distance, base_seed)
        _check(load().pt_gather_points_device(self._h, C.c_void_p(d_points_ptr), C.c_size_t(n), C.byref(gp), C.c_void_p(d_out_ptr), C.c_void_p(stream_ptr)))

    def gather_frame(self, camera, options, kind, samples, epsilon, distance=np.inf, base_seed=0):
        """pt_gather_frame: the gather at the first hit of every pixel's centre ray, the normal turned against the ray: an (H, W) array of
        dtype GatherResult; all zero where the ray hits nothing."""
        out = np.zeros((options["image_height"], options["image_width"]), GatherResult)
        cp, op, gp = _camera(camera), _options(options), gather_params(kind, samples, epsilon, distance, base_seed)
        _check(load().pt_gather_frame(self._h, C.byref(cp), C.byref(op), C.byref(gp), _ptr(out)))
        return out

    def gather_frame_device(self, camera, options, d_out_ptr, kind, samples, epsilon, distance=np.inf, base_seed=0, stream_ptr=0):
        """pt_gather_frame_device: H*W records in device memory, ordered on stream_ptr."""
        cp, op, gp = _camera(camera), _options(options), gather_params(kind, samples, epsilon, distance, base_seed)
        _check(load().pt_gather_frame_device(self._h, C.byref(cp), C.byref(op), C.byref(gp), C.c_void_p(d_out_ptr), C.c_void_p(stream_ptr)))

    def bake_instance(self, instance, kind, samples, epsilon, distance=np.inf, base_seed=0):
        """pt_gather_instance: the gather at the three corners of every surviving triangle of a mesh instance, with the corner normals:
        an (n, 3) array of dtype GatherResult, n the instance's object count (instance_ranges)."""
        _, count = self.instance_ranges()
        if not 0 <= instance < len(count):
            raise PtError(1, "instance %d out of range: the scene has %d" % (instance, len(count)))
        out = np.zeros((int(count[instance]), 3), GatherResult)
        gp = gather_params(kind, samples, epsilon, distance, base_seed)
        _check(load().pt_gather_instance(self._h, C.c_uint32(instance), C.byref(gp), _ptr(out)))
        return out

    def light_probes(self, positions, samples, epsilon, base_seed=0):
        """pt_light_probes_points: the radiance that arrives at the free points (n, 3) from every direction, `samples` samples each,
        projected onto SH bands 0..2: (n,) records of dtype LightProbe."""
        pos = np.ascontiguousarray(np.asarray(positions, np.float32).reshape(-1, 3))
        out = np.zeros(len(pos), LightProbe)
        lp = light_probe_params(samples, epsilon, base_seed)
        _check(load().pt_light_probes_points(self._h, _ptr(pos), C.c_size_t(len(pos)), C.byref(lp), _ptr(out)))
        return out

    def light_probes_device(self, d_positions_ptr, n, d_out_ptr, samples, epsilon, base_seed=0, stream_ptr=0):
        """pt_light_probes_points_device: n positions (3 floats each) and n records (128 bytes each) in device memory, ordered on stream_ptr."""
        lp = light_probe_params(samples, epsilon, base_seed)
        _check(load().pt_light_probes_points_device(self._h, C.c_void_p(d_positions_ptr), C.c_size_t(n), C.byref(lp), C.c_void_p(d_out_ptr), C.c_void_p(stream_ptr)))

    def light_probe_grid(self, origin, step, count, samples=256, epsilon=1e-3, base_seed=0):
        """pt_light_probes_grid: the light probes at origin + i * step, count = (nx, ny, nz): (grid, records (nz, ny, nx) of dtype
        LightProbe); the grid is what shade_with_light_probes takes.  The positions are made on the device."""
        grid = light_probe_grid(origin, step, count)
        nx, ny, nz = (int(c) for c in grid["count"])
        out = np.zeros((nz, ny, nx), LightProbe)
        lp = light_probe_params(samples, epsilon, base_seed)
        _check(load().pt_light_probes_grid(self._h, _ptr(grid), C.byref(lp), _ptr(out)))
        return grid, out

    def shade_with_light_probes(self, grid, probes, points, normals, max_backfacing=0.25):
        """pt_light_probes_shade: what a white Lambertian receiver at each point (n, 3) that faces its normal (n, 3) sends out under the
        grid's probes, blended from the eight probes around it: (n, 4) float32, rgb and the sum of the blend weights (0: no probe counted)."""
        grid = light_probe_grid(grid, None, None)
        probes = np.ascontiguousarray(probes, dtype=LightProbe).reshape(-1)
        if len(probes) != int(np.prod(grid["count"].astype(np.int64))):
            raise ValueError("as many probes as the grid has nodes")
        pts = _gather_points(points, normals)
        out = np.zeros((len(pts), 4), np.float32)
        lp = light_probe_params(1, 0.0, 0, max_backfacing)
        _check(load().pt_light_probes_shade(self._h, _ptr(grid), _ptr(probes), C.byref(lp), _ptr(pts), C.c_size_t(len(pts)), _ptr(out)))
        return out

    def shade_with_light_probes_device(self, grid, d_probes_ptr, d_points_ptr, n, d_out_ptr, max_backfacing=0.25, stream_ptr=0):
        """pt_light_probes_shade_device: the grid's records, n points (6 floats each) and n results (4 floats each) in device memory."""
        grid = light_probe_grid(grid, None, None)
        lp = light_probe_params(1, 0.0, 0, max_backfacing)
        _check(load().pt_light_probes_shade_device(self._h, _ptr(grid), C.c_void_p(d_probes_ptr), C.byref(lp), C.c_void_p(d_points_ptr), C.c_size_t(n), C.c_void_p(d_out_ptr),
                                                   C.c_void_p(stream_ptr)))

    def radiance(self, rays, samples=64, epsilon=1e-3, base_seed=0):
        """pt_radiance_rays: the radiance that arrives along each ray (n, 6) -- origin, direction as given --, the mean of `samples`
        paths: (n,) records of dtype RadianceResult."""
        rays = np.ascontiguousarray(np.asarray(rays, np.float32).reshape(-1, 6))
        out = np.zeros(len(rays), RadianceResult)
        rp = radiance_params(samples, epsilon, base_seed)
        _check(load().pt_radiance_rays(self._h, _ptr(rays), C.c_size_t(len(rays)), C.byref(rp), _ptr(out)))
        return out

    def radiance_device(self, d_rays_ptr, n, d_out_ptr, samples=64, epsilon=1e-3, base_seed=0, stream_ptr=0):
        """pt_radiance_rays_device: n rays (6 floats each) and n records (32 bytes each) in device memory, ordered on stream_ptr."""
        rp = radiance_params(samples, epsilon, base_seed)
        _check(load().pt_radiance_rays_device(self._h, C.c_void_p(d_rays_ptr), C.c_size_t(n), C.byref(rp), C.c_void_p(d_out_ptr), C.c_void_p(stream_ptr)))

    def capture(self, desc, samples=64, epsilon=1e-3, base_seed=0):
        """pt_radiance_capture: the image of a CaptureDesc (capture_desc makes one), rays made on the device: (height, width) records of
        dtype RadianceResult."""
        out = np.zeros((max(int(desc.height), 0), max(int(desc.width), 0)), RadianceResult)
        rp = radiance_params(samples, epsilon, base_seed)
        _check(load().pt_radiance_capture(self._h, C.byref(desc), C.byref(rp), _ptr(out)))
        return out

    def capture_device(self, desc, d_out_ptr, samples=64, epsilon=1e-3, base_seed=0, stream_ptr=0):
        """pt_radiance_capture_device: height * width records (32 bytes each) in device memory, ordered on stream_ptr."""
        rp = radiance_params(samples, epsilon, base_seed)
        _check(load().pt_radiance_capture_device(self._h, C.byref(desc), C.byref(rp), C.c_void_p(d_out_ptr), C.c_void_p(stream_ptr)))

    def light_passes(self, rays, groups, samples=64, epsilon=1e-3, base_seed=0, want_total=True):
        """pt_light_passes_rays: radiance()'s samples split by emitter group and bounce depth (groups: light_groups makes one):
        (passes (n, P) records of dtype LightPass, total (n,) records of dtype RadianceResult -- radiance()'s own, bit for bit -- or None)."""
        rays = np.ascontiguousarray(np.asarray(rays, np.float32).reshape(-1, 6))
        passes = np.zeros((len(rays), groups.n_passes), LightPass)
        total = np.zeros(len(rays), RadianceResult) if want_total else None
        rp = radiance_params(samples, epsilon, base_seed)
        _check(load().pt_light_passes_rays(self._h, _ptr(rays), C.c_size_t(len(rays)), C.byref(groups), C.byref(rp), _ptr(passes), _ptr(total)))
        return passes, total

    def light_passes_device(self, d_rays_ptr, n, groups, d_passes_ptr, d_total_ptr=0, samples=64, epsilon=1e-3, base_seed=0, stream_ptr=0):
        """pt_light_passes_rays_device: n rays, n * P pass records (16 bytes each) and, unless d_total_ptr is 0, n records (32 bytes each)
        in device memory, ordered on stream_ptr."""
        rp = radiance_params(samples, epsilon, base_seed)
        _check(load().pt_light_passes_rays_device(self._h, C.c_void_p(d_rays_ptr), C.c_size_t(n), C.byref(groups), C.byref(rp), C.c_void_p(d_passes_ptr), C.c_void_p(d_total_ptr),
                                                  C.c_void_p(stream_ptr)))

    def capture_light_passes(self, desc, groups, samples=64, epsilon=1e-3, base_seed=0, want_total=True):
        """pt_light_passes_capture: capture()'s samples split the same way: (passes (height, width, P), total (height, width) or None)."""
        shape = (max(int(desc.height), 0), max(int(desc.width), 0))
        passes = np.zeros(shape + (groups.n_passes,), LightPass)
        total = np.zeros(shape, RadianceResult) if want_total else None
        rp = radiance_params(samples, epsilon, base_seed)
        _check(load().pt_light_passes_capture(self._h, C.byref(desc), C.byref(groups), C.byref(rp), _ptr(passes), _ptr(total)))
        return passes, total

    def capture_light_passes_device(self, desc, groups, d_passes_ptr, d_total_ptr=0, samples=64, epsilon=1e-3, base_seed=0, stream_ptr=0):
        """pt_light_passes_capture_device: height * width * P pass records and, unless d_total_ptr is 0, height * width records in device
        memory, ordered on stream_ptr."""
        rp = radiance_params(samples, epsilon, base_seed)
        _check(load().pt_light_passes_capture_device(self._h, C.byref(desc), C.byref(groups), C.byref(rp), C.c_void_p(d_passes_ptr), C.c_void_p(d_total_ptr), C.c_void_p(stream_ptr)))

    def mix_light_passes_device(self, d_passes_ptr, n, n_passes, d_gains_ptr, d_out_ptr, d_total_ptr=0, stream_ptr=0):
        """pt_light_passes_mix_device: n * n_passes pass records, n_passes * 3 gains, n * 4 floats out and, unless d_total_ptr is 0, n
        records in device memory, one thread per ray or pixel on this scene's device, ordered on stream_ptr."""
        _check(load().pt_light_passes_mix_device(self._h, C.c_void_p(d_passes_ptr), C.c_size_t(n), C.c_uint32(n_passes), C.c_void_p(d_gains_ptr), C.c_void_p(d_total_ptr),
                                                 C.c_void_p(d_out_ptr), C.c_void_p(stream_ptr)))

    def process_item(self, camera, options, streams, image=None, want_stats=False):
        """processItem for many WorkItems at once; streams: array of STREAM_DTYPE (rect + raw engine state)."""
        streams = np.ascontiguousarray(streams, dtype=STREAM_DTYPE)
        if image is None:
            image = np.zeros((options["image_height"], options["image_width"], 4), np.float32)
        states = np.empty(len(streams), np.uint64)
        cp, op, st = _camera(camera), _options(options), Stats()
        _check(load().pt_render_streams(self._h, C.byref(cp), C.byref(op), _ptr(streams), C.c_size_t(len(streams)), _ptr(image), _ptr(states),
                                        C.byref(st) if want_stats else None))
        return (image, states, st.as_dict()) if want_stats else (image, states)

    def process_job(self, camera, options, base_seed=1234, tiles=None, image=None, want_stats=False, allow_bias=False):
        """processJob: every pixel of the given tiles (default: all tiles of the image) with per-pixel engines.  allow_bias (RenderOptions::
        allow_bias) returns the finished frame denoised: denoise(image, render_features(camera, options)) -- a new array, `image` keeps the
        noisy frame."""
        if tiles is None:
            tiles = job_tiles(options["image_width"], options["image_height"])
        tiles = np.ascontiguousarray(tiles, dtype=TILE_DTYPE)
        if image is None:
            image = np.zeros((options["image_height"], options["image_width"], 4), np.float32)
        cp, op, st = _camera(camera), _options(options), Stats()
        _check(load().pt_render_tiles(self._h, C.byref(cp), C.byref(op), _ptr(tiles), C.c_size_t(len(tiles)), C.c_uint64(base_seed), _ptr(image),
                                      C.byref(st) if want_stats else None))
        if allow_bias:
            image = denoise(image, self.render_features(camera, options), device=self.device)
        return (image, st.as_dict()) if want_stats else image

    def render_features(self, camera, options, followed=None):
        """First-hit features of the frame (pt_render_features): an (H, W, 3, 4) float32 array, the mean over 4 deterministic primary rays
        per pixel of [albedo rgb, coverage], [normal xyz, t], [position xyz, emission luminance].  followed: a FeatureParams or a dict of
        its fields ({} = the defaults) makes the rays go on through mirrors and glass to the first diffuse hit
        (pt_render_features_followed; options' epsilon is read too); None = first-hit."""
        out = np.empty((options["image_height"], options["image_width"], 3, 4), np.float32)
        cp, op = _camera(camera), _options(options)
        if followed is not None:
            fp = _feature_params(followed)
            _check(load().pt_render_features_followed(self._h, C.byref(cp), C.byref(op), C.byref(fp), _ptr(out)))
            return out
        _check(load().pt_render_features(self._h, C.byref(cp), C.byref(op), _ptr(out)))
        return out

    def _previous(self, previous):
        if previous is None:
            return None
        prev = np.ascontiguousarray(previous, dtype=np.float32).reshape(-1, 16)
        if self.n_instances and len(prev) != self.n_instances:
            raise ValueError("previous: %d matrices for %d instances" % (len(prev), self.n_instances))
        return prev

    def render_features_motion(self, camera, options, previous=None):
        """render_features and, from the same walks, the frame's motion (pt_render_features_motion): (features, motion), motion an
        (H, W, 2, 4) float32 array, the mean over the 4 rays of [previous position xyz, fraction moved], [previous normal xyz, fraction
        without a previous position].  previous: the matrices (n_instances, 4, 4) the instances had at the previous frame (a NaN matrix:
        the instance was not there); None = nothing moved.  The current matrices are the scene's (pose_transforms)."""
        h, w = options["image_height"], options["image_width"]
        feat, mot = np.empty((h, w, 3, 4), np.float32), np.empty((h, w, 2, 4), np.float32)
        cp, op, prev = _camera(camera), _options(options), self._previous(previous)
        _check(load().pt_render_features_motion(self._h, C.byref(cp), C.byref(op), _ptr(prev), _ptr(feat), _ptr(mot)))
        return feat, mot

    def render_features_motion_device(self, camera, options, d_features_ptr, d_motion_ptr, stream_ptr=0, previous=None):
        """render_features_motion into device memory (H*W*12 and H*W*8 floats), ordered on stream_ptr."""
        cp, op, prev = _camera(camera), _options(options), self._previous(previous)
        _check(load().pt_render_features_motion_device(self._h, C.byref(cp), C.byref(op), _ptr(prev), C.c_void_p(d_features_ptr), C.c_void_p(d_motion_ptr),
                                                       C.c_void_p(stream_ptr)))

    def mark_motion(self):
        """pt_scene_motion_mark: the scene as it is now becomes "the previous frame" of render_features_motion_marked: the instance
        matrices and every mesh's vertices are remembered (a deformed mesh's are copied on the device).  Returns the info as a dict."""
        info = MotionMarkInfo()
        _check(load().pt_scene_motion_mark(self._h, C.byref(info)))
        return info.as_dict()

    def unmark_motion(self):
        """pt_scene_motion_unmark: forgets the mark and frees what it kept."""
        _check(load().pt_scene_motion_unmark(self._h))

    def motion_mark(self):
        """pt_scene_get_motion_mark: (the marked matrices (n_instances, 4, 4), the kind (n_instances,) uint8 every instance has against
        the mark now: MOTION_STATIC | MOTION_MOVED | MOTION_NONE | MOTION_DEFORMED)."""
        m, kind = np.zeros((self.n_instances, 4, 4), np.float32), np.zeros(self.n_instances, np.uint8)
        _check(load().pt_scene_get_motion_mark(self._h, _ptr(m), _ptr(kind)))
        return m, kind

    def triangle_faces(self):
        """pt_scene_get_triangle_faces: for every instance triangle, in object order, the scene-wide face it came from (the faces of all
        instances end to end, before rejection), uint32.  Needs a mark and a pose / deform / morph since the first mark."""
        n = C.c_uint32()
        _check(load().pt_scene_get_triangle_faces(self._h, None, C.byref(n)))
        out = np.zeros(n.value, np.uint32)
        _check(load().pt_scene_get_triangle_faces(self._h, _ptr(out), None))
        return out

    def render_features_motion_marked(self, camera, options):
        """render_features_motion with the scene's mark as the previous frame (pt_render_features_motion_marked): meshes deformed or
        morphed since the mark are reprojected per vertex.  (features, motion) as render_features_motion."""
        h, w = options["image_height"], options["image_width"]
        feat, mot = np.empty((h, w, 3, 4), np.float32), np.empty((h, w, 2, 4), np.float32)
        cp, op = _camera(camera), _options(options)
        _check(load().pt_render_features_motion_marked(self._h, C.byref(cp), C.byref(op), _ptr(feat), _ptr(mot)))
        return feat, mot

    def render_features_motion_marked_device(self, camera, options, d_features_ptr, d_motion_ptr, stream_ptr=0):
        """render_features_motion_marked into device memory (H*W*12 and H*W*8 floats), ordered on stream_ptr."""
        cp, op = _camera(camera), _options(options)
        _check(load().pt_render_features_motion_marked_device(self._h, C.byref(cp), C.byref(op), C.c_void_p(d_features_ptr), C.c_void_p(d_motion_ptr),
                                                              C.c_void_p(stream_ptr)))

    def denoise_sequence(self, frames, cameras, options, params=None, poses=None):
        """Temporal denoising of a sequence of frames of this scene, frames[v] seen through cameras[v] (e.g. process_views' output): a fresh
        TemporalDenoiser pushes every frame with its render_features; returns a (V, H, W, 4) float32 array.  poses: poses[v] are the
        matrices of all instances at frame v, (V, n_instances, 4, 4): the scene is posed to poses[v], the frame's features and motion are
        rendered with poses[v - 1] as the previous pose (none for the first frame) and pushed with that motion; the scene is left at the
        last pose."""
        frames = np.asarray(frames, dtype=np.float32)
        if len(frames) != len(cameras):
            raise ValueError("one camera per frame")
        if poses is not None and len(poses) != len(frames):
            raise ValueError("one pose per frame")
        out = np.empty_like(frames)
        with TemporalDenoiser(options["image_width"], options["image_height"], params=params, device=self.device) as t:
            for v, cam in enumerate(cameras):
                if poses is None:
                    out[v], _ = t.denoise(frames[v], self.render_features(cam, options), cam)
                    continue
                self.pose(poses[v])
                feat, mot = self.render_features_motion(cam, options, previous=poses[v - 1] if v > 0 else None)
                out[v], _ = t.denoise(frames[v], feat, cam, motion=mot)
        return out

    def denoise_sequence_shapes(self, frames, cameras, options, params=None, poses=None, deforms=None, morphs=None):
        """denoise_sequence for a scene whose meshes change shape between the frames.  poses[v]: as there; deforms[v] / morphs[v]: a dict
        of deform() / morph() arguments for frame v (None or {}: nothing).  Frame 0 is posed / deformed / morphed and pushed with a motion
        in which nothing moved; every later frame is: mark_motion(), then pose, deform, morph as given, then
        render_features_motion_marked and the push with that motion.  The scene is left at the last frame's shape with that frame's
        predecessor as its mark.  (A method of its own: denoise_sequence keeps its signature and, with poses alone, its route and bits.)"""
        frames = np.asarray(frames, dtype=np.float32)
        if len(frames) != len(cameras):
            raise ValueError("one camera per frame")
        for name, per_frame in (("pose", poses), ("deform", deforms), ("morph", morphs)):
            if per_frame is not None and len(per_frame) != len(frames):
                raise ValueError("one %s per frame" % name)
        out = np.empty_like(frames)
        with TemporalDenoiser(options["image_width"], options["image_height"], params=params, device=self.device) as t:
            for v, cam in enumerate(cameras):
                if v > 0:
                    self.mark_motion()
                if poses is not None:
                    self.pose(poses[v])
                if deforms is not None and deforms[v]:
                    self.deform(**deforms[v])
                if morphs is not None and morphs[v]:
                    self.morph(**morphs[v])
                feat, mot = self.render_features_motion_marked(cam, options) if v > 0 else self.render_features_motion(cam, options)
                out[v], _ = t.denoise(frames[v], feat, cam, motion=mot)
        return out

    def render_features_views(self, cameras, options, followed=None):
        """render_features for V cameras in one launch (pt_render_features_views): a (V, H, W, 3, 4) float32 array whose view v equals
        render_features(cameras[v], options) bit for bit.  followed: as in render_features (pt_render_features_followed_views)."""
        cams, _ = _view_tables(cameras, 0)
        out = np.empty((len(cams), options["image_height"], options["image_width"], 3, 4), np.float32)
        op = _options(options)
        if followed is not None:
            fp = _feature_params(followed)
            _check(load().pt_render_features_followed_views(self._h, cams, C.c_int32(len(cams)), C.byref(op), C.byref(fp), _ptr(out)))
            return out
        _check(load().pt_render_features_views(self._h, cams, C.c_int32(len(cams)), C.byref(op), _ptr(out)))
        return out

    def render_features_views_device(self, cameras, options, d_features_ptr, stream_ptr=0, followed=None):
        """render_features_views into device memory (d_features_ptr: device address of V*H*W*12 floats), ordered on stream_ptr."""
        cams, _ = _view_tables(cameras, 0)
        op = _options(options)
        if followed is not None:
            fp = _feature_params(followed)
            _check(load().pt_render_features_followed_views_device(self._h, cams, C.c_int32(len(cams)), C.byref(op), C.byref(fp), C.c_void_p(d_features_ptr),
                                                                   C.c_void_p(stream_ptr)))
            return
        _check(load().pt_render_features_views_device(self._h, cams, C.c_int32(len(cams)), C.byref(op), C.c_void_p(d_features_ptr), C.c_void_p(stream_ptr)))

    def render_features_device(self, camera, options, d_features_ptr, stream_ptr=0, followed=None):
        """render_features into device memory (d_features_ptr: device address of H*W*12 floats, e.g. an (H, W, 3, 4) tensor), ordered on stream_ptr."""
        cp, op = _camera(camera), _options(options)
        if followed is not None:
            fp = _feature_params(followed)
            _check(load().pt_render_features_followed_device(self._h, C.byref(cp), C.byref(op), C.byref(fp), C.c_void_p(d_features_ptr), C.c_void_p(stream_ptr)))
            return
        _check(load().pt_render_features_device(self._h, C.byref(cp), C.byref(op), C.c_void_p(d_features_ptr), C.c_void_p(stream_ptr)))

    def process_work_item(self, camera, options, x, y, w, h, rng_state, want_stats=False):
        """processItem(WorkItem(job, x, y, w, h), engine) returning the item's own (h, w, 4) tile and the engine state afterwards."""
        item = np.zeros(1, dtype=STREAM_DTYPE)
        item["x"], item["y"], item["w"], item["h"], item["rng_state"] = x, y, w, h, rng_state
        tile = np.zeros((max(h, 0), max(w, 0), 4), np.float32)
        state = C.c_uint64()
        cp, op, st = _camera(camera), _options(options), Stats()
        _check(load().pt_render_item(self._h, C.byref(cp), C.byref(op), _ptr(item), _ptr(tile) if tile.size else None, C.byref(state),
                                     C.byref(st) if want_stats else None))
        return (tile, state.value, st.as_dict()) if want_stats else (tile, state.value)

    def process_job_progress(self, camera, options, progress, base_seed=1234, tiles=None):
        """processJob with its progress callback (worker.h:75-84): progress(completed, total) from the calling thread while the device renders."""
        if tiles is None:
            tiles = job_tiles(options["image_width"], options["image_height"])
        tiles = np.ascontiguousarray(tiles, dtype=TILE_DTYPE)
        image = np.zeros((options["image_height"], options["image_width"], 4), np.float32)
        cb = PROGRESS_FN(lambda done, total, user: progress(done, total))
        cp, op = _camera(camera), _options(options)
        _check(load().pt_render_tiles_progress(self._h, C.byref(cp), C.byref(op), _ptr(tiles), C.c_size_t(len(tiles)), C.c_uint64(base_seed), _ptr(image), None,
                                               cb, None))
        return image

    def process_job_controlled(self, camera, options, base_seed=1234, tiles=None, budget_ms=0, progress=None, control=None, image=None):
        """processJob that stops early when `control.cancel()` is called (from `progress` or any other thread) or after `budget_ms` of wall
        time (0 = no budget).  Returns (image, tile_done, info).  A stop is a result, not an exception: info["status"] is PT_OK or
        PT_ERR_CANCELLED, and info holds the stream counts, drain_ms and the launch statistics.  Finished pixels equal process_job's bit for
        bit; every other pixel keeps its value in `image` (default: zeros), and tile_done[i] says whether tiles[i] finished."""
        return _render_controlled([self], camera, options, base_seed, tiles, budget_ms, progress, control, image)

    def process_views(self, cameras, options, base_seeds=1234, want_stats=False, progress=None):
        """processJob for V cameras of this scene in one launch: a (V, H, W, 4) float32 array whose view v equals
        process_job(cameras[v], options, base_seed=base_seeds[v]) bit for bit.  base_seeds: one int for every view, or V ints.
        progress(completed, total) counts the tiles of all views."""
        out = process_views_multi([self], cameras, options, base_seeds=base_seeds, progress=progress, want_stats=want_stats)
        return (out[0], out[1][0]) if want_stats else out

    def process_views_device(self, cameras, options, d_images_ptr, stream_ptr, base_seeds=1234, want_stats=False):
        """process_views writing into device memory (d_images_ptr: device address of V*H*W*4 floats, e.g. a [V, H, W, 4] tensor)."""
        cams, seeds = _view_tables(cameras, base_seeds)
        op, st = _options(options), Stats()
        _check(load().pt_render_views_device(self._h, cams, seeds.ctypes.data_as(C.POINTER(C.c_uint64)), C.c_int32(len(seeds)), C.byref(op),
                                             C.c_void_p(d_images_ptr), C.c_void_p(stream_ptr), C.byref(st) if want_stats else None))
        return st.as_dict() if want_stats else None

    def process_job_device(self, camera, options, d_image_ptr, stream_ptr, base_seed=1234, tiles=None, want_stats=False):
        """processJob writing into device memory (d_image_ptr: device address of width*height*4 floats)."""
        if tiles is None:
            tiles = job_tiles(options["image_width"], options["image_height"])
        tiles = np.ascontiguousarray(tiles, dtype=TILE_DTYPE)
        cp, op, st = _camera(camera), _options(options), Stats()
        _check(load().pt_render_tiles_device(self._h, C.byref(cp), C.byref(op), _ptr(tiles), C.c_size_t(len(tiles)), C.c_uint64(base_seed),
                                             C.c_void_p(d_image_ptr), C.c_void_p(stream_ptr), C.byref(st) if want_stats else None))
        return st.as_dict() if want_stats else None


PROGRESS_FN = C.CFUNCTYPE(None, C.c_int, C.c_int, C.c_void_p)


def _render_controlled(scenes, camera, options, base_seed, tiles, budget_ms, progress, control, image):
    if tiles is None:
        tiles = job_tiles(options["image_width"], options["image_height"])
    tiles = np.ascontiguousarray(tiles, dtype=TILE_DTYPE)
    if image is None:
        image = np.zeros((options["image_height"], options["image_width"], 4), np.float32)
    assert image.dtype == np.float32 and image.flags.c_contiguous and image.shape == (options["image_height"], options["image_width"], 4)
    ctl = control if control is not None else RenderControl()
    ctl.budget_ms = float(budget_ms or 0.0)
    tile_done = np.zeros(len(tiles), np.uint8)
    ctl.tile_done = tile_done.ctypes.data
    handles = (C.c_void_p * len(scenes))(*[s._h for s in scenes])
    stats = (Stats * len(scenes))()
    cb = PROGRESS_FN(lambda done, total, user: progress(done, total)) if progress is not None else None
    cp, op = _camera(camera), _options(options)
    try:
        rc = load().pt_render_tiles_ctl(handles, C.c_int(len(scenes)), C.byref(cp), C.byref(op), _ptr(tiles), C.c_size_t(len(tiles)), C.c_uint64(base_seed),
                                        _ptr(image), stats, cb, None, C.byref(ctl))
    finally:
        ctl.tile_done = None
    if rc not in (PT_OK, PT_ERR_CANCELLED):
        _check(rc)
    info = {"status": rc, "cancelled": rc == PT_ERR_CANCELLED, "streams_finished": ctl.streams_finished, "streams_abandoned": ctl.streams_abandoned,
            "streams_unclaimed": ctl.streams_unclaimed, "drain_ms": ctl.drain_ms, "stats": [s.as_dict() for s in stats]}
    return image, tile_done.astype(bool), info


def process_job_controlled_multi(scenes, camera, options, base_seed=1234, tiles=None, budget_ms=0, progress=None, control=None, image=None):
    """process_job_multi that can be stopped: see Scene.process_job_controlled."""
    return _render_controlled(list(scenes), camera, options, base_seed, tiles, budget_ms, progress, control, image)


class Frame:
    """A processJob that can be stopped and continued (pt_frame_*): each render() goes on where the last one stopped, and the finished
    frame equals process_job / process_job_multi with the same seed bit for bit.  scenes: one Scene, or several replicas (tiles are dealt
    as process_job_multi deals them).  The scenes must stay open while the frame lives."""

    def __init__(self, scenes, camera, options, base_seed=1234, tiles=None):
        self._scenes = list(scenes) if isinstance(scenes, (list, tuple)) else [scenes]
        if tiles is None:
            tiles = job_tiles(options["image_width"], options["image_height"])
        self.tiles = np.ascontiguousarray(tiles, dtype=TILE_DTYPE)
        self.image = np.zeros((options["image_height"], options["image_width"], 4), np.float32)
        handles = (C.c_void_p * len(self._scenes))(*[sc._h for sc in self._scenes])
        cp, op = _camera(camera), _options(options)
        h = C.c_void_p()
        _check(load().pt_frame_create(handles, C.c_int(len(self._scenes)), C.byref(cp), C.byref(op), _ptr(self.tiles), C.c_size_t(len(self.tiles)),
                                      C.c_uint64(base_seed), C.byref(h)))
        self._h = h

    def render(self, budget_ms=0, progress=None, control=None):
        """Continue the frame for at most `budget_ms` of wall time (0 = until it is complete), or until `control.cancel()`.  Returns
        (image, tile_done, info) as Scene.process_job_controlled does: image is the frame so far (the same array every call), tile_done the
        frame's finished tiles, info["status"] PT_OK once the frame is complete and PT_ERR_CANCELLED before; info["frame"] is info()."""
        if self._h is None:
            raise ValueError("frame is closed")
        ctl = control if control is not None else RenderControl()
        ctl.budget_ms = float(budget_ms or 0.0)
        tile_done = np.zeros(len(self.tiles), np.uint8)
        ctl.tile_done = tile_done.ctypes.data
        stats = (Stats * len(self._scenes))()
        cb = PROGRESS_FN(lambda done, total, user: progress(done, total)) if progress is not None else None
        try:
            rc = load().pt_frame_render(self._h, _ptr(self.image), stats, cb, None, C.byref(ctl))
        finally:
            ctl.tile_done = None
        if rc not in (PT_OK, PT_ERR_CANCELLED):
            _check(rc)
        info = {"status": rc, "cancelled": rc == PT_ERR_CANCELLED, "streams_finished": ctl.streams_finished, "streams_abandoned": ctl.streams_abandoned,
                "streams_unclaimed": ctl.streams_unclaimed, "drain_ms": ctl.drain_ms, "stats": [st.as_dict() for st in stats], "frame": self.info()}
        return self.image, tile_done.astype(bool), info

    def info(self):
        fi = FrameInfo()
        _check(load().pt_frame_get_info(self._h, C.byref(fi)))
        return fi.as_dict()

    def set_feature_params(self, params):
        """pt_frame_set_feature_params: the frame's denoised previews use followed features (a FeatureParams or a dict of its fields);
        None restores the first-hit features.  The cached features are dropped either way."""
        if params is None:
            _check(load().pt_frame_set_feature_params(self._h, None))
            return
        fp = _feature_params(params)
        _check(load().pt_frame_set_feature_params(self._h, C.byref(fp)))

    def set_progressive(self, quantum, max_passes_per_call=0):
        """Progressive mode (pt_frame_set_progressive): render() then works in passes, each bringing every unfinished pixel to `quantum`
        more samples, so the preview has samples everywhere; it returns (status PT_ERR_CANCELLED) after max_passes_per_call passes if that
        is > 0.  quantum 0 turns the mode off.  Between two render() calls only; the finished image does not depend on it."""
        if self._h is None:
            raise ValueError("frame is closed")
        if quantum < 0:
            raise ValueError("quantum must be >= 0")
        _check(load().pt_frame_set_progressive(self._h, C.c_int32(quantum), C.c_int32(max_passes_per_call)))

    def progress(self):
        """pt_frame_get_progress as a dict: passes_completed, target, pass_in_progress, min_samples / max_samples over the unfinished
        pixels, streams_at_target, samples_lost (always 0)."""
        if self._h is None:
            raise ValueError("frame is closed")
        fp = FrameProgress()
        _check(load().pt_frame_get_progress(self._h, C.byref(fp)))
        return fp.as_dict()

    def set_noise_target(self, target_error, floor=1e-5, fraction=1.0):
        """A noise target (pt_frame_set_noise_target): a progressive frame then holds every pixel rated at or below target_error out of
        its passes, and render() returns (status PT_ERR_CANCELLED, noise()["target_reached"] 1) once finished + held pixels are `fraction`
        of the frame.  0 clears the target: render on and the finished image is what it always is.  floor: added to the denominator of
        the rating, raise it to keep dark pixels from dominating.  Between two render() calls only."""
        if self._h is None:
            raise ValueError("frame is closed")
        if not (np.isfinite(target_error) and target_error >= 0 and np.isfinite(floor) and floor >= 0 and 0 < fraction <= 1):
            raise ValueError("target_error and floor must be finite and >= 0, fraction in (0, 1]")
        _check(load().pt_frame_set_noise_target(self._h, C.c_float(target_error), C.c_float(floor), C.c_float(fraction)))

    def _noise(self, error):
        if self._h is None:
            raise ValueError("frame is closed")
        fn = FrameNoise()
        _check(load().pt_frame_get_noise(self._h, C.byref(fn), _ptr(error)))
        return fn.as_dict()

    def noise(self):
        """pt_frame_get_noise as a NoiseSummary: streams_rated / unrated / held / finished / total, max_error, the 64-bin histogram of the
        rated streams by the exponent of their error (error_bin), target_reached and the target as set; percentile(p) reads the histogram."""
        return self._noise(None)

    def error_map(self):
        """One rating per pixel, float32 in the shape of the preview's sample counts: -1 finished, +inf unrated, untouched or in no
        tile, else the standard error of the pixel's mean relative to 9 * its mean + floor."""
        if self._h is None:
            raise ValueError("frame is closed")
        error = np.empty(self.image.shape[:-1], np.float32)
        self._noise(error)
        return error

    def preview(self, denoise=None):
        """The frame as it stands (pt_frame_preview): (rgba, samples).  rgba (h, w, 4) float32: finished pixels as self.image, parked ones
        the running mean of their samples so far, holes (untouched pixels) 0.  samples (h, w) int32: -1 finished, the samples a parked
        pixel has taken, 0 a hole.  denoise: None or False = the raw preview; True = filtered with the default DenoiseParams; a dict as
        binding.denoise takes.  Changes nothing the frame will do."""
        if self._h is None:
            raise ValueError("frame is closed")
        rgba = np.empty_like(self.image)
        samples = np.empty(self.image.shape[:2], np.int32)
        params = None if denoise is None or denoise is False else _denoise_params({} if denoise is True else denoise)
        _check(load().pt_frame_preview(self._h, _ptr(self.image), params, _ptr(rgba), _ptr(samples)))
        return rgba, samples

    def variance(self):
        """The measured variance of the unfinished pixels (pt_frame_get_variance): float32 in the shape of self.image -- the variance of the
        mean of r, g, b from the estimator's batch statistics and the batch means B, (0, 0, 0, 0) for a pixel that is finished, untouched,
        in no tile or has B < 2."""
        if self._h is None:
            raise ValueError("frame is closed")
        var = np.empty_like(self.image)
        _check(load().pt_frame_get_variance(self._h, _ptr(var)))
        return var

    def preview_measured(self, params=None):
        """preview(denoise=...) with each rated pixel's measured variance in place of the filter's 3x3 estimate (pt_frame_preview_measured):
        (rgba, samples).  params: None = defaults, or a flat dict of DenoiseParams fields and sigma_measured.  Not for a ViewsFrame."""
        if self._h is None:
            raise ValueError("frame is closed")
        rgba = np.empty_like(self.image)
        samples = np.empty(self.image.shape[:-1], np.int32)
        _check(load().pt_frame_preview_measured(self._h, _ptr(self.image), _denoise_measured_params(params), _ptr(rgba), _ptr(samples)))
        return rgba, samples

    def checkpoint(self):
        """The frame as it stands, as a checkpoint (pt_frame_checkpoint_save): a uint8 array that Frame.restore turns back into a frame
        -- in another process, on another machine, on any number of replicas of the same scene -- which finishes bit-identically.
        Between two render() calls only; changes nothing the frame will do."""
        if self._h is None:
            raise ValueError("frame is closed")
        need = C.c_size_t()
        _check(load().pt_frame_checkpoint_size(self._h, C.byref(need)))
        blob = np.empty(need.value, np.uint8)
        written = C.c_size_t()
        _check(load().pt_frame_checkpoint_save(self._h, _ptr(self.image), _ptr(blob), C.c_size_t(len(blob)), C.byref(written)))
        return blob[:written.value]

    def save(self, path):
        """checkpoint() into the file `path`: written beside it under a temporary name and moved into place, so that a reader never
        sees half a checkpoint."""
        blob = self.checkpoint()
        tmp = "%s.%d.tmp" % (os.fspath(path), os.getpid())
        try:
            with open(tmp, "wb") as fh:
                fh.write(memoryview(blob))
            os.replace(tmp, path)
        finally:
            if os.path.exists(tmp):
                os.remove(tmp)

    @classmethod
    def restore(cls, scenes, blob_or_path):
        """The frame of a checkpoint (pt_frame_checkpoint_load) on `scenes`: one Scene or several replicas of the scene the frame was
        made on, however many it had then.  A Frame, or a ViewsFrame when the checkpoint is of a view batch, with .image holding the
        finished pixels and zeros elsewhere.  Raises PtError (PT_ERR_INVALID) for a damaged blob or another scene."""
        blob = _blob(blob_or_path)
        info = checkpoint_inspect(blob)
        scenes = list(scenes) if isinstance(scenes, (list, tuple)) else [scenes]
        views = info["n_views"]
        frame = object.__new__(ViewsFrame if views > 1 else Frame)
        frame._h = None
        frame._scenes = scenes
        at = (CHECKPOINT_HEADER_BYTES + info["bytes_tables"] + 15) // 16 * 16
        frame.tiles = blob[at:at + info["bytes_tiles"]].copy().view(TILE_DTYPE)
        h, w = info["options"]["image_height"], info["options"]["image_width"]
        frame.image = np.zeros((views, h, w, 4) if views > 1 else (h, w, 4), np.float32)
        handles = (C.c_void_p * len(scenes))(*[sc._h for sc in scenes])
        handle = C.c_void_p()
        _check(load().pt_frame_checkpoint_load(handles, C.c_int(len(scenes)), _ptr(blob), C.c_size_t(len(blob)), _ptr(frame.image), C.byref(handle)))
        frame._h = handle
        return frame

    @property
    def done(self):
        i = self.info()
        return i["streams_finished"] == i["streams_total"]

    def close(self):
        if self._h is not None:
            load().pt_frame_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ViewsFrame(Frame):
    """process_views that can be stopped and continued (pt_frame_create_views): a Frame over a view batch.  render, info, preview, done,
    set_progressive, progress, set_noise_target, noise, error_map and close are Frame's (the error map is (V, H, W)); image and the preview are (V, H, W, 4), the preview's sample counts (V, H, W), tile_done
    covers the tiles of all views (V x job_tiles(W, H), view after view).  The finished images equal process_views / process_views_multi
    with the same seeds bit for bit, however the calls were sliced.  base_seeds: one int for every view, or V ints."""

    def __init__(self, scenes, cameras, options, base_seeds=1234):
        self._scenes = list(scenes) if isinstance(scenes, (list, tuple)) else [scenes]
        cams, seeds = _view_tables(cameras, base_seeds)
        per_view = job_tiles(options["image_width"], options["image_height"])
        self.tiles = np.concatenate([per_view] * len(seeds))
        self.tiles["y"] += np.repeat(np.arange(len(seeds), dtype=np.int32) * options["image_height"], len(per_view))
        self.image = np.zeros((len(seeds), options["image_height"], options["image_width"], 4), np.float32)
        handles = (C.c_void_p * len(self._scenes))(*[sc._h for sc in self._scenes])
        op = _options(options)
        h = C.c_void_p()
        self._h = None
        _check(load().pt_frame_create_views(handles, C.c_int(len(self._scenes)), cams, seeds.ctypes.data_as(C.POINTER(C.c_uint64)), C.c_int32(len(seeds)),
                                            C.byref(op), C.byref(h)))
        self._h = h

    def preview(self, denoise=None):
        """Frame.preview per view: (rgba (V, H, W, 4), samples (V, H, W)).  Denoised, a hole is filled from pixels of its own view only."""
        if self._h is None:
            raise ValueError("frame is closed")
        rgba = np.empty_like(self.image)
        samples = np.empty(self.image.shape[:3], np.int32)
        params = None if denoise is None or denoise is False else _denoise_params({} if denoise is True else denoise)
        _check(load().pt_frame_preview(self._h, _ptr(self.image), params, _ptr(rgba), _ptr(samples)))
        return rgba, samples


def process_job_multi(scenes, camera, options, base_seed=1234, tiles=None, progress=None, want_stats=False):
    """processJob over several Scene replicas (one per device): tile k is rendered by scenes[k % len(scenes)]."""
    if tiles is None:
        tiles = job_tiles(options["image_width"], options["image_height"])
    tiles = np.ascontiguousarray(tiles, dtype=TILE_DTYPE)
    image = np.zeros((options["image_height"], options["image_width"], 4), np.float32)
    handles = (C.c_void_p * len(scenes))(*[s._h for s in scenes])
    stats = (Stats * len(scenes))()
    cb = PROGRESS_FN(lambda done, total, user: progress(done, total)) if progress is not None else None
    cp, op = _camera(camera), _options(options)
    _check(load().pt_render_tiles_multi(handles, C.c_int(len(scenes)), C.byref(cp), C.byref(op), _ptr(tiles), C.c_size_t(len(tiles)), C.c_uint64(base_seed),
                                        _ptr(image), stats if want_stats else None, cb, None))
    return (image, [s.as_dict() for s in stats]) if want_stats else image


_CAMERA_KEYS = ("origin", "look_at", "up", "focal_length", "height", "aspect_ratio")


def _view_tables(cameras, base_seeds):
    """The camera and seed tables of a view batch, checked before the library is touched: cameras must be a non-empty list of camera
    dicts (scenes.camera), base_seeds one int or one int per camera, each in [0, 2**64)."""
    if isinstance(cameras, dict) or not isinstance(cameras, (list, tuple)) or len(cameras) == 0:
        raise ValueError("cameras must be a non-empty list of camera dicts")
    for i, cam in enumerate(cameras):
        if not isinstance(cam, dict) or any(k not in cam for k in _CAMERA_KEYS):
            raise ValueError("camera %d is not a camera dict (it needs %s)" % (i, ", ".join(_CAMERA_KEYS)))
        for k in ("origin", "look_at", "up"):
            if len(cam[k]) != 3:
                raise ValueError("camera %d: %s must have 3 components" % (i, k))
    if isinstance(base_seeds, (int, np.integer)) and not isinstance(base_seeds, bool):
        base_seeds = [int(base_seeds)] * len(cameras)
    if isinstance(base_seeds, (str, bytes, dict)) or not hasattr(base_seeds, "__len__") or len(base_seeds) != len(cameras):
        raise ValueError("base_seeds must be an int or one int per camera (%d)" % len(cameras))
    seeds = []
    for s in base_seeds:
        if isinstance(s, bool) or not isinstance(s, (int, np.integer)) or not 0 <= int(s) < 2 ** 64:
            raise ValueError("base seed %r is not an int in [0, 2**64)" % (s,))
        seeds.append(int(s))
    cams = (CameraParams * len(cameras))(*[_camera(c) for c in cameras])
    return cams, np.array(seeds, dtype=np.uint64)


def process_views_multi(scenes, cameras, options, base_seeds=1234, progress=None, want_stats=False):
    """Scene.process_views over several Scene replicas (one per device): the views' tiles are dealt as process_job_multi deals a frame's."""
    cams, seeds = _view_tables(cameras, base_seeds)
    scenes = list(scenes)
    if len(scenes) == 0:
        raise ValueError("no scenes")
    image = np.zeros((len(seeds), options["image_height"], options["image_width"], 4), np.float32)
    handles = (C.c_void_p * len(scenes))(*[s._h for s in scenes])
    stats = (Stats * len(scenes))()
    cb = PROGRESS_FN(lambda done, total, user: progress(done, total)) if progress is not None else None
    op = _options(options)
    _check(load().pt_render_views(handles, C.c_int(len(scenes)), cams, seeds.ctypes.data_as(C.POINTER(C.c_uint64)), C.c_int32(len(seeds)), C.byref(op),
                                  _ptr(image), stats if want_stats else None, cb, None))
    return (image, [s.as_dict() for s in stats]) if want_stats else image


def pixel_streams(xs, ys, states):
    s = np.zeros(len(xs), dtype=STREAM_DTYPE)
    s["x"], s["y"], s["w"], s["h"], s["rng_state"] = xs, ys, 1, 1, states
    return s
