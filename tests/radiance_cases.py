"""The rays and captures of scenes S, L and G of tests/gather_cases.py, shared by tests/test_radiance_cpu.py and tests/test_gpu_radiance.py
(include/pt_radiance.h).  numpy only; everything is deterministic from fixed seeds.

The rays of a scene: a few hand-made ones first -- from the camera at the middle of the scene; from above everything upwards, which hits
nothing; the first one again with a direction of length 2.5, since the call takes directions as they are --, then the finite rays of
query_cases.rays.  pt_radiance_rays draws nothing before the loop, so a ray's first walk ends the same way for every sample: the set holds
rays of each kind, and tests/test_radiance_cpu.py checks on the yardstick that it also holds at least 10 % of samples that reach a third
real vertex, all three BSDF kinds and both emitter kinds.

The captures: the four models at the sizes the GPU tests compare against the yardstick, from the scene camera's origin looking at its
look_at and, in G, from the centre of the closed box.  The orthographic window is wider and higher than G's room, so its outer pixels
miss."""
import numpy as np

from cpupathtrace_amd import binding
from tests import gather_cases
from tests import query_cases

F = np.float32
N_RAYS = 257
BATCHES = [1, 63, 64, 65, 257]
SAMPLES = [1, 2, 63, 64, 65, 130]
CHUNKS = [1, 17, 64, 130, 200, 1000]
SEED = 37
OPTIONS = gather_cases.OPTIONS
CAMERA = gather_cases.CAMERA
FRAME_W, FRAME_H = gather_cases.FRAME_W, gather_cases.FRAME_H
BOX_CENTRE = tuple(0.5 * (np.asarray(gather_cases.BOX_LO) + np.asarray(gather_cases.BOX_HI)))
ORTHO_EXTENT = (1.5, 1.5)
# (model, width, height, keyword arguments of binding.capture_desc) of the captures compared against the yardstick ...
SMALL = [("equirect", binding.CAPTURE_EQUIRECT, 8, 4, {}), ("cube", binding.CAPTURE_CUBE, 18, 3, {}), ("fisheye_pi", binding.CAPTURE_FISHEYE, 5, 5, dict(fov=np.pi)),
         ("fisheye_2pi", binding.CAPTURE_FISHEYE, 5, 5, dict(fov=2.0 * np.pi)), ("ortho", binding.CAPTURE_ORTHO, 7, 3, dict(extent=ORTHO_EXTENT))]
# ... and of those compared against the rays call
LARGE = [("equirect", binding.CAPTURE_EQUIRECT, 64, 32, {}), ("cube", binding.CAPTURE_CUBE, 48, 8, {}), ("fisheye", binding.CAPTURE_FISHEYE, 32, 32, dict(fov=np.pi)),
         ("ortho", binding.CAPTURE_ORTHO, 64, 32, dict(extent=ORTHO_EXTENT))]

build = gather_cases.build


def hand_made():
    o, at = np.asarray(CAMERA["origin"], np.float64), np.asarray(CAMERA["look_at"], np.float64) + np.array([0.05, -0.1, 0.0])
    d = (at - o) / np.linalg.norm(at - o)
    return np.asarray([np.concatenate([o, d]), [0.1, 3.0, 0.6, 0.0, 1.0, 0.0], np.concatenate([o, 2.5 * d])], F)


def rays(flat):
    """N_RAYS finite rays (n, 6) of a scene, the hand-made ones first."""
    r = query_cases.rays(flat)
    r = r[np.isfinite(r).all(axis=1) & (r[:, 3:] != 0).any(axis=1)]
    r = np.concatenate([hand_made(), r])
    assert len(r) >= N_RAYS, len(r)
    return np.ascontiguousarray(r[:N_RAYS], F)


def origins(name):
    """The origins and targets of a scene's captures: the scene camera's, and in G the centre of the closed box looking along +z."""
    views = [(CAMERA["origin"], CAMERA["look_at"])]
    if name == "G":
        views.append((BOX_CENTRE, (BOX_CENTRE[0], BOX_CENTRE[1], BOX_CENTRE[2] + 1.0)))
    return views


def desc(model, width, height, view, jitter, **kw):
    return binding.capture_desc(model, width, height, view[0], view[1], CAMERA["up"], jitter=jitter, **kw)
