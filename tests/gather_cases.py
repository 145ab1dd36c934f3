"""Scenes and points shared by tests/test_gather_cpu.py and tests/test_gpu_gather.py (include/pt_gather.h).  numpy only;
everything is deterministic from fixed seeds.

Scenes S and L are tests/query_cases.py's: the tree in LDS, and device-built with walks past the stack window.  Scene G is a closed room
(floor, ceiling and four walls, Lambertian; the front wall is culled, so the camera in front of it looks through it) that holds a glass
mesh instance (the smooth patch), a flat instance that lost degenerate faces, a culled Lambertian instance of the patch, an emissive
sphere, an emissive triangle, two point lights, a one-way mirror and a closed box.

The points of a scene: a few hand-made ones first -- above everything, exactly on an emitter, and in G inside the closed box --, then
the hit positions of query_cases.rays with the shading normals turned against the rays, and for every other one along them: the near
sides look out of the scene towards the rays' origins, the far sides into it."""
import numpy as np

from cpupathtrace_amd import scenes
from tests import gather_ref
from tests import motion_shapes_cases as msc
from tests import query_cases

F = np.float32
N_POINTS = 257
BATCHES = [1, 63, 64, 65, 257]
SAMPLES = [1, 2, 17]
OPTIONS = query_cases.OPTIONS
CAMERA = query_cases.CAMERA
FRAME_W, FRAME_H = query_cases.FRAME_W, query_cases.FRAME_H
DISTANCE = 1.0  # of the occlusion cases: some occluders lie beyond it
SEED = 29
BOX_LO, BOX_HI = (0.45, -0.85, 0.15), (0.85, -0.45, 0.55)
GLOW_TRIANGLE = [[-0.2, -0.9, 0.4], [0.3, -0.9, 0.5], [0.05, -0.55, 0.45]]  # query_cases.build's emitter
G_EMISSIVE_SPHERE = (-0.5, 0.55, 0.9, 0.14)
G_EMISSIVE_TRIANGLE = [[-0.15, 0.93, 0.7], [0.25, 0.93, 0.7], [0.05, 0.93, 1.1]]

FRONT_WALL = scenes.make_plane((-1.0, -0.95, -0.2), (1.0, 0.95, -0.2))  # (makePlane's winding: seen from inside)

INSTANCES_G = [("m1", msc.place(-0.1, -0.1, 0.8, 0.8, degrees=10.0), "glass", False, True), ("m2", msc.place(0.35, 0.3, 1.3, 0.9, degrees=-8.0), "red", False, False),
               ("m1", msc.place(0.4, -0.3, 1.05, 0.6, degrees=25.0), "red", True, True)]


def build_g():
    """(scene dict for pt_scene_create_meshes, instance list, mesh dict), as query_cases.build returns them."""
    sb = scenes.SceneBuilder()
    kw = {"red": dict(diffuse=(0.8, 0.2, 0.2, 1)), "grey": dict(diffuse=(0.7, 0.7, 0.7, 1)), "glass": dict(bsdf=scenes.BSDF_GLASS, ior=1.5, specular=(0.95, 0.95, 0.95, 1)),
          "mirror": dict(bsdf=scenes.BSDF_MIRROR), "oneway": dict(bsdf=scenes.BSDF_MIRROR, one_way=True, specular=(0.9, 0.9, 0.9, 1)),
          "lamp": dict(emission=(1.0, 0.9, 0.8, 3.0)), "glow": dict(emission=(0.3, 0.5, 1.0, 2.0))}
    mats = {name: sb.material(**k) for name, k in kw.items()}
    mats[None] = scenes.NO_MATERIAL
    sb.sphere(G_EMISSIVE_SPHERE[:3], G_EMISSIVE_SPHERE[3], mats["lamp"])
    sb.sphere((0.55, 0.1, 0.5), 0.2, mats["mirror"])
    sb.triangles([G_EMISSIVE_TRIANGLE], mats["glow"])
    sb.triangles(scenes.make_plane((-1.0, -0.95, -0.2), (1.0, -0.95, 1.9)), mats["grey"])  # floor
    sb.triangles(scenes.make_plane((-1.0, 0.95, -0.2), (1.0, 0.95, 1.9)), mats["grey"])    # ceiling
    sb.triangles(scenes.make_plane((-1.0, -0.95, 1.9), (1.0, 0.95, 1.9)), mats["red"])     # back wall
    sb.triangles(scenes.make_plane((-1.0, -0.95, -0.2), (-1.0, 0.95, 1.9)))                # left wall, no material
    sb.triangles(scenes.make_plane((1.0, -0.95, -0.2), (1.0, 0.95, 1.9)), mats["grey"])    # right wall
    sb.triangles(FRONT_WALL, mats["grey"], cull=True)                                      # front wall
    sb.triangles(scenes.make_plane((-0.9, -0.6, 0.35), (-0.3, 0.1, 0.35)), mats["oneway"])  # the one-way mirror, facing the camera side or away
    sb.triangles(scenes.make_box(BOX_LO, BOX_HI), mats["grey"])
    sb.point_light((-0.6, 0.7, -0.1), (0.5, 0.5, 0.4, 1.0))
    sb.point_light((0.7, 0.2, 1.5), (0.2, 0.3, 0.5, 1.0))
    shapes = {"m1": query_cases.m1(), "m2": query_cases.m2()}
    for name, m, material, cull, smooth in INSTANCES_G:
        sb.mesh(shapes[name][0], shapes[name][1], m, mats[material], cull=cull, smooth=smooth)
    return sb.build(), list(INSTANCES_G), shapes


def build(name):
    return build_g() if name == "G" else query_cases.build(name == "L")


def _face_normal(tri):
    tri = np.asarray(tri, np.float64)
    n = np.cross(tri[1] - tri[0], tri[2] - tri[0])
    return n / np.linalg.norm(n)


def hand_made(name):
    """(positions, normals): above everything, looking up and looking down; exactly on an emitter, on both of its sides; in G also inside
    the closed box and on the emissive sphere."""
    tri = np.asarray(G_EMISSIVE_TRIANGLE if name == "G" else GLOW_TRIANGLE, np.float64)
    centre, n = tri.mean(axis=0), _face_normal(tri)
    pos = [(0.1, 3.0, 0.6), (0.1, 3.0, 0.6), centre, centre]
    nrm = [(0.0, 1.0, 0.0), (0.0, -1.0, 0.0), n, -n]
    if name == "G":
        inside = 0.5 * (np.asarray(BOX_LO) + np.asarray(BOX_HI))
        c, r = np.asarray(G_EMISSIVE_SPHERE[:3]), G_EMISSIVE_SPHERE[3]
        out = np.array([0.6, -0.48, -0.64])
        pos += [inside, inside, c + r * out]
        nrm += [(0.0, 0.0, 1.0), (0.6, 0.8, 0.0), out]
    return np.asarray(pos, F), np.asarray(nrm, F)


def points(handle, flat, name):
    """N_POINTS points of a scene: (positions (n, 3), normals (n, 3)), the hand-made ones first."""
    rays = query_cases.rays(flat)
    t, obj = handle.intersect(rays)
    hit = np.nonzero((t >= 0) & (obj >= 0))[0]
    d = rays[hit, 3:]
    pos = (rays[hit, :3] + d * t[hit, None]).astype(F)
    nrm = handle.normal(obj[hit], pos)[0].astype(F)
    away = gather_ref._dot(nrm, d) > 0
    nrm = np.where(away[:, None], -nrm, nrm).astype(F)
    nrm[1::2] = -nrm[1::2]  # (every other one: the far side)
    hp, hn = hand_made(name)
    pos, nrm = np.concatenate([hp, pos]), np.concatenate([hn, nrm])
    assert len(pos) >= N_POINTS, len(pos)
    return np.ascontiguousarray(pos[:N_POINTS]), np.ascontiguousarray(nrm[:N_POINTS])


def emitter_kinds(name, light_pos):
    """(samples on emissive spheres, samples on emissive triangles) of the sampled emitter positions: a scene's emissive spheres are known."""
    if len(light_pos) == 0:
        return 0, 0
    if name != "G":
        return 0, len(light_pos)
    c, r = np.asarray(G_EMISSIVE_SPHERE[:3], np.float64), G_EMISSIVE_SPHERE[3]
    on_sphere = np.abs(np.linalg.norm(light_pos.astype(np.float64) - c, axis=1) - r) < 1e-4
    return int(on_sphere.sum()), int((~on_sphere).sum())
