"""Scenes, rays, pixels and occlusion thresholds shared by tests/test_query_cpu.py and tests/test_gpu_query.py (include/pt_query.h,
DESIGN.md 4.17).  numpy only; everything is deterministic from fixed seeds.

Scene S (below 1024 objects: host-built tree, records in LDS): 2 spheres; 3 triangles of the description, one culled, one without a
material; mesh M1, the smooth 6 x 6 patch, twice; mesh M2, flat, 40 faces of which 5 are degenerate, once -- so M2's instance keeps
fewer triangles than its mesh has faces.  Scene L: S plus a 24 x 24 grid instance (1152 faces: device-built tree, records in HBM) and a
row of 300 sliver triangles in the description, a run of overlapping boxes that drives a walk's stack past its 8-entry window."""
import numpy as np

from cpupathtrace_amd import scenes
from tests import motion_ref
from tests import motion_shapes_cases as msc
from tests import motion_shapes_ref as msr

F = np.float32
BATCHES = [1, 63, 64, 65, 257, 1000]
N_RAYS = 1000
FRAME_W, FRAME_H = 33, 17
CAMERA = scenes.camera((0.0, 0.0, -1.6), (0.0, 0.0, 1.0), (0, 1, 0), 1.6, 1.0, -FRAME_W / float(FRAME_H))
OPTIONS = scenes.options(FRAME_W, FRAME_H, 1, 1)
N_SLIVERS = 300


def m1():
    return msc.patch()


def m2():
    """A flat 6 x 3-quad grid without its last face (35 faces) with 5 degenerate faces spliced in: 40 faces, 35 survive."""
    v, f = msc.grid(6, 3, (-0.6, -0.3), (0.6, 0.3))
    good = f[:35]
    bad = np.array([[0, 0, 1], [3, 4, 3], [7, 7, 7], [2, 9, 2], [5, 5, 6]], np.int32)
    faces = np.concatenate([good[:4], bad[:1], good[4:11], bad[1:3], good[11:30], bad[3:4], good[30:], bad[4:]]).astype(np.int32)
    assert len(faces) == 40
    return v, faces


def big():
    return msc.grid(24, 24, (-0.9, -0.9), (0.9, 0.9), lambda x, y: 0.05 * np.cos(4.0 * x) * np.sin(3.0 * y))


def slivers():
    """300 long thin triangles side by side along x, all spanning the same y range: their boxes overlap along the row."""
    x = (F(-0.9) + F(0.006) * np.arange(N_SLIVERS, dtype=F)).astype(F)
    tri = np.zeros((N_SLIVERS, 3, 3), F)
    tri[:, 0] = np.stack([x, np.full(N_SLIVERS, -0.8, F), np.full(N_SLIVERS, 1.6, F)], axis=1)
    tri[:, 1] = np.stack([x + F(0.004), np.full(N_SLIVERS, -0.8, F), np.full(N_SLIVERS, 1.9, F)], axis=1)
    tri[:, 2] = np.stack([x + F(0.002), np.full(N_SLIVERS, 0.8, F), np.full(N_SLIVERS, 1.75, F)], axis=1)
    return tri


INSTANCES_S = [("m1", msc.place(-0.45, -0.35, 0.6, 0.7), "red", False, True), ("m1", msc.place(0.45, 0.4, 0.8, 0.6, degrees=20.0), "mirror", True, True),
               ("m2", msc.place(0.0, 0.05, 1.1, 1.2, degrees=-8.0), None, False, False)]
INSTANCE_L = ("big", msc.place(0.0, 0.0, 1.4, 1.0), "red", False, True)


def build(large, matrices=None, meshes=None, materials=None, instance_materials=None):
    """(scene dict for pt_scene_create_meshes, instance list [(mesh name, matrix, material name, cull, smooth)], mesh dict).  matrices:
    other instance matrices; meshes: other vertices for the named meshes {name: vertices}; materials: other keyword sets by name; instance_materials: {instance: material name}."""
    sb = scenes.SceneBuilder()
    kw = {"red": dict(diffuse=(0.8, 0.2, 0.2, 1)), "mirror": dict(bsdf=scenes.BSDF_MIRROR), "glow": dict(emission=(1.0, 0.9, 0.8, 2.0))}
    kw.update(materials or {})
    mats = {name: sb.material(**k) for name, k in kw.items()}
    mats[None] = scenes.NO_MATERIAL
    sb.sphere((-0.55, 0.45, 0.3), 0.25, mats["red"])
    sb.sphere((0.6, -0.5, 0.2), 0.2, mats["mirror"])
    sb.triangles([[[-0.2, -0.9, 0.4], [0.3, -0.9, 0.5], [0.05, -0.55, 0.45]]], mats["glow"])
    sb.triangles([[[-0.95, -0.1, 0.9], [-0.95, 0.5, 0.7], [-0.6, 0.1, 0.8]]], mats["red"], cull=True)
    sb.triangles([[[0.75, 0.0, 0.5], [0.95, 0.3, 0.55], [0.7, 0.35, 0.6]]])  # no material
    if large:
        sb.triangles(slivers(), mats["red"])
    sb.point_light((-0.6, 0.7, -0.6), (0.5, 0.5, 0.4, 1.0))
    shapes = {"m1": m1(), "m2": m2(), "big": big()}
    for name, vertices in (meshes or {}).items():
        shapes[name] = (np.asarray(vertices, F), shapes[name][1])
    instances = list(INSTANCES_S) + ([INSTANCE_L] if large else [])
    if matrices is not None:
        instances = [(n, np.asarray(m, F), mat, c, s) for (n, _, mat, c, s), m in zip(instances, matrices)]
    instances = [(n, m, (instance_materials or {}).get(i, mat), c, s) for i, (n, m, mat, c, s) in enumerate(instances)]
    for name, m, material, cull, smooth in instances:
        sb.mesh(shapes[name][0], shapes[name][1], m, mats[material], cull=cull, smooth=smooth)
    return sb.build(), instances, shapes


MATERIAL_INDEX = {"red": 0, "mirror": 1, "glow": 2, None: scenes.NO_MATERIAL}


def flatten(scene, instances, shapes, probe):
    """The scene as the oracle takes it: the description's objects, then every instance's surviving triangles, assembled by the product's
    own assembler compiled for the host (tests/pose_probe.py).  Returns a dict: scene (flat), first / count (object ranges), n_faces and
    face_first per instance, face_of (scene-wide face per instance triangle), local_face (face of its mesh per instance triangle)."""
    names = sorted({n for n, _, _, _, _ in instances})
    room = sum(len(shapes[n][1]) for n, _, _, _, _ in instances)
    pos, nrm = np.zeros((room, 9), F), np.zeros((room, 9), F)
    total, counts, _, _, _ = probe.assemble([shapes[n] for n in names], [(names.index(n), m, s) for n, m, _, _, s in instances], room, pos, nrm)
    pos, nrm = pos[:total], nrm[:total]
    description = {k: v for k, v in scene.items() if k not in ("meshes", "instances")}
    mat_index = {i: inst["material"] for i, inst in enumerate(scene["instances"])}
    cull = np.concatenate([np.full(c, 1 if instances[i][3] else 0, np.uint8) for i, c in enumerate(counts)])
    material = np.concatenate([np.full(c, mat_index[i], np.uint32) for i, c in enumerate(counts)])
    flat = motion_ref.flat_scene(description, pos, nrm, cull, material)
    n_desc = len(description["obj_kind"])
    first = n_desc + np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)
    face_of, face_first, want_counts = msr.face_table([(m, shapes[n][0], shapes[n][1]) for n, m, _, _, _ in instances])
    assert want_counts == [int(c) for c in counts], (want_counts, counts)
    local = face_of.astype(np.int64) - np.repeat(np.asarray(face_first, np.int64), counts)
    return dict(scene=flat, first=first, count=np.asarray(counts, np.int64), n_faces=[len(shapes[n][1]) for n, _, _, _, _ in instances], face_first=face_first,
                face_of=face_of, local_face=local, n_desc=n_desc)


def rays(flat, seed=20):
    """N_RAYS rays: at the centroid of every object kind and instance, at shared edges and vertices of the meshes (ties), from origins
    inside the scene's boxes, rays that miss the root box, one with a NaN direction and one of zero length."""
    rng = np.random.default_rng(seed)
    sc = flat["scene"]
    tri = np.asarray(sc["tri_pos"], F).reshape(-1, 3, 3)
    sph = np.asarray(sc["sph"], F).reshape(-1, 4)
    centroids = tri.mean(axis=1)
    n_desc_tri = int((np.asarray(sc["obj_kind"])[:flat["n_desc"]] == 0).sum())
    # every sphere, the description's first three triangles, some slivers, and up to 60 triangles of every instance
    targets = [sph[:, :3], centroids[:3], centroids[3:n_desc_tri][::30]]
    at = n_desc_tri
    for count in flat["count"]:
        targets.append(centroids[at + rng.choice(count, min(int(count), 60), replace=False)])
        at += int(count)
    # ties: the midpoints of edges and the corners of the instances' triangles (shared between neighbours of a grid)
    mesh = tri[n_desc_tri:]
    pick = rng.choice(len(mesh), 150, replace=False)
    targets += [0.5 * (mesh[pick, 0] + mesh[pick, 1]), mesh[pick, 2]]
    targets = np.concatenate(targets).astype(F)
    n_aimed = N_RAYS - 260
    assert len(targets) <= n_aimed
    targets = np.concatenate([targets, centroids[rng.choice(len(centroids), n_aimed - len(targets))]])  # ... and any object again, from elsewhere
    origins = np.stack([rng.uniform(-0.8, 0.8, len(targets)), rng.uniform(-0.8, 0.8, len(targets)), rng.uniform(-1.5, -0.5, len(targets))], axis=1)
    d = targets - origins
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    out = [np.concatenate([origins, d], axis=1)]
    # origins inside the boxes: between the instances, any direction
    o = rng.uniform(-0.7, 0.7, (200, 3)) + np.array([0, 0, 0.9])
    dd = rng.normal(size=(200, 3))
    dd /= np.linalg.norm(dd, axis=1, keepdims=True)
    out.append(np.concatenate([o, dd], axis=1))
    # along the row of slivers (scene L), grazing: many boxes in a row are entered
    o = np.stack([np.full(20, -1.5), rng.uniform(-0.7, 0.7, 20), rng.uniform(1.62, 1.88, 20)], axis=1)
    t = np.stack([np.full(20, 1.5), rng.uniform(-0.7, 0.7, 20), rng.uniform(1.62, 1.88, 20)], axis=1)
    dd = t - o
    dd /= np.linalg.norm(dd, axis=1, keepdims=True)
    out.append(np.concatenate([o, dd], axis=1))
    # misses of the root box
    o = rng.uniform(5.0, 6.0, (38, 3))
    dd = np.abs(rng.normal(size=(38, 3))) + 0.1
    dd /= np.linalg.norm(dd, axis=1, keepdims=True)
    out.append(np.concatenate([o, dd], axis=1))
    r = np.concatenate(out).astype(F)
    r = r[rng.permutation(len(r))]
    special = np.array([[0.0, 0.0, -1.0, np.nan, 0.0, 1.0], [0.0, 0.0, -1.0, 0.0, 0.0, 0.0]], F)
    r = np.concatenate([r[:40], special, r[40:]])[:N_RAYS]
    assert r.shape == (N_RAYS, 6)
    return np.ascontiguousarray(r, F)


def thresholds(t):
    """The occlusion cases of rays with the hit distances t (hits only): (ray index, t_max) for t, its two neighbours, 0, -1, +inf,
    FLT_MAX and NaN."""
    t = np.asarray(t, F)
    idx = np.nonzero(t >= 0)[0]
    th = t[idx]
    cases = [th, np.nextafter(th, F(np.inf)), np.nextafter(th, F(-np.inf)), np.zeros_like(th), np.full_like(th, -1.0), np.full_like(th, np.inf),
             np.full_like(th, np.finfo(F).max), np.full_like(th, np.nan)]
    return np.tile(idx, len(cases)), np.concatenate(cases).astype(F)


def pixel_rays(checker, camera, width, height, xy):
    """The oracle's camera rays through the centres of the pixels xy (n, 2): camera_shoot at 2 ((p + 1/2) / size - 1/2), y negated,
    without aperture and with pixel sizes of 0."""
    xy = np.asarray(xy, np.int64).reshape(-1, 2)
    half = F(0.5)
    xc = (F(2.0) * ((xy[:, 0].astype(F) + half) / F(width) - half)).astype(F)
    yc = (-(F(2.0) * ((xy[:, 1].astype(F) + half) / F(height) - half))).astype(F)
    cam = dict(camera)
    cam["aperture_kind"] = scenes.APERTURE_NONE
    r, _ = checker.camera_shoot(cam, np.stack([xc, yc], axis=1), 0.0, 0.0, np.zeros(len(xy), np.uint64))
    return r


def frame_pixels(width, height):
    ys, xs = np.mgrid[0:height, 0:width]
    return np.stack([xs.ravel(), ys.ravel()], axis=1).astype(np.int32)


def check_conditions(flat, t, obj):
    """The conditions of the issue, from the oracle's own answers: at least half of the rays hit, and every object kind and every
    instance is hit at least once; at least 30 % of the occlusion cases are 1 and at least 30 % are 0."""
    hit = (obj >= 0) & (t >= 0)
    assert hit.mean() >= 0.5, hit.mean()
    okind = np.asarray(flat["scene"]["obj_kind"])
    o = obj[hit]
    assert (okind[o] == 1).any() and ((okind[o] == 0) & (o < flat["n_desc"])).any()
    for i, (first, count) in enumerate(zip(flat["first"], flat["count"])):
        assert ((o >= first) & (o < first + count)).any(), "instance %d is never hit" % i
    idx, t_max = thresholds(np.where(hit, t, F(-1.0)))
    with np.errstate(invalid="ignore"):
        want = (t[idx] >= 0) & (t[idx] < t_max)
    assert 0.3 <= want.mean() <= 0.7, want.mean()
    return hit
