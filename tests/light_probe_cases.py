"""The light probes of scenes S, L and G of tests/gather_cases.py, shared by tests/test_light_probes_cpu.py and tests/test_gpu_light_probes.py
(include/pt_light_probes.h).  numpy only; everything is deterministic from fixed seeds.

The probes of a scene: a few hand-made ones first -- above everything; exactly on the emissive triangle; at a point light's position; in
G the centre of the closed box --, then the midpoints between origin and hit of query_cases.rays (the midpoint of origin and origin +
direction where a ray hits nothing).  The faces of scenes.make_box are wound both ways, so the box centre sees about half of its walls
from behind: enough to be excluded by the default max_backfacing, but not every sample.  (A probe inside one of G's spheres would not do
either: the reference's sphere has the near root only, so it is not seen from inside.)  The probe with backfacing == samples is the centre
of furnace(), a closed sphere of triangles wound outwards.  Together the sets hold a probe with 0 < missed < samples, at least 10 % of
samples that reach a third real vertex, all three BSDF kinds and both emitter kinds; tests/test_light_probes_cpu.py checks all that on
the yardstick."""
import numpy as np

from cpupathtrace_amd import scenes
from tests import gather_cases
from tests import query_cases

F = np.float32
N_PROBES = 257
BATCHES = [1, 63, 64, 65, 257]
SAMPLES = [1, 2, 63, 64, 65, 130]
CHUNKS = [1, 17, 64, 1000]
GRIDS = [(1, 1, 1), (2, 1, 3), (3, 4, 2)]
SEED = 31
OPTIONS = gather_cases.OPTIONS
CAMERA = gather_cases.CAMERA
FRAME_W, FRAME_H = gather_cases.FRAME_W, gather_cases.FRAME_H
POINT_LIGHT = {"S": (-0.6, 0.7, -0.6), "L": (-0.6, 0.7, -0.6), "G": (0.7, 0.2, 1.5)}
BOX_CENTRE = tuple(0.5 * (np.asarray(gather_cases.BOX_LO) + np.asarray(gather_cases.BOX_HI)))
BOX_CENTRE_INDEX = 3  # of G's probes
FURNACE_EMISSION = (0.75, 0.5, 0.25, 1.0)
FURNACE_SAMPLES = 1024

build = gather_cases.build


def hand_made(name):
    """Above everything, exactly on the emissive triangle, at a point light's position; in G also the centre of the closed box."""
    tri = np.asarray(gather_cases.G_EMISSIVE_TRIANGLE if name == "G" else gather_cases.GLOW_TRIANGLE, np.float64)
    pos = [(0.1, 3.0, 0.6), tuple(tri.mean(axis=0)), POINT_LIGHT[name]]
    if name == "G":
        pos.append(BOX_CENTRE)
    return np.asarray(pos, F)


def probes(handle, flat, name):
    """N_PROBES positions (n, 3) of a scene, the hand-made ones first."""
    rays = query_cases.rays(flat)
    t, obj = handle.intersect(rays)
    with np.errstate(invalid="ignore"):
        reach = np.where((t >= 0) & (obj >= 0), t, F(1.0)).astype(F)
    mid = (rays[:, :3] + rays[:, 3:] * (F(0.5) * reach)[:, None]).astype(F)
    mid = mid[np.isfinite(mid).all(axis=1)]
    pos = np.concatenate([hand_made(name), mid])
    assert len(pos) >= N_PROBES, len(pos)
    return np.ascontiguousarray(pos[:N_PROBES], F)


def grid_of(name, count):
    """A grid over the middle of the scene; in G one whose node (1, 0, 0) -- where the count has one -- or whose only node is the centre
    of the closed box."""
    count = tuple(int(c) for c in count)
    if name == "G":
        step = (0.5, 0.45, 0.5)  # (0.5: origin + 1 * step is the centre's x again, exactly, in float32)
        first = 1 if count[0] > 1 else 0
        origin = (float(F(BOX_CENTRE[0]) - F(first * step[0])), BOX_CENTRE[1], BOX_CENTRE[2])
        return origin, step, count
    return (-0.5, -0.4, 0.1), (0.45, 0.3, 0.7), count


def lookup_points(grid, seed=3):
    """Points (n, 3) and unit normals (n, 3) for a grid (origin, step, count): inside cells, exactly on every node, outside on every
    side, and one with a NaN coordinate."""
    origin, step, count = (np.asarray(v, np.float64) for v in grid)
    rng = np.random.default_rng(seed)
    extent = step * np.maximum(count - 1, 1)
    inside = origin + rng.uniform(0.0, 1.0, (40, 3)) * extent
    iz, iy, ix = np.meshgrid(*(np.arange(int(c)) for c in count[::-1]), indexing="ij")
    idx = np.stack([ix.ravel(), iy.ravel(), iz.ravel()], axis=1).astype(F)
    nodes = (np.asarray(grid[0], F) + (idx * np.asarray(grid[1], F)).astype(F)).astype(F)
    outside = []
    for a in range(3):
        for side in (-1.5, 2.5):
            p = origin + rng.uniform(0.0, 1.0, (3, 3)) * extent
            p[:, a] = origin[a] + side * extent[a]
            outside.append(p)
    corner = origin + np.array([[-2.0, -2.0, -2.0], [3.0, 3.0, 3.0]]) * extent
    nan = origin + 0.4 * extent
    nan = np.array([[np.nan, nan[1], nan[2]], [nan[0], np.nan, nan[2]], [nan[0], nan[1], np.nan]])
    pos = np.concatenate([inside, nodes, np.concatenate(outside), corner, nan]).astype(F)
    nrm = rng.normal(size=(len(pos), 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return np.ascontiguousarray(pos, F), np.ascontiguousarray(nrm, F)


def furnace(emission=FURNACE_EMISSION, radius=1.0, rings=6, sectors=8):
    """One closed sphere of triangles around the origin, wound outwards, with diffuse (0, 0, 0, 1) and the given emission: (scene dict,
    the flat scene for the oracle -- a scene without instances is its own flat scene)."""
    theta = np.pi * np.arange(rings + 1) / rings
    phi = 2.0 * np.pi * np.arange(sectors) / sectors
    def at(i, j):
        return (radius * np.sin(theta[i]) * np.cos(phi[j % sectors]), radius * np.cos(theta[i]), radius * np.sin(theta[i]) * np.sin(phi[j % sectors]))
    tris = []
    for i in range(rings):
        for j in range(sectors):
            a, b, c, d = at(i, j), at(i + 1, j), at(i + 1, j + 1), at(i, j + 1)
            if i > 0:
                tris.append([a, d, c])
            if i < rings - 1:
                tris.append([a, c, b])
    tris = np.asarray(tris, F)
    n = np.cross(tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0])
    assert ((n * tris.mean(axis=1)).sum(axis=1) > 0).all()  # wound outwards
    sb = scenes.SceneBuilder()
    sb.triangles(tris, sb.material(diffuse=(0.0, 0.0, 0.0, 1.0), emission=emission))
    scene = sb.build()
    return scene, dict(scene=scene)
