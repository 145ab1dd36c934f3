"""The yardstick of include/pt_gather.h: a numpy composition of the three gather kinds out of a CPU checker's own pieces
-- intersect, sample_lights, bsdf_propagate, bsdf_spectrum, normal, each taking and returning the engine state -- with the arithmetic
between them in float32 / float64 numpy in the order of the reference's worker.cpp:44-139, and a numpy xorshift engine with libstdc++'s
uniform_real_distribution<float> (pinned to the checkers' rng_draws / uniform_floats by tests/test_gather_cpu.py).  The core is
paths_from_vertex, vectorised over the set of paths that are still alive; tests/test_gather_cpu.py pins it to the compiled reference's
getSample by feeding it camera rays.  Works against either checker (oracle.Checker("oracle") or ("ref")): the material of an object is
taken from the flat scene, not from the checker."""
import numpy as np

from cpupathtrace_amd import binding

F, D, U64 = np.float32, np.float64, np.uint64
NO_MATERIAL = 0xFFFFFFFF
OCCLUSION, DIRECT, PATHS = binding.GATHER_OCCLUSION, binding.GATHER_DIRECT, binding.GATHER_PATHS
MAX_LIGHTS = 32


# ---- the engine (base.h:24-38) and uniform_real_distribution<float>(0, 1) -------------------------------------------------------------------

def pixel_seed(base_seed, x, y):
    """pt_pixel_seed for arrays of x and y."""
    with np.errstate(over="ignore"):
        x, y = np.asarray(x, np.int64).astype(np.uint32).astype(U64), np.asarray(y, np.int64).astype(np.uint32).astype(U64)
        z = U64(base_seed & 0xFFFFFFFFFFFFFFFF) + U64(0x9E3779B97F4A7C15) * (U64(1) + (y << U64(32)) + x)
        z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
        return z ^ (z >> U64(31))


def seed_to_state(seed):
    seed = np.asarray(seed, U64)
    return seed ^ (~seed << U64(32))


def draw(states):
    """One 32-bit draw of every engine: (values uint32, new states)."""
    s = np.asarray(states, U64)
    with np.errstate(over="ignore"):
        result = s * U64(0xD989BCACC137DCD5)
    s = s ^ (s >> U64(11))
    s = s ^ (s << U64(31))
    s = s ^ (s >> U64(18))
    return (result >> U64(32)).astype(np.uint32), s


def uniform01(states):
    """dist(re) of uniform_real_distribution<float>(0, 1): generate_canonical<float, 24> is one draw / 2^32, clamped below 1."""
    v, s = draw(states)
    r = (v.astype(F) / F(4294967296.0)).astype(F)
    r = np.where(r >= F(1.0), np.nextafter(F(1.0), F(0.0)), r).astype(F)
    return (r * (F(1.0) - F(0.0)) + F(0.0)).astype(F), s


def sample_states(base_seed, n_points, samples, first_point=0):
    """The engines of a call: RandomEngine(pt_pixel_seed(base_seed, x = sample, y = point)), (n_points, samples)."""
    point, sample = np.meshgrid(np.arange(first_point, first_point + n_points), np.arange(samples), indexing="ij")
    return seed_to_state(pixel_seed(base_seed, sample, point))


# ---- float32 vector arithmetic in the reference's order (vector.h) ----------------------------------------------------------------------------

def _dot(a, b):
    d = F(0.0) + a[:, 0] * b[:, 0]
    d = d + a[:, 1] * b[:, 1]
    return (d + a[:, 2] * b[:, 2]).astype(F)


def _len(a):
    return np.sqrt(_dot(a, a)).astype(F)


def _normalize(a):
    return (a * (F(1.0) / _len(a))[:, None]).astype(F)


def _fmin_std(a, b):
    """std::min(a, b) = (b < a) ? b : a"""
    return np.where(b < a, b, a).astype(F)


# ---- materials of a flat scene ------------------------------------------------------------------------------------------------------------------

def material_of_object(scene):
    """The material index of every object of a flat scene (NO_MATERIAL: the default handler)."""
    kind = np.asarray(scene["obj_kind"])
    which = np.where(kind == 0, np.cumsum(kind == 0) - 1, np.cumsum(kind == 1) - 1)
    tri = np.asarray(scene["tri_material"], np.uint32).reshape(-1)
    sph = np.asarray(scene["sph_material"], np.uint32).reshape(-1)
    out = np.full(len(kind), NO_MATERIAL, np.uint32)
    if (kind == 0).any():
        out[kind == 0] = tri[which[kind == 0]]
    if (kind == 1).any():
        out[kind == 1] = sph[which[kind == 1]]
    return out


def material_rows(scene, index):
    """diffuse, specular, emission (n, 4), ior, bsdf, one_way (n,) of the material indices; the default handler is white Lambertian
    without emission (object.cpp:9-11, material.cpp:3-17)."""
    index = np.asarray(index, np.uint32)
    n = len(index)
    diffuse, specular, emission = np.ones((n, 4), F), np.ones((n, 4), F), np.zeros((n, 4), F)
    ior, bsdf, one_way = np.ones(n, F), np.zeros(n, np.int32), np.zeros(n, np.int32)
    has = index != NO_MATERIAL
    if has.any():
        table = np.asarray(scene["materials"])
        rows = table[index[has].astype(np.int64)]
        diffuse[has], specular[has], emission[has] = rows["diffuse"], rows["specular"], rows["emission"]
        ior[has], bsdf[has], one_way[has] = rows["ior"], rows["bsdf"], rows["one_way"]
    return diffuse, specular, emission, ior, bsdf, one_way


def _by_bsdf(bsdf, one_way):
    """The lanes of every (bsdf kind, one_way) pair that occurs."""
    key = bsdf.astype(np.int64) * 2 + (one_way != 0)
    return [(int(k) // 2, int(k) % 2, np.nonzero(key == k)[0]) for k in np.unique(key)]


def _spectrum(checker, bsdf, one_way, from_dir, to_dir, nrm, light, diffuse, specular, synthetic):
    n = len(bsdf)
    rgba, shade, p = np.zeros((n, 4), F), np.zeros(n, F), np.zeros(n, F)
    for kind, ow, idx in _by_bsdf(bsdf, one_way):
        rgba[idx], shade[idx], p[idx] = checker.bsdf_spectrum(kind, ow, from_dir[idx], to_dir[idx], nrm[idx], light[idx], diffuse[idx], specular[idx], synthetic)
    return rgba, shade, p


def _propagate(checker, bsdf, one_way, ray_dir, pos, nrm, epsilon, ior, states):
    n = len(bsdf)
    out_ray, fac, pd, st = np.zeros((n, 6), F), np.zeros(n, F), np.zeros(n, F), np.zeros(n, U64)
    rays = np.concatenate([pos, ray_dir], axis=1).astype(F)
    for kind, ow, idx in _by_bsdf(bsdf, one_way):
        out_ray[idx], fac[idx], pd[idx], st[idx] = checker.bsdf_propagate(kind, ow, rays[idx], pos[idx], nrm[idx], epsilon, ior[idx], states[idx])
    return out_ray, fac, pd, st


# ---- getSample from a vertex on (worker.cpp:50-139) ------------------------------------------------------------------------------------------------

def paths_from_vertex(handle, flat, ray_dir, pos, nrm, material, states, epsilon, path_length0, direct_only=False, roulette=True, bounces=True):
    """getSample's loop entered behind its intersection test (worker.cpp:50) for n paths that stand on a vertex: the ray that came in has
    the direction ray_dir (n, 3), the vertex the position pos, the normal nrm and the material index `material`; path_length0 vertices
    came before it, and every accumulator has its initial value.  states (n,) are the engines' raw states.
      direct_only: the vertex's light samples alone (worker.cpp:74-103), nothing behind them;  roulette = False: no roulette number is
      drawn (the bounce is not taken);  bounces = False: the roulette number is drawn and the bounce is not taken.
    Returns (out_spectrum (n, 4) -- the alpha is whatever the sums make it, getSample overwrites it --, end states (n,), a dict: vertices
    (n,) shaded per path, bsdf_kinds: the set of BSDF kinds a bounce was sampled from, light_pos: the positions sampled on emitters)."""
    checker, scene = handle.c, flat["scene"]
    eps = F(epsilon)
    n = len(pos)
    states = np.array(states, U64).reshape(n)
    out, spectrum = np.zeros((n, 4), F), np.ones((n, 4), F)
    contribution_unweighted = np.ones(n, F)
    divisor, bounce_pd = np.ones(n, D), np.ones(n, D)
    path_length = np.full(n, int(path_length0), np.int64)
    vertices = np.zeros(n, np.int64)
    bsdf_kinds, emitter_pos = set(), []
    of_object = material_of_object(scene)
    n_point_lights = len(np.asarray(scene["light_pos"]).reshape(-1, 3))
    live = np.arange(n)
    ray_dir, pos, nrm, material = (np.array(ray_dir, F).reshape(n, 3), np.array(pos, F).reshape(n, 3), np.array(nrm, F).reshape(n, 3),
                                   np.array(material, np.uint32).reshape(n))
    with np.errstate(all="ignore"):
        while len(live) > 0:
            path_length[live] += 1
            vertices[live] += 1
            diffuse, specular, emission, ior, bsdf, one_way = material_rows(scene, material)
            # :62-64
            w = (divisor[live] * bounce_pd[live]).astype(F)
            out[live] = (out[live] + ((spectrum[live] * emission).astype(F) / w[:, None]).astype(F)).astype(F)
            # :67-70
            sp = spectrum[live]
            contribution = (((sp[:, 0] + sp[:, 1]).astype(F) + sp[:, 2]).astype(F) / F(3.0)).astype(F)
            probability = (F(0.1) + F(0.1) * _fmin_std((contribution_unweighted[live] * contribution).astype(F), F(1.0))).astype(F)
            probability = np.where(path_length[live] <= 4, F(1.0), probability).astype(F)
            do_bounce = np.zeros(len(live), bool)
            if roulette and not direct_only:
                u, states[live] = uniform01(states[live])
                do_bounce = u < probability
            # :74-103
            count, light_pos, light_rgba, light_pd, states[live] = handle.sample_lights(pos, states[live], MAX_LIGHTS)
            assert (count <= MAX_LIGHTS).all()
            for j in range(int(count.max()) if len(count) else 0):
                sel = np.nonzero(j < count)[0]
                if j >= n_point_lights:
                    emitter_pos.append(light_pos[sel, j].copy())
                to_light = (light_pos[sel, j] - pos[sel]).astype(F)
                light_dir = _normalize(to_light)
                origin = (pos[sel] + light_dir * eps).astype(F)
                light_t, _ = handle.intersect(np.concatenate([origin, light_dir], axis=1))
                visible = (light_t < F(0.0)) | (light_t >= (_len(to_light) - eps).astype(F))
                base, shading_factor, shadow_ray_pd = _spectrum(checker, bsdf[sel], one_way[sel], ray_dir[sel], light_dir, nrm[sel], light_rgba[sel, j], diffuse[sel],
                                                                specular[sel], True)
                lanes = live[sel]
                combined = ((base * shading_factor[:, None]).astype(F) * spectrum[lanes]).astype(F)
                weight = (divisor[lanes] * bounce_pd[lanes] * light_pd[sel, j].astype(D) * shadow_ray_pd.astype(D)).astype(F)
                weighed = (combined / weight[:, None]).astype(F)
                add = visible & (shadow_ray_pd > F(0.0))
                out[lanes[add]] = (out[lanes[add]] + weighed[add]).astype(F)
            if direct_only:
                break
            # :106-114
            if not bounces:
                do_bounce[:] = False
            bounce_pd[live] = np.where(do_bounce, bounce_pd[live] * probability.astype(D), bounce_pd[live] * (F(1.0) - probability).astype(F).astype(D))
            go = np.nonzero(do_bounce & ~(bounce_pd[live] <= 1E-20))[0]
            if len(go) == 0:
                break
            live, ray_dir, pos, nrm = live[go], ray_dir[go], pos[go], nrm[go]
            diffuse, specular, ior, bsdf, one_way = diffuse[go], specular[go], ior[go], bsdf[go], one_way[go]
            bsdf_kinds.update(int(k) for k in np.unique(bsdf))
            # :117-136
            next_ray, ray_factor, ray_pd, states[live] = _propagate(checker, bsdf, one_way, ray_dir, pos, nrm, float(eps), ior, states[live])
            divisor[live] = divisor[live] * ray_pd.astype(D)
            divisor[live] = divisor[live] / ray_factor.astype(D)
            contribution_unweighted[live] = (contribution_unweighted[live] * ray_factor).astype(F)
            shaded, shading_factor, shading_pd = _spectrum(checker, bsdf, one_way, ray_dir, next_ray[:, 3:], nrm, spectrum[live], diffuse, specular, False)
            divisor[live] = divisor[live] * shading_pd.astype(D)
            divisor[live] = divisor[live] / shading_factor.astype(D)
            contribution_unweighted[live] = (contribution_unweighted[live] * shading_factor).astype(F)
            spectrum[live] = shaded
            # :134-138, :45-49
            t, obj = handle.intersect(next_ray)
            go = np.nonzero(~(divisor[live] <= 1E-20) & ~(t < F(0.0)))[0]
            live, next_ray, t, obj = live[go], next_ray[go], t[go], obj[go]
            if len(live) == 0:
                break
            ray_dir = next_ray[:, 3:].astype(F)
            pos = (next_ray[:, :3] + ray_dir * t[:, None]).astype(F)
            nrm = handle.normal(obj, pos)[0].astype(F)
            material = of_object[obj]
    return out, states, dict(vertices=vertices, bsdf_kinds=bsdf_kinds, light_pos=np.concatenate(emitter_pos) if emitter_pos else np.zeros((0, 3), F))


def paths_from_rays(handle, flat, rays, states, epsilon):
    """getSample behind its camera ray: (rgba with getSample's alpha (n, 4), collected (n,), end states (n,), paths_from_vertex's dict)."""
    rays = np.asarray(rays, F).reshape(-1, 6)
    states = np.array(states, U64).reshape(-1)
    t, obj = handle.intersect(rays)
    hit = np.nonzero(~(t < F(0.0)))[0]
    rgba = np.zeros((len(rays), 4), F)
    pos = (rays[hit, :3] + rays[hit, 3:] * t[hit, None]).astype(F)
    nrm = handle.normal(obj[hit], pos)[0].astype(F)
    out, states[hit], info = paths_from_vertex(handle, flat, rays[hit, 3:], pos, nrm, material_of_object(flat["scene"])[obj[hit]], states[hit], epsilon, 0)
    rgba[hit] = out
    rgba[hit, 3] = F(1.0)
    collected = np.zeros(len(rays), np.uint8)
    collected[hit] = 1
    return rgba, collected, states, info


# ---- the three kinds ----------------------------------------------------------------------------------------------------------------------------------

def samples_of(handle, flat, kind, points, normals, samples, epsilon, distance=np.inf, base_seed=0, first_point=0):
    """Every sample of every point: kind OCCLUSION -> (occluded (n, samples) bool, None); else (out_spectrum (n, samples, 4), paths_from_vertex's dict)."""
    points, normals = np.asarray(points, F).reshape(-1, 3), np.asarray(normals, F).reshape(-1, 3)
    n = len(points)
    states = sample_states(base_seed, n, samples, first_point).reshape(-1)
    pos, nrm = np.repeat(points, samples, axis=0), np.repeat(normals, samples, axis=0)
    ray_dir = (-nrm).astype(F)
    if kind == OCCLUSION:
        next_ray, _, _, _ = handle.c.bsdf_propagate(0, 0, np.concatenate([pos, ray_dir], axis=1), pos, nrm, float(F(epsilon)), np.ones(len(pos), F), states)
        t, _ = handle.intersect(next_ray)
        with np.errstate(invalid="ignore"):
            return ((t >= F(0.0)) & (t < F(distance))).reshape(n, samples), None
    material = np.full(len(pos), NO_MATERIAL, np.uint32)
    out, _, info = paths_from_vertex(handle, flat, ray_dir, pos, nrm, material, states, epsilon, 0, direct_only=kind == DIRECT)
    return out.reshape(n, samples, 4), info


def gather(handle, flat, kind, points, normals, samples, epsilon, distance=np.inf, base_seed=0):
    """pt_gather_points: (n,) records of dtype binding.GatherResult."""
    got, _ = samples_of(handle, flat, kind, points, normals, samples, epsilon, distance, base_seed)
    return records(kind, got, samples)


def records(kind, got, samples):
    n = len(got)
    out = np.zeros(n, binding.GatherResult)
    out["samples"] = samples
    out["value"][:, 3] = F(1.0)
    if kind == OCCLUSION:
        occluded = got.sum(axis=1).astype(np.uint32)
        out["occluded"] = occluded
        out["value"][:, :3] = ((samples - occluded).astype(F) / F(samples)).astype(F)[:, None]
        return out
    acc = np.zeros((n, 3), F)
    with np.errstate(all="ignore"):
        for s in range(samples):
            acc = (acc + got[:, s, :3]).astype(F)
        out["value"][:, :3] = (acc / F(samples)).astype(F)
    return out


def assert_records_equal(got, want, what=""):
    """Bit for bit; two NaNs of any payload compare equal."""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    for name in ("samples", "occluded", "pad"):
        bad = got[name] != want[name]
        assert not bad.any(), "%s: %s differs for %d records, first at %s: got %s want %s" % (what, name, bad.sum(), np.argwhere(bad)[0].tolist(), got[name][bad][0], want[name][bad][0])
    g, w = np.ascontiguousarray(got["value"]), np.ascontiguousarray(want["value"])
    bad = (g.view(np.uint32) != w.view(np.uint32)) & ~(np.isnan(g) & np.isnan(w))
    assert not bad.any(), "%s: value differs for %d numbers, first at %s: got %r want %r" % (what, bad.sum(), np.argwhere(bad)[0].tolist(), g[bad][0], w[bad][0])
